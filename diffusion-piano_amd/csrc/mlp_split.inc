// mlp_split.inc - the rows half of the PPO minibatch step (ppo_v2.py:266-293) with each
// network's 16-row tile split over NSPL workgroups by hidden columns (included by pianorl.hip
// after mlp_step.inc; prl_mlp_step* select it for minibatches of <= 256 rows whose hidden
// widths are 128 or 256; PIANORL_MLP_SPLIT=0 keeps mlp_rows_kernel).
//
// Why: mlp_rows_kernel runs a tile's eight layer passes on ONE CU (16 of 256 CUs busy at 128
// rows, 83 us per step, 2 TFLOP/s). Here member s of a (tile, network) group computes hidden
// columns [s cw, (s + 1) cw) of every layer GEMM (cw = width / NSPL): a quarter of the matrix
// work and of the weight bytes per CU. The group exchanges one [16][cw] fp32 slice per member
// six times per step - forward the ReLU outputs of layers 0..2 (LayerNorm needs whole rows),
// backward dY = dZ W of layers 2..0 (LayerNorm backward's row means need whole rows) - and
// after each exchange every member holds the whole rows and runs the row work (LayerNorm
// forward / backward, dropout, the output layer and both heads) redundantly: identical inputs
// and arithmetic, identical results in every member. A member writes only its own columns
// (the weight-gradient inputs X / dZ, the column-sum partials); member 0 writes the output
// layer's and the heads' rows. Dropout (the critic's): each member draws the Philox keep bits
// of its own columns in the GEMM epilogue and sends them with the values (the sign bit of the
// non-negative ReLU output: a dropped element travels as -z, -0.0 for z = 0).
//
// Hand-off (MI355X_MICROARCH.md, visibility, "R2": the data IS the flag): every element
// travels as one 8-byte {tag, value} granule written by ONE sc1 store (untorn), tag = the
// group's call count x 6 + exchange + 1; a consumer wave re-reads its share of the other
// members' granules with 8-byte sc1 (agent-scope relaxed atomic) loads until every tag
// matches - no drain, no counter, no fence. The call count (one word per group in the work
// space) is read by every member at its start and advanced by member 0 after its last wait
// (every member has read it by then: their last granules carry it). Memory: the caller's
// hipMalloc'd work space, zeroed before the first call (tags 0 never match); one workgroup per
// CU (the LDS request is over half a CU; the host takes this kernel only when the groups'
// workgroups fit the device's CU count). Every wait is bounded (SPLIT_SPIN_TICKS of the 100 MHz
// wall clock by default): a timeout writes 1 + the exchange index to the error word (the
// caller's guard word, or the work space's last word) and that step's outputs are garbage,
// never a hang. The guard is what keeps the garbage out of the weights: the gradient kernel
// does not advance the Adam step counts and prl_clip_adam* apply nothing while it is set, and
// the host (ppo.py) reads it once per update, re-zeroes the exchange region and raises.
// Placement: the NSPL members of a group are blocks b, b + 8, b + 16, b + 24 (one XCD under the
// round-robin dispatch: speed only, never correctness).
//
// Weights: each wave's slice of the next GEMM's weights is loaded into registers one GEMM
// ahead (issued before an exchange's wait, landing while the wave waits for the others).

namespace mlp {

constexpr int NSPL = 4;           // members per (tile, network) group
constexpr int SWV = 4;            // waves per member: one 16-column tile of the member's slice each
constexpr int ST = SWV * 64;
constexpr int NHAND = 6;          // exchanges per step
constexpr int SCW = HMAX / NSPL;  // slice width bound (64 columns)
constexpr int SBF = 24;           // 16-k blocks of a layer-0 weight row slice: state width <= 384
constexpr int SBH = HMAX / 16;    // 16-k blocks of a hidden-layer row / column slice
constexpr int SPLIT_MAX_SDIM = SBF * 16;
constexpr int SPLIT_MAX_ROWS = 256;  // 32 groups x 4 members = 128 workgroups at most
constexpr uint64_t SPLIT_SPIN_TICKS = 200000000ull;  // 2 s
typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;

// the work space's tail: granules [groups][NHAND][NSPL][MT][SCW] (8 bytes = 2 floats each),
// then the call counts [groups] u32, then the error word (the last word)
__host__ __device__ inline size_t split_hand_floats(int groups) { return (size_t)groups * NHAND * NSPL * MT * SCW * 2; }

// LDS (floats): S tile [16][KS] | XH [3][16][HS] | Y (forward: the layer input; backward: the
// layer's dZ) [16][HS] | Zf (forward: ReLU outputs; backward: column-sum terms) [16][HS] | dY
// [16][HS] | output layer [16][64] | 1/std [3][16] | ReLU bits, dropout keep bits [2][3][256]
// u16 | head scratch [64] | state row indices [16] i64 | LayerNorm gamma / beta [3][2][256]
// (every offset 16 B aligned)
__host__ __device__ inline size_t split_lds_floats(int KS) {
  return (size_t)MT * KS + 3 * MT * HS + 3 * MT * HS + MT * 64 + 3 * MT + 2 * 3 * 256 / 2 + 64 + 2 * MT +
         3 * 2 * HMAX;
}

// Weight slices are loaded without branches: a load whose result joins another path's at a
// branch makes the compiler wait for it there (and, vmcnt being in order, for every load
// before it), which serialises a prefetch batch into one L2 / HBM round trip per block.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// forward row slice of a wave, K a multiple of 16: w[u] = W[min(n0 + i, N - 1)][16u + 4q ..]
// for u < K / 16 (blocks past that repeat the last one, unused)
template <int NB>
__device__ __forceinline__ void ld_rows(f4 (&w)[NB], const float* __restrict__ W, int N, int K, int n0, int lane) {
  const int i = lane & 15, q = lane >> 4;
  const float* wrow = W + (size_t)min(n0 + i, N - 1) * K + 4 * q;
  const int nb = K >> 4;
#pragma unroll
  for (int u = 0; u < NB; u++) w[u] = *reinterpret_cast<const f4u*>(wrow + 16 * min(u, nb - 1));
}

// layer 0's row slice (K = the state width, any K >= 32): the full blocks u < nb - 1 as one
// 16-byte load each (4-byte aligned when K % 4 != 0: gfx950 global loads take any 4-byte
// aligned address, and the compiler emits global_load_dwordx4 for this type), the last block
// (nb - 1, partial when K % 16 != 0) as four clamped dword loads into wt (its columns past K
// meet the state tile's zero padding)
template <int NB>
__device__ __forceinline__ void ld_rows0(f4 (&w)[NB], f4& wt, const float* __restrict__ W, int N, int K, int n0,
                                         int lane) {
  const int i = lane & 15, q = lane >> 4;
  const float* wrow = W + (size_t)min(n0 + i, N - 1) * K + 4 * q;
  const int nb = (K + 15) >> 4;
#pragma unroll
  for (int u = 0; u < NB; u++) w[u] = *reinterpret_cast<const f4u*>(wrow + 16 * min(u, nb - 2));
  const int k0 = 16 * (nb - 1);
#pragma unroll
  for (int s = 0; s < 4; s++) wt[s] = wrow[min(k0 + s, K - 1 - 4 * q)];
}

// Z[16][16] = X[16][K] W_slice^T (X in LDS, zero past K up to a multiple of 16): block u, MFMA
// s takes k = 16u + 4q + s (gemm_xwt's order); block nb - 1 from wt when given (layer 0)
template <int NB, bool TAIL>
__device__ __forceinline__ f4 mm_rows(const f4 (&w)[NB], f4 wt, const float* X, int xs, int K, int lane) {
  const int i = lane & 15, q = lane >> 4;
  const float* xrow = X + i * xs + 4 * q;
  const int nb = (K + 15) >> 4;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NB; u++) {
    if (u < nb) {
      const f4 a4 = *reinterpret_cast<const f4*>(xrow + 16 * u);
      const f4 b4 = TAIL && u == nb - 1 ? wt : w[u];
#pragma unroll
      for (int s = 0; s < 4; s++) acc = mfma(a4[s], b4[s], acc);
    }
  }
  return acc;
}

// backward column slice of a wave, in the MFMA's B layout directly: w[u][s] = W[min(16u + 4q
// + s, N - 1)][min(k0 + i, K - 1)] (four dword loads per block; the 16 lanes of a row group read 64
// consecutive bytes of a row). The same values, in the same order, as gemm_dzw's float4 loads
// transposed through LDS - without the per-block LDS round trip.
template <int NB>
__device__ __forceinline__ void ld_cols(f4 (&w)[NB], const float* __restrict__ W, int N, int K, int k0, int lane) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int u = 0; u < NB; u++)
#pragma unroll
    for (int s = 0; s < 4; s++) w[u][s] = W[(size_t)min(16 * u + 4 * q + s, N - 1) * K + min(k0 + i, K - 1)];
}

// dX[16][16] = dZ[16][N] W[N][k-tile] (dZ in LDS, zero past N up to a multiple of 16), the k
// (= n) order of gemm_dzw
template <int NB>
__device__ __forceinline__ f4 mm_cols(const f4 (&w)[NB], const float* dZ, int zs, int N, int lane) {
  const int i = lane & 15, q = lane >> 4;
  const float* zrow = dZ + i * zs + 4 * q;
  const int nb = (N + 15) >> 4;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NB; u++) {
    if (u < nb) {
      const f4 a4 = *reinterpret_cast<const f4*>(zrow + 16 * u);
#pragma unroll
      for (int s = 0; s < 4; s++) acc = mfma(a4[s], w[u][s], acc);
    }
  }
  return acc;
}

// s_waitcnt vmcnt(0) (expcnt / lgkmcnt left at their maxima), gfx9 encoding
constexpr unsigned VMCNT0 = 0x0F70;

// ---------------------------------------------------------------- the group's exchanges
struct Hand {
  gu64* buf;     // this group's [NHAND][NSPL][MT][SCW] granules
  gu32* err;     // the error word
  unsigned gen;  // this group's call count
  int sp;        // this member
  uint64_t spin; // the bounded wait (wall-clock ticks)
  int fault;     // test hook (Args::fault)
};
__device__ __forceinline__ unsigned hand_tag(const Hand& H, int h) { return H.gen * NHAND + h + 1; }

// the wave's 16 x 16 accumulator tile (rows 4q + r, column i) into column cc of this member's
// slice of exchange h: one {tag, value} granule per element, one 8-byte sc1 store each
__device__ __forceinline__ void hand_put(const Hand& H, int h, int cc, f4 v, int lane) {
  gu64* dst = H.buf + (size_t)(h * NSPL + H.sp) * MT * SCW + cc + (lane & 15);
  // (the test hook publishes member 1's exchange 0 with tag 0, which no wait accepts)
  const unsigned long long tag = (H.fault && h == 0 && H.sp == 1) ? 0ull : (unsigned long long)hand_tag(H, h) << 32;
#pragma unroll
  for (int r = 0; r < 4; r++)
    __hip_atomic_store(dst + (4 * (lane >> 4) + r) * SCW, tag | __float_as_uint(v[r]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// every thread re-reads its share of the other members' granules of exchange h - two granules
// (16 bytes) per load, all of a pass issued before any tag is checked; sc1 (+ volatile: sc0,
// and never hoisted out of the loop) buffer loads - until every tag in its wave matches, then
// writes the values into dst [MT][ds] at their columns; the barrier publishes them. CW = the
// slice width (the layer width / NSPL).
template <int CW>
__device__ __forceinline__ void hand_get(const Hand& H, int h, float* dst, int ds, bool& dead) {
  constexpr int PER = MT * CW / 2, NG = (NSPL - 1) * PER / ST;  // granule pairs per slice / per thread
  static_assert((NSPL - 1) * PER % ST == 0, "whole granule pairs per thread");
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(H.buf + (size_t)h * NSPL * MT * SCW, (short)0,
                                                    NSPL * MT * SCW * 8, 0x00020000);
  const unsigned tag = hand_tag(H, h);
  int src[NG], dix[NG];
#pragma unroll
  for (int u = 0; u < NG; u++) {
    const int j = threadIdx.x + u * ST, o = j / PER, rem = j % PER;
    const int sm = o + (o >= H.sp ? 1 : 0), r = rem / (CW / 2), c = 2 * (rem % (CW / 2));
    src[u] = ((sm * MT + r) * SCW + c) * 8;
    dix[u] = r * ds + sm * CW + c;
  }
  using u4 = __attribute__((ext_vector_type(4))) unsigned;
  u4 g[NG];
  uint64_t t0 = 0;
  for (int pass = 0;; pass++) {
#pragma unroll
    for (int u = 0; u < NG; u++) g[u] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, src[u], 0, (int)0x80000010));
    bool ok = true;
#pragma unroll
    for (int u = 0; u < NG; u++) ok &= g[u][1] == tag && g[u][3] == tag;
    if (__all(ok) || dead) break;  // (wave-uniform)
    __builtin_amdgcn_s_sleep(1);
    const uint64_t t = wall_clock64();
    if (pass == 0) {
      t0 = t;
    } else if (t - t0 > H.spin) {
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(H.err, 1u + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      dead = true;  // later exchanges of this wave do not wait again
      break;
    }
  }
  // every load of this wave done (the granules', and the weights / row parameters prefetched
  // before the wait): stated as a wait the compiler sees
  __builtin_amdgcn_s_waitcnt(VMCNT0);
#pragma unroll
  for (int u = 0; u < NG; u++) {
    dst[dix[u]] = __uint_as_float(g[u][0]);
    dst[dix[u] + 1] = __uint_as_float(g[u][2]);
  }
  __syncthreads();
}

// the epilogue of a hidden layer's GEMM tile: bias, ReLU, and the dropout keep bit of (row,
// column n) in the sign (dropped: the value negated, -0.0 for 0); rows row0 .. row0 + 3
__device__ __forceinline__ f4 relu_keep(f4 v, float bias, float p, uint64_t seed, uint64_t step, int l, int row0,
                                        int n) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float z = v[r] + bias;
    float y = z > 0.f ? z : 0.f;
    if (p > 0.f && !keep_elem(seed, step, l, row0 + r, n, p)) y = __uint_as_float(__float_as_uint(y) | 0x80000000u);
    v[r] = y;
  }
  return v;
}

// ---------------------------------------------------------------- whole-row work
// thread t = (row r = t >> 4, j = t & 15) takes columns j + 16m of row r; a row's 16 threads
// are one DPP row, summed by row16_sum and broadcast from its lane 15
__device__ __forceinline__ float row_total(float v, int lane) { return __shfl(row16_sum(v), lane | 15, 64); }

// LayerNorm forward of layer l over whole rows (N = 16 NM columns): Zf = the members' ReLU
// outputs with their keep bits -> XH[l], Y (the next layer's input, dropout applied), the ReLU
// and keep bits, 1/std; this member's columns of Y to Xrow. gamma / beta from LDS (LNP). Means and variances divide by N
// as a multiplication by 1/N (a power of two: the same bits). Every argument a value: a
// reference into the kernel argument block would be re-read behind each global store.
template <int NM>
__device__ __forceinline__ void ln_fwd(int l, int sp, bool rowok, float eps, float p, const float* LNP, const float* Zf,
                                       float* Y, float* XH, float* RS, uint16_t* RM, uint16_t* DM, float* Xrow) {
  constexpr int N = 16 * NM, CW = N / NSPL;
  constexpr float inv = 1.f / (float)N;
  const int t = threadIdx.x, r = t >> 4, j = t & 15, lane = t & 63;
  float z[NM];
  float s = 0.f;
  unsigned bits = 0, keep = 0;
#pragma unroll
  for (int m = 0; m < NM; m++) {
    const unsigned u = __float_as_uint(Zf[r * HS + j + 16 * m]);
    keep |= ((u >> 31) ^ 1u) << m;
    z[m] = __uint_as_float(u & 0x7fffffffu);
    s += z[m];
    bits |= (z[m] > 0.f ? 1u : 0u) << m;
  }
  const float mean = row_total(s, lane) * inv;
  float s2 = 0.f;
#pragma unroll
  for (int m = 0; m < NM; m++) {
    z[m] -= mean;
    s2 += z[m] * z[m];
  }
  const float rs = 1.f / sqrtf(row_total(s2, lane) * inv + eps);
  const float ps = p > 0.f ? 1.f / (1.f - p) : 1.f;
#pragma unroll
  for (int m = 0; m < NM; m++) {
    const int c = j + 16 * m;
    const float xh = z[m] * rs;
    float y = xh * LNP[(2 * l) * HMAX + c] + LNP[(2 * l + 1) * HMAX + c];
    if (p > 0.f) y = (keep >> m) & 1 ? y * ps : 0.f;
    XH[(l * MT + r) * HS + c] = xh;
    Y[r * HS + c] = y;
  }
  RM[l * 256 + t] = (uint16_t)bits;
  DM[l * 256 + t] = (uint16_t)keep;
  if (j == 0) RS[l * MT + r] = rs;
  if (rowok)  // the member's columns, read back (a global store inside the loop would make
              // every later iteration wait for the one before)
#pragma unroll
    for (int o = 0; o < CW / 16; o++) {
      const int c = j + 16 * (sp * (CW / 16) + o);
      Xrow[c] = Y[r * HS + c];
    }
}

// LayerNorm / ReLU / dropout backward of layer l over whole rows: dYf -> dZ (LDS, the next dX
// GEMM's input); this member's columns to the layer's dZ rows (dZrow) and their column sums
// (gamma, beta, bias) to the tile's partial row at pog / pobe / pob, summed over the rows in order
template <int NM>
__device__ __forceinline__ void ln_bwd(int l, int sp, bool rowok, float p, const float* LNP, const float* dYf, float* dZ,
                                       const float* XH, const float* RS, const uint16_t* RM, const uint16_t* DM,
                                       float* CS, float* dZrow, float* pog, float* pobe, float* pob) {
  constexpr int N = 16 * NM, CW = N / NSPL;
  constexpr float inv = 1.f / (float)N;
  const int t = threadIdx.x, r = t >> 4, j = t & 15, lane = t & 63;
  const unsigned keep = DM[l * 256 + t], bits = RM[l * 256 + t];
  const float ps = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float dxh[NM], xh[NM];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int m = 0; m < NM; m++) {
    const int c = j + 16 * m;
    float gg = dYf[r * HS + c];
    if (p > 0.f) gg = (keep >> m) & 1 ? gg * ps : 0.f;
    dxh[m] = gg * LNP[(2 * l) * HMAX + c];
    xh[m] = XH[(l * MT + r) * HS + c];
    s1 += dxh[m];
    s2 += dxh[m] * xh[m];
  }
  const float m1 = row_total(s1, lane) * inv, m2 = row_total(s2, lane) * inv;
  const float rsr = RS[l * MT + r];
#pragma unroll
  for (int m = 0; m < NM; m++) {
    const float dr = rsr * (dxh[m] - m1 - xh[m] * m2);
    dZ[r * HS + j + 16 * m] = (bits >> m) & 1 ? dr : 0.f;
  }
  // the member's columns (read back from LDS): dZ rows, and the column-sum terms
#pragma unroll
  for (int o = 0; o < CW / 16; o++) {
    const int m = sp * (CW / 16) + o, c = j + 16 * m, cc = j + 16 * o;
    float gg = dYf[r * HS + c];
    if (p > 0.f) gg = (keep >> m) & 1 ? gg * ps : 0.f;
    const float x = XH[(l * MT + r) * HS + c], dz = dZ[r * HS + c];
    CS[(0 * MT + r) * SCW + cc] = gg * x;
    CS[(1 * MT + r) * SCW + cc] = gg;
    CS[(2 * MT + r) * SCW + cc] = dz;
    if (rowok) dZrow[c] = dz;
  }
  __syncthreads();
  if (t < CW) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int rr = 0; rr < MT; rr++) {
      t0 += CS[(0 * MT + rr) * SCW + t];
      t1 += CS[(1 * MT + rr) * SCW + t];
      t2 += CS[(2 * MT + rr) * SCW + t];
    }
    const int c = sp * CW + t;
    pog[c] = t0;
    pobe[c] = t1;
    pob[c] = t2;
  }
}

#ifdef MLP_TIMING
#define SPL_STAMP(i)                                                      \
  do {                                                                    \
    __syncthreads();                                                      \
    if (tile == 0 && sp == 0 && threadIdx.x == 0) g_tstamp[ni][i] = clock64(); \
  } while (0)
#else
#define SPL_STAMP(i) \
  do {               \
  } while (0)
#endif

// a hidden layer's constants, read from the kernel arguments before the first global store
struct HLayer {
  const float *W, *b, *g, *be;
  float* dZ;
  float p;
  int out, ob, og, obe;
};
__device__ __forceinline__ HLayer hlayer(const Layer& L) {
  return HLayer{L.W, L.b, L.g, L.be, L.dZ, L.p, L.out, L.ob, L.og, L.obe};
}

// the width dispatch of the whole-row work and the exchanges (hidden widths 128 or 256)
#define SPL_W(N, call) \
  do {                 \
    if ((N) == 256) {  \
      constexpr int NM = 16; \
      call;            \
    } else {           \
      constexpr int NM = 8; \
      call;            \
    }                  \
  } while (0)

// ---------------------------------------------------------------- the split rows kernel
__global__ void __launch_bounds__(ST) mlp_split_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) float slds[];
  const int bx = blockIdx.x & 7, by = blockIdx.x >> 3;
  const int sp = by % NSPL, grp = bx + 8 * (by / NSPL);
  const int B = a.B;
  const int ntiles = (B + MT - 1) / MT;
  if (grp >= 2 * ntiles) return;  // (the grid is a multiple of 32 workgroups)
  const int tile = grp >> 1, ni = grp & 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int r0 = tile * MT;
  const int sdim = a.sdim, adim = a.adim;
  const int KS = ((sdim + 15) & ~15) + 4;
  const float eps = a.eps;
  float* part = a.part + (size_t)tile * a.total;
  float* stat = part + a.ostat;
  float* S_l = slds;
  float* XH = S_l + MT * KS;
  float* Yb = XH + 3 * MT * HS;
  float* Zf = Yb + MT * HS;
  float* dYf = Zf + MT * HS;
  float* Ob = dYf + MT * HS;
  float* RS = Ob + MT * 64;
  uint16_t* RM = reinterpret_cast<uint16_t*>(RS + 3 * MT);
  uint16_t* DM = RM + 3 * 256;
  float* red = RS + 3 * MT + 2 * 3 * 256 / 2;
  int64_t* srow = reinterpret_cast<int64_t*>(red + 64);
  float* LNP = red + 64 + 2 * MT;
  const uint64_t seed = a.seed;
  const uint64_t step = *a.step + (a.idx ? 1 : 0);
  gu32* gen_word = (gu32*)a.cnt + grp;
  const Hand H{(gu64*)a.hand + (size_t)grp * NHAND * NSPL * MT * SCW, (gu32*)a.err,
               __hip_atomic_load(gen_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), sp, a.spin_ticks, a.fault};
  bool dead = false;
  const HLayer L0 = hlayer(a.net[ni].L[0]), L1 = hlayer(a.net[ni].L[1]), L2 = hlayer(a.net[ni].L[2]);
  const float* OW = a.net[ni].L[3].W;
  const float* Obias = a.net[ni].L[3].b;
  float* OdZ = a.net[ni].L[3].dZ;
  float* X1 = a.net[ni].L[1].X;
  float* X2 = a.net[ni].L[2].X;
  float* X3 = a.net[ni].L[3].X;
  const int NO = a.net[ni].L[3].out, Oob = a.net[ni].L[3].ob;
  const int head = a.net[ni].head, ols = a.net[ni].ols;
  const int N0 = L0.out, N1 = L1.out, N2 = L2.out;
  const int cw0 = N0 / NSPL, cw1 = N1 / NSPL, cw2 = N2 / NSPL;
  SPL_STAMP(0);

  // Loads are issued in the order they are needed, each batch right after an exchange (an
  // exchange's wait is an in-order vmcnt wait: everything issued before its granule loads
  // lands first), so that a batch has the row work, a GEMM and the next exchange to land in.
  const bool on0 = 16 * wave < cw0, on1 = 16 * wave < cw1, on2 = 16 * wave < cw2;
  const int n0 = sp * cw0 + 16 * wave + i, n1 = sp * cw1 + 16 * wave + i, n2 = sp * cw2 + 16 * wave + i;
  const bool onO = 16 * wave < NO;
  if (tid < MT) srow[tid] = r0 + tid >= B ? -1 : a.idx ? a.idx[r0 + tid] : r0 + tid;
  __syncthreads();
  SPL_STAMP(30);
  const int rr_ = tid >> 4, jr = tid & 15;  // the row / column phase of the thread's whole-row work
  const bool rowok = r0 + rr_ < B;
  // the tile's state rows (16 threads per row on 16 consecutive floats, unconditional loads at
  // clamped addresses), the three LayerNorms' gamma / beta (for LDS), the biases and layer 0's
  // weights: 62 loads, under the 63 a wave's vmcnt counts (more would make the wait for the
  // rows a wait for everything); layer 1's weights behind the LDS writes (compiler barriers
  // keep the order)
  constexpr int SG = (SPLIT_MAX_SDIM + 4 + 15) / 16;
  const int64_t sr = srow[rr_];
  float xv[SG], lnv[6];
  {
    const float* srcrow = a.S + (size_t)(sr < 0 ? 0 : sr) * sdim;
#pragma unroll
    for (int u = 0; u < SG; u++) xv[u] = srcrow[min(jr + 16 * u, sdim - 1)];
    const float* lsrc[6] = {L0.g, L0.be, L1.g, L1.be, L2.g, L2.be};
    const int lw[3] = {N0, N1, N2};
#pragma unroll
    for (int k = 0; k < 6; k++) lnv[k] = lsrc[k][min(tid, lw[k / 2] - 1)];
  }
  // (unconditional loads at clamped indices: a load under a branch blurs the compiler's in-order
  // wait counts after it)
  const float b0 = L0.b[min(n0, N0 - 1)], b1 = L1.b[min(n1, N1 - 1)], b2 = L2.b[min(n2, N2 - 1)];
  asm volatile("" ::: "memory");
  f4 wF0[SBF], wF1[SBH], wT0;
  ld_rows0(wF0, wT0, L0.W, N0, sdim, sp * cw0 + 16 * wave, lane);
#pragma unroll
  for (int u = 0; u < SG; u++) {
    const int k = jr + 16 * u;
    xv[u] = sr >= 0 && k < sdim ? xv[u] : 0.f;
    if (k < KS) S_l[rr_ * KS + k] = xv[u];
  }
#pragma unroll
  for (int k = 0; k < 6; k++) LNP[k * HMAX + tid] = lnv[k];
  asm volatile("" ::: "memory");
  ld_rows(wF1, L1.W, N1, N0, sp * cw1 + 16 * wave, lane);
  __syncthreads();
  SPL_STAMP(31);

  // ---------------- forward, layer 0
  if (on0) {
    f4 v = relu_keep(mm_rows<SBF, true>(wF0, wT0, S_l, KS, sdim, lane), b0, L0.p, seed, step, 0, r0 + 4 * q, n0);
#pragma unroll
    for (int r = 0; r < 4; r++) Zf[(4 * q + r) * HS + n0] = v[r];
    hand_put(H, 0, 16 * wave, v, lane);
  }
  if (a.Sg && ni == 0 && sp == 0 && sr >= 0) {  // the gathered state rows, for the weight gradient
    // (idx set only: prl_mlp_step passes no Sg, its weight gradient reads S itself)
    float* Sg = a.Sg + (size_t)(r0 + rr_) * sdim;
#pragma unroll
    for (int u = 0; u < SG; u++)
      if (jr + 16 * u < sdim) Sg[jr + 16 * u] = xv[u];
  }
  SPL_STAMP(21);
  SPL_W(N0, hand_get<NM * 4>(H, 0, Zf, HS, dead));
  SPL_STAMP(24);
  f4 wF2[SBH];
  ld_rows(wF2, L2.W, N2, N1, sp * cw2 + 16 * wave, lane);
  SPL_W(N0, ln_fwd<NM>(0, sp, rowok, eps, L0.p, LNP, Zf, Yb, XH, RS, RM, DM, X1 + (size_t)(r0 + rr_) * N0));
  __syncthreads();
  SPL_STAMP(1);

  // ---------------- forward, layer 1
  if (on1) {
    f4 v = relu_keep(mm_rows<SBH, false>(wF1, f4{}, Yb, HS, N0, lane), b1, L1.p, seed, step, 1, r0 + 4 * q, n1);
#pragma unroll
    for (int r = 0; r < 4; r++) Zf[(4 * q + r) * HS + n1] = v[r];
    hand_put(H, 1, 16 * wave, v, lane);
  }
  SPL_STAMP(22);
  SPL_W(N1, hand_get<NM * 4>(H, 1, Zf, HS, dead));
  SPL_STAMP(25);
  // the heads' per-row inputs (actor: wave w takes rows w + 4k, lane = action dimension)
  // (both networks load both heads' inputs: unconditional loads keep the compiler's wait
  // counts exact; the actor's log_std stands in for the critic's, which has none)
  float hact[MT / SWV], hlp[MT / SWV], hadv[MT / SWV];
#pragma unroll
  for (int k = 0; k < MT / SWV; k++) {
    const int rr = wave + SWV * k;
    const int64_t srk = r0 + rr < B ? srow[rr] : 0;
    hact[k] = a.A[(size_t)srk * adim + min(lane, adim - 1)];
    hlp[k] = a.LP[srk];
    hadv[k] = a.ADV[srk];
  }
  const float ob_l = Obias[min(lane, NO - 1)];
  const float lsr = a.net[0].log_std[min(lane, a.net[0].L[3].out - 1)];
  const float hret = a.RET[tid < MT && r0 + tid < B ? srow[tid] : 0];  // (thread r < 16: row r)
  f4 wFO[SBH];
  ld_rows(wFO, OW, NO, N2, 16 * wave, lane);
  SPL_W(N1, ln_fwd<NM>(1, sp, rowok, eps, L1.p, LNP, Zf, Yb, XH, RS, RM, DM, X2 + (size_t)(r0 + rr_) * N1));
  __syncthreads();
  SPL_STAMP(2);

  // ---------------- forward, layer 2
  if (on2) {
    f4 v = relu_keep(mm_rows<SBH, false>(wF2, f4{}, Yb, HS, N1, lane), b2, L2.p, seed, step, 2, r0 + 4 * q, n2);
#pragma unroll
    for (int r = 0; r < 4; r++) Zf[(4 * q + r) * HS + n2] = v[r];
    hand_put(H, 2, 16 * wave, v, lane);
  }
  SPL_STAMP(23);
  SPL_W(N2, hand_get<NM * 4>(H, 2, Zf, HS, dead));
  SPL_STAMP(26);
  f4 wBO[4], wB2[SBH];
  ld_cols(wBO, OW, NO, N2, sp * cw2 + 16 * wave, lane);
  ld_cols(wB2, L2.W, N2, N1, sp * cw1 + 16 * wave, lane);
  SPL_W(N2, ln_fwd<NM>(2, sp, rowok, eps, L2.p, LNP, Zf, Yb, XH, RS, RM, DM, X3 + (size_t)(r0 + rr_) * N2));
  __syncthreads();
  SPL_STAMP(3);

  // ---------------- output layer + head (every member; member 0 writes the rows out)
  if (onO) {
    const f4 v = mm_rows<SBH, false>(wFO, f4{}, Yb, HS, N2, lane);
#pragma unroll
    for (int r = 0; r < 4; r++) Ob[(4 * q + r) * 64 + 16 * wave + i] = v[r];
  }
  __syncthreads();
  SPL_STAMP(4);
  const float clip = a.clip, entc = a.ent;
  if (head == 0) {
    // actor_head_kernel, rows w + 4k of wave w: the per-action constants and the entropy
    // (the same for every row) once, then the four rows' log-probabilities reduced together
    const bool act_on = lane < NO;
    const bool inr = lsr >= -20.f && lsr <= 2.f;
    const float ls = act_on ? fminf(fmaxf(lsr, -20.f), 2.f) : 0.f;
    const float sd = act_on ? expf(ls) : 1.f;
    const float iv = 1.f / (sd * sd), i2 = 1.f / (2.f * sd * sd);
    float ent = act_on ? 0.5f + 0.91893853f + ls : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ent += __shfl_xor(ent, off, 64);
    ent /= (float)NO;
    float mu[MT / SWV], lp[MT / SWV];
#pragma unroll
    for (int k = 0; k < MT / SWV; k++) {
      const int rr = wave + SWV * k;
      mu[k] = act_on ? tanhf(Ob[rr * 64 + lane] + ob_l) : 0.f;
      const float dx = hact[k] - mu[k];
      lp[k] = act_on ? -(dx * dx) * i2 - ls - 0.91893853f : 0.f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < MT / SWV; k++) lp[k] += __shfl_xor(lp[k], off, 64);
#pragma unroll
    for (int k = 0; k < MT / SWV; k++) {
      const int rr = wave + SWV * k, r = r0 + rr;
      float g_out = 0.f, dls = 0.f, arow = 0.f, e = 0.f, adv = 0.f;
      if (r < B) {
        const float ratio = expf(lp[k] - hlp[k]);
        const float A_ = hadv[k];
        const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
        const float s1 = ratio * A_, s2 = rc * A_;
        const float w1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
        const float w2 = 1.f - w1;
        const float inclip = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? 1.f : 0.f;
        const float gr = -(w1 * A_ + w2 * A_ * inclip) / (float)B;
        const float gl = gr * ratio;
        if (act_on) {
          const float dx = hact[k] - mu[k];
          g_out = gl * dx * iv * (1.f - mu[k] * mu[k]);
          dls = inr ? gl * (dx * dx * iv - 1.f) - entc / ((float)NO * (float)B) : 0.f;
        }
        arow = -fminf(s1, s2) - entc * ent;
        e = ent;
        adv = A_;
      }
      Ob[rr * 64 + lane] = act_on ? g_out : 0.f;  // Z -> dZ of the output layer
      dYf[rr * HS + lane] = dls;                  // per-row log_std terms (dY is free here)
      if (lane == 0) {
        red[rr * 3] = arow;
        red[rr * 3 + 1] = e;
        red[rr * 3 + 2] = adv;
      }
    }
    __syncthreads();
    if (sp == 0) {
      if (tid < NO) {
        float t = 0.f;
        for (int w = 0; w < MT; w++) t += dYf[w * HS + tid];
        part[ols + tid] = t;
      }
      if (tid == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int w = 0; w < MT; w++) { s0 += red[w * 3]; s1 += red[w * 3 + 1]; s2 += red[w * 3 + 2]; }
        stat[0] = s0;  // actor loss rows
        stat[2] = s1;  // entropy
        stat[5] = s2;  // advantage
      }
    }
  } else {
    // critic_head_kernel: v = z + c, (v - ret)^2, d loss / d z = 2 (v - ret) / B
    if (tid < MT) {
      const int r = r0 + tid;
      float g_out = 0.f, sq = 0.f, v = 0.f, ret = 0.f;
      if (r < B) {
        v = Ob[tid * 64] + ob_l;
        ret = hret;
        const float e = v - ret;
        g_out = 2.f * e / (float)B;
        sq = e * e;
      }
      Ob[tid * 64] = g_out;
      for (int c = 1; c < 64; c++) Ob[tid * 64 + c] = 0.f;
      red[tid * 3] = sq;
      red[tid * 3 + 1] = v;
      red[tid * 3 + 2] = ret;
    }
    __syncthreads();
    if (sp == 0 && tid == 0) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < MT; r++) { s0 += red[r * 3]; s1 += red[r * 3 + 1]; s2 += red[r * 3 + 2]; }
      stat[1] = s0;  // critic loss rows
      stat[3] = s1;  // value
      stat[4] = s2;  // return
    }
  }
  __syncthreads();
  SPL_STAMP(5);

  // ---------------- backward: dY of layer 2 (and member 0: the output layer's dZ rows, bias sums)
  if (on2) {
    const f4 v = mm_cols(wBO, Ob, 64, NO, lane);
#pragma unroll
    for (int r = 0; r < 4; r++) dYf[(4 * q + r) * HS + n2] = v[r];
    hand_put(H, 3, 16 * wave, v, lane);
  }
  if (sp == 0) {
    for (int j = tid; j < MT * NO; j += ST) {
      const int r = j / NO, c = j - r * NO;
      if (r0 + r < B) OdZ[(size_t)(r0 + r) * NO + c] = Ob[r * 64 + c];
    }
    if (tid < NO) {
      float t = 0.f;
      for (int r = 0; r < MT; r++) t += Ob[r * 64 + tid];
      part[Oob + tid] = t;
    }
  }
  SPL_STAMP(7);
  SPL_W(N2, hand_get<NM * 4>(H, 3, dYf, HS, dead));
  SPL_STAMP(27);
  f4 wB1[SBH];
  ld_cols(wB1, L1.W, N1, N0, sp * cw0 + 16 * wave, lane);
  SPL_W(N2, ln_bwd<NM>(2, sp, rowok, L2.p, LNP, dYf, Yb, XH, RS, RM, DM, Zf, L2.dZ + (size_t)(r0 + rr_) * N2,
                       part + L2.og, part + L2.obe, part + L2.ob));
  __syncthreads();
  SPL_STAMP(8);

  // ---------------- backward: layer 2's dX = dY of layer 1
  if (on1) {
    const f4 v = mm_cols(wB2, Yb, HS, N2, lane);
#pragma unroll
    for (int r = 0; r < 4; r++) dYf[(4 * q + r) * HS + n1] = v[r];
    hand_put(H, 4, 16 * wave, v, lane);
  }
  SPL_STAMP(11);
  SPL_W(N1, hand_get<NM * 4>(H, 4, dYf, HS, dead));
  SPL_STAMP(28);
  SPL_W(N1, ln_bwd<NM>(1, sp, rowok, L1.p, LNP, dYf, Yb, XH, RS, RM, DM, Zf, L1.dZ + (size_t)(r0 + rr_) * N1,
                       part + L1.og, part + L1.obe, part + L1.ob));
  __syncthreads();
  SPL_STAMP(12);

  // ---------------- backward: layer 1's dX = dY of layer 0
  if (on0) {
    const f4 v = mm_cols(wB1, Yb, HS, N1, lane);
#pragma unroll
    for (int r = 0; r < 4; r++) dYf[(4 * q + r) * HS + n0] = v[r];
    hand_put(H, 5, 16 * wave, v, lane);
  }
  SPL_STAMP(15);
  SPL_W(N0, hand_get<NM * 4>(H, 5, dYf, HS, dead));
  // every member has read the call count (its exchange-5 granules carry it): advance it
  if (sp == 0 && tid == 0) __hip_atomic_store(gen_word, H.gen + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  SPL_STAMP(29);
  SPL_W(N0, ln_bwd<NM>(0, sp, rowok, L0.p, LNP, dYf, Yb, XH, RS, RM, DM, Zf, L0.dZ + (size_t)(r0 + rr_) * N0,
                       part + L0.og, part + L0.obe, part + L0.ob));
  SPL_STAMP(16);
  SPL_STAMP(20);
}

}  // namespace mlp
