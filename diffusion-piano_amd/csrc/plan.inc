// plan.inc - the kernels of the predictive-sampling planner (prl_plan_*, include/pianorl.h;
// driven by planning.py). Included at the end of pianorl.hip, at file scope.
//
// Candidates are N = G * C envs: group g owns envs [g C, (g + 1) C), candidate c of it is env
// g C + c. A plan is P knots of A actions over H control steps; knot p sits at step
// p (H - 1) / (P - 1) (P = 1: one knot at step 0). Time is kept in integers: step t is
// t (P - 1) / (H - 1) in knot units, the quotient the knot at or before it, the remainder over
// H - 1 the fraction towards the next one.
namespace {

// the plan `k` [P][A] of one candidate, column a, at knot-unit time num / den (den = H - 1; not
// read when P = 1). Past the last knot the last knot is held. Zero-order: the knot at or before
// the time. Linear: exactly that knot at a knot time, otherwise k0 + f (k1 - k0) with f = rem / den
// rounded once, k1 - k0 rounded once and one fused multiply-add: three roundings, then kept inside
// [min(k0, k1), max(k0, k1)] (a rounding at the far end cannot leave the action bounds).
__device__ __forceinline__ float plan_eval(const float* __restrict__ k, int P, int A, int a, int num, int den,
                                           int linear) {
  if (P == 1) return k[a];
  const int j = num / den, rem = num - j * den;
  if (j >= P - 1) return k[(size_t)(P - 1) * A + a];
  const float k0 = k[(size_t)j * A + a];
  if (!linear || rem == 0) return k0;
  const float k1 = k[(size_t)(j + 1) * A + a];
  const float f = __fdiv_rn((float)rem, (float)den);
  const float v = __fmaf_rn(f, __fsub_rn(k1, k0), k0);
  return fminf(fmaxf(v, fminf(k0, k1)), fmaxf(k0, k1));
}

// one thread per knot entry: knots[n][p][a] = clamp(nominal[g][p][a] + sigma[a] z, lo[a], hi[a]),
// z the draw of gauss_sample_kernel at column p A + a, row n (candidate 0 of a group: z = 0)
__global__ void __launch_bounds__(256) plan_perturb_kernel(const float* __restrict__ nominal,
                                                           const float* __restrict__ sigma,
                                                           const float* __restrict__ lo, const float* __restrict__ hi,
                                                           int C, int PA, int A, size_t total, uint64_t seed,
                                                           uint64_t offset, float* __restrict__ knots) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / (size_t)PA;
  const int col = (int)(i - n * (size_t)PA), a = col % A;
  const size_t g = n / (size_t)C;
  float x = nominal[g * (size_t)PA + col];
  if (n != g * (size_t)C) {
    uint32_t c[4] = {(uint32_t)col, (uint32_t)n, (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)c[0] + 1.f) * 2.3283064e-10f;  // (0, 1]
    const float u2 = (float)c[1] * 2.3283064e-10f;
    const float z = sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2);
    x = x + sigma[a] * z;
  }
  knots[i] = fminf(fmaxf(x, lo[a]), hi[a]);
}

// one thread per action entry: action[n][a] = the plan of candidate n at step h
__global__ void __launch_bounds__(256) plan_action_kernel(const float* __restrict__ knots, size_t total, int P, int A,
                                                          int H, int h, int linear, float* __restrict__ action) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / (size_t)A;
  const int a = (int)(i - n * (size_t)A);
  action[i] = plan_eval(knots + n * (size_t)P * A, P, A, a, h * (P - 1), H - 1, linear);
}

// ret += w reward; w *= gamma discount; w = 0 from a LAST step on: the rewards of the episode that
// the auto-reset starts after it (its FIRST step's among them) are not added at all - a candidate
// whose weight is 0 adds nothing, whatever the reward holds. init: ret = 0, w = 1 first.
__global__ void __launch_bounds__(256) plan_accumulate_kernel(const float* __restrict__ reward,
                                                              const float* __restrict__ discount,
                                                              const uint8_t* __restrict__ step_type, int n, float gamma,
                                                              int init, float* __restrict__ ret,
                                                              float* __restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r = init ? 0.f : ret[i], wi = init ? 1.f : w[i];
  if (wi != 0.f) r = __fmaf_rn(wi, reward[i], r);
  wi = step_type[i] == PRL_STEP_LAST ? 0.f : __fmul_rn(wi, __fmul_rn(gamma, discount[i]));
  ret[i] = r;
  w[i] = wi;
}

// is candidate (v, i) a better choice than (u, j)? A NaN never beats a number; equal returns (and
// two NaNs) go to the lower index
__device__ __forceinline__ bool plan_better(float v, int i, float u, int j) {
  const bool vn = v != v, un = u != u;
  if (vn || un) return vn == un ? i < j : un;
  return v > u || (v == u && i < j);
}

constexpr int SELECT_THREADS = 1024;
// one workgroup per group: a strided pass over its C returns (64 per thread at C = 65536), a
// shuffle reduction in each wave, the 16 wave winners through LDS. Then the whole workgroup copies
// the winner's plan.
__global__ void __launch_bounds__(SELECT_THREADS) plan_select_kernel(const float* __restrict__ ret,
                                                                     const float* __restrict__ knots, int C, int P,
                                                                     int A, int H, int linear, int shift,
                                                                     int* __restrict__ best, float* __restrict__ best_ret,
                                                                     float* __restrict__ nominal_out,
                                                                     float* __restrict__ chosen) {
  __shared__ float sv[SELECT_THREADS / 64];
  __shared__ int si[SELECT_THREADS / 64];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* r = ret + (size_t)g * C;
  float v = __builtin_nanf("");
  int idx = 0x7fffffff;
  for (int c = tid; c < C; c += SELECT_THREADS) {
    const float u = r[c];
    if (plan_better(u, c, v, idx)) { v = u; idx = c; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float u = __shfl_down(v, off, 64);
    const int j = __shfl_down(idx, off, 64);
    if (plan_better(u, j, v, idx)) { v = u; idx = j; }
  }
  if (lane == 0) { sv[wave] = v; si[wave] = idx; }
  __syncthreads();
  if (wave == 0) {
    const bool has = lane < SELECT_THREADS / 64;
    v = has ? sv[lane] : __builtin_nanf("");
    idx = has ? si[lane] : 0x7fffffff;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const float u = __shfl_down(v, off, 64);
      const int j = __shfl_down(idx, off, 64);
      if (plan_better(u, j, v, idx)) { v = u; idx = j; }
    }
    if (lane == 0) {
      if (v != v) idx = 0;  // every return is NaN: the unperturbed plan
      si[0] = idx;
      best[g] = idx;
      best_ret[g] = r[idx];
    }
  }
  __syncthreads();
  const int win = si[0];
  const float* k = knots + ((size_t)g * C + win) * (size_t)P * A;
  const int PA = P * A;
  for (int i = tid; i < PA; i += SELECT_THREADS) {
    const int p = i / A, a = i - p * A;
    // shift: knot p of the new nominal is the winner's plan one control step after knot p's time
    nominal_out[(size_t)g * PA + i] = shift ? plan_eval(k, P, A, a, p * (H - 1) + (P - 1), H - 1, linear) : k[i];
  }
  for (int a = tid; a < A; a += SELECT_THREADS) chosen[(size_t)g * A + a] = k[a];
}

int plan_dims(const char* what, int G, int C, int P, int A, int H) {
  if (G <= 0 || C <= 0 || P <= 0 || A <= 0 || H <= 0)
    return fail(std::string(what) + ": groups, candidates, knots, actions and horizon must be positive");
  if (P > H) return fail(std::string(what) + ": more knots than horizon steps");
  if ((int64_t)G * C > 0x7fffffff || (int64_t)P * A > (1 << 20) || (int64_t)H * P > 0x7fffffff ||
      (int64_t)G * C * P * A > ((int64_t)1 << 38))
    return fail(std::string(what) + ": sizes out of range");
  return 0;
}

}  // namespace

extern "C" {

int prl_plan_perturb(const float* nominal, const float* sigma, const float* lo, const float* hi, int G, int C, int P,
                     int A, uint64_t seed, uint64_t offset, float* knots, void* stream) {
  if (!nominal || !sigma || !lo || !hi || !knots) return fail("prl_plan_perturb: null pointer");
  if (plan_dims("prl_plan_perturb", G, C, P, A, P)) return -1;
  const size_t total = (size_t)G * C * P * A;
  plan_perturb_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(nominal, sigma, lo, hi, C, P * A,
                                                                                       A, total, seed, offset, knots);
  HIPCHK(hipGetLastError());
  return 0;
}

int prl_plan_action(const float* knots, int N, int P, int A, int H, int h, int interpolation, float* action,
                    void* stream) {
  if (!knots || !action) return fail("prl_plan_action: null pointer");
  if (plan_dims("prl_plan_action", 1, N, P, A, H)) return -1;
  if (h < 0 || h >= H) return fail("prl_plan_action: step outside the horizon");
  if (interpolation != PRL_PLAN_ZERO && interpolation != PRL_PLAN_LINEAR)
    return fail("prl_plan_action: interpolation is PRL_PLAN_ZERO or PRL_PLAN_LINEAR");
  const size_t total = (size_t)N * A;
  plan_action_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(knots, total, P, A, H, h,
                                                                                      interpolation, action);
  HIPCHK(hipGetLastError());
  return 0;
}

int prl_plan_accumulate(const float* reward, const float* discount, const uint8_t* step_type, int N, float gamma,
                        int init, float* ret, float* w, void* stream) {
  if (!reward || !discount || !step_type || !ret || !w) return fail("prl_plan_accumulate: null pointer");
  if (N <= 0) return fail("prl_plan_accumulate: N must be positive");
  plan_accumulate_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>(reward, discount, step_type, N, gamma, init,
                                                                          ret, w);
  HIPCHK(hipGetLastError());
  return 0;
}

int prl_plan_select(const float* ret, const float* knots, int G, int C, int P, int A, int H, int interpolation,
                    int shift, int32_t* best, float* best_ret, float* nominal_out, float* chosen, void* stream) {
  if (!ret || !knots || !best || !best_ret || !nominal_out || !chosen) return fail("prl_plan_select: null pointer");
  if (plan_dims("prl_plan_select", G, C, P, A, H)) return -1;
  if (interpolation != PRL_PLAN_ZERO && interpolation != PRL_PLAN_LINEAR)
    return fail("prl_plan_select: interpolation is PRL_PLAN_ZERO or PRL_PLAN_LINEAR");
  plan_select_kernel<<<G, SELECT_THREADS, 0, (hipStream_t)stream>>>(ret, knots, C, P, A, H, interpolation, shift ? 1 : 0,
                                                                    best, best_ret, nominal_out, chosen);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
