// kernel_v2.inc - the batched step kernel (included by pianosim.hip).
//
// One 64-lane wavefront (= one workgroup) per environment, the whole control step in one
// launch. Every lane OWNS objects of the env and keeps them in registers:
//   lane l < 52 : hand dof l   (q, v, forces, its row of the tree LDL of M and M + hD)
//   lane l < 50 : hand body l  (R, o, world inertia, velocities)
//   lane l < 40 : capsule l    (endpoints)
//   lane l      : piano keys l and l + 64 (q, v, forces)
// LDS holds only what lanes exchange: parent/child body data per tree level, the
// broadcast LDL row, solve vectors, contacts and the dense constraint rows. The static
// model data a lane needs is loaded once per launch into registers, so no phase walks a
// chain of dependent global loads.

#ifdef PS_TIMING
#define NPHASE 56
enum : int { TS_FINAL = 52, TS_FINAL_SKIP = 53 };  // counters: env-steps, and those without the final collide pass
// counters: box / hull narrow-phase rounds with both an MPR and a capsule-box / box-box pair; without a touching pair
enum : int { TS_XMIXED = 54, TS_XNOHIT = 55 };
#define TARG , uint64_t *tacc, uint64_t &tlast
#define TPASS , tacc, tlast
#define TSTAMP(slot)                                     \
  do {                                                   \
    __syncthreads();                                     \
    uint64_t t_ = __builtin_amdgcn_s_memtime();         \
    tacc[slot] += t_ - tlast;                            \
    tlast = t_;                                          \
  } while (0)
__device__ uint64_t* g_timing = nullptr;
#else
#define TSTAMP(slot) \
  do {               \
  } while (0)
#define TARG
#define TPASS
#endif

#ifdef PS_CHECK_A
__device__ int g_dbg_count = 0;  // (debug build: MFMA vs scalar Delassus mismatches printed)
#endif
// body exchange record (one per hand body, one substep): the top-down pass writes R, o and
// the RNE forward terms w, al, ac; the bottom-up pass folds the composite inertia CP (over
// the dead R) and the RNE force/torque F, N
enum : int { BX_R = 0, BX_CP = 0, BX_O = 10, BX_W = 13, BX_AL = 16, BX_AC = 19, BX_F = 22, BX_N = 25, BXS = 28 };
static_assert(NKB == 64, "collide2 stages one key-range bucket per lane");
constexpr int FROW = 2 * MAXDEP + 2;
__device__ __forceinline__ int tri(int r, int s) { return s * (s + 1) / 2 + r; }  // A(r,s), r <= s

constexpr int NSL = 28;  // Newton slot registers per hand group (26 used; slot lanes stay 32g + s)
// Newton scratch in LDS (the phase-2 union area, Shared::nw; dead across factor2, which the
// Md staging precedes)
struct NewtonLDS {
  union {
    struct {
      float Jc[3 * MAXCON][YS];           // contact direction rows n, t1, t2 (compressed: r_mask slots, YKEY)
      float P[68];                        // pivot row(s) (+ the diagonal, [64])
      float Bd[3][64];                    // staging of one contact's direction rows by slot; the factor's second pivot row
      float vx[64];                       // a slot vector by slot (x - x_s, the direction)
      float xd[NDT + 1];                  // a hand vector by dof (x, the direction) for the contact dots
      float kx[NK], kg[NK];               // keys: x (or direction), gradient partial sums
      uint64_t cmask[MAXCON];             // contact support masks (hand dofs)
      int ckey[MAXCON];
      float red[4];
    };
  };
};
// ... and what lives from newton_prep (before factor2) to the end of the solve
struct NewtonMap {
  int slot_dof[64];                       // slot lane -> hand dof (-1: none)
  int dof_slot[NDT];                      // hand dof -> slot lane
  int nc[2];                              // C dofs per hand (slots 0..nc-1)
  uint32_t cm[4];                         // C mask (lo, hi)
  int khand[NK];                          // keys: bit h = touched by hand h this substep
};

struct Shared {
  // Phase-exclusive storage (one substep: kinematics -> dynamics -> collide | Newton prep ->
  // factor -> Newton solve -> integrate). bx/cap die at the end of collide2; the Newton prep's
  // dense M staging dies before factor2 (whose fstage / Lr are dead after it), the Newton
  // scratch lives from the contact rows to the end of the solve. Keeps the workgroup under
  // 20 KB of LDS = 8 resident waves per CU.
  union {
    struct {
      float bx[NBT][BXS];   // per-body exchange, layout BX_* below
      float cap[NGT][8];    // capsules (world): p0, p1, radius, half-length
      float xg[NXT][12];    // extra colliders (world): centre, rotation (row-major)
      alignas(16) float kg[NK][KGEO];  // collide2: per-key collision records (DevModel::key_geo)
      uint8_t kb[2][NKB];   // collide2: key-range buckets (DevModel::kb_first, kb_end)
    };
    struct {
      union {
        struct {
          float fstage[NDT + 1][FROW];  // factor2: pivot rows of a level (M row, Mh row, 1/D, 1/Dh); +1: fold read overrun
          float Lr[NDT][MAXDEP];        // factor2: factored rows of M: [0] = D, [a] = L(k, anc_a)
        };
        NewtonLDS nw;       // Newton scratch (newton.inc), from the contact rows on
      };
      float Mp[NH][ND * (ND + 1) / 2];  // Newton prep -> end of the solve: M per hand, packed by slot (upper)
      NewtonMap nm;
    };
  };
  float dx[NDT][8];         // per-dof: world axis(3), body origin(3), q
  float dinv[NDT];          // 1 / D of the factor of M
  int anc[NDT][2];          // packed ancestors (bytes) of every dof
  int8_t depth[NDT];
  int8_t dtype[NDT];
  float x[NDT], x2[NDT];
  float kc[NK], ks[NK], knorm[NK], kw[NK], kminv[NK];
  int ncon;
  Contact con[MAXCON];
  int keyhit[3];
  int act_bits[3];
  float sustain;
};

struct Song {
  int T;
  const float* goal;
  const int* count;
  const int* keys;
  const int* fingers;
  // per-episode MIDI augmentations (augment.inc): env e has rows [e * stride, e * stride + T_env[e])
  // of the four tables, rebuilt by song_build_kernel before its episode. A plain handle: stride 0,
  // T_env null, every env reads the one song above.
  int stride;
  const int* T_env;
};
// env e's song (wave-uniform)
__device__ __forceinline__ Song song_of(const Song& s, const int e) {
  if (!s.T_env) return s;
  const size_t row = (size_t)e * (size_t)s.stride;
  return Song{s.T_env[e], s.goal + row * (NK + 1), s.count + row, s.keys + row * PS_MAX_NOTES,
              s.fingers + row * PS_MAX_NOTES, s.stride, s.T_env};
}

struct Cfg {
  int lookahead, fingering, forearm, wrong_press, newton_cap, maxcon, obs_dim, canonical;
  int obs_base;   // the default part of the row (write_obs2); obs_dim - obs_base extras follow (write_obs_extras)
  float energy_coef;
  int randomize;  // randomize_hand_positions: per-episode y shift of the hand roots
  uint32_t seed_lo, seed_hi;
  uint32_t env0;  // global id of this handle's env 0 (ps_set_env_offset): Philox draws keyed by global env
  int full_cpl;   // test hook (PIANOSIM_DEBUG_FULL_COUPLED): coupled substeps take the 28-column C block
  int refine;     // ps_task_cfg.solver_refine: 0 none, 1 a refining Newton step on coupled substeps, 2 all
  int hand;       // ps_task_cfg.hand_side: 0 both hands; 1 right / 2 left only (the one-hand task layer)
};

struct Bufs {
  float *qpos, *qvel, *qws, *ctrl, *sustain;
  int* t_idx;
  uint8_t* last;
  const float* applied;  // may be null
  float* terms;
  float* tips;
  int* ncon;
  float *mus_acc, *mus_ep;
  int* mus_cnt;
  float* hand_dy;  // this episode's y shift of both hand roots (randomize_hand_positions)
  int* episode;    // resets so far (the draw counter of hand_dy)
  int* stats;      // [N][PS_NSTATS] solver / cap counters of the last step
  Contact* con_out;  // [N][MAXCON] contacts of the last step (ps_record_contacts), or null
  int* warnings;     // [N][PS_NWARN] mj_checkPos / Vel / Acc resets since create
  float* park;       // [N][PARK_WORDS][64] lane state parked around the Newton solve
  uint32_t* keybits; // [N][KB_HDR + nsub * KB_ROW] the MIDI recorder's capture (ps_record_midi), or null
};
// The MIDI recorder's capture row of one env (midi_events.inc reads it after the launch): a header
// word - the number of valid substep rows of this launch, or KB_NEW_EPISODE with none - then one
// row per substep of the control step: the 88 key activations (key k = bit k & 31 of word k >> 5)
// and the sustain activation (bit KB_SUSTAIN_BIT of word 2) at the end of that substep.
constexpr int KB_HDR = 1, KB_ROW = 3, KB_SUSTAIN_BIT = 24;
constexpr uint32_t KB_NEW_EPISODE = 0x80000000u;
__device__ __forceinline__ size_t kb_stride(int nsub) { return (size_t)(KB_HDR + nsub * KB_ROW); }
// LaneDyn words that outlive the constraint solve but are not used by it (the factor of
// M + hD for the integration, the warm-start and key force terms): parked in the env's row of
// bufs.park (L2-resident while in use) so their registers are free during the solve
constexpr int PARK_SUB = 30;  // 17 around the solve, 7 more inside it (newton_solve); 30 around
                              // the box / hull collision (the XG kernel, before the solve)
// ... and, on the queue path (pianosim_queue_kernel), what is live across a substep boundary:
// written at the end of a chunk of substeps, read by the workgroup that runs the env's next one
enum : int {
  CW_Q = PARK_SUB, CW_V, CW_KQ, CW_KV = CW_KQ + 2, CW_CTRL = CW_KV + 2, CW_ACTF,
  CW_ZF, CW_ZL, CW_ZC, CW_CID, CW_ZK,  // the Newton guess (NGuess)
  CW_SCAL = CW_ZK + 2,                 // wave-uniform words, one per lane (CS_*)
  PARK_WORDS
};
enum : int { CS_SOLVES = 0, CS_CONCAP, CS_CAP, CS_MAXROW, CS_COUPLED, CS_PIV, CS_CDOFS, CS_WARN,
             CS_GVALID = CS_WARN + PS_NWARN, CS_NOAPPLIED, CS_COUNT };
static_assert(CS_COUNT <= 64, "one carried scalar per lane");
constexpr int PS_MAX_CHUNKS = 15;  // a queue item is env * 16 + chunk
// The carried words are handed from one workgroup to another inside a launch: write-through
// stores and L1-bypassing loads (global_store / global_load ... sc1), see pianosim_queue_kernel
__device__ __forceinline__ void st_wt(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_wt(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int anc_of(int p0, int p1, int a) {  // a in 1..8
  return (a <= 4 ? (p0 >> (8 * (a - 1))) : (p1 >> (8 * (a - 5)))) & 255;
}
// v_rcp_f32 (1 ulp) where the IEEE division sequence would sit on a serial chain
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float rdlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// key box frame (rotation about +y by q), from the LDS trig table
__device__ __forceinline__ void key_frame2(const DevModel* __restrict__ m, const Shared& S, int k, float* R, f3* centre,
                                           f3* anchor) {
  float c = S.kc[k], s = S.ks[k];
  R[0] = c; R[1] = 0; R[2] = s; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = -s; R[7] = 0; R[8] = c;
  f3 P = ld3(m->key_pos[k]), al = ld3(m->key_anchor[k]);
  f3 A = P + al;
  *anchor = A;
  *centre = A + mv3(R, al * -1.f);
}

// Candidate (capsule, key) pairs of one capsule: AABB overlap with the key's box record (key
// range from the bucket table) and with the piano base (key id BASEKEY), in canonical order.
// `emit` = nullptr counts only.
constexpr int BASEKEY = 255;
__device__ __forceinline__ int piano_candidates(const DevModel* __restrict__ m, const Shared& S, int c, float r,
                                                uint16_t* emit, int cap) {
  const f3 p0 = ld3(&S.cap[c][0]), p1 = ld3(&S.cap[c][3]);
  const float lo[3] = {fminf(p0.x, p1.x) - r, fminf(p0.y, p1.y) - r, fminf(p0.z, p1.z) - r};
  const float hi[3] = {fmaxf(p0.x, p1.x) + r, fmaxf(p0.y, p1.y) + r, fmaxf(p0.z, p1.z) + r};
  // conservative prefilter: above every key / outside the piano's x extent -> nothing
  if (lo[2] > m->key_top_zmax || hi[0] < m->piano_xmin || lo[0] > m->piano_xmax) return 0;
  // candidate keys: bucket table (conservative superset of the keys overlapping [lo, hi] in y)
  const int b0 = min(max((int)floorf((lo[1] - 1e-5f - m->kb_y0) * m->kb_inv), 0), NKB - 1);
  const int b1 = min(max((int)floorf((hi[1] + 1e-5f - m->kb_y0) * m->kb_inv), 0), NKB - 1);
  const int k0 = S.kb[0][b0], k1 = S.kb[1][b1];
  int n = 0;
  for (int k = k0; k < k1; k++) {
    const float* g = S.kg[k];
    if (lo[2] > g[13] || hi[0] < g[9] || lo[0] > g[10] || hi[1] < g[11] || lo[1] > g[12]) continue;
    if (emit && n < cap) emit[n] = (uint16_t)((c << 8) | k);
    n++;
  }
  const f3 bc = ld3(m->base_pos), bh = ld3(m->base_half);
  if (hi[0] < bc.x - bh.x || lo[0] > bc.x + bh.x || hi[1] < bc.y - bh.y || lo[1] > bc.y + bh.y ||
      hi[2] < bc.z - bh.z || lo[2] > bc.z + bh.z)
    return n;  // AABBs apart: no contact with the base
  if (emit && n < cap) emit[n] = (uint16_t)((c << 8) | BASEKEY);
  return n + 1;
}

// narrow phase of one candidate pair (capsule vs key box or base box); up to 2 contacts
template <int WPE>
__device__ __forceinline__ int piano_pair(const DevModel* __restrict__ m, const Shared& S, int pr, Contact* out,
                                          int slot, int maxc) {
  const int c = pr >> 8, k = pr & 255;
  const f3 p0 = ld3(&S.cap[c][0]), p1 = ld3(&S.cap[c][3]);
  const float r = S.cap[c][6];
  if (k == BASEKEY) return capsule_box<WPE>(p0, p1, r, ld3(m->base_pos), 1.f, 0.f, ld3(m->base_half), out, slot, maxc, 1, -1, c);
  const float* g = S.kg[k];
  const float cq = S.kc[k], sq = S.ks[k];
  const float R[9] = {cq, 0.f, sq, 0.f, 1.f, 0.f, -sq, 0.f, cq};
  const f3 al = ld3(g + 6), A = ld3(g) + al;
  const f3 centre = A + mv3(R, al * -1.f);
  return capsule_box<WPE>(p0, p1, r, centre, cq, sq, ld3(g + 3), out, slot, maxc, 0, k, c);
}

// ---- box / hull colliders (models with extra colliders only; oracle collide / extra_pair)
// candidate (extra, key|base) pairs of extra lane c: the bounding sphere's AABB against the
// key records and the base, in canonical order (emit = nullptr counts only)
__device__ __forceinline__ int xpiano_candidates(const DevModel* __restrict__ m, const Shared& S, int c, uint16_t* emit,
                                                 int cap) {
  const int e = c - NGT;
  const f3 ctr = ld3(S.xg[e]);
  const float rb = m->x_rb[e];
  const float lo[3] = {ctr.x - rb, ctr.y - rb, ctr.z - rb}, hi[3] = {ctr.x + rb, ctr.y + rb, ctr.z + rb};
  int n = 0;
  if (!(lo[2] > m->key_top_zmax || hi[0] < m->piano_xmin || lo[0] > m->piano_xmax)) {
    // the keys from the bucket table (piano_candidates), a superset of those meeting [lo, hi] in y
    const int b0 = min(max((int)floorf((lo[1] - 1e-5f - m->kb_y0) * m->kb_inv), 0), NKB - 1);
    const int b1 = min(max((int)floorf((hi[1] + 1e-5f - m->kb_y0) * m->kb_inv), 0), NKB - 1);
    const int k0 = S.kb[0][b0], k1 = S.kb[1][b1];
    for (int k = k0; k < k1; k++) {
      const float* g = S.kg[k];
      if (lo[2] > g[13] || hi[0] < g[9] || lo[0] > g[10] || hi[1] < g[11] || lo[1] > g[12]) continue;
      {  // the bounding sphere against the key's oriented box (x_pairs' key frame): a sphere
         // apart from the box holds a collider apart from it, so its narrow phase finds nothing
        const float cq = S.kc[k], sq = S.ks[k];
        const f3 al = ld3(g + 6), hs = ld3(g + 3);
        const f3 d = ctr - (ld3(g) + al);  // from the anchor; the centre is anchor - R al
        const f3 l = mk3(cq * d.x - sq * d.z + al.x, d.y + al.y, sq * d.x + cq * d.z + al.z);
        const f3 e = mk3(fmaxf(fabsf(l.x) - hs.x, 0.f), fmaxf(fabsf(l.y) - hs.y, 0.f), fmaxf(fabsf(l.z) - hs.z, 0.f));
        if (dot3(e, e) > rb * rb) continue;
      }
      if (emit && n < cap) emit[n] = (uint16_t)((c << 8) | k);
      n++;
    }
  }
  const f3 bc = ld3(m->base_pos), bh = ld3(m->base_half);
  if (hi[0] < bc.x - bh.x || lo[0] > bc.x + bh.x || hi[1] < bc.y - bh.y || lo[1] > bc.y + bh.y ||
      hi[2] < bc.z - bh.z || lo[2] > bc.z + bh.z)
    return n;
  if (emit && n < cap) emit[n] = (uint16_t)((c << 8) | BASEKEY);
  return n + 1;
}

// (m, S: the model and the workgroup's LDS through typed pointers, prims.h PS_GLB / PS_LDS - the
// callers are out of line, where a generic pointer's reads would be flat_loads)
__device__ __forceinline__ XShape coll_shape(const PS_GLB DevModel* m, const PS_LDS Shared* S, int g) {
  XShape s;
  s.cells = nullptr;
  s.cellv = nullptr;
  s.v0 = s.nv = 0;
  s.r = 0.f;
  s.er = 0.f;
  s.tie = 0.f;
  s.hs = mk3(0.f, 0.f, 0.f);
  if (g < NGT) {
    s.type = 0;
    s.p0 = ld3(&S->cap[g][0]);
    s.p1 = ld3(&S->cap[g][3]);
    s.r = S->cap[g][6];
    s.c = (s.p0 + s.p1) * 0.5f;
    s.e0 = s.e1 = s.c;
#pragma unroll
    for (int i = 0; i < 9; i++) s.R[i] = (i % 4 == 0) ? 1.f : 0.f;
  } else {
    const int e = g - NGT;
    s.type = m->x_type[e];
    s.c = ld3(S->xg[e]);
#pragma unroll
    for (int i = 0; i < 9; i++) s.R[i] = S->xg[e][3 + i];
    s.hs = ld3(m->x_hs[e]);
    s.v0 = m->x_v0[e];
    s.nv = m->x_nv[e];
    s.p0 = s.p1 = s.e0 = s.e1 = s.c;
    if (s.type == PS_GEOM_HULL) {
      s.cells = m->x_cell[e];
      s.cellv = m->x_cellv_ok[e] ? reinterpret_cast<const PS_GLB f4g*>(&m->x_cellv[e][0][0][0]) : nullptr;
      s.e0 = s.c + mv3(s.R, ld3(&m->x_ec[e][0]));
      s.e1 = s.c + mv3(s.R, ld3(&m->x_ec[e][3]));
      s.er = m->x_ec[e][6];
      s.tie = SUP_TIE_HULL * m->x_rb[e];
    }
  }
  return s;
}

// Narrow phase of one pair with a box / hull collider per lane (lanes with act == false test
// nothing). ga < 0: geom1 is key `key` (BASEKEY: the base), geom2 = extra gb (kind 0 / 1); else
// hand-hand pair ga < gb (kind 2). Normal geom1 -> geom2; capsule-box pairs take the box as
// geom1, the pair of lanes 2k and 2k + 1 (paired MPR: both lanes pass the same pair). The pairs'
// contacts (up to 4 per pair) are placed in pair order at out[base..] (below maxc) by a wave
// scan, in one pass: each pair's MPR / box-box / capsule-box runs once. Called by the whole wave
// (uniform control flow); returns the contacts of all pairs. Out of line: one
// copy of the narrow phases for the piano and the hand-hand call sites.
// The two colliders of a box / hull pair (x_pairs' argument meaning): geom1 A is the key / base
// box (ga < 0) or hand collider ga, geom2 B is hand collider gb.
__device__ __forceinline__ void x_pair_shapes(const PS_GLB DevModel* m, const PS_LDS Shared* S, int ga, int gb, int key,
                                              XShape& A, XShape& B, int& kind, int& ckey) {
  B = coll_shape(m, S, gb);
  kind = 2;
  ckey = -1;
  if (ga < 0) {
    A.type = PS_GEOM_BOX;
    A.cells = nullptr;
    A.cellv = nullptr;
    A.v0 = A.nv = 0;
    A.r = 0.f;
    if (key == BASEKEY) {
      kind = 1;
      A.c = ld3(m->base_pos);
      A.hs = ld3(m->base_half);
#pragma unroll
      for (int i = 0; i < 9; i++) A.R[i] = (i % 4 == 0) ? 1.f : 0.f;
    } else {
      kind = 0;
      ckey = key;
      const PS_LDS float* g = S->kg[key];
      const float cq = S->kc[key], sq = S->ks[key];
      const float R[9] = {cq, 0.f, sq, 0.f, 1.f, 0.f, -sq, 0.f, cq};
#pragma unroll
      for (int i = 0; i < 9; i++) A.R[i] = R[i];
      const f3 al = ld3(g + 6), an = ld3(g) + al;
      A.c = an + mv3(R, al * -1.f);
      A.hs = ld3(g + 3);
    }
    A.p0 = A.p1 = A.e0 = A.e1 = A.c;
    A.er = 0.f;
    A.tie = 0.f;
  } else {
    A = coll_shape(m, S, ga);
  }
}

// A box / hull pair list entry: (gb << 8) | key for a collider against a key or the base
// (BASEKEY), XHH | (gb << 8) | ga for a hand-hand pair (collider ids below 128).
constexpr int XHH = 0x8000;
static_assert(NGT + 2 * NX <= 128, "pair list entry fields");
__device__ __forceinline__ void x_entry(int pk, int& ga, int& gb, int& key) {
  const bool hh = pk & XHH;
  ga = hh ? pk & 255 : -1;
  key = hh ? -1 : pk & 255;
  gb = (pk >> 8) & 127;
}
// In-place compaction (order kept) of a box / hull pair list to the pairs whose hull is not
// held apart by its enclosing capsule (x_apart), so that the MPR rounds after it run on dense
// lanes. Called by the whole wave; every lane reads its entry before any lane writes.
#ifndef PS_XREFINE_ATTR
#define PS_XREFINE_ATTR __noinline__
#endif
#ifndef PS_XPAIRS_ATTR
#define PS_XPAIRS_ATTR __noinline__
#endif
// (WPE: the calling kernel instantiation's waves per SIMD - each instantiation gets its own
// out-of-line copy, compiled to its register budget)
template <int WPE>
// (the address spaces are in the parameter types - the model in global memory, the workgroup's
// Shared and the list in LDS: a caller with anything else does not compile)
__device__ PS_XREFINE_ATTR int x_refine(const PS_GLB DevModel* mg, const PS_LDS Shared* S, PS_LDS uint16_t* ll, int n,
                                     int lane) {
  int kept = 0;
  for (int r0 = 0; r0 < n; r0 += 64) {
    const int i = r0 + lane;
    const int pk = i < n ? (int)ll[i] : 0;
    bool keep = false;
    if (i < n) {
      XShape A, B;
      int kind, ckey, ga, gb, key;
      x_entry(pk, ga, gb, key);
      x_pair_shapes(mg, S, ga, gb, key, A, B, kind, ckey);
      keep = !x_apart(A, B);
    }
    const uint64_t mask = __ballot(keep);
    wsync();
    if (keep) ll[kept + lanes_below(mask, lane)] = (uint16_t)pk;
    kept += __popcll(mask);
    wsync();
  }
  return kept;
}

template <int WPE>
__device__ PS_XPAIRS_ATTR int x_pairs(const PS_GLB DevModel* mg, const PS_LDS Shared* S, bool act, int ga, int gb, int key,
                                    Contact* out, int base, int maxc, int lane,
                                    int* its = nullptr) {
  if (!act) { ga = -1; gb = NGT; key = BASEKEY; }  // (inert shapes; the count is forced to 0)
  XShape A, B;
  int kind, ckey;
  x_pair_shapes(mg, S, ga, gb, key, A, B, kind, ckey);
  const DevModel* m = (const DevModel*)mg;  // (the support functions of collide_x.h type their own reads)
  int g1 = ga < 0 ? -1 : ga, g2 = gb;
  f3 pos[BB_MAXPT], nrm[BB_MAXPT];
  float dist[BB_MAXPT];
  bool swap = false;
  int nit = 0;
  // paired lanes (mpr_sup_t): lanes 2k and 2k + 1 run pair k, the odd lane's count is dropped
  const bool role = lane & 1;
  int cnt = act ? x_narrow_local<true>(m, A, B, pos, dist, nrm, swap, its ? &nit : nullptr, role) : 0;
  if (its) {  // (timing build) the call's most MPR steps of a pair; active / contact pairs, their steps
    its[0] = -(int)wave_min(-(float)nit);
    its[1] = __popcll(__ballot(act && !role));
    its[2] = __popcll(__ballot(act && !role && cnt > 0));
    its[3] = wave_sum_i(act && !role ? nit : 0);
    its[4] = wave_sum_i(act && !role && cnt > 0 ? nit : 0);
#ifdef PS_TIMING
    // the round holds both an MPR pair and a capsule-box / box-box pair (x_narrow runs every kind
    // present, one after the other); no pair of the round touches
    const bool mpr = !((A.type == 0 || A.type == PS_GEOM_BOX) && B.type == PS_GEOM_BOX);
    its[5] = __ballot(act && mpr) != 0ull && __ballot(act && !mpr) != 0ull;
    its[6] = __ballot(act && !role && cnt > 0) == 0ull;
#endif
  }
  if (role) cnt = 0;
  if (swap) {  // capsule (geom a) vs box (geom b): the box is geom1
    g1 = gb;
    g2 = ga;
  }
  int rt;
  const int slot = base + small_excl_scan<3>(cnt, lane, &rt);  // <= 4 contacts per pair
  {
#pragma unroll
    for (int j = 0; j < BB_MAXPT; j++) {
      if (j < cnt && slot + j < maxc) {
        Contact& cc = out[slot + j];
        st3(cc.pos, pos[j]);
        st3(cc.n, nrm[j]);
        cc.dist = dist[j];
        f3 t1, t2;
        make_frame(nrm[j], &t1, &t2);
        st3(cc.t1, t1);
        st3(cc.t2, t2);
        cc.kind = kind;
        cc.key = ckey;
        cc.g1 = g1;
        cc.g2 = g2;
      }
    }
  }
  return rt;
}

// single-pass piano narrow phase for up to NSTAGE candidates: 2 staged contacts per lane
// after the candidate list in the body-exchange buffer
constexpr int NSTAGE = 32, STAGE_OFF = 2 * 256;
static_assert(STAGE_OFF >= 2 * NSTAGE, "candidate list overlaps the staging area");
// single-pass piano candidates: CPL per capsule lane, staged past the longest compacted list
constexpr int CPL = 8, CSTAGE_OFF = 2 * NGT * CPL;

// Returns the contacts found (>= maxc: the cap may have dropped some).
// XG: the model has box / hull colliders (a separate kernel instantiation, so the capsule-only
// kernel carries none of their code or register pressure)
template <bool XG, int WPE>
__device__ __forceinline__ int collide2(const DevModel* __restrict__ m, Shared& S, int maxc, int lane, float c_r TARG) {
  static_assert(STAGE_OFF + 2 * NSTAGE * sizeof(Contact) <= sizeof(S.bx), "contact staging exceeds bx");
  static_assert(CSTAGE_OFF + 2 * 64 * CPL <= sizeof(S.bx), "candidate staging exceeds bx");
  const bool isc = lane < NGT;
  {  // stage the key collision records (L2-resident model table -> LDS, float4 per lane)
    const float4* src = reinterpret_cast<const float4*>(&m->key_geo[0][0]);
    float4* dst = reinterpret_cast<float4*>(&S.kg[0][0]);
    for (int i = lane; i < NK * KGEO / 4; i += 64) dst[i] = src[i];
    S.kb[0][lane] = m->kb_first[lane];
    S.kb[1][lane] = m->kb_end[lane];
  }
  // lane NGT + e: the type and bounding radius of box / hull collider e, fetched once per pass with
  // the staging above (the hand boxes, the collider lanes and the hand-hand spheres read them here)
  const int x_ty = XG ? m->x_type[lane >= NGT ? lane - NGT : 0] : (int)PS_GEOM_NONE;
  const float x_rbl = XG ? m->x_rb[lane >= NGT ? lane - NGT : 0] : 0.f;
  wsync();
  // piano: the (capsule, key|base) candidate pairs of all capsules, compacted in canonical
  // order into the (dead between dynamics and the next kinematics) body exchange buffer,
  // then one narrow-phase test per lane - balanced across lanes instead of each capsule
  // lane walking its own keys
  uint16_t* cand = reinterpret_cast<uint16_t*>(&S.bx[0][0]);
  constexpr int MAXCAND = (int)(sizeof(S.bx) / sizeof(uint16_t));
  int ncand;
  {
    // one pass: each capsule lane writes up to CPL candidates to its own staging slots,
    // copied to their compacted places after the scan (a second pass only on overflow)
    uint16_t* cst = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(&S.bx[0][0]) + CSTAGE_OFF) + lane * CPL;
    const int cnt = isc ? piano_candidates(m, S, lane, c_r, cst, CPL) : 0;
    const int off = small_excl_scan<7>(cnt, lane, &ncand);  // cnt <= NK + 1 < 2^7
    if (__ballot(cnt > CPL) == 0ull) {
      for (int j = 0; j < cnt; j++) cand[off + j] = cst[j];  // off + cnt <= NGT * CPL < MAXCAND
    } else if (isc && cnt && off + cnt <= MAXCAND) {
      piano_candidates(m, S, lane, c_r, cand + off, cnt);
    }
    ncand = min(ncand, MAXCAND);
  }
  wsync();
  TSTAMP(11);
  int total = 0;
  if (ncand <= NSTAGE) {
    // one narrow-phase pass: each candidate lane writes its (<= 2) contacts to a private
    // staging pair in the dead body-exchange buffer, then the scan places them in order
    Contact* stage = reinterpret_cast<Contact*>(reinterpret_cast<char*>(&S.bx[0][0]) + STAGE_OFF);
    const int pr = lane < ncand ? (int)cand[lane] : 0;
    const int cnt = lane < ncand ? piano_pair<WPE>(m, S, pr, stage, 2 * lane, 2 * lane + 2) : 0;
    int rt;
    const int off = small_excl_scan<2>(cnt, lane, &rt);
    for (int j = 0; j < cnt; j++)
      if (total + off + j < maxc) S.con[total + off + j] = stage[2 * lane + j];
    total += rt;
    ncand = 0;  // done
  }
  for (int r0 = 0; r0 < ncand && total < maxc; r0 += 64) {
    const int i = r0 + lane;
    const int pr = i < ncand ? (int)cand[i] : 0;
    const int cnt = i < ncand ? piano_pair<WPE>(m, S, pr, nullptr, 0, 0) : 0;
    int rt;
    const int off = small_excl_scan<2>(cnt, lane, &rt);  // <= 2 contacts per pair
    if (cnt) piano_pair<WPE>(m, S, pr, S.con, total + off, maxc);
    total += rt;
  }
  TSTAMP(7);
  int base = total;
  // capsule pairs; cross-hand pairs are skipped wholesale when the hands' boxes are apart
  float lo[3], hi[3];
  {
    f3 p0 = isc ? ld3(&S.cap[lane][0]) : mk3(0, 0, 0), p1 = isc ? ld3(&S.cap[lane][3]) : mk3(0, 0, 0);
    lo[0] = fminf(p0.x, p1.x) - c_r; lo[1] = fminf(p0.y, p1.y) - c_r; lo[2] = fminf(p0.z, p1.z) - c_r;
    hi[0] = fmaxf(p0.x, p1.x) + c_r; hi[1] = fmaxf(p0.y, p1.y) + c_r; hi[2] = fmaxf(p0.z, p1.z) + c_r;
  }
  // hand boxes: lanes 0..19 = hand 0 capsules, 20..39 = hand 1; XG: lanes 40..51 / 52..63 =
  // the hands' box / hull colliders by their bounding spheres (min over the box's lanes)
  bool inb = isc;
  int hb = lane < NG ? 0 : 1;
  if (XG && lane >= NGT) {
    const int e = lane - NGT;
    inb = x_ty != PS_GEOM_NONE;
    hb = e / NX;
    if (inb) {
      const f3 ctr = ld3(S.xg[e]);
      const float rb = x_rbl;
      lo[0] = ctr.x - rb; lo[1] = ctr.y - rb; lo[2] = ctr.z - rb;
      hi[0] = ctr.x + rb; hi[1] = ctr.y + rb; hi[2] = ctr.z + rb;
    }
  }
  bool apart = false;
  {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float l0 = wave_min(inb && hb == 0 ? lo[i] : INFINITY), l1 = wave_min(inb && hb == 1 ? lo[i] : INFINITY);
      const float h0 = -wave_min(inb && hb == 0 ? -hi[i] : INFINITY),
                  h1 = -wave_min(inb && hb == 1 ? -hi[i] : INFINITY);
      if (h0 < l1 || h1 < l0) apart = true;
    }
  }
  const int npairs = apart ? m->npairs_same : m->npairs;
  // pass 1: bounding-sphere test of every filtered pair, survivors compacted (pair order kept)
  // into the candidate buffer; pass 2: segment-segment distance on the survivors only
  uint16_t* near = cand;
  int nnear = 0;
  // (PTRIPS trips' table entries are loaded together, lanes past the list with their index clamped
  // into it, and consumed after one round trip; the survivors are compacted trip by trip, in pair
  // order)
  constexpr int PTRIPS = 4;
  for (int p0 = 0; p0 < npairs; p0 += 64 * PTRIPS) {
    int pks[PTRIPS];
#pragma unroll
    for (int u = 0; u < PTRIPS; u++) pks[u] = m->pair[min(p0 + 64 * u + lane, npairs - 1)];
#pragma unroll
    for (int u = 0; u < PTRIPS; u++) {
      const int p = p0 + 64 * u + lane;
      const int pk = pks[u];
      bool pass = false;
      if (p < npairs) {
        const float* A = S.cap[pk & 255];
        const float* B = S.cap[pk >> 8];
        const f3 ca = (ld3(A) + ld3(A + 3)) * 0.5f, cb = (ld3(B) + ld3(B + 3)) * 0.5f;
        pass = norm3(ca - cb) <= A[7] + B[7] + A[6] + B[6];
      }
      const uint64_t mask = __ballot(pass);
      if (pass) near[nnear + lanes_below(mask, lane)] = (uint16_t)pk;
      nnear += __popcll(mask);
    }
  }
  wsync();
  for (int q0 = 0; q0 < nnear && base < maxc; q0 += 64) {
    const int q = q0 + lane;
    bool hit = false;
    f3 c1, c2;
    float ra = 0, rb = 0, dn = 0;
    int ga = 0, gb = 0;
    if (q < nnear) {
      const int pk = near[q];
      ga = pk & 255;
      gb = pk >> 8;
      const float* A = S.cap[ga];
      const float* B = S.cap[gb];
      ra = A[6];
      rb = B[6];
      seg_seg(ld3(A), ld3(A + 3), ld3(B), ld3(B + 3), &c1, &c2);
      dn = norm3(c2 - c1);
      hit = dn - ra - rb <= 0.f;
    }
    uint64_t mask = __ballot(hit);
    int slot = base + lanes_below(mask, lane);
    if (hit && slot < maxc) {
      Contact& cc = S.con[slot];
      f3 dv = c2 - c1;
      f3 n = dn > 1e-9f ? dv * (1.f / dn) : mk3(0, 0, 1);
      float dist = dn - ra - rb;
      st3(cc.n, n);
      cc.dist = dist;
      st3(cc.pos, c1 + n * (ra + 0.5f * dist));
      f3 t1, t2;
      make_frame(n, &t1, &t2);
      st3(cc.t1, t1); st3(cc.t2, t2);
      cc.kind = 2; cc.key = -1; cc.g1 = ga; cc.g2 = gb;
    }
    base += __popcll(mask);
  }
  if (XG && (m->nx || m->nxpairs)) {
    // box / hull colliders, after every capsule pair (the checker's order, oracle/pianosim_ref.c
    // collide): their piano candidates, then the hand-hand pairs with a box / hull collider, in
    // ONE list - one refine pass and one series of narrow-phase rounds (32 pairs per round)
    // instead of one of each per list, and one out-of-line call of each
    TSTAMP(2);
    int nl = 0;
    if (m->nx) {
      // one pass, as the capsules' candidates: each collider lane stages up to CPL candidates in
      // its own slots (past the longest list without overflow: NXT * CPL < CSTAGE_OFF / 2), copied
      // to their compacted places after the scan; a second pass only on overflow
      static_assert(NXT * CPL * 2 <= CSTAGE_OFF, "x candidates overlap the staging");
      const bool isx = lane >= NGT && x_ty != PS_GEOM_NONE;
      uint16_t* cst = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(&S.bx[0][0]) + CSTAGE_OFF) + lane * CPL;
      wsync();  // (the capsule pairs' list has been read)
      const int cnt = isx ? xpiano_candidates(m, S, lane, cst, CPL) : 0;
      const int off = small_excl_scan<7>(cnt, lane, &nl);
      wsync();
      if (__ballot(cnt > CPL) == 0ull) {
        for (int j = 0; j < cnt; j++) cand[off + j] = cst[j];
      } else if (isx && cnt && off + cnt <= MAXCAND) {
        xpiano_candidates(m, S, lane, cand + off, cnt);
      }
      nl = min(nl, MAXCAND);
      wsync();
    }
    TSTAMP(32);
    if (m->nxpairs) {  // hand-hand: bounding spheres
      const int nxp = apart ? m->nxpairs_same : m->nxpairs;  // cross-hand ones: only when the boxes meet
      for (int p0 = 0; p0 < nxp; p0 += 64 * PTRIPS) {  // (entries of PTRIPS trips per round trip, as above)
        int pks[PTRIPS];
#pragma unroll
        for (int u = 0; u < PTRIPS; u++) pks[u] = m->xpair[min(p0 + 64 * u + lane, nxp - 1)];
#pragma unroll
        for (int u = 0; u < PTRIPS; u++) {
          const int p = p0 + 64 * u + lane;
          const int pk = pks[u];
          const int ga = pk & 255, gb = pk >> 8;
          // (the bounding radii from the collider lanes: an exchange of the whole wave)
          const float rba = __shfl(x_rbl, ga, 64), rbb = __shfl(x_rbl, gb, 64);
          bool pass = false;
          if (p < nxp) {
            f3 c2[2];
            float rad = 0.f;
#pragma unroll
            for (int q = 0; q < 2; q++) {
              const int g = q ? gb : ga;
              if (g < NGT) {
                c2[q] = (ld3(&S.cap[g][0]) + ld3(&S.cap[g][3])) * 0.5f;
                rad += S.cap[g][6] + S.cap[g][7];
              } else {
                c2[q] = ld3(S.xg[g - NGT]);
                rad += q ? rbb : rba;
              }
            }
            pass = norm3(c2[0] - c2[1]) <= rad;
          }
          const uint64_t mask = __ballot(pass);
          const int at = nl + lanes_below(mask, lane);
          if (pass && at < MAXCAND) cand[at] = (uint16_t)(pk | XHH);
          nl = min(nl + __popcll(mask), MAXCAND);
        }
      }
#ifdef PS_TIMING
      tacc[45] += nl;  // (hand-hand pairs past the bounding spheres + piano candidates)
#endif
    }
    wsync();
    TSTAMP(35);
    // (the out-of-line narrow phases take typed pointers: S is the workgroup's LDS, m the kernel's model argument)
    const PS_GLB DevModel* mg = (const PS_GLB DevModel*)m;
    const PS_LDS Shared* Sl = (const PS_LDS Shared*)&S;
    nl = x_refine<WPE>(mg, Sl, (PS_LDS uint16_t*)cand, nl, lane);
#ifdef PS_TIMING
    tacc[42] += nl > 0;
#endif
    TSTAMP(36);
    for (int q0 = 0; q0 < nl && base < maxc; q0 += 32) {  // 32 pairs on lane pairs per round
      const int q = q0 + (lane >> 1);
      int ga, gb, key;
      x_entry(q < nl ? (int)cand[q] : 0, ga, gb, key);
#ifdef PS_TIMING
      int its[7] = {0, 0, 0, 0, 0, 0, 0};
      base += x_pairs<WPE>(mg, Sl, q < nl, ga, gb, key, S.con, base, maxc, lane, its);
      tacc[30] += its[0];
      tacc[31] += 1;
      tacc[38] += its[1];
      tacc[39] += its[2];
      tacc[40] += its[3];
      tacc[41] += its[4];
      tacc[TS_XMIXED] += its[5];
      tacc[TS_XNOHIT] += its[6];
#else
      base += x_pairs<WPE>(mg, Sl, q < nl, ga, gb, key, S.con, base, maxc, lane);
#endif
    }
    TSTAMP(37);
  }
  if (lane == 0) S.ncon = base < maxc ? base : maxc;
  wsync();
  return base;
}

// The forearm term's prefilter, after kinematics2 of the state: can any pair of colliders on the
// two hands' root bodies (DevModel::fore_pair, one per lane) touch? A contact of such a pair is
// all the forearm term looks for. Two capsules: collide2 reports a contact when the points seg_seg
// finds on the two segments are at most ra + rb apart, and no two points of the segments are
// closer than the gap between the segments' bounding boxes - so none when that gap exceeds
// ra + rb by the margin (0.1 mm: five orders above the rounding of either side). A pair with a
// box / hull collider: collide2 tests its shapes only past the bounding spheres, the test repeated
// here with a margin for the rounding of the sums. When no pair passes, no contact list - capped
// or not - holds a forearm hit. Wave-uniform.
template <bool XG>
__device__ __forceinline__ bool fore_near(const DevModel* __restrict__ m, const Shared& S, int lane) {
  const int nf = m->nfore;
  if (nf < 0) return true;  // (too many pairs for one trip: no prefilter)
  bool pass = false;
  if (lane < nf) {
    const int pk = m->fore_pair[lane];
    const int ga = pk & 255, gb = pk >> 8;
    if (ga < NGT && gb < NGT) {
      const float *A = S.cap[ga], *B = S.cap[gb];
      const float reach = A[6] + B[6] + 1e-4f;
      float d2 = 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float alo = fminf(A[i], A[3 + i]), ahi = fmaxf(A[i], A[3 + i]);
        const float blo = fminf(B[i], B[3 + i]), bhi = fmaxf(B[i], B[3 + i]);
        const float gap = fmaxf(0.f, fmaxf(alo - bhi, blo - ahi));
        d2 += gap * gap;
      }
      pass = !(d2 > reach * reach);
    } else if (XG) {
      f3 c2[2];
      float rad = 0.f;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const int g = q ? gb : ga;
        if (g < NGT) {
          c2[q] = (ld3(&S.cap[g][0]) + ld3(&S.cap[g][3])) * 0.5f;
          rad += S.cap[g][6] + S.cap[g][7];
        } else {
          c2[q] = ld3(S.xg[min(g - NGT, NXT - 1)]);
          rad += m->x_rb[min(g - NGT, NXT - 1)];
        }
      }
      pass = !(norm3(c2[0] - c2[1]) > rad * 1.00001f + 1e-6f);
    } else {
      pass = true;  // (a box / hull pair in the capsule-only kernel: never skipped)
    }
  }
  return __ballot(pass) != 0ull;
}

// ------------------------------------------------------------------ per-lane state
struct LaneStatic {
  // dof role
  int d_type, d_body, d_depth, d_ap0, d_ap1, d_act;
  uint64_t d_ancmask, d_desc;
  float d_axl[3], d_lo, d_hi, d_damp, d_arm, d_dinv, d_actc;
  bool d_lim;
  // body role (geometry and inertia are re-read from the model at use: keeps VGPRs low)
  int b_parent, b_level, b_dof, b_ndof, b_chp, b_nch;
  // capsule role
  int c_body;
  float c_r;
};

__device__ __forceinline__ void load_static(const DevModel* __restrict__ m, Shared& S, LaneStatic& L, int lane) {
  const int d = lane < NDT ? lane : 0, b = lane < NBT ? lane : 0, c = lane < NGT ? lane : 0;
  L.d_type = m->dof_type[d];
  L.d_body = m->dof_body[d];
  L.d_depth = lane < NDT ? m->dof_depth[d] : -1;
  L.d_ap0 = m->dof_anc_pack[d][0];
  L.d_ap1 = m->dof_anc_pack[d][1];
  L.d_act = m->dof_act[d];
  L.d_ancmask = m->dof_ancmask[d];
  L.d_desc = lane < NDT ? m->dof_descmask[d] : 0ull;
  for (int i = 0; i < 3; i++) L.d_axl[i] = m->dof_axis[d][i];
  L.d_lo = m->dof_lo[d];
  L.d_hi = m->dof_hi[d];
  L.d_lim = m->dof_limited[d] && lane < NDT;
  L.d_damp = m->dof_damp[d];
  L.d_arm = m->dof_arm[d];
  L.d_dinv = m->dof_dinv[d];
  L.d_actc = m->dof_act_coef[d];
  L.b_parent = m->body_parent[b];
  L.b_level = lane < NBT ? m->body_level[b] : -1;
  L.b_dof = m->body_dof[b];
  L.b_ndof = m->body_ndof[b];
  L.b_chp = m->body_child_pack[b];
  L.b_nch = lane < NBT ? m->body_nchild[b] : 0;
  L.c_body = m->geom_body[c];
  L.c_r = m->geom_r[c];
  #pragma unroll
  for (int j = 0; j < 2; j++) {
    int kk = lane + 64 * j;
    if (kk < NK) S.kminv[kk] = m->key_Minv[kk];
  }
  if (lane < NDT) {
    S.anc[lane][0] = L.d_ap0;
    S.anc[lane][1] = L.d_ap1;
    S.depth[lane] = L.d_depth;
    S.dtype[lane] = L.d_type;
  }
}

struct LaneDyn {
  // dof, then keys
  // M: D and the L row of the factor of M (then also staged in S.Lr); Mh: the factor of
  // M + hD, its L row replaced by the row of Gh = Lh^-1 after factor2; G: the row of L^-1
  float q, v, qws, qfs, M[MAXDEP], Mh[MAXDEP], G[MAXDEP], Dinv, Dhinv;
  float kq[2], kv[2], kws[2], kqfs[2], kfree[2];
  // dead at the constraint solve (rewritten before their next use): dof, body, keys
  float w, qas, actf, axw[3], ob[3];
  float R[9], o[3];
  float kqas[2];
};

// ------------------------------------------------------------------ kinematics
// Top-down over the tree levels: body frames and, with RNE, the recursive Newton-Euler
// forward terms (angular velocity w, angular acceleration al, linear acceleration ac of the
// body origin with gravity as base acceleration, qacc = 0) in the same pass.
template <bool RNE, bool XG>
__device__ __forceinline__ void kinematics2(const DevModel* __restrict__ m, Shared& S, const LaneStatic& L, LaneDyn& D, int lane,
                                            float hand_dy TARG) {
  // the body / dof frame registers are rewritten here for the lanes that own a body / dof;
  // clearing them for every lane first ends their live range at the last use of the previous
  // substep (otherwise the untouched lanes' stale values stay live through the solve phases)
#pragma unroll
  for (int i = 0; i < 9; i++) D.R[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) D.o[i] = D.axw[i] = D.ob[i] = 0.f;
  float qb0 = __shfl(D.q, L.b_dof, 64), qb1 = __shfl(D.q, L.b_ndof > 1 ? L.b_dof + 1 : L.b_dof, 64);
  const float qd = RNE ? __shfl(D.v, L.b_dof, 64) : 0.f;
  const int bb = lane < NBT ? lane : 0;
  const f3 bpos = ld3(m->body_pos[bb]), axl0 = ld3(m->dof_axis[L.b_dof]);
  const f3 axl1 = L.b_ndof > 1 ? ld3(m->dof_axis[L.b_dof + 1]) : mk3(0, 0, 0);
  // The body's rotation relative to its parent, Q * A(q), does not depend on the parent:
  // formed for every body at once, off the level-serial chain (only Rp * QA stays on it).
  float QA[9];
  {
    float bQ[9];
#pragma unroll
    for (int i = 0; i < 9; i++) bQ[i] = m->body_Q[bb][i];
    if (L.b_level == 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) QA[i] = bQ[i];
    } else {
      float s, c;
      fsincos(qb0, &s, &c);
      float C1 = 1.f - c, x = axl0.x, y = axl0.y, z = axl0.z;
      float A[9] = {c + x * x * C1,     x * y * C1 - z * s, x * z * C1 + y * s,
                    y * x * C1 + z * s, c + y * y * C1,     y * z * C1 - x * s,
                    z * x * C1 - y * s, z * y * C1 + x * s, c + z * z * C1};
      mm3(bQ, A, QA);
    }
  }
  // capsule model data loaded before the level loop (its LDS exchange points are compiler
  // barriers: issued here, the L2 round trip overlaps the loop instead of following it)
  const int gl = lane < NGT ? lane : 0;
  const f3 g_pos = ld3(m->geom_pos[gl]), g_axis = ld3(m->geom_axis[gl]);
  const float g_hl = m->geom_hl[gl];
  if (RNE) TSTAMP(24);
  for (int lev = 0; lev < m->nlev; lev++) {
    if (L.b_level == lev) {
      f3 w = mk3(0, 0, 0), al = mk3(0, 0, 0), ac = mk3(-m->hgrav[0], -m->hgrav[1], -m->hgrav[2]);
      if (lev == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) D.R[i] = QA[i];
        f3 t = axl0 * qb0 + axl1 * qb1;
        st3(D.o, bpos + mk3(0.f, hand_dy, 0.f) + mv3(D.R, t));
      } else {
        const float* P = S.bx[L.b_parent];
        float Rp[9];
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = P[BX_R + i];
        f3 op = ld3(P + BX_O);
        mm3(Rp, QA, D.R);
        st3(D.o, op + mv3(Rp, bpos));
        if (RNE) {
          const f3 wp = ld3(P + BX_W), alp = ld3(P + BX_AL), acp = ld3(P + BX_AC);
          const f3 r = ld3(D.o) - op, aw = mv3(D.R, axl0);
          ac = acp + cross3(alp, r) + cross3(wp, cross3(wp, r));
          al = alp + cross3(wp, aw) * qd;
          w = wp + aw * qd;
        }
      }
      float* B = S.bx[lane];
#pragma unroll
      for (int i = 0; i < 9; i++) B[BX_R + i] = D.R[i];
      st3(B + BX_O, ld3(D.o));
      if (RNE) { st3(B + BX_W, w); st3(B + BX_AL, al); st3(B + BX_AC, ac); }
    }
    wsync();
  }
  if (RNE) TSTAMP(25);
  if (lane < NDT) {
    const float* B = S.bx[L.d_body];
    float Rb[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rb[i] = B[BX_R + i];
    f3 aw = mv3(Rb, ld3(L.d_axl));
    st3(D.axw, aw);
    st3(D.ob, ld3(B + BX_O));
    st3(S.dx[lane], aw);
    st3(S.dx[lane] + 3, ld3(D.ob));
    S.dx[lane][6] = D.q;
  }
  if (lane < NGT) {
    const float* B = S.bx[L.c_body];
    float Rb[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rb[i] = B[BX_R + i];
    f3 cc = ld3(B + BX_O) + mv3(Rb, g_pos);
    f3 a = mv3(Rb, g_axis);
    float hl = g_hl;
    st3(&S.cap[lane][0], cc - a * hl);
    st3(&S.cap[lane][3], cc + a * hl);
    S.cap[lane][6] = L.c_r;
    S.cap[lane][7] = hl;
  }
  if (XG && m->nx && lane >= NGT) {  // box / hull colliders (lanes NGT..63), only in models that have them
    const int e = lane - NGT;
    if (m->x_type[e] != PS_GEOM_NONE) {
      const float* B = S.bx[m->geom_body[lane]];
      float Rb[9], Rx[9];
#pragma unroll
      for (int i = 0; i < 9; i++) Rb[i] = B[BX_R + i];
      st3(S.xg[e], ld3(B + BX_O) + mv3(Rb, ld3(m->x_pos[e])));
      mm3(Rb, m->x_Q[e], Rx);
#pragma unroll
      for (int i = 0; i < 9; i++) S.xg[e][3 + i] = Rx[i];
    }
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int k = lane + 64 * j;
    if (k < NK) {
      float s, c;
      fsincos(D.kq[j], &s, &c);
      S.kc[k] = c;
      S.ks[k] = s;
    }
  }
  wsync();
}

// ------------------------------------------------------------------ dynamics
// Needs kinematics2<true> of the same state. One bottom-up pass folds both the composite
// rigid-body inertias (CRB, for the mass matrix) and the RNE backward forces (bias).
__device__ __forceinline__ void dynamics2(const DevModel* __restrict__ m, Shared& S, const LaneStatic& L, LaneDyn& D,
                          const float* __restrict__ applied, int lane TARG) {
  const bool isb = lane < NBT;
  // world inertia about COM and COM offset (body lanes, registers)
  float Iw[6];
  f3 dd;
  const int bb = lane < NBT ? lane : 0;
  const float b_mass = m->body_mass[bb];
  {
    const float* bI = m->body_I[bb];
    float Il[9] = {bI[0], bI[3], bI[4], bI[3], bI[1], bI[5], bI[4], bI[5], bI[2]};
    float T[9], F9[9];
    mm3(D.R, Il, T);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) F9[3 * i + k] = T[3 * i] * D.R[3 * k] + T[3 * i + 1] * D.R[3 * k + 1] + T[3 * i + 2] * D.R[3 * k + 2];
    Iw[0] = F9[0]; Iw[1] = F9[4]; Iw[2] = F9[8]; Iw[3] = F9[1]; Iw[4] = F9[2]; Iw[5] = F9[5];
    dd = mv3(D.R, ld3(m->body_ipos[bb]));
  }
  // actuator and key model data loaded before the bottom-up loop (see kinematics2)
  const int ua = lane < NU ? lane : 0;
  const int u_d0 = m->act_dof0[ua], u_d1 = m->act_dof1[ua], u_kind = m->act_kind[ua], u_flim = m->act_flim[ua];
  const float u_c0 = m->act_c0[ua], u_c1 = m->act_c1[ua], u_clo = m->act_clo[ua], u_chi = m->act_chi[ua];
  const float u_kp = m->act_kp[ua], u_flo = m->act_flo[ua], u_fhi = m->act_fhi[ua];
  float k_hx[2], k_mass[2], k_stiff[2], k_sref[2], k_damp[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int k = lane + 64 * j < NK ? lane + 64 * j : 0;
    k_hx[j] = -m->key_anchor[k][0];
    k_mass[j] = m->key_mass[k];
    k_stiff[j] = m->key_stiff[k];
    k_sref[j] = m->key_sref[k];
    k_damp[j] = m->key_damp[k];
  }
  // composite inertia about the body origin: {ms, h[3], Is[6]}
  float cp[10];
  {
    float mass = b_mass, d2 = dot3(dd, dd);
    cp[0] = mass;
    cp[1] = dd.x * mass; cp[2] = dd.y * mass; cp[3] = dd.z * mass;
    cp[4] = Iw[0] + mass * (d2 - dd.x * dd.x);
    cp[5] = Iw[1] + mass * (d2 - dd.y * dd.y);
    cp[6] = Iw[2] + mass * (d2 - dd.z * dd.z);
    cp[7] = Iw[3] - mass * dd.x * dd.y;
    cp[8] = Iw[4] - mass * dd.x * dd.z;
    cp[9] = Iw[5] - mass * dd.y * dd.z;
  }
  // RNE backward seed: the body's own inertial force / torque about its origin
  f3 F, N;
  {
    const float* B = S.bx[bb];
    const f3 w = ld3(B + BX_W), al = ld3(B + BX_AL), ac = ld3(B + BX_AC);
    f3 acom = ac + cross3(al, dd) + cross3(w, cross3(w, dd));
    F = acom * b_mass;
    N = sym_mv(Iw, al) + cross3(w, sym_mv(Iw, w)) + cross3(dd, F);
  }
  if (isb) {  // own record only: its w/al/ac were read above (program order within the wave)
    float* B = S.bx[lane];
#pragma unroll
    for (int i = 0; i < 10; i++) B[BX_CP + i] = cp[i];
    st3(B + BX_F, F);
    st3(B + BX_N, N);
  }
  wsync();
  for (int lev = m->nlev - 2; lev >= 0; lev--) {
    if (L.b_level == lev && L.b_nch > 0) {
      f3 op = ld3(D.o);
      for (int c = 0; c < L.b_nch; c++) {
        int ch = (L.b_chp >> (6 * c)) & 63;
        const float* sb = S.bx[ch];
        f3 r = ld3(sb + BX_O) - op;
        f3 hb = mk3(sb[BX_CP + 1], sb[BX_CP + 2], sb[BX_CP + 3]);
        float msb = sb[BX_CP], r2 = dot3(r, r), rh = dot3(r, hb);
        cp[4] += sb[BX_CP + 4] + msb * (r2 - r.x * r.x) + (2.f * rh - 2.f * r.x * hb.x);
        cp[5] += sb[BX_CP + 5] + msb * (r2 - r.y * r.y) + (2.f * rh - 2.f * r.y * hb.y);
        cp[6] += sb[BX_CP + 6] + msb * (r2 - r.z * r.z) + (2.f * rh - 2.f * r.z * hb.z);
        cp[7] += sb[BX_CP + 7] - msb * r.x * r.y - (r.x * hb.y + hb.x * r.y);
        cp[8] += sb[BX_CP + 8] - msb * r.x * r.z - (r.x * hb.z + hb.x * r.z);
        cp[9] += sb[BX_CP + 9] - msb * r.y * r.z - (r.y * hb.z + hb.y * r.z);
        cp[1] += hb.x + r.x * msb; cp[2] += hb.y + r.y * msb; cp[3] += hb.z + r.z * msb;
        cp[0] += msb;
        const f3 Fb = ld3(sb + BX_F), Nb = ld3(sb + BX_N);
        N = N + Nb + cross3(r, Fb);
        F = F + Fb;
      }
      float* B = S.bx[lane];
#pragma unroll
      for (int i = 0; i < 10; i++) B[BX_CP + i] = cp[i];
      st3(B + BX_F, F);
      st3(B + BX_N, N);
    }
    wsync();
  }
  TSTAMP(26);
  // mass matrix rows (dof lane i): entries with its ancestors-or-self
  if (lane < NDT) {
    const float* s = S.bx[L.d_body];
    f3 ai = ld3(D.axw), h = mk3(s[BX_CP + 1], s[BX_CP + 2], s[BX_CP + 3]), flin, fang;
    if (L.d_type == 0) {
      flin = cross3(ai, h);
      const float Is[6] = {s[BX_CP + 4], s[BX_CP + 5], s[BX_CP + 6], s[BX_CP + 7], s[BX_CP + 8], s[BX_CP + 9]};
      fang = sym_mv(Is, ai);
    } else {
      flin = ai * s[BX_CP];
      fang = cross3(h, ai);
    }
    f3 oi = ld3(D.ob);
#pragma unroll
    for (int a = 0; a < MAXDEP; a++) {
      float val = 0.f;
      if (a <= L.d_depth) {
        int j = a == 0 ? lane : anc_of(L.d_ap0, L.d_ap1, a);
        f3 aj = ld3(S.dx[j]), oj = ld3(S.dx[j] + 3);
        // dof j is a hinge unless it sits on the root (slides): depth < 2
        bool jslide = S.dtype[j] == 1;
        val = jslide ? dot3(aj, flin) : dot3(aj, fang + cross3(oi - oj, flin));
      }
      D.M[a] = val + (a == 0 ? L.d_arm : 0.f);
      D.Mh[a] = D.M[a] + (a == 0 ? m->timestep * L.d_damp : 0.f);
    }
    // a locked dof: its row and column of M decouple (identity row), so its acceleration is 0
    // and the others move as without the joint
    const uint64_t lk = m->dof_lockmask;
    if (lk) {
#pragma unroll
      for (int a = 0; a < MAXDEP; a++) {
        if (a <= L.d_depth) {
          const int j = a == 0 ? lane : anc_of(L.d_ap0, L.d_ap1, a);
          if (((lk >> lane) | (lk >> j)) & 1ull) D.M[a] = D.Mh[a] = a == 0 ? 1.f : 0.f;
        }
      }
    }
  }
  TSTAMP(27);
  // actuators (lane = actuator): force from q of its dofs
  {
    float q0 = __shfl(D.q, u_d0, 64), q1 = __shfl(D.q, u_d1, 64);
    float len = u_c0 * q0 + (u_kind == 1 ? u_c1 * q1 : 0.f);
    float c = clampf(D.actf, u_clo, u_chi);  // D.actf holds ctrl on entry
    float f = u_kp * (c - len);
    if (u_flim) f = clampf(f, u_flo, u_fhi);
    float fa = __shfl(f, L.d_act >= 0 ? L.d_act : 0, 64);
    if (lane < NDT) {
      const float* B = S.bx[L.d_body];
      float bias = L.d_type == 1 ? dot3(ld3(D.axw), ld3(B + BX_F)) : dot3(ld3(D.axw), ld3(B + BX_N));
      float frc = -L.d_damp * D.v - bias + (L.d_act >= 0 ? L.d_actc * fa : 0.f);
      if (applied) frc += applied[NK + lane];
      D.qfs = ((m->dof_lockmask >> lane) & 1ull) ? 0.f : frc;
    }
    // keep the actuator force for the energy term (lane = actuator)
    D.w = f;  // scratch: overwritten by the PGS init
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int k = lane + 64 * j;
    if (k < NK) {
      float c = S.kc[k], s = S.ks[k];
      // COM relative to the hinge: R_y(q) (hx, 0, 0)
      float hx = k_hx[j];
      float rx = c * hx, rz = -s * hx;
      float bias = -k_mass[j] * (rz * m->grav[0] - rx * m->grav[2]);
      float f = -k_stiff[j] * (D.kq[j] - k_sref[j]) - k_damp[j] * D.kv[j] - bias;
      if (applied) f += applied[k];
      D.kqfs[j] = f;
    }
  }
  wsync();
}

// Tree LDL of M and Mh (M = L^T D L, MuJoCo mj_factorI), rows in the owning lanes, level
// synchronous: the dofs of one depth are pivots together (none is an ancestor of another,
// and all their descendants are done), each ancestor lane folds in the pivots of its
// subtree at that depth. 9 levels instead of 26 sequential pivots per hand.
__device__ __forceinline__ void factor2(const DevModel* __restrict__ m, Shared& S, const LaneStatic& L, LaneDyn& D, int lane) {
  for (int d = m->ndepth - 1; d >= 0; d--) {
    const bool piv = L.d_depth == d;
    if (piv) {
      float* fr = S.fstage[lane];
      const float Dk = fmaxf(D.M[0], MINVALF), Dhk = fmaxf(D.Mh[0], MINVALF);
      D.M[0] = Dk;
      D.Mh[0] = Dhk;
      const float iD = frcp(Dk), iDh = frcp(Dhk);
#pragma unroll
      for (int a = 0; a < MAXDEP; a++) { fr[a] = D.M[a]; fr[MAXDEP + a] = D.Mh[a]; }
      fr[2 * MAXDEP] = iD;
      fr[2 * MAXDEP + 1] = iDh;
#pragma unroll
      for (int a = 1; a < MAXDEP; a++) { D.M[a] *= iD; D.Mh[a] *= iDh; }
    }
    const uint64_t pivots = __ballot(piv);
    if (d == 0) break;
    wsync();
    // entry c of this lane's row pairs with entry a + c of pivot k's row, a = d - depth.
    // Folded unmasked: for c <= depth the entries read are the pivot's own (a + c <= d);
    // the ones past it (c > depth) only ever receive values that are not the row's and are
    // cleared after the last level.
    const int a = d - L.d_depth;
    uint64_t todo = L.d_desc & pivots;
    while (todo) {
      const int k = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const float* fr = &S.fstage[k][a];
      float vM[MAXDEP], vH[MAXDEP];
#pragma unroll
      for (int c = 0; c < MAXDEP; c++) {
        vM[c] = fr[c];
        vH[c] = fr[MAXDEP + c];
      }
      const float tk = vM[0] * S.fstage[k][2 * MAXDEP], thk = vH[0] * S.fstage[k][2 * MAXDEP + 1];
#pragma unroll
      for (int c = 0; c < MAXDEP; c++) {
        D.M[c] = fmaf(-tk, vM[c], D.M[c]);
        D.Mh[c] = fmaf(-thk, vH[c], D.Mh[c]);
      }
    }
    wsync();
  }
#pragma unroll
  for (int c = 1; c < MAXDEP; c++) {
    const bool on = c <= L.d_depth;
    D.M[c] = on ? D.M[c] : 0.f;
    D.Mh[c] = on ? D.Mh[c] : 0.f;
  }
  if (lane < NDT) {
    D.Dinv = frcp(D.M[0]);
    D.Dhinv = frcp(D.Mh[0]);
#pragma unroll
    for (int a = 0; a < MAXDEP; a++) S.Lr[lane][a] = D.M[a];
    S.dinv[lane] = D.Dinv;
  }
  // Rows of G = L^-1 and Gh = Lh^-1 (unit lower with the same ancestor pattern), from
  // G L = I:  G(i, a) = -L(i, a) - sum_{b < a} G(i, b) L(anc_b(i), a - b)
  // (the a-th ancestor of i is the (a-b)-th of its b-th): every dof lane at once from the
  // ancestors' L rows (S.Lr; Lh rows staged in fstage, dead until the constraint rows), no
  // level loop. Past a dof's depth L = 0, so its G entries come out exactly 0. The tree
  // solves then take one level each way (solve2) instead of one per depth.
  if (lane < NDT) {
#pragma unroll
    for (int a = 0; a < MAXDEP; a++) S.fstage[lane][a] = D.Mh[a];
  }
  wsync();
  {
    const int i = lane < NDT ? lane : 0;
    float g[MAXDEP], gh[MAXDEP];
    g[0] = gh[0] = 0.f;
#pragma unroll
    for (int a = 1; a < MAXDEP; a++) {
      float sg = -D.M[a], sh = -D.Mh[a];
#pragma unroll
      for (int b = 1; b < a; b++) {
        const int k = b <= L.d_depth ? anc_of(L.d_ap0, L.d_ap1, b) : i;
        sg = fmaf(-g[b], S.Lr[k][a - b], sg);
        sh = fmaf(-gh[b], S.fstage[k][a - b], sh);
      }
      g[a] = sg;
      gh[a] = sh;
    }
#pragma unroll
    for (int a = 0; a < MAXDEP; a++) {
      D.G[a] = lane < NDT ? g[a] : 0.f;
      if (a > 0) D.Mh[a] = lane < NDT ? gh[a] : 0.f;
    }
  }
  wsync();
  // S.Lr now takes the G rows: the constraint rows' L^-T is G^T (row_LT)
  if (lane < NDT) {
#pragma unroll
    for (int a = 1; a < MAXDEP; a++) S.Lr[lane][a] = D.G[a];
  }
  wsync();
}

// x <- M^-1 x (and, when TWO, x2 <- Mh^-1 x2) for the hand dofs; values in lane registers.
// HONLY: x <- Mh^-1 x alone (x2 untouched). With G = L^-1 (factor2): z = G^T x (every dof
// adds its G-weighted value to all its ancestors at once, LDS float atomics), z <- D^-1 z,
// x = G z (every dof reads its ancestors' z at once): two tree levels, not 2 x depth.
template <bool TWO, bool HONLY = false>
__device__ __forceinline__ void solve2(const DevModel* __restrict__ m, Shared& S, const LaneStatic& L, const LaneDyn& D, float& x,
                       float& x2, int lane) {
  static_assert(!(TWO && HONLY), "HONLY solves one system");
  const float* GM = HONLY ? D.Mh : D.G;
  const float LDinv = HONLY ? D.Dhinv : D.Dinv;
  const bool isd = lane < NDT;
  if (isd) { S.x[lane] = x; if (TWO) S.x2[lane] = x2; }
  wsync();
  if (isd) {  // G^T: push to the ancestors
    const float xi = x, xi2 = TWO ? x2 : 0.f;
#pragma unroll
    for (int a = 1; a < MAXDEP; a++) {
      if (a <= L.d_depth) {
        const int j = anc_of(L.d_ap0, L.d_ap1, a);
        atomicAdd(&S.x[j], GM[a] * xi);
        if (TWO) atomicAdd(&S.x2[j], D.Mh[a] * xi2);
      }
    }
  }
  wsync();
  float xi = 0.f, xi2 = 0.f;
  if (isd) {
    xi = S.x[lane] * LDinv;
    S.x[lane] = xi;
    if (TWO) { xi2 = S.x2[lane] * D.Dhinv; S.x2[lane] = xi2; }
  }
  wsync();
  if (isd) {  // G: pull from the ancestors (past its depth a dof's packed ancestor is
              // itself and its G entry is 0: those terms add exactly 0)
    float xa[MAXDEP], xa2[MAXDEP];
#pragma unroll
    for (int a = 1; a < MAXDEP; a++) {
      const int j = anc_of(L.d_ap0, L.d_ap1, a);
      xa[a] = S.x[j];
      if (TWO) xa2[a] = S.x2[j];
    }
    float s = xi, s2 = xi2;
#pragma unroll
    for (int a = 1; a < MAXDEP; a++) {
      s = fmaf(GM[a], xa[a], s);
      if (TWO) s2 = fmaf(D.Mh[a], xa2[a], s2);
    }
    x = s;
    if (TWO) x2 = s2;
  }
  wsync();
}

__device__ __forceinline__ float wave_max(float v) { return -wave_min(-v); }

// ------------------------------------------------------------------ constraints
#include "newton.inc"

// ------------------------------------------------------------------ task layer helpers
__device__ __forceinline__ f3 site_world2(const DevModel* __restrict__ m, const LaneDyn& D, int s) {
  // site body's R, o live in the body lane: fetch by shuffle (all lanes call)
  int B = m->site_body[s];
  float R[9];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = __shfl(D.R[i], B, 64);
  f3 o = mk3(__shfl(D.o[0], B, 64), __shfl(D.o[1], B, 64), __shfl(D.o[2], B, 64));
  return o + mv3(R, ld3(m->site_pos[s]));
}

__device__ __forceinline__ f3 key_target2(const DevModel* __restrict__ m, const Shared& S, int k) {
  float R[9];
  f3 c, a;
  key_frame2(m, S, k, R, &c, &a);
  c.x += 0.35f * m->key_half[k][0];
  c.z += 0.5f * m->key_half[k][2];
  return c;
}

// The one-hand task (cfg.hand; piano_with_one_shadow_hand.py:297-345): the fingering row is 5
// wide, the kept hand's fingers only (0-4 right, 5-9 left -> slot f - 5); joints_pos is the kept
// hand's (obs_dof lists no other), and the row ends with `root`, the world position of that
// hand's root body
__device__ __forceinline__ void write_obs2(const DevModel* __restrict__ m, const Song& song, const Cfg& cfg, const Shared& S,
                           int t_obs, float* __restrict__ obs, int lane, const f3 root) {
  const bool one = cfg.hand != 0;
  int G = (cfg.lookahead + 1) * (NK + 1);
  int o_f = G, o_s = G + (cfg.fingering ? (one ? 5 : 10) : 0);
  for (int i = lane; i < cfg.obs_base; i += 64) {
    float val;
    if (i < G) {
      int j = i / (NK + 1), k = i - j * (NK + 1);
      int t = t_obs + j;
      val = t < song.T ? song.goal[t * (NK + 1) + k] : 0.f;
    } else if (i < o_s) {
      int slot = i - o_f;
      val = 0.f;
      for (int n = 0; n < song.count[t_obs]; n++) {
        int f = song.fingers[t_obs * PS_MAX_NOTES + n];
        int idx = f < 5 ? (f < 0 ? f + 5 : f) : f;
        if (one) {
          if ((f < 5) != (cfg.hand == 1)) continue;  // the other hand's note
          if (f >= 5) idx = f - 5;
        }
        if (idx == slot) val = 1.f;
      }
    } else if (i < o_s + NK) {
      val = S.knorm[i - o_s];
    } else if (i == o_s + NK) {
      val = S.sustain;
    } else if (one && i >= cfg.obs_base - 3) {
      const int c = i - (cfg.obs_base - 3);
      val = c == 0 ? root.x : c == 1 ? root.y : root.z;
    } else {
      val = S.dx[m->obs_dof[i - o_s - NK - 1]][6];
    }
    obs[i] = val;
  }
}

// Transmission velocity of actuator `lane` (the joint's, or the fixed tendon's sum over its two
// dofs): the energy term's and the actuators_velocity observable's. All lanes call.
__device__ __forceinline__ float act_velocity(const DevModel* __restrict__ m, const LaneDyn& D, int lane) {
  const int a = lane < NU ? lane : 0;
  const float v0 = __shfl(D.v, m->act_dof0[a], 64), v1 = __shfl(D.v, m->act_dof1[a], 64);
  return m->act_c0[a] * v0 + (m->act_kind[a] == 1 ? m->act_c1[a] * v1 : 0.f);
}

// The actuation stage's force of actuator `lane` at the lanes' D.q for the control `ctrl`
// (dynamics2's rule, restated for the reset row: mj_forward at the reset state). All lanes call.
__device__ __forceinline__ float act_force(const DevModel* __restrict__ m, const LaneDyn& D, float ctrl, int lane) {
  const int a = lane < NU ? lane : 0;
  const float q0 = __shfl(D.q, m->act_dof0[a], 64), q1 = __shfl(D.q, m->act_dof1[a], 64);
  const float len = m->act_c0[a] * q0 + (m->act_kind[a] == 1 ? m->act_c1[a] * q1 : 0.f);
  float f = m->act_kp[a] * (clampf(ctrl, m->act_clo[a], m->act_chi[a]) - len);
  if (m->act_flim[a]) f = clampf(f, m->act_flo[a], m->act_fhi[a]);
  return f;
}

// The requested extra observables (ps_task_cfg.observables): entries [cfg.obs_base, cfg.obs_dim)
// of the row. DevModel::obsx says for each where its value comes from (OX_* << 8 | index:
// build_obs_extras in model_build.h owns the layout, the kernel only gathers). The lane-owned
// values - hand dof velocities, raw key angles, actuator force and velocity (lane = actuator),
// fingertips (lane = site), the root bodies' origins (lane = body) - are staged in LDS, in the
// Newton scratch that is dead after the substeps (as the OT term's work area), and the row is
// written lane-strided as write_obs2's part. Called only by a handle that asked for extras.
// `actf`: the actuator force to report; `tip`: lane s holds fingertip site s.
enum : int { XS_V = 0, XS_KQ = 64, XS_F = 192, XS_AV = 256, XS_TIP = 320, XS_ROOT = 352, XS_END = 358 };
__device__ __forceinline__ void write_obs_extras(const DevModel* __restrict__ m, const Cfg& cfg, Shared& S, const LaneDyn& D,
                                                 float* __restrict__ obs, int lane, float actf, const f3 tip) {
  float* xs = &S.nw.Jc[0][0];
  static_assert(XS_END <= 3 * MAXCON * YS, "extras staging area");
  static_assert(NDT <= 64 && NK <= 128 && NU <= 64 && 6 * PS_NFINGER <= XS_ROOT - XS_TIP, "extras staging slots");
  const float av = act_velocity(m, D, lane);
  wsync();
  xs[XS_V + lane] = D.v;
  xs[XS_KQ + lane] = D.kq[0];
  xs[XS_KQ + 64 + lane] = D.kq[1];
  xs[XS_F + lane] = actf;
  xs[XS_AV + lane] = av;
  if (lane < 2 * PS_NFINGER) st3(xs + XS_TIP + 3 * lane, tip);
  if (lane == 0 || lane == NB) st3(xs + XS_ROOT + (lane ? 3 : 0), ld3(D.o));
  wsync();
  const int n = cfg.obs_dim - cfg.obs_base;
  for (int i = lane; i < n; i += 64) {
    const int code = m->obsx[i], kind = code >> 8, k = code & 255;
    float val;
    if (kind == OX_KQ) {
      val = xs[XS_KQ + k];
    } else if (kind == OX_KACT) {
      val = (S.act_bits[k >> 5] >> (k & 31)) & 1 ? 1.f : 0.f;
    } else if (kind == OX_SUSACT) {
      val = S.sustain >= SUSTAIN_THRESHOLD ? 1.f : 0.f;
    } else if (kind == OX_COS || kind == OX_SIN) {
      float s, c;
      fsincos(S.dx[k][6], &s, &c);  // (the kinematics' own sine / cosine: ~1 ulp on the joint range)
      val = kind == OX_COS ? c : s;
    } else if (kind == OX_V) {
      val = xs[XS_V + k];
    } else if (kind == OX_ACTF) {
      val = xs[XS_F + k];
    } else if (kind == OX_ACTV) {
      val = xs[XS_AV + k];
    } else if (kind == OX_ACTP) {
      val = fabsf(xs[XS_F + k]) * fabsf(xs[XS_AV + k]);
    } else if (kind == OX_TIP) {
      val = xs[XS_TIP + k];
    } else {  // OX_ROOT
      val = xs[XS_ROOT + k];
    }
    obs[cfg.obs_base + i] = val;
  }
}

__device__ __forceinline__ void key_state2(const DevModel* __restrict__ m, Shared& S, const LaneDyn& D, int lane) {
  uint64_t bits[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int k = lane + 64 * j;
    bool act = false;
    if (k < NK) {
      float khi = m->key_hi[k];
      float s = clampf(D.kq[j], m->key_lo[k], khi);
      S.knorm[k] = s / khi;
      act = fabsf(s - khi) <= KEY_THRESHOLD;
    }
    bits[j] = __ballot(act);
  }
  if (lane == 0) {
    S.act_bits[0] = (int)(bits[0] & 0xffffffffull);
    S.act_bits[1] = (int)(bits[0] >> 32);
    S.act_bits[2] = (int)(bits[1] & 0xffffffull);
  }
  wsync();
}

// ------------------------------------------------------------------ the kernel
#ifndef PS_BIG_SWEEPS
#define PS_BIG_SWEEPS 2  // warm-up sweeps above 32 coupled rows (BPP exchanges are single pivots there)
#endif
#ifndef PS_WAVES_PER_EU
#define PS_WAVES_PER_EU 2
#endif
#ifndef PS_CHUNKS
#define PS_CHUNKS 6  // chunks of substeps per env-step on the time-sliced path (pianosim_queue_kernel):
                     // 10 substeps as 2 2 2 2 1 1; measured 3 to 10, profiles/r09_v1_bench_ab.txt
#endif
// WPE: resident waves per SIMD the register allocation is built for. 2 (the default): 256 VGPRs,
// the solve's overflow spilled to scratch; 1: 256 VGPRs + AGPRs, no scratch - chosen by the host
// when the launch is at most one wave per SIMD anyway (launch() below)
//
// env_step: the control step of env e by one wave, or (Q, the queue path) its chunk `chunk` of
// `chunks`: nsub / chunks substeps, one more in the first nsub % chunks chunks (the env's last
// chunk, which also runs the task layer, is never the one with more). A chunk that is not
// the env's last leaves the state live across the substep boundary in the env's park row (CW_*)
// and returns true: the caller publishes the continuation; the last chunk also runs the task
// layer and writes the outputs. Every chunk sets up what it uses (LDS words, lane constants,
// counters) itself, so any workgroup can run any chunk, and the arithmetic is the monolithic
// step's: the results do not depend on the chunk count or on who ran which chunk. !Q: the
// whole step, `chunk` / `chunks` unused (pianosim_kernel).
template <bool XG, int WPE, bool Q>
__device__ __forceinline__ bool env_step(Shared& S, const DevModel* __restrict__ m, const Song& songs, const Cfg& cfg,
                                         const Bufs& bufs, const float* __restrict__ action,
                                         const uint8_t* __restrict__ mask, float* __restrict__ obs,
                                         float* __restrict__ reward, float* __restrict__ discount,
                                         uint8_t* __restrict__ step_type, const int mode, const int e, const int lane,
                                         const int chunk, const int chunks) {
  const bool first = !Q || chunk == 0;  // the chunk that starts from the env's rows
  const Song song = song_of(songs, e);
  float* obs_e = obs + (size_t)e * cfg.obs_dim;
  bool do_reset;
  if (mode == 1) {
    if (mask && !mask[e]) return false;
    do_reset = true;
  } else {
    do_reset = first && bufs.last[e] != 0;  // (an env due for its auto-reset has one chunk only)
  }
  const float* applied = bufs.applied ? bufs.applied + (size_t)e * NV : nullptr;
  // the carried lane words and wave-uniform scalars of a continued step (Q, chunk > 0)
  const float* cw = bufs.park + (size_t)e * PARK_WORDS * 64 + lane;
  int cscal = 0;
  if (Q && !first) {
    cscal = __float_as_int(ld_wt(cw + 64 * CW_SCAL));
    // mj_resetData cleared qfrc_applied in an earlier chunk: none for the rest of the step
    if (__builtin_amdgcn_readlane(cscal, CS_NOAPPLIED)) applied = nullptr;
  }
  // randomize_hand_positions (piano_with_shadow_hands.py:491-499): one U(-0.05, 0.05) y shift
  // of both hand roots per episode, drawn at reset (counter-based: seed, env, episode)
  float hand_dy = 0.f;
  if (do_reset) {
    const int ep = bufs.episode[e];
    if (cfg.randomize) hand_dy = hand_offset_draw(cfg.seed_lo, cfg.seed_hi, (int)(cfg.env0 + (uint32_t)e), ep);
    if (lane == 0) {
      bufs.episode[e] = ep + 1;
      bufs.hand_dy[e] = hand_dy;
    }
  } else if (cfg.randomize) {
    hand_dy = bufs.hand_dy[e];
  }
  LaneStatic L;
  load_static(m, S, L, lane);
  LaneDyn D;
  const size_t rowoff = (size_t)e * NV;
  // qacc_warmstart is output only (cold-start PGS): set on the last substep, never read
  D.qws = 0.f;
#pragma unroll
  for (int j = 0; j < 2; j++) D.kws[j] = 0.f;
  if (do_reset) {
    D.q = D.v = 0.f;
    #pragma unroll
    for (int j = 0; j < 2; j++) { D.kq[j] = D.kv[j] = 0.f; }
    if (lane == 0) S.sustain = 0.f;
  } else if (Q && !first) {
    D.q = ld_wt(cw + 64 * CW_Q);
    D.v = ld_wt(cw + 64 * CW_V);
#pragma unroll
    for (int j = 0; j < 2; j++) {
      D.kq[j] = ld_wt(cw + 64 * (CW_KQ + j));
      D.kv[j] = ld_wt(cw + 64 * (CW_KV + j));
    }
  } else {
    int d = lane < NDT ? lane : 0;
    D.q = bufs.qpos[rowoff + NK + d];
    D.v = bufs.qvel[rowoff + NK + d];
    if ((m->dof_lockmask >> d) & 1ull) D.q = D.v = 0.f;  // a locked dof stays at its joint zero
#pragma unroll
    for (int j = 0; j < 2; j++) {
      int k = lane + 64 * j;
      int kk = k < NK ? k : 0;
      D.kq[j] = bufs.qpos[rowoff + kk];
      D.kv[j] = bufs.qvel[rowoff + kk];
    }
  }
  float ctrl = 0.f;  // lane = actuator
  if (!do_reset) {
    // the caller's row: the model's actuators in their columns (an absent one: ctrl 0), then
    // the sustain pedal
    const float* a_e = action + (size_t)e * m->n_action;
    const int a = lane < NU ? lane : 0;
    const int src = m->act_src[a];
    const float av = src >= 0 ? a_e[src] : 0.f;
    ctrl = cfg.canonical ? m->act_clo[a] + (av + 1.f) * 0.5f * (m->act_chi[a] - m->act_clo[a]) : av;
    if (src < 0) ctrl = 0.f;
    if (Q && !first) ctrl = ld_wt(cw + 64 * CW_CTRL);  // (0 since a physics reset of an earlier chunk)
    const float sv = a_e[m->n_action - 1];
    if (lane == 0) S.sustain = cfg.canonical ? (sv + 1.f) * 0.5f : sv;
  }
  wsync();
  float actf_last = 0.f;
  int st_solves = 0, st_concap = 0, st_cap = 0, st_maxrow = 0, st_coupled = 0, st_piv = 0, st_cdofs = 0;  // solver / cap counters
#ifdef PS_TIMING
  uint64_t tacc[NPHASE] = {0};
  uint64_t tlast = __builtin_amdgcn_s_memtime();
#endif
  int warn[PS_NWARN] = {0, 0, 0};
  if (Q && !first) {
    actf_last = ld_wt(cw + 64 * CW_ACTF);
    st_solves = __builtin_amdgcn_readlane(cscal, CS_SOLVES);
    st_concap = __builtin_amdgcn_readlane(cscal, CS_CONCAP);
    st_cap = __builtin_amdgcn_readlane(cscal, CS_CAP);
    st_maxrow = __builtin_amdgcn_readlane(cscal, CS_MAXROW);
    st_coupled = __builtin_amdgcn_readlane(cscal, CS_COUPLED);
    st_piv = __builtin_amdgcn_readlane(cscal, CS_PIV);
    st_cdofs = __builtin_amdgcn_readlane(cscal, CS_CDOFS);
    static_assert(PS_NWARN == 3, "carried warning counters");
    warn[0] = __builtin_amdgcn_readlane(cscal, CS_WARN);
    warn[1] = __builtin_amdgcn_readlane(cscal, CS_WARN + 1);
    warn[2] = __builtin_amdgcn_readlane(cscal, CS_WARN + 2);
  }
  // mj_resetData (after mj_checkPos / Vel / Acc): qpos = qpos0 (0), qvel, qacc_warmstart,
  // ctrl and qfrc_applied = 0 for the rest of the step
#define PS_RESET_PHYSICS()                                                              \
  do {                                                                                  \
    D.q = D.v = D.qws = 0.f;                                                            \
    for (int j_ = 0; j_ < 2; j_++) D.kq[j_] = D.kv[j_] = D.kws[j_] = 0.f;               \
    ctrl = 0.f;                                                                         \
    if (applied) {                                                                      \
      for (int i_ = lane; i_ < NV; i_ += 64) const_cast<float*>(applied)[i_] = 0.f;     \
      applied = nullptr;                                                                \
    }                                                                                   \
  } while (0)
  if (!do_reset) {
    bool acc_reset = false;
    NGuess guess;  // Newton: the previous substep's zones (none for the first substep of a step)
    guess.zf = guess.zl = guess.zc = 0;
    guess.cid = -2;
    guess.zk[0] = guess.zk[1] = 0;
    guess.valid = false;
    if (Q && !first) {
      guess.zf = __float_as_int(ld_wt(cw + 64 * CW_ZF));
      guess.zl = __float_as_int(ld_wt(cw + 64 * CW_ZL));
      guess.zc = __float_as_int(ld_wt(cw + 64 * CW_ZC));
      guess.cid = __float_as_int(ld_wt(cw + 64 * CW_CID));
      guess.zk[0] = __float_as_int(ld_wt(cw + 64 * CW_ZK));
      guess.zk[1] = __float_as_int(ld_wt(cw + 64 * (CW_ZK + 1)));
      guess.valid = __builtin_amdgcn_readlane(cscal, CS_GVALID) != 0;
    }
    // (acc_reset is false at every substep boundary: a substep that completes clears it)
    // (the substeps that do not divide evenly go to the first chunks: 10 in 3 = [0,4) [4,7) [7,10))
    const int s_each = Q ? m->nsub / chunks : 0, s_more = Q ? m->nsub - s_each * chunks : 0;
    const int s_begin = Q ? chunk * s_each + min(chunk, s_more) : 0;
    const int s_end = Q ? (chunk + 1) * s_each + min(chunk + 1, s_more) : m->nsub;
    for (int s = s_begin; s < (Q ? s_end : m->nsub); s++) {
      {  // mj_checkPos, mj_checkVel (mju_isBad: NaN or |x| > 1e10)
        bool bq = lane < NDT && !(fabsf(D.q) <= 1e10f), bv = false;
#pragma unroll
        for (int j = 0; j < 2; j++)
          if (lane + 64 * j < NK) bq |= !(fabsf(D.kq[j]) <= 1e10f);
        if (__ballot(bq)) { warn[PS_WARN_BADQPOS]++; PS_RESET_PHYSICS(); }
        bv = lane < NDT && !(fabsf(D.v) <= 1e10f);
#pragma unroll
        for (int j = 0; j < 2; j++)
          if (lane + 64 * j < NK) bv |= !(fabsf(D.kv[j]) <= 1e10f);
        if (__ballot(bv)) { warn[PS_WARN_BADQVEL]++; PS_RESET_PHYSICS(); }
      }
      // opaque per substep: keeps model-table loads inside the loop (no LICM of ~100
      // per-lane constants across the substeps, which would cost occupancy)
      // (an opaque zero offset rather than an opaque pointer: the pointer keeps its global
      // address space, so these stay global loads; a flat load also counts in lgkmcnt and
      // would make every later LDS wait wait for the memory round trip)
      int zoff = 0;
      asm volatile("" : "+s"(zoff));
      const DevModel* __restrict__ mq = m + zoff;
      int lq = lane;  // likewise for lane-derived LDS/global addresses
      asm volatile("" : "+v"(lq));
      kinematics2<true, XG>(mq, S, L, D, lq, hand_dy TPASS);
      TSTAMP(0);
      D.actf = ctrl;
      dynamics2(mq, S, L, D, applied, lq TPASS);
      actf_last = D.w;
      TSTAMP(1);
      if (XG) {
        // the box / hull narrow phases are out-of-line calls (x_pairs, x_refine): the dynamics'
        // lane state live across them is parked in the env's park row and the lane constants are
        // re-read after, so the calls find few live values (in registers across them this state
        // spilled through the whole substep: factor, Newton setup, integrate 1.5-2x slower)
        float* pkc = bufs.park + (size_t)e * PARK_WORDS * 64 + lq;
#pragma unroll
        for (int a = 0; a < MAXDEP; a++) {
          pkc[64 * a] = D.M[a];
          pkc[64 * (9 + a)] = D.Mh[a];
        }
        pkc[64 * 18] = D.q; pkc[64 * 19] = D.v; pkc[64 * 20] = D.qws; pkc[64 * 21] = D.qfs;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          pkc[64 * (22 + j)] = D.kq[j];
          pkc[64 * (24 + j)] = D.kv[j];
          pkc[64 * (26 + j)] = D.kws[j];
          pkc[64 * (28 + j)] = D.kqfs[j];
        }
        asm volatile("" ::: "memory");
      }
      st_concap += collide2<XG, WPE>(mq, S, cfg.maxcon, lq, L.c_r TPASS) >= cfg.maxcon;
      if (XG) {
        asm volatile("" ::: "memory");
        const float* pkc = bufs.park + (size_t)e * PARK_WORDS * 64 + lq;
#pragma unroll
        for (int a = 0; a < MAXDEP; a++) {
          D.M[a] = pkc[64 * a];
          D.Mh[a] = pkc[64 * (9 + a)];
        }
        D.q = pkc[64 * 18]; D.v = pkc[64 * 19]; D.qws = pkc[64 * 20]; D.qfs = pkc[64 * 21];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          D.kq[j] = pkc[64 * (22 + j)];
          D.kv[j] = pkc[64 * (24 + j)];
          D.kws[j] = pkc[64 * (26 + j)];
          D.kqfs[j] = pkc[64 * (28 + j)];
        }
        int zo = 0;
        asm volatile("" : "+s"(zo));
        load_static(mq + zo, S, L, lq);
      }
      TSTAMP(2);
      const bool coupled = newton_prep(mq, S, L, D, lq);
      st_coupled += coupled;
      TSTAMP(18);
      factor2(mq, S, L, D, lq);
      TSTAMP(3);
      D.qas = D.qfs;
      float dummy = 0.f;
      solve2<false>(mq, S, L, D, D.qas, dummy, lq);
#pragma unroll
      for (int j = 0; j < 2; j++) D.kqas[j] = lq + 64 * j < NK ? D.kqfs[j] * S.kminv[lq + 64 * j] : 0.f;
      TSTAMP(4);
      // key limits of keys no contact touches: 1-dof problems in closed form
      if (lq < 3) S.keyhit[lq] = 0;
      wsync();
      if (lq < S.ncon && S.con[lq].kind == 0) atomicOr(&S.keyhit[S.con[lq].key >> 5], 1 << (S.con[lq].key & 31));
      wsync();
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int k = lq + 64 * j;
        D.kfree[j] = 0.f;
        if (k < NK && !((S.keyhit[k >> 5] >> (k & 31)) & 1)) {
          const float klo = mq->key_lo[k], khi = mq->key_hi[k], kdinv = mq->key_dinv[k];
          const float dlo = D.kq[j] - klo, dhi = khi - D.kq[j];
          float pos = 0.f, sgn = 0.f;
          if (dlo < 0.f) { pos = dlo; sgn = 1.f; }
          else if (dhi < 0.f) { pos = dhi; sgn = -1.f; }
          if (sgn != 0.f) {
            const float imp = impedance(mq->lim_solimp, pos);
            const float dmax = clampf(mq->lim_solimp[1], MINIMP, MAXIMP);
            const float tc = fmaxf(mq->lim_solref[0], 2.f * mq->timestep), dr = mq->lim_solref[1];
            const float K = 1.f / (dmax * dmax * tc * tc * dr * dr), Bc = 2.f / (dmax * tc);
            const float aref = -Bc * sgn * D.kv[j] - K * imp * pos;
            const float Rk = fmaxf(MINVALF, (1.f - imp) / imp * kdinv);
            const float b = sgn * D.kqas[j] - aref;
            D.kfree[j] = sgn * fmaxf(0.f, -b / (S.kminv[k] + Rk));
          }
        }
      }
      TSTAMP(46);
      // constraint forces: primal Newton (newton.inc)
      float F, xq, kxq[2];
      // contact rows (4 pyramid edges per contact; the 52 friction-loss rows and the violated
      // limits come on top, see PS_STAT_MAX_ROWS)
      st_maxrow = max(st_maxrow, 4 * __builtin_amdgcn_readfirstlane(S.ncon));
      const int maxit = cfg.newton_cap > 0 ? cfg.newton_cap : PS_NEWTON_CAP;
      const int ncmax = max(S.nm.nc[0], S.nm.nc[1]), ncsum = S.nm.nc[0] + S.nm.nc[1];
      st_cdofs = max(st_cdofs, ncsum);
      float* pk = bufs.park + (size_t)e * PARK_WORDS * 64 + lq;
      {
#pragma unroll
        for (int a = 0; a < MAXDEP; a++) pk[64 * a] = D.Mh[a];
        pk[64 * 9] = D.Dhinv;
        pk[64 * 10] = D.qws;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          pk[64 * (11 + j)] = D.kws[j];
          pk[64 * (13 + j)] = D.kqfs[j];
          pk[64 * (15 + j)] = D.kfree[j];
        }
      }
      asm volatile("" ::: "memory");
      TSTAMP(47);
#ifdef PS_TIMING
      const int st_solves0 = st_solves;
#endif
      if (!coupled)
        st_solves += newton_solve<0, !XG>(mq, S, L, D, lq, maxit, cfg.refine, F, xq, kxq, guess, st_cap, st_piv, pk TPASS);
      else if (ncmax <= 16 && ncsum <= NSL && !cfg.full_cpl)  // (16 + 16 > NSL kappa registers)
        st_solves += newton_solve<16>(mq, S, L, D, lq, maxit, cfg.refine, F, xq, kxq, guess, st_cap, st_piv, pk TPASS);
      else
        st_solves += newton_solve<28>(mq, S, L, D, lq, maxit, cfg.refine, F, xq, kxq, guess, st_cap, st_piv, pk TPASS);
      asm volatile("" ::: "memory");
#ifdef PS_TIMING
      if (lq == 0) {  // Newton iterations: first substep (cold) / later substeps (guessed piece)
        const int its = st_solves - st_solves0;
        if (s == 0) { tacc[19] += its; tacc[20] += 1; }
        else { tacc[21] += its; tacc[22] += its == 1; tacc[23] += 1; }
      }
#endif
      {
#pragma unroll
        for (int a = 0; a < MAXDEP; a++) D.Mh[a] = pk[64 * a];
        D.Dhinv = pk[64 * 9];
        D.qws = pk[64 * 10];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          D.kws[j] = pk[64 * (11 + j)];
          D.kqfs[j] = pk[64 * (13 + j)];
          D.kfree[j] = pk[64 * (15 + j)];
        }
      }
      TSTAMP(8);
      {  // the lane constants are re-read after the solve: not live (in registers) through it
        int zo = 0;
        asm volatile("" : "+s"(zo));
        load_static(mq + zo, S, L, lq);
      }
      {  // mj_checkAcc: a bad qacc resets the env and recomputes this substep from the reset state
        bool ba = lq < NDT && !(fabsf(xq) <= 1e10f);
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int k = lq + 64 * j;
          if (k < NK) {
            const bool hit = (S.keyhit[k >> 5] >> (k & 31)) & 1;
            const float ka = hit ? kxq[j] : (D.kqfs[j] + D.kfree[j]) * S.kminv[k];
            ba |= !(fabsf(ka) <= 1e10f);
          }
        }
        if (__ballot(ba) && !acc_reset) {
          warn[PS_WARN_BADQACC]++;
          PS_RESET_PHYSICS();
          acc_reset = true;
          s--;
          continue;
        }
        acc_reset = false;
      }
      // semi-implicit Euler with implicit damping: v += h (M + hD)^-1 F (qacc = the Newton x)
      float F2 = F;
      solve2<false, true>(mq, S, L, D, F2, F, lq);
      const bool last_sub = s == mq->nsub - 1;
      const float h = mq->timestep;
      if (lq < NDT) {
        if (last_sub) D.qws = xq;
        D.v += h * F2;
        D.q += h * D.v;
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        int k = lq + 64 * j;
        if (k < NK) {
          const bool hit = (S.keyhit[k >> 5] >> (k & 31)) & 1;
          float Fk = D.kqfs[j] + (hit ? S.kw[k] : D.kfree[j]);
          if (last_sub) D.kws[j] = hit ? kxq[j] : Fk * S.kminv[k];
          D.kv[j] += h * Fk * mq->key_Mhinv[k];
          D.kq[j] += h * D.kv[j];
        }
      }
      wsync();
      if (bufs.keybits) {
        // the recorder's capture: key_state2's activation rule on this substep's key angles.
        // Nothing is kept for it: a later chunk of the step writes its own rows, and a substep
        // that mj_checkAcc redoes gets here once
        uint64_t kb[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int k = lq + 64 * j;
          bool act = false;
          if (k < NK) {
            const float khi = mq->key_hi[k];
            act = fabsf(clampf(D.kq[j], mq->key_lo[k], khi) - khi) <= KEY_THRESHOLD;
          }
          kb[j] = __ballot(act);
        }
        if (lq == 0) {
          uint32_t* row = bufs.keybits + (size_t)e * kb_stride(mq->nsub) + KB_HDR + s * KB_ROW;
          row[0] = (uint32_t)kb[0];
          row[1] = (uint32_t)(kb[0] >> 32);
          row[2] = ((uint32_t)kb[1] & 0xffffffu) | (S.sustain >= SUSTAIN_THRESHOLD ? 1u << KB_SUSTAIN_BIT : 0u);
        }
      }
      TSTAMP(6);
#ifdef PS_TIMING
      if (lq == 0) { tacc[9] += 52 + 4 * S.ncon; tacc[10] += S.ncon; }
#endif
    }
    if (Q && s_end < m->nsub) {
      // the step continues in another chunk: everything live across the substep boundary goes
      // to the env's park row (D.qws / D.kws are outputs of the last substep only; S.sustain
      // and hand_dy are re-read from the action row / the env's rows by every chunk)
      float* pw = bufs.park + (size_t)e * PARK_WORDS * 64 + lane;
      st_wt(pw + 64 * CW_Q, D.q);
      st_wt(pw + 64 * CW_V, D.v);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        st_wt(pw + 64 * (CW_KQ + j), D.kq[j]);
        st_wt(pw + 64 * (CW_KV + j), D.kv[j]);
      }
      st_wt(pw + 64 * CW_CTRL, ctrl);
      st_wt(pw + 64 * CW_ACTF, actf_last);
      st_wt(pw + 64 * CW_ZF, __int_as_float(guess.zf));
      st_wt(pw + 64 * CW_ZL, __int_as_float(guess.zl));
      st_wt(pw + 64 * CW_ZC, __int_as_float(guess.zc));
      st_wt(pw + 64 * CW_CID, __int_as_float(guess.cid));
      st_wt(pw + 64 * CW_ZK, __int_as_float(guess.zk[0]));
      st_wt(pw + 64 * (CW_ZK + 1), __int_as_float(guess.zk[1]));
      const int sc = lane == CS_SOLVES ? st_solves : lane == CS_CONCAP ? st_concap : lane == CS_CAP ? st_cap
                   : lane == CS_MAXROW ? st_maxrow : lane == CS_COUPLED ? st_coupled : lane == CS_PIV ? st_piv
                   : lane == CS_CDOFS ? st_cdofs : lane == CS_WARN ? warn[0] : lane == CS_WARN + 1 ? warn[1]
                   : lane == CS_WARN + 2 ? warn[2] : lane == CS_GVALID ? (int)guess.valid
                   : (int)(bufs.applied && !applied);  // CS_NOAPPLIED
      st_wt(pw + 64 * CW_SCAL, __int_as_float(sc));
      return true;
    }
  }
  // ---- mj_step1 at the final state + task layer
  kinematics2<false, XG>(m, S, L, D, lane, hand_dy TPASS);
  // The final state's contact list has three readers: the forearm term, ps_contact_count and
  // ps_contacts. The pass runs when contacts are recorded (con_out) or the forearm term could find
  // its contact (fore_near); otherwise it is skipped and bufs.ncon[e] is left as it was: the host
  // knows the counts are stale and materialises them when asked (pianosim_ncon_kernel).
  const bool final_con = bufs.con_out != nullptr || (!do_reset && cfg.forearm && fore_near<XG>(m, S, lane));
  if (final_con) collide2<XG, WPE>(m, S, cfg.maxcon, lane, L.c_r TPASS);
#ifdef PS_TIMING
  if (lane == 0 && !do_reset) { tacc[TS_FINAL] += 1; tacc[TS_FINAL_SKIP] += !final_con; }
#endif
  key_state2(m, S, D, lane);
  // the one-hand task's <rh|lh>_shadow_hand/position: the kept hand's root body (hands/base.py:
  // 112-114); its lane is the body's (as site_world2)
  f3 root = mk3(0, 0, 0);
  if (cfg.hand) {
    const int B = (cfg.hand - 1) * NB;
    root = mk3(__shfl(D.o[0], B, 64), __shfl(D.o[1], B, 64), __shfl(D.o[2], B, 64));
  }
  if (do_reset) {
    write_obs2(m, song, cfg, S, 0, obs_e, lane, root);
    if (lane < NDT) {
      bufs.qpos[rowoff + NK + lane] = 0.f;
      bufs.qvel[rowoff + NK + lane] = 0.f;
      bufs.qws[rowoff + NK + lane] = 0.f;
    }
    for (int k = lane; k < NK; k += 64) {
      bufs.qpos[rowoff + k] = 0.f;
      bufs.qvel[rowoff + k] = 0.f;
      bufs.qws[rowoff + k] = 0.f;
    }
    if (lane < NU) bufs.ctrl[(size_t)e * NU + lane] = 0.f;
    if (lane < PS_NTERMS) bufs.terms[(size_t)e * PS_NTERMS + lane] = 0.f;
    if (lane < PS_NMUSIC) bufs.mus_acc[(size_t)e * PS_NMUSIC + lane] = 0.f;  // a new episode
    f3 tip_own = mk3(0, 0, 0);
    for (int s = 0; s < 2 * PS_NFINGER; s++) {
      f3 p = site_world2(m, D, s);
      if (lane == s) tip_own = p;
    }
    if (lane < 2 * PS_NFINGER) st3(bufs.tips + ((size_t)e * 2 * PS_NFINGER + lane) * 3, tip_own);
    // the extras of a reset row: mj_forward at the reset state with ctrl = 0 (velocities 0)
    if (cfg.obs_dim > cfg.obs_base) write_obs_extras(m, cfg, S, D, obs_e, lane, act_force(m, D, 0.f, lane), tip_own);
    if (lane < PS_NSTATS) bufs.stats[(size_t)e * PS_NSTATS + lane] = 0;
    if (lane == 0) {
      bufs.sustain[e] = 0.f;
      bufs.t_idx[e] = 0;
      bufs.last[e] = 0;
      if (final_con) bufs.ncon[e] = S.ncon;
      if (bufs.keybits) bufs.keybits[(size_t)e * kb_stride(m->nsub)] = KB_NEW_EPISODE;
      if (mode == 0) {
        reward[e] = 0.f;
        discount[e] = 1.f;
        step_type[e] = PS_FIRST;
      }
    }
    return false;
  }
  const int t_cur = bufs.t_idx[e];
  const int t_new = t_cur + 1;
  const float* gc = song.goal + (size_t)t_cur * (NK + 1);
  float on_tol = 0.f, on_cnt = 0.f;
  bool fail_l = false;
  for (int k = lane; k < NK; k += 64) {
    float g = gc[k];
    bool act = (S.act_bits[k >> 5] >> (k & 31)) & 1;
    if (g != 0.f) { on_tol += tolerance(g - S.knorm[k], 0.f, 0.05f, 0.5f); on_cnt += 1.f; }
    else if (act) fail_l = true;
  }
  float sum_tol = wave_sum(on_tol), n_on = wave_sum(on_cnt);
  bool failure = __ballot(fail_l) != 0ull;
  // MidiEvaluationWrapper (wrappers/evaluation.py:114-177): this step's key activation vs
  // the notes of step t_cur (the goal row), binary precision / recall / F1, zero_division 1
  float mus[PS_NMUSIC];
  {
    int tp = 0, fp = 0, fn = 0;
    for (int k = lane; k < NK; k += 64) {
      const bool g = gc[k] != 0.f, a = (S.act_bits[k >> 5] >> (k & 31)) & 1;
      tp += g && a;
      fp += !g && a;
      fn += g && !a;
    }
    tp = wave_sum_i(tp);
    fp = wave_sum_i(fp);
    fn = wave_sum_i(fn);
    prf(tp, fp, fn, mus);
    const bool sg = gc[NK] != 0.f, sa = S.sustain >= SUSTAIN_THRESHOLD;
    prf(sg && sa, !sg && sa, sg && !sa, mus + 3);
  }
  float kp = (n_on > 0.f ? 0.5f * (sum_tol / n_on) : 0.f) + 0.5f * (1.f - (failure ? 1.f : 0.f));
  float sus = tolerance(gc[NK] - (S.sustain >= SUSTAIN_THRESHOLD ? 1.f : 0.f), 0.f, 0.05f, 0.5f);
  float en = 0.f;
  {
    const float vel = act_velocity(m, D, lane);
    if (lane < NU) en = fabsf(actf_last) * fabsf(vel);
  }
  float energy = -cfg.energy_coef * wave_sum(en);
  // fingertip sites (all lanes gather; lane s keeps site s)
  f3 tip_own = mk3(0, 0, 0);
  for (int s = 0; s < 2 * PS_NFINGER; s++) {
    f3 p = site_world2(m, D, s);
    if (lane == s) tip_own = p;
  }
  float fing = 0.f;
  if (cfg.fingering) {
    float ds = 0.f, dc = 0.f;
    int cnt = song.count[t_cur];
    int f = lane < cnt ? song.fingers[t_cur * PS_MAX_NOTES + lane] : 0;
    int k = lane < cnt ? song.keys[t_cur * PS_MAX_NOTES + lane] : 0;
    bool rh = f < 5;
    int site = (rh ? 0 : 1) * PS_NFINGER + (rh ? (f < 0 ? f + 5 : f) : f - 5);
    float tx = __shfl(tip_own.x, site, 64), ty = __shfl(tip_own.y, site, 64), tz = __shfl(tip_own.z, site, 64);
    // the one-hand task: the kept hand's fingered notes only (piano_with_one_shadow_hand.py:244-275,
    // 304-313)
    if (lane < cnt && (!cfg.hand || rh == (cfg.hand == 1))) {
      ds = tolerance(norm3(key_target2(m, S, k) - mk3(tx, ty, tz)), 0.f, 0.01f, 0.1f);
      dc = 1.f;
    }
    float s = wave_sum(ds), c = wave_sum(dc);
    fing = c > 0.f ? s / c : 0.f;
  } else if (!cfg.hand) {  // (the one-hand task has no OT term: slot 3 stays 0)
    // ot_fingering (piano_with_shadow_hands.py:333-369): goal keys by ballot (ps_create rejects
    // a song with more than PS_MAX_NOTES goal keys in a step, so the min below never binds),
    // the K x 10 distance matrix lane-parallel, the assignment on lane 0 with its work arrays
    // in LDS (the Delassus area is dead after the substeps)
    float* owa = &S.nw.Jc[0][0];  // the Newton scratch is dead after the substeps
    int* okeys = reinterpret_cast<int*>(owa);
    float* ocost = owa + PS_MAX_NOTES;
    float* owork = ocost + 10 * PS_MAX_NOTES;
    static_assert(PS_MAX_NOTES + 10 * PS_MAX_NOTES + 6 * (PS_MAX_NOTES + 1) <= 3 * MAXCON * YS, "OT work area");
    int K = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int k = lane + 64 * j;
      const bool on = k < NK && gc[k] != 0.f;
      const uint64_t mk = __ballot(on);
      const int pos = K + lanes_below(mk, lane);
      if (on && pos < PS_MAX_NOTES) okeys[pos] = k;
      K += __popcll(mk);
    }
    K = min(K, PS_MAX_NOTES);
    wsync();
    float res = 1.f;
    if (K > 0) {
      // fingertips: lh first, then rh (row/column i < 5 -> site PS_NFINGER + i)
      for (int t0 = 0; t0 < 10 * K; t0 += 64) {
        const int t = t0 + lane;
        const int j = min(t / 10, K - 1), i = t - 10 * (t / 10);
        const int site = i < 5 ? PS_NFINGER + i : i - 5;
        const float tx = __shfl(tip_own.x, site, 64), ty = __shfl(tip_own.y, site, 64), tz = __shfl(tip_own.z, site, 64);
        const float dcost = norm3(key_target2(m, S, okeys[j]) - mk3(tx, ty, tz));
        if (t < 10 * K) ocost[K <= 10 ? j * 10 + i : i * K + j] = dcost < 1e30f ? dcost : 1e30f;  // NaN -> finite
      }
      wsync();
      if (lane == 0) res = K <= 10 ? hungarian_tol(K, 10, ocost, owork) / K : hungarian_tol(10, K, ocost, owork) / 10.f;
    }
    fing = rdlane(res, 0);
  }
  float fore = 0.f;
  if (cfg.forearm) {
    bool hit = false;
    if (final_con && lane < S.ncon) {  // (no pass: fore_near found no root-body pair near)
      const Contact& cc = S.con[lane];
      if (cc.kind == 2) {
        // rh root-body geom against lh root-body geom (piano_with_shadow_hands.py:251-259)
        const int b1 = m->geom_body[cc.g1], b2 = m->geom_body[cc.g2];
        hit = b1 % NB == 0 && b2 % NB == 0 && b1 != b2;
      }
    }
    fore = __ballot(hit) ? 0.f : 0.5f;
  }
  bool terminal = t_new == song.T;
  float disc = 1.f;
  if (!terminal && cfg.wrong_press && failure) { terminal = true; disc = 0.f; }
  write_obs2(m, song, cfg, S, t_new < song.T ? t_new : t_new - 1, obs_e, lane, root);
  if (cfg.obs_dim > cfg.obs_base) write_obs_extras(m, cfg, S, D, obs_e, lane, actf_last, tip_own);
  if (lane < NDT) {
    bufs.qpos[rowoff + NK + lane] = D.q;
    bufs.qvel[rowoff + NK + lane] = D.v;
    bufs.qws[rowoff + NK + lane] = D.qws;
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    int k = lane + 64 * j;
    if (k < NK) {
      bufs.qpos[rowoff + k] = D.kq[j];
      bufs.qvel[rowoff + k] = D.kv[j];
      bufs.qws[rowoff + k] = D.kws[j];
    }
  }
  if (lane < NU) bufs.ctrl[(size_t)e * NU + lane] = ctrl;
  if (lane < PS_NWARN && (warn[0] | warn[1] | warn[2]))
    bufs.warnings[(size_t)e * PS_NWARN + lane] += lane == 0 ? warn[0] : lane == 1 ? warn[1] : warn[2];
  if (lane < 2 * PS_NFINGER) st3(bufs.tips + ((size_t)e * 2 * PS_NFINGER + lane) * 3, tip_own);
  if (lane < PS_NSTATS)
    bufs.stats[(size_t)e * PS_NSTATS + lane] = lane == 0 ? st_solves : lane == 1 ? st_concap : lane == 2 ? st_cap
                                               : lane == 3 ? st_maxrow : lane == 4 ? st_coupled
                                               : lane == 5 ? st_piv : st_cdofs;
  if (lane == 0) {
    float* tm = bufs.terms + (size_t)e * PS_NTERMS;
    tm[0] = kp; tm[1] = sus; tm[2] = energy; tm[3] = fing; tm[4] = fore;
    reward[e] = kp + sus + energy + fing + fore;
    discount[e] = disc;
    step_type[e] = terminal ? PS_LAST : PS_MID;
    float* ma = bufs.mus_acc + (size_t)e * PS_NMUSIC;
#pragma unroll
    for (int i = 0; i < PS_NMUSIC; i++) ma[i] += mus[i];
    if (terminal) {  // episode metrics = mean over its steps (t_new of them)
      float* me = bufs.mus_ep + (size_t)e * PS_NMUSIC;
      const float inv = 1.f / (float)t_new;
#pragma unroll
      for (int i = 0; i < PS_NMUSIC; i++) me[i] = ma[i] * inv;
      bufs.mus_cnt[e] += 1;
    }
    bufs.sustain[e] = S.sustain;
    bufs.t_idx[e] = t_new;
    bufs.last[e] = terminal ? 1 : 0;
    if (final_con) bufs.ncon[e] = S.ncon;
    if (bufs.keybits) bufs.keybits[(size_t)e * kb_stride(m->nsub)] = (uint32_t)m->nsub;
  }
  if (bufs.con_out) {  // inspection copy of the contact list (ps_contacts)
    constexpr int CW = (int)(sizeof(Contact) / sizeof(int));
    const int* src = reinterpret_cast<const int*>(S.con);
    int* dst = reinterpret_cast<int*>(bufs.con_out) + (size_t)e * MAXCON * CW;
    for (int w = lane; w < S.ncon * CW; w += 64) dst[w] = src[w];
  }
#ifdef PS_TIMING
  TSTAMP(5);  // final kinematics + collide + task layer + writes
  if (lane == 0 && g_timing)
    for (int i = 0; i < NPHASE; i++) g_timing[(size_t)e * NPHASE + i] += tacc[i];
#endif
  return false;
}

// One workgroup per env, the whole step (or reset, mode 1) of env order[blockIdx.x].
template <bool XG, int WPE = PS_WAVES_PER_EU>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) pianosim_kernel(const DevModel* __restrict__ m, Song song, Cfg cfg, Bufs bufs,
                                                      const float* __restrict__ action, const uint8_t* __restrict__ mask,
                                                      float* __restrict__ obs, float* __restrict__ reward,
                                                      float* __restrict__ discount, uint8_t* __restrict__ step_type,
                                                      int mode, int n_envs, const int* __restrict__ order) {
#ifdef PS_DYN_LDS  // (experiment builds: LDS size set at launch)
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  Shared& S = *reinterpret_cast<Shared*>(smem_);
#else
  __shared__ Shared S;
#endif
  const int e = order ? order[blockIdx.x] : (int)blockIdx.x;
  const int lane = threadIdx.x;
  if (e >= n_envs) return;
  env_step<XG, WPE, false>(S, m, song, cfg, bufs, action, mask, obs, reward, discount, step_type, mode, e, lane, 0, 1);
}

// The contact counts of the envs' current state rows, on demand (ps_contact_count after steps or
// resets that skipped the final-state pass): the rows hold the lane state env_step's final
// kinematics2 + collide2 had, so this is that pass, and bufs.ncon[e] the count it would have
// written. One workgroup per env.
template <bool XG>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PS_WAVES_PER_EU))) pianosim_ncon_kernel(
    const DevModel* __restrict__ m, Cfg cfg, Bufs bufs, int n_envs) {
  __shared__ Shared S;
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= n_envs) return;
#ifdef PS_TIMING
  uint64_t tacc[NPHASE] = {0};
  uint64_t tlast = 0;
#endif
  LaneStatic L;
  load_static(m, S, L, lane);
  LaneDyn D;
  const size_t rowoff = (size_t)e * NV;
  D.v = 0.f;
  D.q = bufs.qpos[rowoff + NK + (lane < NDT ? lane : 0)];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int k = lane + 64 * j;
    D.kq[j] = bufs.qpos[rowoff + (k < NK ? k : 0)];
    D.kv[j] = 0.f;
  }
  const float hand_dy = cfg.randomize ? bufs.hand_dy[e] : 0.f;
  wsync();
  kinematics2<false, XG>(m, S, L, D, lane, hand_dy TPASS);
  collide2<XG, PS_WAVES_PER_EU>(m, S, cfg.maxcon, lane, L.c_r TPASS);
  if (lane == 0) bufs.ncon[e] = S.ncon;
}

enum : int { QC_HEAD = 0, QC_WORDS = 32 };  // (the ticket counter on a line of its own)
#ifndef PS_TIMING  // (the timing build's per-env accumulators are those of whole steps)
// The step of a launch of more envs than resident wave slots, time-sliced: the grid is the
// resident slots, and every workgroup takes (env, chunk) items off a queue in global memory
// until the tickets run out. Every item's slot is known in advance: (chunk c, rank r) lives at
// queue[c * n + r], r = rank[env] the env's position in order_kernel's order of this step
// (longest expected first). order_kernel has written the n chunk-0 items (queue[0..n)), set
// queue[n..cap) to QE_NONE (unpublished) and ctr[QC_HEAD] = the grid (workgroup b starts with
// item b). Tickets t = ctr[QC_HEAD]++ walk the slots in that order - round 0 by rank, round 1
// by rank, ... - so in every round the envs expected longest are picked up first and the items
// that end the launch are the short ones. (With tail append - every continuation at
// ctr[tail]++ - the queue was in completion order from round 1 on: every env's next chunk
// waited behind a whole batch, the expensive envs' as long as any, and the launch ended 1 ms
// after the first workgroup found the queue empty, on the longest last chunks;
// profiles/r09_v1_queue_trace_parent.txt.)
//
// No workgroup ever waits for another, and every loop is bounded by the ticket count. A pop
// takes a ticket t and EXCHANGES queue[t] with QE_LEFT: it gets the item, or (QE_NONE: the env
// is behind its schedule, or has no such chunk - an env due for its auto-reset has one) takes
// the next ticket; at t >= cap the workgroup EXITS: at most cap + grid tickets are taken in a
// launch. A publisher exchanges its item into its slot: if it gets QE_LEFT back, the ticket's
// holder has passed and nobody else will ever read the slot, so the publisher runs the item
// itself, at once: an env behind its schedule stays on its workgroup and waits for nobody. The
// exchange decides every slot for exactly one of the two sides, so no item is orphaned and
// none runs twice, and whoever holds an item is running.
// (A compare-and-swap pop of the head - read head, read entry, swap - was measured first: under
// 2048 workgroups it succeeds once per round trip, 2-4 us per item, and the 4096-env step took
// 22 ms against 5.5 ms.)
//
// Hand-off (per-XCD L2s are not coherent with each other, a CU's L1 is not refreshed by other
// CUs' stores): the carried words are stored write-through (st_wt), the wave drains its stores,
// then lane 0 exchanges the item in; the consumer's lane 0 gets the item by its exchange, then
// one agent-scope acquire (the L1 invalidate) and the wave barrier come before the env's rows
// are read, the carried words again past L1 (ld_wt). No agent-scope release fence: it writes
// back the XCD's whole L2, which here holds every resident wave's scratch - measured, a release
// per chunk boundary and per pop made the 4096-env step 16x slower (89 ms). Nothing else is
// handed over inside a launch: the env's other rows are read by its first chunk and written by
// its last.
enum : int { QE_NONE = -1, QE_LEFT = -2 };
// The queue kernel's one parameter: it sits at offset 0 of the kernel-argument segment, and the
// item loop reads it there (below).
struct QArgs {
  const DevModel* m;
  Song song;
  Cfg cfg;
  Bufs bufs;
  const float* action;
  float *obs, *reward, *discount;
  uint8_t* step_type;
  int n_envs;
  int *queue, *ctr;
  int cap, chunks;
  const int* rank;
#ifdef PS_QTRACE
  unsigned long long* trace;  // the trace build's records (QT_*), zeroed before every launch
#endif
};
// The trace build (-DPS_QTRACE, libpianosim_qtrace.so, tools/queue_trace.py): lane 0 records, for
// every item run, QT_ITEM words at trace[(chunk * n + env) * QT_ITEM] - the 100 MHz clock when
// its workgroup turned to the queue (or to the item it already held), when the chunk began and
// when it ended (stores drained), and ticket << 32 | workgroup (ticket -1: not popped, the
// workgroup's first item or a continuation it ran itself) - and for every workgroup, behind the
// cap items, QT_EXIT words: when it left, and the tickets it took that held no item. The
// product build has none of this.
enum : int { QT_ITEM = 4, QT_EXIT = 2 };
#ifdef PS_QTRACE
#define QT(...) __VA_ARGS__
#else
#define QT(...)
#endif
// Nothing is item-invariant in the loop: every trip reads what it uses - and what env_step
// receives - through a pointer to the kernel-argument segment that an empty asm makes opaque,
// and takes its lane id through another. With `a` = the parameter itself the compiler hoists
// the address arithmetic and lane constants derived from the arguments and the lane id out of
// the loop, has no registers for them across the step body, and spills them: +592 B of scratch
// per lane in both instantiations, ~160 more VGPR spills (measured; DESIGN.md section 5). Through
// the opaque pointer the arguments are scalar loads (constant address space, the pointer is
// uniform) where the body first uses them, and only the pointer itself is live across the back
// edge: 219 fewer SGPR spills than with the arguments held from the prologue.
template <bool XG>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PS_WAVES_PER_EU))) pianosim_queue_kernel(
    const QArgs ka) {
  __shared__ Shared S;
  typedef __attribute__((address_space(4))) const QArgs* KArgs;
  const uint64_t kbase = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  // the first item: queue[blockIdx.x] (grid <= n_envs; written by order_kernel)
  int own = ka.queue[blockIdx.x];  // an item this workgroup already holds, or QE_NONE: pop one
  for (;;) {
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    uint64_t kp = kbase;
    asm volatile("" : "+s"(kp));
    const QArgs& a = *(const QArgs*)(KArgs)kp;
    int item = own;
    QT(const unsigned long long qt_turn = __builtin_amdgcn_s_memrealtime(); int qt_ticket = -1;)
    if (own < 0 && lane == 0) {
      for (;;) {  // (every trip takes a ticket: at most cap + grid trips in the whole launch)
        const int t = __hip_atomic_fetch_add(&a.ctr[QC_HEAD], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        QT(qt_ticket = t;)
        if (t >= a.cap) break;
        item = __hip_atomic_exchange(&a.queue[t], QE_LEFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (item >= 0) break;
        QT(a.trace[(size_t)a.cap * QT_ITEM + blockIdx.x * QT_EXIT + 1] += 1;)
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the acquire's invalidate has completed)
    item = __builtin_amdgcn_readfirstlane(item);
    // opaque per item: nothing derived from the env is hoisted across items
    asm volatile("" : "+s"(item));
    wsync();
    if (item < 0) {
      QT(if (lane == 0) a.trace[(size_t)a.cap * QT_ITEM + blockIdx.x * QT_EXIT] = __builtin_amdgcn_s_memrealtime();)
      return;
    }
    const int e = item >> 4, chunk = item & 15;
    if (e >= a.n_envs) return;  // (never: order_kernel and the continuations write valid items only)
    QT(if (lane == 0) {
      unsigned long long* rec = a.trace + ((size_t)chunk * a.n_envs + e) * QT_ITEM;
      rec[0] = qt_turn;
      rec[1] = __builtin_amdgcn_s_memrealtime();
      rec[3] = (unsigned long long)(unsigned)qt_ticket << 32 | blockIdx.x;
    })
    const bool more = env_step<XG, PS_WAVES_PER_EU, true>(S, a.m, a.song, a.cfg, a.bufs, a.action, nullptr, a.obs, a.reward,
                                                          a.discount, a.step_type, 0, e, lane, chunk, a.chunks);
    // (uniform: the whole wave returns the same) every lane's write-through stores have completed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wsync();
    QT(if (lane == 0) a.trace[((size_t)chunk * a.n_envs + e) * QT_ITEM + 2] = __builtin_amdgcn_s_memrealtime();)
    own = QE_NONE;
    if (more) {
      const int next = (e << 4) | (chunk + 1);
      int old = QE_NONE;
      if (lane == 0) {
        const int slot = (chunk + 1) * a.n_envs + a.rank[e];
        // (slot < cap always: chunk + 1 < chunks, rank < n; past it the item stays here)
        old = (unsigned)slot < (unsigned)a.cap
                  ? __hip_atomic_exchange(&a.queue[slot], next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : (int)QE_LEFT;
      }
      if (__builtin_amdgcn_readfirstlane(old) == QE_LEFT) own = next;
    }
    wsync();  // the next item's LDS writes come after this chunk's reads
  }
}
#endif
