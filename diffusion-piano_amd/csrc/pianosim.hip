// pianosim.hip - MI355X (gfx950) batched PianoWithShadowHands step/reset + C-ABI.
//
// Device code: prims.h (math, wave primitives, narrow phase) and kernel_v2.inc (the
// step kernel, one wavefront per env, lane-owned registers, LDS for exchange only).
// The algorithm and every result-affecting ordering are stated sequentially in the CPU
// checker; this file adds the host side: buffers, launches, and the extern "C"
// entry points of include/pianosim.h. Descriptor -> device tables: model_build.h (host only).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "devmodel.h"
#include "model_build.h"
#include "render_build.h"
#include "prims.h"
#include "collide_x.h"

using namespace ps;

#include "kernel_v2.inc"
#include "augment.inc"
#include "midi_events.inc"

// ------------------------------------------------------------------ host side
static thread_local std::string g_err;
static int fail(const std::string& s) {
  g_err = s;
  return -1;
}
#define HIPCHK(x)                                                                    \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The owner of device memory: every buffer of a handle is allocated through one of these and
// freed by its destructor (or clear()), on whatever path the handle or a half-built one leaves.
struct DevMem {
  std::vector<void*> mem;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { clear(); }
  void clear() {
    for (void* p : mem) (void)hipFree(p);
    mem.clear();
  }
  template <class T>
  hipError_t alloc(T*& ptr, size_t count, bool zero) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, sizeof(T) * count);
    if (e != hipSuccess) return e;
    mem.push_back(p);
    ptr = static_cast<T*>(p);
    return zero ? hipMemset(p, 0, sizeof(T) * count) : hipSuccess;
  }
  template <class T>
  hipError_t upload(T*& ptr, const void* host, size_t count) {  // a buffer with a copy of the host's
    const hipError_t e = alloc(ptr, count, false);
    return e != hipSuccess ? e : hipMemcpy(ptr, host, sizeof(T) * count, hipMemcpyHostToDevice);
  }
};

struct ps_env {
  int n, device, obs_dim, action_dim;
  int obs_base;             // the default part of obs_dim; the rest: ps_task_cfg.observables
  int64_t env_offset;       // global id of local env 0 (Philox key of the per-env draws)
  int full_cpl;             // PIANOSIM_DEBUG_FULL_COUPLED: every coupled solve on the 28-column C block
  ps_task_cfg cfg;
  DevModel* d_model;
  int T;
  float* d_goal;
  int *d_count, *d_keys, *d_fingers;
  float *qpos, *qvel, *qws, *ctrl, *sustain, *applied, *terms, *tips;
  int *t_idx, *ncon;
  float *mus_acc, *mus_ep;  // MidiEvaluationWrapper: running sums of this episode, last episode
  int* mus_cnt;             // finished episodes per env
  int* order;               // dispatch order of the step launch (longest-expected first)
  bool ordered;
  uint8_t* last;
  bool applied_on;
  float* hand_dy;           // randomize_hand_positions: this episode's y shift of both hands
  int* episode;             // resets so far per env (the draw counter)
  int* stats;               // [N][PS_NSTATS] solver / cap counters of the last step
  int* warnings;            // [N][PS_NWARN] physics warnings since create
  float* park;              // [N][PARK_WORDS][64] kernel scratch (lane state around the Newton solve,
                            // and between the chunks of a time-sliced step)
  uint64_t seed;
  bool has_x;               // box / hull colliders: the pianosim_kernel<true> instantiation
  int wave_slots;           // SIMDs of the device: a step launch of at most this many envs runs one
                            // wave per SIMD and takes the one-wave (no-scratch) instantiation
  // the time-sliced step (pianosim_queue_kernel): chunks per env-step (0: never), the grid
  // (resident wave slots, or PIANOSIM_STEP_GRID), whether PIANOSIM_CHUNKS forces it for every n
  int chunks, step_grid;
  bool chunks_forced;
  int *queue, *qctr;        // [chunks][n] items (round, rank), [QC_WORDS] the ticket counter
  int* qrank;               // [n] env -> its position in order_kernel's order of this step
  uint64_t* qtrace;         // -DPS_QTRACE: [n * chunks][QT_ITEM] + [grid][QT_EXIT] (ps_debug_qtrace)
  Contact* con_out;         // [N][MAXCON] contact lists of the last step (ps_record_contacts)
  // ncon is lazy: a step or reset launch without contact recording may skip the final-state
  // collision pass (env_step) and then leaves its envs' counts unwritten. ncon_stale: set by such
  // a launch, cleared by materialise_ncon (the pass alone, from the state rows). ncon_sticky: such
  // a launch was captured into a graph - replays set no flag, so the counts stay stale for good
  bool ncon_stale, ncon_sticky;
  // per-episode MIDI augmentations (ps_set_augmentations): the device bank and per-env tables,
  // the builder's dynamic LDS bytes
  bool aug_on;
  AugDev aug;
  size_t aug_lds;
  // the MIDI recorder (ps_record_midi): the step kernel's capture rows [N][KB_HDR + nsub * KB_ROW]
  // (null: not recording), the event banks and per-env words behind them
  int nsub;
  uint32_t* keybits;
  MidiRec midi;
  // the device allocations: the handle's own (freed with it), the augmentation bank's (replaced
  // by ps_set_augmentations), con_out (switched by ps_record_contacts), the MIDI recorder's
  // (replaced or freed by ps_record_midi)
  DevMem mem, aug_mem, con_mem, midi_mem;
  // counts the calls that changed the set of per-env buffers (ps_set_augmentations, ps_record_midi,
  // ps_record_contacts): a snapshot lists the buffers of one generation (snapshot.inc)
  uint64_t row_gen;
  // the ray caster (render.inc), all made by the handle's first ps_render: the hulls' face planes
  // [NXT][HULL_MAXPLANE] float4 and their counts, the tile-list counter, and the scene scratch of
  // r_rec_cap selected envs (no per-env state: not snapshot rows)
  bool r_ready;
  float* r_planes;
  int* r_nplane;
  unsigned long long* r_stat;
  float* r_rec;
  size_t r_rec_cap;
  DevMem render_mem, render_rec_mem;
};

// Every entry point that touches device memory or launches binds the handle's device for its
// duration and restores the caller's afterwards: two handles on two GPUs in one process, or a
// null/default stream, never reach the wrong device ("handles are independent", pianosim.h).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
#define GUARD(E)                                                                  \
  DeviceGuard guard_((E)->device);                                                \
  if (!guard_.ok) return fail("hipSetDevice(" + std::to_string((E)->device) + ") failed")

#include "snapshot.inc"
#include "render.inc"

// n elements device to device on the stream; a null caller pointer (dst or src) skips the copy
template <class T>
static int copy_dd(T* dst, const T* src, size_t n, void* stream) {
  if (!dst || !src) return 0;
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// the builder of an augmented handle, before the step / reset kernel that reads its rows
static int launch_builder(ps_env* E, int mode, const uint8_t* mask, const int* f_song, const double* f_factor,
                          const int* f_shift, void* stream) {
  hipLaunchKernelGGL(song_build_kernel, dim3(E->n), dim3(64), E->aug_lds, (hipStream_t)stream, E->aug, mode, mask,
                     E->last, E->episode, (uint32_t)E->seed, (uint32_t)(E->seed >> 32), (uint32_t)E->env_offset, E->n,
                     f_song, f_factor, f_shift);
  HIPCHK(hipGetLastError());
  return 0;
}

// the recorder's compaction, after the step / reset kernel that wrote the capture rows
static int launch_midi(ps_env* E, void* stream) {
  const size_t stride = (size_t)KB_HDR + (size_t)E->nsub * KB_ROW;
  hipLaunchKernelGGL(midi_events_kernel, dim3(E->n), dim3(64), 0, (hipStream_t)stream, E->midi,
                     (const uint32_t*)E->keybits + KB_HDR, stride, E->keybits, stride, 0, E->n);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

const char* ps_last_error(void) { return g_err.c_str(); }
// 4: ps_task_cfg.struct_size; 5: ps_task_cfg.hand_side; 6: ps_record_midi; 7: ps_task_cfg.observables;
// 8: ps_snapshot_*; 9: ps_render
int ps_version(void) { return 9; }
int ps_model_desc_size(void) { return (int)sizeof(ps_model_desc); }
int ps_obs_dim(const ps_task_cfg* cfg) {
  std::string err;
  const int dim = obs_dim(cfg, err);
  return dim < 0 ? fail(err) : dim;
}

#ifdef PS_QTRACE
static int qtrace_grid(const ps_env* E) { return E->n < E->step_grid ? E->n : E->step_grid; }
static size_t qtrace_words(const ps_env* E) {
  return (size_t)E->n * E->chunks * QT_ITEM + (size_t)qtrace_grid(E) * QT_EXIT;
}
#endif

int ps_create(const ps_model_desc* model, const ps_song_desc* song, const ps_task_cfg* cfg, int n_envs, int device,
              uint64_t seed, ps_env** out) {
  if (!model || !song || !cfg || !out) return fail("null argument");
  // the arguments and the model are checked, and the device tables built, on the host alone
  // (model_build.h): a bad descriptor is refused before the device is touched
  std::string err;
  if (check_create_args(model, song, cfg, n_envs, err)) return fail(err);
  std::unique_ptr<DevModel> hm(new DevModel);
  if (build_dev_model(model, hm.get(), cfg->hand_side, err)) return fail(err);
  DeviceGuard guard_(device);
  if (!guard_.ok) return fail("hipSetDevice(" + std::to_string(device) + ") failed");
  // every early return below frees what E->mem holds so far, on the handle's device
  std::unique_ptr<ps_env> E(new ps_env());
  E->n = n_envs;
  E->device = device;
  E->cfg = *cfg;
  // the model's joints_pos entries (the one-hand task: the kept hand's), then the extras asked for
  build_obs_extras(hm.get(), cfg->observables, cfg->hand_side);
  E->obs_base = obs_base_dim(cfg, hm->n_obsj);
  E->obs_dim = E->obs_base + hm->n_obsx;
  E->action_dim = hm->n_action;
  E->has_x = hm->nx > 0 || hm->nxpairs > 0;
  E->T = song->T;
  E->nsub = model->n_substeps;
  E->seed = seed;
  const size_t N = (size_t)n_envs, T = (size_t)song->T;
  DevMem& mem = E->mem;
  HIPCHK(mem.upload(E->d_model, hm.get(), 1));
  hm.reset();
  HIPCHK(mem.upload(E->d_goal, song->goal, T * (NK + 1)));
  HIPCHK(mem.upload(E->d_count, song->count, T));
  HIPCHK(mem.upload(E->d_keys, song->keys, T * PS_MAX_NOTES));
  HIPCHK(mem.upload(E->d_fingers, song->fingers, T * PS_MAX_NOTES));
  HIPCHK(mem.alloc(E->qpos, N * NV, true));
  HIPCHK(mem.alloc(E->qvel, N * NV, true));
  HIPCHK(mem.alloc(E->qws, N * NV, true));
  HIPCHK(mem.alloc(E->applied, N * NV, true));
  HIPCHK(mem.alloc(E->ctrl, N * NU, true));
  HIPCHK(mem.alloc(E->sustain, N, true));
  HIPCHK(mem.alloc(E->terms, N * PS_NTERMS, true));
  HIPCHK(mem.alloc(E->tips, N * 2 * PS_NFINGER * 3, true));
  HIPCHK(mem.alloc(E->t_idx, N, true));
  HIPCHK(mem.alloc(E->ncon, N, true));
  HIPCHK(mem.alloc(E->mus_acc, N * PS_NMUSIC, true));
  HIPCHK(mem.alloc(E->mus_ep, N * PS_NMUSIC, true));
  HIPCHK(mem.alloc(E->mus_cnt, N, true));
  HIPCHK(mem.alloc(E->last, N, true));
  HIPCHK(mem.alloc(E->hand_dy, N, true));
  HIPCHK(mem.alloc(E->episode, N, true));
  HIPCHK(mem.alloc(E->stats, N * PS_NSTATS, true));
  HIPCHK(mem.alloc(E->warnings, N * PS_NWARN, true));
  // (written before they are read: order and the queue by order_kernel, park by the step kernels)
  HIPCHK(mem.alloc(E->order, N, false));
  HIPCHK(mem.alloc(E->park, N * PARK_WORDS * 64, false));
  E->ordered = !(getenv("PIANOSIM_NO_ORDER") && atoi(getenv("PIANOSIM_NO_ORDER")));
  E->full_cpl = getenv("PIANOSIM_DEBUG_FULL_COUPLED") && atoi(getenv("PIANOSIM_DEBUG_FULL_COUPLED"));
  {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    E->wave_slots = 4 * cus;  // 4 SIMDs per CDNA compute unit
    const char* w = getenv("PIANOSIM_ONE_WAVE_MAX");  // (A/B runs: the threshold; 0 never)
    if (w) E->wave_slots = atoi(w);
    // PIANOSIM_CHUNKS (A/B runs, tests): 0 or 1 = every step monolithic; k >= 2 = every step
    // launch time-sliced in k chunks. Unset: PS_CHUNKS chunks where launch() takes that path.
    // PIANOSIM_STEP_GRID: workgroups of the time-sliced launch (tests: items cross workgroups
    // at small n); default the resident slots of the two-wave build.
    const char* c = getenv("PIANOSIM_CHUNKS");
    E->chunks_forced = c != nullptr;
    E->chunks = c ? atoi(c) : PS_CHUNKS;
    if (E->chunks > PS_MAX_CHUNKS) E->chunks = PS_MAX_CHUNKS;
    if (E->chunks > model->n_substeps) E->chunks = model->n_substeps;
    if (E->chunks < 2) E->chunks = 0;
    const char* g = getenv("PIANOSIM_STEP_GRID");
    E->step_grid = g && atoi(g) > 0 ? atoi(g) : PS_WAVES_PER_EU * 4 * cus;
#ifdef PS_TIMING
    E->chunks = 0;  // (the timing build has no queue kernel)
#endif
    if (E->chunks) {
      HIPCHK(mem.alloc(E->queue, N * E->chunks, false));
      HIPCHK(mem.alloc(E->qctr, QC_WORDS, false));
      HIPCHK(mem.alloc(E->qrank, N, false));
#ifdef PS_QTRACE
      HIPCHK(mem.alloc(E->qtrace, qtrace_words(E.get()), false));
#endif
    }
  }
  HIPCHK(hipDeviceSynchronize());
  *out = E.release();
  return 0;
}

int ps_env_obs_dim(const ps_env* E) { return E ? E->obs_dim : fail("null env"); }
int ps_env_action_dim(const ps_env* E) { return E ? E->action_dim : fail("null env"); }

void ps_destroy(ps_env* E) {
  if (!E) return;
  DeviceGuard guard_(E->device);
  delete E;  // (its DevMem members free the device memory)
}


// Dispatch order of a step launch: envs by the cost of their previous step, descending -
// the Newton iterations its substeps took (PS_STAT_SOLVES: each is a Hessian assembly,
// factorization and line search) - envs about to auto-reset (no physics this step) last.
// Workgroups are dispatched in blockIdx order, so the expensive envs start in the first wave
// of workgroups and the cheap ones fill the slots freed late (longest-processing-time-first):
// the launch's tail is shorter. Each env's result is independent of the order.
// With a queue (the time-sliced step, pianosim_queue_kernel) the order is written as the
// queue's first n items (env << 4 | chunk 0) instead - in env order when `sorted` is false -
// with every env's position in it (qrank: its slot in each later round of the queue); the
// other entries are set to -1 (unpublished) and the ticket counter to the step's grid
// (workgroup b starts with item b): launched before every such step, so the queue is reset
// in stream order (and under graph capture).
#ifdef PS_DYN_LDS
#define PS_LAUNCH_LDS PS_DYN_LDS
#else
#define PS_LAUNCH_LDS 0
#endif
constexpr int ORDER_THREADS = 1024;
constexpr int ORDER_BUCKETS = 130;  // 0: resets, 1 + min(Newton iterations of the last step, 128)
__global__ void __launch_bounds__(ORDER_THREADS) order_kernel(const int* __restrict__ stats,
                                                              const uint8_t* __restrict__ last,
                                                              int* __restrict__ order, int n, int* __restrict__ queue,
                                                              int* __restrict__ qctr, int qcap, int qhead,
                                                              bool sorted, int* __restrict__ qrank) {
  __shared__ int hist[ORDER_BUCKETS], base[ORDER_BUCKETS];
  if (queue) {
    for (int i = n + threadIdx.x; i < qcap; i += blockDim.x) queue[i] = -1;
    if (threadIdx.x == 0) qctr[QC_HEAD] = qhead;
    if (!sorted) {
      for (int e = threadIdx.x; e < n; e += blockDim.x) {
        queue[e] = e << 4;
        qrank[e] = e;
      }
      return;
    }
  }
  if (threadIdx.x < ORDER_BUCKETS) hist[threadIdx.x] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const int b = last[e] ? 0 : 1 + min(max(stats[(size_t)e * PS_NSTATS + PS_STAT_SOLVES], 0), 128);
    atomicAdd(&hist[b], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int b = ORDER_BUCKETS - 1; b >= 0; b--) {  // most iterations first, resets last
      base[b] = acc;
      acc += hist[b];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const int b = last[e] ? 0 : 1 + min(max(stats[(size_t)e * PS_NSTATS + PS_STAT_SOLVES], 0), 128);
    const int pos = atomicAdd(&base[b], 1);
    if (queue) {
      queue[pos] = e << 4;
      qrank[e] = pos;
    } else {
      order[pos] = e;
    }
  }
}

// the kernels' view of the handle: its task options and its buffers
static Cfg make_cfg(const ps_env* E) {
  // (the one-hand task has no forearm term: forearm_reward is ignored)
  Cfg cfg{};
  cfg.lookahead = E->cfg.n_steps_lookahead;
  cfg.fingering = E->cfg.fingering_reward;
  cfg.forearm = E->cfg.hand_side != PS_HAND_BOTH ? 0 : E->cfg.forearm_reward;
  cfg.wrong_press = E->cfg.wrong_press_termination;
  cfg.newton_cap = E->cfg.solver_iterations;
  cfg.maxcon = E->cfg.max_contacts;
  cfg.obs_dim = E->obs_dim;
  cfg.obs_base = E->obs_base;
  cfg.canonical = E->cfg.canonical_actions;
  cfg.energy_coef = (float)E->cfg.energy_penalty_coef;
  cfg.randomize = E->cfg.randomize_hand_positions != 0;
  cfg.seed_lo = (uint32_t)E->seed; cfg.seed_hi = (uint32_t)(E->seed >> 32);
  cfg.env0 = (uint32_t)E->env_offset;
  cfg.full_cpl = E->full_cpl;
  cfg.refine = E->cfg.solver_refine;
  cfg.hand = E->cfg.hand_side;
  return cfg;
}

static Bufs make_bufs(const ps_env* E) {
  Bufs b{};  // (the handle's buffer of the same name, but `applied`)
  b.qpos = E->qpos; b.qvel = E->qvel; b.qws = E->qws; b.ctrl = E->ctrl; b.sustain = E->sustain;
  b.t_idx = E->t_idx; b.last = E->last; b.terms = E->terms; b.tips = E->tips; b.ncon = E->ncon;
  b.mus_acc = E->mus_acc; b.mus_ep = E->mus_ep; b.mus_cnt = E->mus_cnt; b.hand_dy = E->hand_dy;
  b.episode = E->episode; b.stats = E->stats; b.con_out = E->con_out; b.warnings = E->warnings; b.park = E->park;
  b.applied = E->applied_on ? E->applied : nullptr;
  b.keybits = E->keybits;
  return b;
}

// is work put on the stream being captured into a graph (it runs at the graph's replays, not now)?
static bool capturing(void* stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs != hipStreamCaptureStatusNone;
}

// bufs.ncon of the envs' current state rows (pianosim_ncon_kernel), if a launch since the last
// call may have left it unwritten. Called before the counts are read and before anything but a
// step or reset launch overwrites the state rows or hand_dy: the counts stay those of the last
// launch's final state. Under graph capture the pass is always put on the stream - the graph's
// replays cannot know what ran before them - and clears nothing: it has not run.
static int materialise_ncon(ps_env* E, void* stream) {
  const bool cap = capturing(stream);
  if (!E->ncon_stale && !E->ncon_sticky && !cap) return 0;
  const Cfg cfg = make_cfg(E);
  const Bufs b = make_bufs(E);
  if (E->has_x)
    hipLaunchKernelGGL((pianosim_ncon_kernel<true>), dim3(E->n), dim3(64), 0, (hipStream_t)stream,
                       E->d_model, cfg, b, E->n);
  else
    hipLaunchKernelGGL((pianosim_ncon_kernel<false>), dim3(E->n), dim3(64), 0, (hipStream_t)stream,
                       E->d_model, cfg, b, E->n);
  HIPCHK(hipGetLastError());
  if (!cap) E->ncon_stale = false;
  return 0;
}

// a step or reset launch is on the stream: without contact recording it may have skipped the
// final-state collision pass. Captured into a graph, it sets no flag at its replays: from then on
// the counts are taken as stale for good (every read runs the pass)
static void mark_ncon(ps_env* E, void* stream) {
  if (E->con_out) return;
  E->ncon_stale = true;
  if (capturing(stream)) E->ncon_sticky = true;
}

static int launch(ps_env* E, int mode, const float* action, const uint8_t* mask, float* obs, float* reward,
                  float* discount, uint8_t* step_type, void* stream) {
  Song song{E->T, E->d_goal, E->d_count, E->d_keys, E->d_fingers, 0, nullptr};
  if (E->aug_on) {
    song = Song{E->T, E->aug.goal, E->aug.count, E->aug.keys, E->aug.fingers, E->aug.T_cap, E->aug.T};
    if (launch_builder(E, mode == 1 ? AUG_RESET : AUG_STEP, mask, nullptr, nullptr, nullptr, stream)) return -1;
  }
  const Cfg cfg = make_cfg(E);
  const Bufs b = make_bufs(E);
  // the time-sliced step: a launch of more envs than resident slots (below that every env has a
  // slot of its own from the start and there is no second round to balance), or every step
  // when PIANOSIM_CHUNKS says so
  // (a one-hand handle, hand_side != 0, is sliced only when PIANOSIM_CHUNKS says so: on its short
  // chunks the time-sliced step has left envs wrong)
  const bool sliced = mode == 0 && E->chunks >= 2 &&
                      (E->chunks_forced || (E->n > E->step_grid && E->cfg.hand_side == PS_HAND_BOTH));
  if (sliced) {
    const int cap = E->n * E->chunks, grid = E->n < E->step_grid ? E->n : E->step_grid;
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(ORDER_THREADS), 0, (hipStream_t)stream, E->stats, E->last, E->order,
                       E->n, E->queue, E->qctr, cap, grid, E->ordered, E->qrank);
    HIPCHK(hipGetLastError());
#ifndef PS_TIMING
#ifdef PS_QTRACE
    HIPCHK(hipMemsetAsync(E->qtrace, 0, sizeof(uint64_t) * qtrace_words(E), (hipStream_t)stream));
    const QArgs qa{E->d_model, song, cfg, b, action, obs, reward, discount, step_type, E->n, E->queue, E->qctr, cap,
                   E->chunks, E->qrank, (unsigned long long*)E->qtrace};
#else
    const QArgs qa{E->d_model, song, cfg, b, action, obs, reward, discount, step_type, E->n, E->queue, E->qctr, cap,
                   E->chunks, E->qrank};
#endif
#define PS_LAUNCH_Q(XG)                                                                                           \
  hipLaunchKernelGGL((pianosim_queue_kernel<XG>), dim3(grid), dim3(64), 0, (hipStream_t)stream, qa)
    if (E->has_x) PS_LAUNCH_Q(true); else PS_LAUNCH_Q(false);
#undef PS_LAUNCH_Q
#endif
    HIPCHK(hipGetLastError());
    mark_ncon(E, stream);
    return E->keybits ? launch_midi(E, stream) : 0;
  }
  const int* order = nullptr;
  if (mode == 0 && E->ordered && E->n >= 2048) {  // below one wave of workgroups there is no tail to balance
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(ORDER_THREADS), 0, (hipStream_t)stream, E->stats, E->last, E->order,
                       E->n, (int*)nullptr, (int*)nullptr, 0, 0, true, (int*)nullptr);
    HIPCHK(hipGetLastError());
    order = E->order;
  }
  // at most one wave per SIMD: the instantiation built for one resident wave (its spills in
  // AGPRs, no scratch traffic) - the two-wave build's second slot would stay empty anyway
  const bool one = E->n <= E->wave_slots;
#define PS_LAUNCH(XG, WPE)                                                                                    \
  hipLaunchKernelGGL((pianosim_kernel<XG, WPE>), dim3(E->n), dim3(64), PS_LAUNCH_LDS, (hipStream_t)stream, \
                     E->d_model, song, cfg, b, action, mask, obs, reward, discount, step_type, mode, E->n, order)
  if (E->has_x) {
    if (one) PS_LAUNCH(true, 1); else PS_LAUNCH(true, PS_WAVES_PER_EU);
  } else {
    if (one) PS_LAUNCH(false, 1); else PS_LAUNCH(false, PS_WAVES_PER_EU);
  }
#undef PS_LAUNCH
  HIPCHK(hipGetLastError());
  mark_ncon(E, stream);
  return E->keybits ? launch_midi(E, stream) : 0;
}

int ps_reset(ps_env* E, const uint8_t* env_mask, float* obs, void* stream) {
  if (!E || !obs) return fail("null argument");
  GUARD(E);
  return launch(E, 1, nullptr, env_mask, obs, nullptr, nullptr, nullptr, stream);
}

int ps_step(ps_env* E, const float* action, float* obs, float* reward, float* discount, uint8_t* step_type,
            void* stream) {
  if (!E || !action || !obs || !reward || !discount || !step_type) return fail("null argument");
  GUARD(E);
  return launch(E, 0, action, nullptr, obs, reward, discount, step_type, stream);
}

int ps_get_state(ps_env* E, float* qpos, float* qvel, float* qacc_ws, float* ctrl, float* sustain, int32_t* t_idx,
                 uint8_t* last, void* stream) {
  if (!E) return fail("null env");
  GUARD(E);
  const size_t N = E->n;
  return -(copy_dd(qpos, E->qpos, N * NV, stream) || copy_dd(qvel, E->qvel, N * NV, stream) ||
           copy_dd(qacc_ws, E->qws, N * NV, stream) || copy_dd(ctrl, E->ctrl, N * NU, stream) ||
           copy_dd(sustain, E->sustain, N, stream) || copy_dd(t_idx, E->t_idx, N, stream) ||
           copy_dd(last, E->last, N, stream));
}

int ps_set_state(ps_env* E, const float* qpos, const float* qvel, const float* qacc_ws, const float* ctrl,
                 const float* sustain, const int32_t* t_idx, const uint8_t* last, void* stream) {
  if (!E) return fail("null env");
  GUARD(E);
  if (materialise_ncon(E, stream)) return -1;  // (the counts of the state about to be overwritten)
  const size_t N = E->n;
  return -(copy_dd(E->qpos, qpos, N * NV, stream) || copy_dd(E->qvel, qvel, N * NV, stream) ||
           copy_dd(E->qws, qacc_ws, N * NV, stream) || copy_dd(E->ctrl, ctrl, N * NU, stream) ||
           copy_dd(E->sustain, sustain, N, stream) || copy_dd(E->t_idx, t_idx, N, stream) ||
           copy_dd(E->last, last, N, stream));
}

int ps_set_applied(ps_env* E, const float* qfrc_applied, void* stream) {
  if (!E) return fail("null env");
  GUARD(E);
  if (qfrc_applied && copy_dd(E->applied, qfrc_applied, (size_t)E->n * NV, stream)) return -1;
  E->applied_on = qfrc_applied != nullptr;
  return 0;
}

int ps_reward_terms(ps_env* E, float* terms, void* stream) {
  if (!E || !terms) return fail("null argument");
  GUARD(E);
  return copy_dd(terms, E->terms, (size_t)E->n * PS_NTERMS, stream);
}

int ps_fingertips(ps_env* E, float* xpos, void* stream) {
  if (!E || !xpos) return fail("null argument");
  GUARD(E);
  return copy_dd(xpos, E->tips, (size_t)E->n * 2 * PS_NFINGER * 3, stream);
}


#ifdef PS_TIMING
// diagnostic: per-env phase cycle sums [n][NPHASE] since the last call (host buffer)
int ps_debug_timing(ps_env* E, uint64_t* out) {
  static uint64_t* d = nullptr;  // (the process's one, behind g_timing and no handle's: not in a DevMem)
  static size_t cap = 0;
  size_t bytes = sizeof(uint64_t) * E->n * NPHASE;
  if (cap < bytes) {
    if (d) (void)hipFree(d);
    HIPCHK(hipMalloc(&d, bytes));
    cap = bytes;
    HIPCHK(hipMemset(d, 0, bytes));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_timing), &d, sizeof(d)));
    return 0;
  }
  HIPCHK(hipDeviceSynchronize());
  if (out) HIPCHK(hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(d, 0, bytes));
  return 0;
}
#endif

#ifdef PS_QTRACE
// diagnostic (tools/queue_trace.py): the last time-sliced step's trace (host buffers). dims =
// {chunks, grid}; items [chunks * n][QT_ITEM], exits [grid][QT_EXIT] (kernel_v2.inc, QT_*);
// rank [n] = every env's position in order_kernel's order of that step. Null: not copied.
int ps_debug_qtrace(ps_env* E, int32_t* dims, uint64_t* items, uint64_t* exits, int32_t* rank) {
  if (!E || !E->qtrace) return fail("no time-sliced step in this handle");
  GUARD(E);
  HIPCHK(hipDeviceSynchronize());
  const size_t ni = (size_t)E->n * E->chunks * QT_ITEM;
  if (dims) dims[0] = E->chunks, dims[1] = qtrace_grid(E);
  if (items) HIPCHK(hipMemcpy(items, E->qtrace, sizeof(uint64_t) * ni, hipMemcpyDeviceToHost));
  if (exits)
    HIPCHK(hipMemcpy(exits, E->qtrace + ni, sizeof(uint64_t) * qtrace_grid(E) * QT_EXIT, hipMemcpyDeviceToHost));
  if (rank) HIPCHK(hipMemcpy(rank, E->qrank, sizeof(int) * E->n, hipMemcpyDeviceToHost));
  return 0;
}
#endif

int ps_musical_metrics(ps_env* E, float* episode, int32_t* episodes, void* stream) {
  if (!E) return fail("null argument");
  GUARD(E);
  return -(copy_dd(episode, E->mus_ep, (size_t)E->n * PS_NMUSIC, stream) ||
           copy_dd(episodes, E->mus_cnt, (size_t)E->n, stream));
}

int ps_solver_stats(ps_env* E, int32_t* stats, void* stream) {
  if (!E || !stats) return fail("null argument");
  GUARD(E);
  return copy_dd(stats, E->stats, (size_t)E->n * PS_NSTATS, stream);
}

int ps_get_hand_offset(ps_env* E, float* dy, int32_t* episodes, void* stream) {
  if (!E) return fail("null argument");
  GUARD(E);
  return -(copy_dd(dy, E->hand_dy, (size_t)E->n, stream) || copy_dd(episodes, E->episode, (size_t)E->n, stream));
}

int ps_set_hand_offset(ps_env* E, const float* dy, void* stream) {
  if (!E || !dy) return fail("null argument");
  GUARD(E);
  if (!E->cfg.randomize_hand_positions) return fail("ps_set_hand_offset needs randomize_hand_positions");
  if (materialise_ncon(E, stream)) return -1;  // (the counts of the last launch's hand positions)
  return copy_dd(E->hand_dy, dy, (size_t)E->n, stream);
}

static_assert(sizeof(ps_contact) == sizeof(Contact), "ps_contact mirrors the kernel's contact record");
int ps_record_contacts(ps_env* E, int on) {
  if (!E) return fail("null argument");
  GUARD(E);
  if (on && !E->con_out) {
    HIPCHK(E->con_mem.alloc(E->con_out, MAXCON * (size_t)E->n, true));
    E->row_gen++;
  } else if (!on && E->con_out) {
    E->con_mem.clear();
    E->con_out = nullptr;
    E->row_gen++;
  }
  return 0;
}

int ps_contacts(ps_env* E, ps_contact* out, void* stream) {
  if (!E || !out) return fail("null argument");
  GUARD(E);
  if (!E->con_out) return fail("contact recording is off (ps_record_contacts)");
  return copy_dd(reinterpret_cast<Contact*>(out), E->con_out, MAXCON * (size_t)E->n, stream);
}

int ps_warnings(ps_env* E, int32_t* warnings, void* stream) {
  if (!E || !warnings) return fail("null argument");
  GUARD(E);
  return copy_dd(warnings, E->warnings, (size_t)E->n * PS_NWARN, stream);
}


static_assert(sizeof(ps_aug_song) == sizeof(psb::Song) && sizeof(ps_variation) == sizeof(psb::Var),
              "pianosim.h mirrors song_build.h");
int ps_set_augmentations(ps_env* E, const ps_augment_desc* d) {
  if (!E) return fail("null env");
  GUARD(E);
  HIPCHK(hipDeviceSynchronize());  // (init-time: nothing of the old bank is in flight)
  DevMem& mem = E->aug_mem;
  mem.clear();
  E->aug_on = false;
  E->row_gen++;
  if (!d) return 0;
  if (d->struct_size != PS_AUGMENT_DESC_SIZE)
    return fail("ps_augment_desc.struct_size != sizeof(ps_augment_desc): rebuild against include/pianosim.h");
  if (d->n_songs < 1 || !d->songs) return fail("ps_set_augmentations: an empty bank");
  if (d->n_variations < 0 || d->n_variations > PS_MAX_VARIATIONS || (d->n_variations && !d->variations))
    return fail("ps_set_augmentations: 0 .. PS_MAX_VARIATIONS variations");
  if (!(d->dt > 0) || d->initial_buffer_time < 0) return fail("ps_set_augmentations: bad dt / initial_buffer_time");
  const long nbuf = (long)nearbyint(d->initial_buffer_time / d->dt);
  if (d->T_cap <= nbuf || d->T_cap > (1 << 20)) return fail("ps_set_augmentations: T_cap out of range");
  for (int i = 0; i < d->n_variations; i++) {
    const ps_variation& v = d->variations[i];
    if (v.kind < PS_VAR_SELECT || v.kind > PS_VAR_OCTAVE) return fail("ps_set_augmentations: unknown variation kind");
    if (!(v.range >= 0) || (v.kind == PS_VAR_STRETCH && !(v.range < 1)) || v.range > 1e6)
      return fail("ps_set_augmentations: variation range out of bounds");
  }
  const long F_cap = d->T_cap - nbuf;
  const size_t lds = (size_t)F_cap * (psb::NKEYS + 1);
  if (lds > 65536)
    return fail("ps_set_augmentations: the builder's roll of " + std::to_string(F_cap) + " frames needs " +
                std::to_string(lds) + " B of LDS; a workgroup may take 65536");
  const size_t N = (size_t)E->n, rows = N * (size_t)d->T_cap;
  const size_t row_bytes = sizeof(float) * (NK + 1) + sizeof(int) * (1 + 2 * PS_MAX_NOTES);
  if (d->max_bytes && rows * row_bytes > d->max_bytes)
    return fail("ps_set_augmentations: the per-env song tables need " + std::to_string(rows * row_bytes) + " B (" +
                std::to_string(E->n) + " envs x " + std::to_string(d->T_cap) + " rows x " +
                std::to_string(row_bytes) + " B), over the budget of " + std::to_string(d->max_bytes) + " B");
  // every song as given has to fit: the builder falls back to it
  const double fps = 1.0 / d->dt;
  {
    std::vector<uint32_t> roll((size_t)F_cap * psb::ROW_WORDS);
    std::vector<uint8_t> sus((size_t)F_cap);
    for (int i = 0; i < d->n_songs; i++) {
      const ps_aug_song& g = d->songs[i];
      if (g.n_notes < 1 || !g.notes || g.n_cc < 0 || (g.n_cc && !g.ccs))
        return fail("ps_set_augmentations: song " + std::to_string(i) + " is empty");
      psb::Song h;
      memcpy(&h, &g, sizeof(h));
      if (psb::build_roll(h, 1.0, 0, fps, F_cap, roll.data(), sus.data(), 0, 1) < 0)
        return fail("ps_set_augmentations: song " + std::to_string(i) + " as given does not fit " +
                    std::to_string(d->T_cap) + " rows of at most " + std::to_string(PS_MAX_NOTES) + " keys");
    }
  }
  AugDev a{};
  a.n_songs = d->n_songs;
  a.n_vars = d->n_variations;
  a.fps = fps;
  a.nbuf = (int)nbuf;
  a.T_cap = d->T_cap;
  std::vector<psb::Song> bank(d->n_songs);
  for (int i = 0; i < d->n_songs; i++) {
    const ps_aug_song& g = d->songs[i];
    memcpy(&bank[i], &g, sizeof(psb::Song));
    double *dn = nullptr, *dc = nullptr;
    HIPCHK(mem.upload(dn, g.notes, (size_t)4 * g.n_notes));
    if (g.n_cc) HIPCHK(mem.upload(dc, g.ccs, (size_t)2 * g.n_cc));
    bank[i].notes = dn;
    bank[i].ccs = dc;
  }
  psb::Song* dbank = nullptr;
  HIPCHK(mem.upload(dbank, bank.data(), (size_t)d->n_songs));
  a.bank = dbank;
  psb::Var* dvars = nullptr;
  HIPCHK(mem.alloc(dvars, (size_t)d->n_variations + 1, false));
  if (d->n_variations)
    HIPCHK(hipMemcpy(dvars, d->variations, sizeof(psb::Var) * d->n_variations, hipMemcpyHostToDevice));
  a.vars = dvars;
  HIPCHK(mem.alloc(a.song, N, true));
  HIPCHK(mem.upload(a.factor, std::vector<double>(N, 1.0).data(), N));
  HIPCHK(mem.alloc(a.shift, N, true));
  HIPCHK(mem.alloc(a.T, N, true));
  HIPCHK(mem.alloc(a.fallbacks, N, false));
  HIPCHK(mem.alloc(a.goal, rows * (NK + 1), true));
  HIPCHK(mem.alloc(a.count, rows, true));
  HIPCHK(mem.alloc(a.keys, rows * PS_MAX_NOTES, false));
  HIPCHK(mem.alloc(a.fingers, rows * PS_MAX_NOTES, false));
  HIPCHK(hipMemset(a.keys, 0xff, sizeof(int) * rows * PS_MAX_NOTES));
  HIPCHK(hipMemset(a.fingers, 0xff, sizeof(int) * rows * PS_MAX_NOTES));
  E->aug = a;
  E->aug_lds = lds;
  // every env starts with song 0 as given (a step before the first reset plays it, as on a plain handle)
  if (launch_builder(E, AUG_FORCED, nullptr, a.song, a.factor, a.shift, nullptr)) return -1;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(a.fallbacks, 0, sizeof(int) * N));
  E->aug_on = true;
  return 0;
}

int ps_get_augmentation(ps_env* E, int32_t* song, double* factor, int32_t* shift, int32_t* T, int32_t* fallbacks,
                        void* stream) {
  if (!E) return fail("null env");
  GUARD(E);
  if (!E->aug_on) return fail("the handle has no augmentations (ps_set_augmentations)");
  const size_t N = E->n;
  return -(copy_dd(song, E->aug.song, N, stream) || copy_dd(factor, E->aug.factor, N, stream) ||
           copy_dd(shift, E->aug.shift, N, stream) || copy_dd(T, E->aug.T, N, stream) ||
           copy_dd(fallbacks, E->aug.fallbacks, N, stream));
}

int ps_set_augmentation(ps_env* E, const int32_t* song, const double* factor, const int32_t* shift, void* stream) {
  if (!E || !song || !factor || !shift) return fail("null argument");
  GUARD(E);
  if (!E->aug_on) return fail("the handle has no augmentations (ps_set_augmentations)");
  return launch_builder(E, AUG_FORCED, nullptr, song, factor, shift, stream);
}

int ps_get_song_tables(ps_env* E, float* goal, int32_t* count, int32_t* keys, int32_t* fingers, void* stream) {
  if (!E) return fail("null env");
  GUARD(E);
  if (!E->aug_on) return fail("the handle has no augmentations (ps_set_augmentations)");
  const size_t rows = (size_t)E->n * E->aug.T_cap;
  return -(copy_dd(goal, E->aug.goal, rows * (NK + 1), stream) || copy_dd(count, E->aug.count, rows, stream) ||
           copy_dd(keys, E->aug.keys, rows * PS_MAX_NOTES, stream) ||
           copy_dd(fingers, E->aug.fingers, rows * PS_MAX_NOTES, stream));
}

int ps_record_midi(ps_env* E, int max_events, uint64_t max_bytes) {
  if (!E) return fail("null env");
  if (max_events < 0 || max_events > (1 << 24)) return fail("ps_record_midi: max_events outside 0 .. 2^24");
  // (a request over the budget is refused before anything changes: a recording handle goes on
  // recording into the banks it has)
  const size_t N = (size_t)E->n, kb = (size_t)KB_HDR + (size_t)E->nsub * KB_ROW;
  const size_t per_env = sizeof(uint32_t) * (2 * (size_t)max_events + kb) + sizeof(int) * MS_WORDS;
  if (max_events && max_bytes && N * per_env > max_bytes)
    return fail("ps_record_midi: the recorder needs " + std::to_string(N * per_env) + " B (" + std::to_string(E->n) +
                " envs x (2 banks x " + std::to_string(max_events) + " events x 4 B + " +
                std::to_string(sizeof(uint32_t) * kb + sizeof(int) * MS_WORDS) + " B)), over the budget of " +
                std::to_string(max_bytes) + " B");
  GUARD(E);
  HIPCHK(hipDeviceSynchronize());  // (init-time: nothing that reads the old buffers is in flight)
  E->midi_mem.clear();
  E->keybits = nullptr;
  E->midi = MidiRec{};
  E->row_gen++;
  if (!max_events) return 0;
  MidiRec r{};
  uint32_t* kbits = nullptr;
  r.max_events = max_events;
  hipError_t e = E->midi_mem.alloc(r.events, N * 2 * (size_t)max_events, true);
  if (e == hipSuccess) e = E->midi_mem.alloc(r.state, N * MS_WORDS, true);
  if (e == hipSuccess) e = E->midi_mem.alloc(kbits, N * kb, true);
  if (e != hipSuccess) {
    E->midi_mem.clear();
    return fail(std::string("ps_record_midi: ") + hipGetErrorString(e));
  }
  HIPCHK(hipDeviceSynchronize());
  E->midi = r;
  E->keybits = kbits;
  return 0;
}

int ps_midi_events(ps_env* E, int which, uint32_t* events, int32_t* count, int32_t* dropped, int32_t* substeps,
                   void* stream) {
  if (!E) return fail("null env");
  if (!E->keybits) return fail("MIDI recording is off (ps_record_midi)");
  if (which != 0 && which != 1) return fail("ps_midi_events: which is 0 (the running episode) or 1 (the last finished one)");
  GUARD(E);
  hipLaunchKernelGGL(midi_gather_kernel, dim3(E->n), dim3(256), 0, (hipStream_t)stream, E->midi, which, events, count,
                     dropped, substeps, E->n);
  HIPCHK(hipGetLastError());
  return 0;
}

int ps_midi_push(ps_env* E, const uint32_t* bits, int rows, void* stream) {
  if (!E || !bits) return fail("null argument");
  if (!E->keybits) return fail("MIDI recording is off (ps_record_midi)");
  if (rows < 1 || rows > E->nsub)
    return fail("ps_midi_push: " + std::to_string(rows) + " rows; one push takes 1 .. " + std::to_string(E->nsub) +
                " (the handle's substeps per step)");
  GUARD(E);
  hipLaunchKernelGGL(midi_events_kernel, dim3(E->n), dim3(64), 0, (hipStream_t)stream, E->midi, bits,
                     (size_t)rows * KB_ROW, (uint32_t*)nullptr, (size_t)0, rows, E->n);
  HIPCHK(hipGetLastError());
  return 0;
}

int ps_set_env_offset(ps_env* E, int64_t global_first_env) {
  if (!E) return fail("null argument");
  if (global_first_env < 0) return fail("negative env offset");
  E->env_offset = global_first_env;
  return 0;
}

// one workgroup: env i by thread i (mod 1024); the finished episodes' sum in a fixed order
// (per-thread partials, then a tree over the 1024 threads): deterministic
__global__ void __launch_bounds__(1024) episode_returns_kernel(const float* __restrict__ reward,
                                                               const uint8_t* __restrict__ step_type, int n,
                                                               double* __restrict__ running, float* __restrict__ last_return,
                                                               double* __restrict__ finished_sum,
                                                               int64_t* __restrict__ finished_count) {
  __shared__ double ssum[1024];
  __shared__ int scnt[1024];
  double fs = 0.0;
  int fc = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const int st = step_type[i];
    const double r = st == PS_FIRST ? 0.0 : running[i] + (double)reward[i];
    running[i] = r;
    if (st == PS_LAST) {
      last_return[i] = (float)r;
      fs += r;
      fc++;
    }
  }
  ssum[threadIdx.x] = fs;
  scnt[threadIdx.x] = fc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
      scnt[threadIdx.x] += scnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *finished_sum += ssum[0];
    *finished_count += scnt[0];
  }
}

int ps_episode_returns(const float* reward, const uint8_t* step_type, int n, double* running, float* last_return,
                       double* finished_sum, int64_t* finished_count, void* stream) {
  if (!reward || !step_type || !running || !last_return || !finished_sum || !finished_count || n <= 0)
    return fail("ps_episode_returns: null argument or n <= 0");
  hipLaunchKernelGGL(episode_returns_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, reward, step_type, n, running,
                     last_return, finished_sum, finished_count);
  HIPCHK(hipGetLastError());
  return 0;
}

int ps_snapshot_create(ps_env* E, uint64_t max_bytes, ps_snapshot** out) {
  if (!E || !out) return fail("null argument");
  std::unique_ptr<ps_snapshot> S(new ps_snapshot());
  std::string err;
  if (snapshot_rows(E, S->table, err)) return fail(err);
  // every buffer's copy starts 256-byte aligned
  const size_t N = (size_t)E->n;
  std::vector<size_t> at(S->table.n);
  size_t total = 0, per_env = 0;
  for (int r = 0; r < S->table.n; r++) {
    at[r] = total;
    total += (N * S->table.row[r].snap_stride + 255) & ~(size_t)255;
    per_env += S->table.row[r].snap_stride;
  }
  if (max_bytes && total > max_bytes)
    return fail("ps_snapshot_create: the snapshot needs " + std::to_string(total) + " B (" + std::to_string(E->n) +
                " envs x " + std::to_string(per_env) + " B in " + std::to_string(S->table.n) +
                " rows), over the budget of " + std::to_string(max_bytes) + " B");
  GUARD(E);
  char* base = nullptr;
  HIPCHK(S->mem.alloc(base, total, true));
  HIPCHK(hipDeviceSynchronize());
  for (int r = 0; r < S->table.n; r++) S->table.row[r].snap = base + at[r];
  S->owner = E;
  S->config = E->row_gen;
  S->bytes = total;
  S->device = E->device;
  *out = S.release();
  return 0;
}

uint64_t ps_snapshot_bytes(const ps_snapshot* S) { return S ? S->bytes : 0; }

void ps_snapshot_destroy(ps_snapshot* S) {
  if (!S) return;
  DeviceGuard guard_(S->device);
  delete S;  // (its DevMem frees the device memory)
}

static int snapshot_usable(const ps_env* E, const ps_snapshot* S, const char* what) {
  if (!E || !S) return fail(std::string(what) + ": null argument");
  if (S->owner != E) return fail(std::string(what) + ": the snapshot was created on another handle");
  if (S->config != E->row_gen)
    return fail(std::string(what) + ": ps_set_augmentations, ps_record_midi or ps_record_contacts changed the "
                "handle's per-env buffers after the snapshot was created; create a new one");
  return 0;
}

int ps_snapshot_save(ps_env* E, ps_snapshot* S, void* stream) {
  if (snapshot_usable(E, S, "ps_snapshot_save")) return -1;
  GUARD(E);
  if (materialise_ncon(E, stream)) return -1;  // (the stored counts are real)
  hipLaunchKernelGGL((snapshot_copy_kernel<false>), dim3(E->n), dim3(SNAP_THREADS), 0, (hipStream_t)stream, S->table,
                     (const int*)nullptr, (int*)nullptr, E->n);
  HIPCHK(hipGetLastError());
  return 0;
}

int ps_snapshot_restore(ps_env* E, const ps_snapshot* S, const int32_t* src, int32_t* n_bad, void* stream) {
  if (snapshot_usable(E, S, "ps_snapshot_restore")) return -1;
  GUARD(E);
  hipLaunchKernelGGL((snapshot_copy_kernel<true>), dim3(E->n), dim3(SNAP_THREADS), 0, (hipStream_t)stream, S->table,
                     src, n_bad, E->n);
  HIPCHK(hipGetLastError());
  // every env has its saved counts again: they are fresh. With src an env may have been left as it
  // was, so the flag stays; a later pass then recomputes every env's count from its state rows,
  // which gives the restored envs the counts they were saved with
  if (!src && !capturing(stream)) E->ncon_stale = false;
  return 0;
}

int ps_contact_count(ps_env* E, int32_t* ncon, void* stream) {
  if (!E || !ncon) return fail("null argument");
  GUARD(E);
  if (materialise_ncon(E, stream)) return -1;
  return copy_dd(ncon, E->ncon, (size_t)E->n, stream);
}

}  // extern "C"
