// augment.inc - per-episode MIDI augmentations on the device (suite/variations.py through
// PianoWithShadowHands(augmentations=...), piano_with_shadow_hands.py:151-157,169-174):
// song_build_kernel, enqueued by launch() before the step / reset kernel of a handle that has
// ps_set_augmentations. One wave per env; an env that is not about to start an episode exits at
// once. An env that is (ps_reset with its mask bit, or an auto-reset after LAST) draws its
// variations - counter-based, keyed by (seed, global env, episode): the step kernel increments
// `episode` afterwards - and rebuilds its own goal / count / keys / fingers rows and its T from
// the bank's song, in LDS (a byte per frame and key). The build itself is song_build.h, the
// code libpianosong.so runs on the host. No host sync, no allocation: legal under stream capture.
#include "song_build.h"

struct AugDev {
  const psb::Song* bank;  // device copies; song 0 is the task's own
  const psb::Var* vars;
  int n_songs, n_vars;
  double fps;
  int nbuf, T_cap;
  // per env: this episode's draw, its rows, fallbacks since ps_set_augmentations
  int* song;
  double* factor;
  int* shift;
  int* T;
  int* fallbacks;
  float* goal;   // [N][T_cap][89]
  int* count;    // [N][T_cap]
  int* keys;     // [N][T_cap][PS_MAX_NOTES]
  int* fingers;  // [N][T_cap][PS_MAX_NOTES]
};
static_assert(psb::MAX_NOTES == PS_MAX_NOTES && psb::GOAL_ROW == NK + 1, "song_build.h writes the step kernel's rows");

enum : int { AUG_STEP = 0, AUG_RESET = 1, AUG_FORCED = 2 };

// mode AUG_STEP: envs with last[e]; AUG_RESET: envs with mask[e] (all when mask is null);
// AUG_FORCED (ps_set_augmentation): every env, with the caller's draw instead of its own.
// Dynamic LDS: (T_cap - nbuf) * 89 bytes.
__global__ void __launch_bounds__(64) song_build_kernel(AugDev a, int mode, const uint8_t* __restrict__ mask,
                                                        const uint8_t* __restrict__ last,
                                                        const int* __restrict__ episode, uint32_t seed_lo,
                                                        uint32_t seed_hi, uint32_t env0, int n,
                                                        const int* f_song, const double* f_factor,
                                                        const int* f_shift) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= n) return;
  if (mode == AUG_RESET) {
    if (mask && !mask[e]) return;
  } else if (mode == AUG_STEP) {
    if (!last[e]) return;
  }
  int song, shift;
  double factor;
  if (mode == AUG_FORCED) {
    song = f_song[e];
    factor = f_factor[e];
    shift = f_shift[e];
    song = song < 0 ? 0 : (song >= a.n_songs ? a.n_songs - 1 : song);
    shift = shift < -127 ? -127 : (shift > 127 ? 127 : shift);
    if (!(factor > 0.0) || !(factor < 1e6)) factor = 1.0;
  } else {
    psb::draw(seed_lo, seed_hi, env0 + (uint32_t)e, (uint32_t)episode[e], a.vars, a.n_vars, a.bank, a.n_songs, &song,
              &factor, &shift);
  }
  const long F_cap = a.T_cap - a.nbuf;
  uint32_t* roll = reinterpret_cast<uint32_t*>(aug_lds);
  uint8_t* sus = aug_lds + F_cap * psb::NKEYS;
  const size_t row = (size_t)e * a.T_cap;
  int fell_back = 0;
  const int T = psb::build_env(a.bank[song], factor, shift, a.fps, a.nbuf, a.T_cap, roll, sus,
                               a.goal + row * psb::GOAL_ROW, a.count + row, a.keys + row * psb::MAX_NOTES,
                               a.fingers + row * psb::MAX_NOTES, &fell_back, lane, 64);
  if (lane == 0) {
    if (fell_back) a.fallbacks[e] += 1;
    a.song[e] = song;
    a.factor[e] = fell_back ? 1.0 : factor;
    a.shift[e] = fell_back ? 0 : shift;
    if (T > 0) a.T[e] = T;
  }
}
