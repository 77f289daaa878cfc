// song_build.h - the per-episode song builder's core: the MIDI augmentation draw and the
// (stretched, transposed) song -> goal / count / keys / fingers tables. Plain C++ that
// compiles as host code under g++ (libpianosong.so: pss_build_tables, pss_draw_augmentation,
// the CPU suite holds it to pss_song_tables(pss_transpose(pss_stretch(seq)))) and as device code
// under hipcc (augment.inc: song_build_kernel, one wave per env). The same statements run in
// both: `lane` / `nl` split the loops over a wave's lanes (host: lane 0 of 1) and the three
// psb_* hooks below are the only places where the two differ.
//
// It restates pss_song_tables (song.cpp) on a byte roll: sequence_to_pianoroll with
// onset_window 0 (a note covers frames [int(s * fps), max(start + 1, ceil(e * fps))), a later
// note of the start-sorted sequence overwrites the fingering, a re-strike leaves a gap in its
// onset frame), the CC64 hold rule, the initial buffer frames. All time arithmetic is fp64
// without contraction, in the operation order of the Python it restates.
#ifndef PIANOSIM_SONG_BUILD_H
#define PIANOSIM_SONG_BUILD_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSB_HD __host__ __device__ inline
#else
#define PSB_HD inline
#endif
#if defined(__clang__)
#define PSB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PSB_NO_CONTRACT  // (g++: built with -ffp-contract=off)
#endif

namespace psb {

constexpr int NKEYS = 88, MIN_PITCH = 21, MAX_PITCH = 108, GOAL_ROW = NKEYS + 1, MAX_NOTES = 16;
constexpr int MAX_VARS = 4;
constexpr int MIN_PART = -1, MAX_PART = 61;  // a fingering is kept as part + 1 in 6 bits
enum : int { VAR_SELECT = 1, VAR_STRETCH = 2, VAR_PITCH = 3, VAR_OCTAVE = 4 };
enum : uint8_t { ACTIVE = 0x80, ONSET = 0x40, FINGER = 0x3f };
constexpr uint32_t DRAW_TAG = 0x6d696469u;  // "midi"

// One song of the bank. notes: (pitch, start, end, part) per note, stably sorted by start time;
// ccs: (time, value) of the CC64 events in sequence order; pitch_mask: bit p of word p / 32 is
// set when a note of MIDI pitch p exists (the pitch bounds of the shift draws).
struct Song {
  const double* notes;
  const double* ccs;
  int n_notes, n_cc;
  double total_time;
  uint32_t pitch_mask[4];
};

struct Var {
  int kind;
  double prob, range;
};

// ---- the three places where a wave and a host thread differ
PSB_HD void psb_sync() {  // the roll written so far is visible to every lane
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}
PSB_HD bool psb_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any(x) != 0;
#else
  return x;
#endif
}
PSB_HD uint32_t psb_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al., SC'11)
PSB_HD void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = psb_mulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = psb_mulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

PSB_HD int floordiv12(int a) { return a >= 0 ? a / 12 : -((-a + 11) / 12); }  // Python's a // 12

// lowest / highest pitch of the song's notes that stay on the piano after `shift` (the running
// song of the reference's variation chain: transpose drops the others); false: none stays
PSB_HD bool pitch_bounds(const uint32_t mask[4], int shift, int* lo, int* hi) {
  int a = 1000, b = -1000;
  for (int p = 0; p < 128; p++) {
    if (!((mask[p >> 5] >> (p & 31)) & 1u)) continue;
    const int q = p + shift;
    if (q < MIN_PITCH || q > MAX_PITCH) continue;
    a = q < a ? q : a;
    b = q > b ? q : b;
  }
  *lo = a;
  *hi = b;
  return b >= a;
}

// The draw of (seed, global env, episode): variations.draw in Python is its specification.
// Variation i takes Philox counter (episode, env, "midi", i); its gate is u = (c0 >> 8) 2^-24
// (skipped when u > prob, variations.py:73,112,163), its value comes from c1. The bank's song 0
// is the constructor's song; MidiSelect picks one of songs 1 .. n_songs - 1 and starts again
// from it (the reference's chain hands each variation the previous one's result).
PSB_HD void draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t env, uint32_t episode, const Var* vars, int n_vars,
                 const Song* bank, int n_songs, int* song_out, double* factor_out, int* shift_out) {
  PSB_NO_CONTRACT
  int song = 0, shift = 0;
  double factor = 1.0;
  for (int i = 0; i < n_vars; i++) {
    uint32_t c[4] = {episode, env, DRAW_TAG, (uint32_t)i};
    philox(c, seed_lo, seed_hi);
    const double u = (double)(c[0] >> 8) * 0x1p-24;
    const int kind = vars[i].kind;
    if (kind == VAR_SELECT) {
      if (n_songs > 1) song = 1 + (int)psb_mulhi(c[1], (uint32_t)(n_songs - 1));
      shift = 0;
      factor = 1.0;
      continue;
    }
    if (u > vars[i].prob) continue;
    if (kind == VAR_STRETCH) {
      const double x = (double)c[1] * 0x1p-32;
      const double y = 2.0 * x;
      const double z = y - 1.0;
      const double w = z * vars[i].range;
      factor = 1.0 + w;
      continue;
    }
    const int r = (int)vars[i].range;
    int pmin, pmax;
    if (r == 0 || !pitch_bounds(bank[song].pitch_mask, shift, &pmin, &pmax)) continue;
    if (kind == VAR_PITCH) {  // variations.py:124-133
      const int low = MIN_PITCH - pmin > -r ? MIN_PITCH - pmin : -r;
      const int high = MAX_PITCH - pmax < r ? MAX_PITCH - pmax : r;
      if (high >= low) shift += low + (int)psb_mulhi(c[1], (uint32_t)(high - low + 1));
    } else if (kind == VAR_OCTAVE) {  // variations.py:175-184 (floor division: may leave the piano)
      const int low = MIN_PITCH - pmin > -12 * r ? MIN_PITCH - pmin : -12 * r;
      const int high = MAX_PITCH - pmax < 12 * r ? MAX_PITCH - pmax : 12 * r;
      const int flo = floordiv12(low), fhi = floordiv12(high);
      if (fhi >= flo) shift += 12 * (flo + (int)psb_mulhi(c[1], (uint32_t)(fhi - flo + 1)));
    }
  }
  *song_out = song;
  *factor_out = factor;
  *shift_out = shift;
}

// total_time of the transposed, stretched song: transpose keeps it unless it drops a note, then
// it is the last end of the notes that stay
PSB_HD double total_time_of(const Song& s, double factor, int shift) {
  PSB_NO_CONTRACT
  bool dropped = false;
  double end = 0.0;
  for (int i = 0; i < s.n_notes; i++) {
    const int p = (int)s.notes[4 * i] + shift;
    if (p < MIN_PITCH || p > MAX_PITCH) {
      dropped = true;
      continue;
    }
    const double e = s.notes[4 * i + 2] * factor;
    end = e > end ? e : end;
  }
  return dropped ? end : s.total_time * factor;
}

// The roll is an array of 32-bit words, 22 per frame, one byte per key (little-endian: key
// 4 w + j is byte j of word w); notes are written bytewise, frames are read by the word.
constexpr int ROW_WORDS = NKEYS / 4;
constexpr uint32_t ACTIVE4 = 0x80808080u;
static_assert(NKEYS % 4 == 0 && ONSET == (ACTIVE >> 1), "four keys per word; onset bit below the active bit");
// keys 4 w .. 4 w + 3 of frame f: ACTIVE in the byte of each key that is a goal of the frame -
// active, and not a re-strike (active in the frame before, onset in this one)
PSB_HD uint32_t goal_word(const uint32_t* roll, long f, int w) {
  const uint32_t v = roll[f * ROW_WORDS + w];
  const uint32_t act = v & ACTIVE4;
  if (f == 0) return act;
  return act & ~(roll[(f - 1) * ROW_WORDS + w] & (v << 1) & ACTIVE4);
}

// The roll of the song at (factor, shift) in roll [F_cap][88] / sus [F_cap]; -> its frames, or
// -1 when it has more than F_cap frames or a frame of more than MAX_NOTES keys (nothing of the
// env's tables has been touched then).
PSB_HD long build_roll(const Song& s, double factor, int shift, double fps, long F_cap, uint32_t* roll, uint8_t* sus,
                       int lane, int nl) {
  PSB_NO_CONTRACT
  const double total = total_time_of(s, factor, shift);
  const double tf = total * fps;
  const double tf1 = tf + 1;
  if (!(tf1 >= 1.0) || !(tf1 <= (double)F_cap + 1.0)) return -1;
  const long nf = (long)tf1;
  if (nf < 1 || nf > F_cap) return -1;
  psb_sync();  // (a second build: the first one's reads are done)
  for (long i = lane; i < nf * ROW_WORDS; i += nl) roll[i] = 0;
  for (long i = lane; i < nf; i += nl) sus[i] = 0;
  psb_sync();
  for (int i = 0; i < s.n_notes; i++) {  // in sequence order: the last writer's fingering stays
    const double* n = s.notes + 4 * i;
    const int p = (int)n[0] + shift;
    if (p < MIN_PITCH || p > MAX_PITCH) continue;
    const double a = n[1] * factor, b = n[2] * factor;
    const double af = a * fps, bf = b * fps;
    // (frames beyond the song, or times no song has: no cell)
    if (!(af > -1.0) || !(af < (double)nf) || !(bf < 4e15)) continue;
    const long sf = (long)af;
    const long e = (long)ceil(bf);
    long ef = e > sf + 1 ? e : sf + 1;
    if (ef > nf) ef = nf;
    const uint8_t fb = (uint8_t)((int)n[3] + 1) & FINGER;
    uint8_t* col = reinterpret_cast<uint8_t*>(roll) + (p - MIN_PITCH);
    for (long t = sf + lane; t < ef; t += nl) {
      const uint8_t old = col[t * NKEYS];
      col[t * NKEYS] = (uint8_t)(ACTIVE | (old & ONSET) | (t == sf ? ONSET : 0) | fb);
    }
  }
  if (lane == 0 && s.n_cc > 0) {  // the frame's last CC64 event: 1 = released (value 0..63), 2 = held (64..127)
    for (int i = 0; i < s.n_cc; i++) {
      const double t = s.ccs[2 * i] * factor;
      const double f = t * fps;
      if (!(f > -1.0) || !(f < (double)nf)) continue;
      const long ev = (long)s.ccs[2 * i + 1] + 1;
      sus[(long)f] = 1 <= ev && ev <= 64 ? 1 : (65 <= ev && ev <= 128 ? 2 : 0);
    }
    uint8_t prev = 0;  // no event: the pedal stays where it was
    for (long f = 0; f < nf; f++) {
      const uint8_t c = sus[f];
      prev = c == 1 ? 0 : (c == 2 ? 1 : prev);
      sus[f] = prev;
    }
  }
  psb_sync();
  bool over = false;
  for (long f = lane; f < nf; f += nl) {
    int c = 0;
    for (int w = 0; w < ROW_WORDS; w++) c += __builtin_popcount(goal_word(roll, f, w));
    over |= c > MAX_NOTES;
  }
  return psb_any(over) ? -1 : nf;
}

// rows [0, nbuf + nf) of one env's tables from the roll (pss_song_tables' second half)
PSB_HD void write_tables(const uint32_t* roll, const uint8_t* sus, long nf, long nbuf, float* goal, int32_t* count,
                         int32_t* keys, int32_t* fingers, int lane, int nl) {
  for (long t = lane; t < nbuf + nf; t += nl) {
    float* g = goal + t * GOAL_ROW;
    int32_t *kk = keys + t * MAX_NOTES, *ff = fingers + t * MAX_NOTES;
    const long f = t - nbuf;
    int c = 0;
    for (int w = 0; w < ROW_WORDS; w++) {
      const uint32_t on = f >= 0 ? goal_word(roll, f, w) : 0u;
      const uint32_t v = f >= 0 ? roll[f * ROW_WORDS + w] : 0u;
      for (int j = 0; j < 4; j++) {
        const bool hit = (on >> (8 * j + 7)) & 1u;
        g[4 * w + j] = hit ? 1.f : 0.f;
        if (hit && c < MAX_NOTES) {
          kk[c] = 4 * w + j;
          ff[c] = (int)((v >> (8 * j)) & FINGER) - 1;
          c++;
        }
      }
    }
    g[NKEYS] = f >= 0 ? (float)sus[f] : 0.f;
    count[t] = c;
    for (; c < MAX_NOTES; c++) kk[c] = ff[c] = -1;
  }
}

// One env's episode: the tables of the song at (factor, shift), or - when that does not fit
// T_cap rows or MAX_NOTES keys per frame - of the song as given (factor 1, shift 0), which is
// counted in *fell_back. -> T, or -1 when the song as given does not fit either (the host
// checks every song of the bank: never) and nothing was written.
PSB_HD int build_env(const Song& s, double factor, int shift, double fps, long nbuf, long T_cap, uint32_t* roll,
                     uint8_t* sus, float* goal, int32_t* count, int32_t* keys, int32_t* fingers, int* fell_back,
                     int lane, int nl) {
  const long F_cap = T_cap - nbuf;
  long nf = build_roll(s, factor, shift, fps, F_cap, roll, sus, lane, nl);
  *fell_back = nf < 0;
  if (nf < 0) nf = build_roll(s, 1.0, 0, fps, F_cap, roll, sus, lane, nl);
  if (nf < 0) return -1;
  write_tables(roll, sus, nf, nbuf, goal, count, keys, fingers, lane, nl);
  return (int)(nbuf + nf);
}

}  // namespace psb
#endif
