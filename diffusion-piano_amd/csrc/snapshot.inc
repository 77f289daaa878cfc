// snapshot.inc - whole-env snapshots on the device (ps_snapshot_*, include/pianosim.h): the row
// table and the one copy kernel that save and restore share. Included by pianosim.hip after
// struct ps_env.
//
// A row table entry names one per-env buffer of the handle: where env 0's row starts, the bytes
// between two envs' rows there (the row's size for all but the MIDI capture header, one word of a
// longer row), where the snapshot keeps env 0's copy, and the row's size. The table is built
// once, by ps_snapshot_create, and passed to the kernel by value: save and restore walk the same
// list and cannot disagree about what an env is. In the snapshot every buffer starts 256-byte
// aligned and its rows are the env's rows rounded up to 16 bytes.
constexpr int SNAP_MAX_ROWS = 32;
constexpr int SNAP_THREADS = 256;
struct SnapRow {
  char* env;            // env 0's row in the handle
  char* snap;           // env 0's row in the snapshot
  uint32_t env_stride;  // bytes from one env's row to the next in the handle
  uint32_t snap_stride; // ... in the snapshot (bytes rounded up to 16)
  uint32_t bytes;       // the row
  uint32_t width;       // 16, 4 or 1: the widest access bytes, both strides and both bases allow
};
struct SnapTable {
  SnapRow row[SNAP_MAX_ROWS];
  int n;
};

struct ps_snapshot {
  ps_env* owner;
  uint64_t config;  // the owner's row-set generation at create
  SnapTable table;
  uint64_t bytes;
  int device;
  DevMem mem;
};

template <class V>
__device__ __forceinline__ void snap_copy(char* __restrict__ to, const char* __restrict__ from, uint32_t bytes) {
  const uint32_t n = bytes / (uint32_t)sizeof(V);
  V* __restrict__ d = reinterpret_cast<V*>(to);
  const V* __restrict__ s = reinterpret_cast<const V*>(from);
  uint32_t i = threadIdx.x;
  // four loads in flight per thread before the first store (the long rows: song tables, event banks)
  for (; i + 3 * SNAP_THREADS < n; i += 4 * SNAP_THREADS) {
    const V a = s[i], b = s[i + SNAP_THREADS], c = s[i + 2 * SNAP_THREADS], e = s[i + 3 * SNAP_THREADS];
    d[i] = a;
    d[i + SNAP_THREADS] = b;
    d[i + 2 * SNAP_THREADS] = c;
    d[i + 3 * SNAP_THREADS] = e;
  }
  for (; i < n; i += SNAP_THREADS) d[i] = s[i];
}

// One workgroup per destination env. RESTORE: env e takes the snapshot's row src[e] (its own when
// src is null); src[e] == -1 skips the env, another index outside [0, n) skips it and counts in
// *n_bad. It reads snapshot memory only and writes env memory only. Save (not RESTORE): the
// snapshot's row e takes env e.
template <bool RESTORE>
__global__ void __launch_bounds__(SNAP_THREADS) snapshot_copy_kernel(const SnapTable t, const int* __restrict__ src,
                                                                     int* __restrict__ n_bad, int n) {
  const int e = blockIdx.x;
  if (e >= n) return;
  int s = e;
  if (RESTORE && src) {
    s = src[e];
    if (s == -1) return;
    if (s < 0 || s >= n) {
      if (threadIdx.x == 0 && n_bad) atomicAdd(n_bad, 1);
      return;
    }
  }
  for (int r = 0; r < t.n; r++) {
    const SnapRow row = t.row[r];
    char* in_env = row.env + (size_t)e * row.env_stride;
    char* in_snap = row.snap + (size_t)s * row.snap_stride;
    char* to = RESTORE ? in_env : in_snap;
    const char* from = RESTORE ? in_snap : in_env;
    if (row.width == 16) snap_copy<uint4>(to, from, row.bytes);
    else if (row.width == 4) snap_copy<uint32_t>(to, from, row.bytes);
    else snap_copy<uint8_t>(to, from, row.bytes);
  }
}

// the handle's per-env buffers, in the order of the list in pianosim.h
static int snapshot_rows(const ps_env* E, SnapTable& t, std::string& err) {
  t.n = 0;
  auto add = [&](const void* base, size_t bytes, size_t env_stride) {
    if (t.n >= SNAP_MAX_ROWS || bytes > 0xffffffffu || env_stride > 0xffffffffu) {
      err = "ps_snapshot_create: a row over 4 GiB, or more than SNAP_MAX_ROWS rows";
      return;
    }
    SnapRow& r = t.row[t.n++];
    r.env = (char*)base;
    r.snap = nullptr;
    r.env_stride = (uint32_t)env_stride;
    r.bytes = (uint32_t)bytes;
    r.snap_stride = (uint32_t)((bytes + 15) & ~(size_t)15);
    r.width = (bytes % 16 == 0 && env_stride % 16 == 0 && (uintptr_t)base % 16 == 0) ? 16
              : (bytes % 4 == 0 && env_stride % 4 == 0 && (uintptr_t)base % 4 == 0) ? 4 : 1;
  };
  auto row = [&](const void* base, size_t bytes) { add(base, bytes, bytes); };
  row(E->qpos, sizeof(float) * NV);
  row(E->qvel, sizeof(float) * NV);
  row(E->qws, sizeof(float) * NV);
  row(E->ctrl, sizeof(float) * NU);
  row(E->sustain, sizeof(float));
  row(E->t_idx, sizeof(int));
  row(E->last, sizeof(uint8_t));
  row(E->applied, sizeof(float) * NV);  // (kept whether ps_set_applied is on: the rows are there)
  row(E->terms, sizeof(float) * PS_NTERMS);
  row(E->tips, sizeof(float) * 2 * PS_NFINGER * 3);
  row(E->ncon, sizeof(int));
  row(E->stats, sizeof(int) * PS_NSTATS);
  row(E->warnings, sizeof(int) * PS_NWARN);
  row(E->mus_acc, sizeof(float) * PS_NMUSIC);
  row(E->mus_ep, sizeof(float) * PS_NMUSIC);
  row(E->mus_cnt, sizeof(int));
  row(E->hand_dy, sizeof(float));
  row(E->episode, sizeof(int));
  if (E->aug_on) {
    const AugDev& a = E->aug;
    const size_t Tc = (size_t)a.T_cap;
    row(a.song, sizeof(int));
    row(a.factor, sizeof(double));
    row(a.shift, sizeof(int));
    row(a.T, sizeof(int));
    row(a.fallbacks, sizeof(int));
    row(a.goal, sizeof(float) * Tc * (NK + 1));
    row(a.count, sizeof(int) * Tc);
    row(a.keys, sizeof(int) * Tc * PS_MAX_NOTES);
    row(a.fingers, sizeof(int) * Tc * PS_MAX_NOTES);
  }
  if (E->con_out) row(E->con_out, sizeof(Contact) * MAXCON);
  if (E->keybits) {
    row(E->midi.events, sizeof(uint32_t) * 2 * (size_t)E->midi.max_events);
    row(E->midi.state, sizeof(int) * MS_WORDS);
    // (the capture rows past the header are rewritten by every launch before midi_events_kernel reads them)
    add(E->keybits, sizeof(uint32_t) * KB_HDR, sizeof(uint32_t) * ((size_t)KB_HDR + (size_t)E->nsub * KB_ROW));
  }
  return err.empty() ? 0 : -1;
}
