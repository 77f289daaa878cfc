// midi_events.inc - the piano's sound module on the device (robopianist/models/piano/
// midi_module.py, driven after every physics substep from piano.py:154-162): midi_events_kernel,
// enqueued by launch() after the step / reset kernel of a handle that has ps_record_midi. The
// step kernel leaves, per env, the key and sustain activations at the end of every substep of
// the launch (Bufs::keybits, kernel_v2.inc); this kernel turns the rows into the module's
// messages - what changed against the previous substep - and appends them to the env's running
// episode. One wave per env, the env's state in registers, every lane's output position from a
// rank in a mask (mbcnt): no LDS, no atomics. No host sync, no allocation: legal under stream
// capture.
//
// An event word: bits 0-7 the MIDI note number (key + 21; 0 for the pedal), bits 8-9 the kind,
// bits 10-31 the substep's ordinal in the episode (first substep = 1): its time is ordinal *
// timestep, physics.data.time after that substep.
enum : int { MIDI_NOTE_ON = 0, MIDI_NOTE_OFF, MIDI_SUSTAIN_ON, MIDI_SUSTAIN_OFF };
constexpr int MIDI_ORD_SHIFT = 10;
constexpr uint32_t MIDI_ORD_MAX = (1u << 22) - 1;  // (5.8 h of 5 ms substeps; later ones keep this ordinal)
constexpr int MIDI_FIRST_PITCH = 21;               // robopianist/music/constants.py MIN_MIDI_PITCH_PIANO

// Per env: two banks of events - the running episode's and the last finished one's - and the
// recorder's words (MS_*): per bank the events held, the events that did not fit, the episode's
// substeps so far; which bank is running; the activations after the last substep seen.
enum : int { MS_COUNT = 0, MS_DROPPED = 2, MS_SUBSTEPS = 4, MS_BANK = 6, MS_PREV = 7, MS_WORDS = MS_PREV + KB_ROW };
struct MidiRec {
  uint32_t* events;  // [N][2][max_events]
  int* state;        // [N][MS_WORDS]
  int max_events;
};

__device__ __forceinline__ uint32_t midi_word(int note, int kind, uint32_t ordinal) {
  return (uint32_t)note | (uint32_t)kind << 8 | ordinal << MIDI_ORD_SHIFT;
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// rows: env e's are bits[e * stride + KB_ROW * s], s < the header's count (hdr[e * hdr_stride];
// cleared here, so a later launch that skips the env adds nothing) or, when hdr is null
// (ps_midi_push), fixed_rows.
__global__ void __launch_bounds__(64) midi_events_kernel(MidiRec r, const uint32_t* bits, size_t stride,
                                                         uint32_t* hdr, size_t hdr_stride,
                                                         int fixed_rows, int n) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= n) return;
  int* st = r.state + (size_t)e * MS_WORDS;
  int rows = fixed_rows;
  if (hdr) {
    const uint32_t h = (uint32_t)uni((int)hdr[(size_t)e * hdr_stride]);
    if (h == 0) return;
    if (h == KB_NEW_EPISODE) {
      // the running episode becomes the last finished one; the other bank starts empty
      if (lane == 0) {
        const int bank = st[MS_BANK] ^ 1;
        st[MS_BANK] = bank;
        st[MS_COUNT + bank] = st[MS_DROPPED + bank] = st[MS_SUBSTEPS + bank] = 0;
        for (int i = 0; i < KB_ROW; i++) st[MS_PREV + i] = 0;
        hdr[(size_t)e * hdr_stride] = 0;
      }
      return;
    }
    rows = (int)h;
  }
  const uint32_t* rw = bits + (size_t)e * stride;
  const int bank = uni(st[MS_BANK]) & 1;
  uint32_t p0 = (uint32_t)uni(st[MS_PREV]), p1 = (uint32_t)uni(st[MS_PREV + 1]), p2 = (uint32_t)uni(st[MS_PREV + 2]);
  const int total = uni(st[MS_SUBSTEPS + bank]);
  constexpr uint32_t W2 = (2u << KB_SUSTAIN_BIT) - 1;  // the 24 keys and the pedal of word 2
  // did anything change in this launch? lane s compares row s with the one before it
  bool any = false;
  for (int s = lane; s < rows; s += 64) {
    const uint32_t* c = rw + (size_t)KB_ROW * s;
    const uint32_t q0 = s ? c[-3] : p0, q1 = s ? c[-2] : p1, q2 = s ? c[-1] : p2;
    any |= ((c[0] ^ q0) | (c[1] ^ q1) | ((c[2] ^ q2) & W2)) != 0;
  }
  if (__ballot(any)) {
    uint32_t* ev = r.events + ((size_t)e * 2 + bank) * (size_t)r.max_events;
    int count = uni(st[MS_COUNT + bank]), dropped = uni(st[MS_DROPPED + bank]);
    for (int s = 0; s < rows; s++) {
      const uint32_t b0 = (uint32_t)uni((int)rw[KB_ROW * s]), b1 = (uint32_t)uni((int)rw[KB_ROW * s + 1]),
                     b2 = (uint32_t)uni((int)rw[KB_ROW * s + 2]) & W2;
      const uint32_t c0 = b0 ^ p0, c1 = b1 ^ p1, c2 = b2 ^ p2;
      p0 = b0; p1 = b1; p2 = b2;
      if (!(c0 | c1 | c2)) continue;
      const uint32_t ord = min((uint32_t)(total + s) + 1u, MIDI_ORD_MAX);
      // lane l owns keys l and l + 64; the reference's order inside one substep: NoteOns by key,
      // NoteOffs by key, SustainOn, SustainOff (midi_module.py:63-94)
      const uint64_t cur[2] = {(uint64_t)b1 << 32 | b0, (uint64_t)(b2 & 0xffffffu)};
      const uint64_t chg[2] = {(uint64_t)c1 << 32 | c0, (uint64_t)(c2 & 0xffffffu)};
      int base = count;
#pragma unroll
      for (int kind = MIDI_NOTE_ON; kind <= MIDI_NOTE_OFF; kind++) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const uint64_t mk = chg[j] & (kind == MIDI_NOTE_ON ? cur[j] : ~cur[j]);
          const int pos = base + lanes_below(mk, lane);
          if (((mk >> lane) & 1) && pos < r.max_events) ev[pos] = midi_word(MIDI_FIRST_PITCH + lane + 64 * j, kind, ord);
          base += __popcll(mk);
        }
      }
      if ((c2 >> KB_SUSTAIN_BIT) & 1) {
        if (lane == 0 && base < r.max_events)
          ev[base] = midi_word(0, (b2 >> KB_SUSTAIN_BIT) & 1 ? MIDI_SUSTAIN_ON : MIDI_SUSTAIN_OFF, ord);
        base++;
      }
      count = min(base, r.max_events);  // an event that does not fit is counted, not written
      dropped += base - count;
    }
    if (lane == 0) {
      st[MS_COUNT + bank] = count;
      st[MS_DROPPED + bank] = dropped;
      st[MS_PREV] = (int)p0; st[MS_PREV + 1] = (int)p1; st[MS_PREV + 2] = (int)p2;
    }
  }
  if (lane == 0) {
    st[MS_SUBSTEPS + bank] = total + rows;
    if (hdr) hdr[(size_t)e * hdr_stride] = 0;
  }
}

// ps_midi_events: bank `which` (0 the running episode, 1 the last finished one) of every env,
// gathered into the caller's arrays (any may be null); the words past an env's count read 0
__global__ void __launch_bounds__(256) midi_gather_kernel(MidiRec r, int which, uint32_t* __restrict__ events,
                                                          int* __restrict__ count, int* __restrict__ dropped,
                                                          int* __restrict__ substeps, int n) {
  const int e = blockIdx.x;
  if (e >= n) return;
  const int* st = r.state + (size_t)e * MS_WORDS;
  const int bank = (st[MS_BANK] ^ which) & 1;
  if (events) {
    const uint32_t* src = r.events + ((size_t)e * 2 + bank) * (size_t)r.max_events;
    uint32_t* dst = events + (size_t)e * r.max_events;
    const int cnt = st[MS_COUNT + bank];
    for (int i = threadIdx.x; i < r.max_events; i += blockDim.x) dst[i] = i < cnt ? src[i] : 0u;
  }
  if (threadIdx.x == 0) {
    if (count) count[e] = st[MS_COUNT + bank];
    if (dropped) dropped[e] = st[MS_DROPPED + bank];
    if (substeps) substeps[e] = st[MS_SUBSTEPS + bank];
  }
}
