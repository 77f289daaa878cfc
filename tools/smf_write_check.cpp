// smf_write_check.cpp - the Standard MIDI File writer of csrc/song.cpp (pss_write_smf) behind a
// main of its own, compiled together with song.cpp by g++ alone (tests/test_midi_record.py builds
// it with -fsanitize=address,undefined: the writer's buffers and shifts under the sanitizers,
// nothing loaded into Python). It writes a sequence with chords, a re-strike of a pitch at the
// tick its previous note ends, notes shorter than a tick, pedal changes and a long gap (a
// four-byte delta time), reads the file back with pss_parse_midi and compares; then the
// refusals. Prints "ok <bytes>" and returns 0, or the first mismatch and 1.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../include/pianosong.h"

static int bad(const char* what) {
  printf("FAILED %s: %s\n", what, pss_last_error());
  return 1;
}

int main() {
  std::vector<pss_note> notes;
  for (int i = 0; i < 40; i++) {  // chords of three on the 5 ms grid, each pitch re-struck at once
    const double t = 0.005 * (3 * i);
    for (int p : {21 + i, 60 + i % 12, 108 - i}) {
      notes.push_back({p, t, t + 0.010, 127, 0});
      notes.push_back({p, t + 0.010, t + 0.015, 1 + i, 0});
    }
  }
  notes.push_back({0, 0.0, 0.0001, 5, 0});       // shorter than a tick: lasts one
  notes.push_back({127, 2000.0, 2000.5, 127, 0});  // a delta time of four bytes before it
  std::vector<pss_cc> ccs = {{0.0, 64, 64}, {0.25, 64, 0}, {0.25, 64, 64}, {1.0, 64, 0}, {1.5, 7, 127}};
  pss_seq* seq = nullptr;
  if (pss_from_notes(notes.data(), (int)notes.size(), ccs.data(), (int)ccs.size(), 2001.0, &seq)) return bad("from_notes");
  const int64_t size = pss_write_smf(seq, nullptr, 0);
  if (size <= 22) return bad("size query");
  std::vector<uint8_t> file((size_t)size);
  if (pss_write_smf(seq, file.data(), file.size()) != size) return bad("write");
  if (memcmp(file.data(), "MThd", 4) || file[9] != 0 || file[12] != 0x03 || file[13] != 0xE8) return bad("header");
  // one byte short: refused, nothing written past the buffer (the sanitizer watches the heap block)
  std::vector<uint8_t> small((size_t)size - 1);
  if (pss_write_smf(seq, small.data(), small.size()) >= 0) return bad("short buffer accepted");
  pss_seq* back = nullptr;
  if (pss_parse_midi(file.data(), file.size(), &back)) return bad("parse");
  int nn = 0, nc = 0;
  double total = 0;
  pss_info(back, &nn, &nc, &total, nullptr);
  if (nn != (int)notes.size() || nc != (int)ccs.size()) return bad("counts");
  std::vector<pss_note> got((size_t)nn);
  std::vector<pss_cc> gotc((size_t)nc);
  pss_get(back, got.data(), gotc.data());
  auto key = [](const pss_note& a, const pss_note& b) {
    return a.start_time != b.start_time ? a.start_time < b.start_time : a.pitch < b.pitch;
  };
  std::sort(notes.begin(), notes.end(), key);
  std::sort(got.begin(), got.end(), key);
  for (int i = 0; i < nn; i++) {
    const double end = std::max(notes[i].end_time, notes[i].start_time + 0.0005);
    if (got[i].pitch != notes[i].pitch || got[i].velocity != notes[i].velocity ||
        fabs(got[i].start_time - notes[i].start_time) > 1e-9 || fabs(got[i].end_time - end) > 1e-9) {
      printf("FAILED note %d: %d %.6f %.6f %d\n", i, got[i].pitch, got[i].start_time, got[i].end_time, got[i].velocity);
      return 1;
    }
  }
  for (int i = 0; i < nc; i++)
    if (gotc[i].control_number != ccs[i].control_number || gotc[i].control_value != ccs[i].control_value ||
        fabs(gotc[i].time - ccs[i].time) > 1e-9)
      return bad("control change");
  pss_free(back);
  pss_free(seq);
  // refusals: every field out of 0..127, a negative and a non-finite time
  const pss_note bad_notes[] = {{128, 0, 1, 80, 0}, {-1, 0, 1, 80, 0}, {60, 0, 1, 128, 0}, {60, 0, 1, -1, 0},
                                {60, -0.5, 1, 80, 0}, {60, 0, NAN, 80, 0}, {60, 0, 1e12, 80, 0}};
  for (const pss_note& n : bad_notes) {
    if (pss_from_notes(&n, 1, nullptr, 0, 1.0, &seq)) return bad("from_notes");
    if (pss_write_smf(seq, nullptr, 0) >= 0) return bad("a bad note accepted");
    pss_free(seq);
  }
  const pss_cc bad_ccs[] = {{0, 64, 128}, {0, 128, 0}, {0, 64, -1}, {-1, 64, 0}};
  for (const pss_cc& c : bad_ccs) {
    if (pss_from_notes(nullptr, 0, &c, 1, 1.0, &seq)) return bad("from_notes");
    if (pss_write_smf(seq, nullptr, 0) >= 0) return bad("a bad control change accepted");
    pss_free(seq);
  }
  for (double tt : {-1.0, (double)NAN, 1e12}) {  // total_time is held to the same rule
    if (pss_from_notes(nullptr, 0, nullptr, 0, tt, &seq)) return bad("from_notes");
    if (pss_write_smf(seq, nullptr, 0) >= 0) return bad("a bad total_time accepted");
    pss_free(seq);
  }
  // an empty sequence is a valid file: tempo and end of track
  if (pss_from_notes(nullptr, 0, nullptr, 0, 0.0, &seq)) return bad("from_notes");
  if (pss_write_smf(seq, nullptr, 0) != 14 + 8 + 7 + 4) return bad("empty sequence");
  pss_free(seq);
  printf("ok %lld\n", (long long)size);
  return 0;
}
