/*
 * pianosong.h - C-ABI of the native song ingestion: MIDI
 * file -> note sequence -> the per-control-step song tables ps_create consumes.
 *
 * The reference does this in Python on top of note_seq / pretty_midi (neither is
 * installable here); each entry point restates one reference function, with the
 * semantics of the library call underneath it:
 *
 *   pss_parse_midi      <- MidiFile.from_file / note_seq.midi_file_to_note_sequence
 *                          (robopianist/music/midi_file.py:179; pretty_midi's note pairing:
 *                          an off closes every open (channel, pitch) note started at an
 *                          earlier tick; instruments keyed (track, channel, program) in
 *                          first-seen order; merged tempo map, default 120 qpm).
 *   pss_add_fingering   <- add_fingering_from_annotation_file
 *                          (data_processing/add_fingering_to_midi.py:26-83).
 *   pss_trim_silence    <- MidiFile.trim_silence (midi_file.py:231-237) with
 *                          note_seq.sequences_lib.extract_subsequence semantics.
 *   pss_song_tables     <- NoteTrajectory.seq_to_trajectory (midi_file.py:315-362) over
 *                          sequence_to_pianoroll (piano_roll.py:59-204, onset_window 0),
 *                          add_initial_buffer_time (midi_file.py:388-401), and the goal /
 *                          finger tables of piano_with_shadow_hands.py:371-412.
 *
 * Host memory only (init-time work). 0 = OK, < 0 = error, message in pss_last_error()
 * (thread-local), e.g. a truncated file, an SMPTE division, a pitch outside the piano,
 * an annotation line with a malformed pitch.
 */
#ifndef PIANOSONG_H
#define PIANOSONG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t pitch;
  double start_time, end_time;
  int32_t velocity;
  int32_t part; /* fingering: 0-4 right hand, 5-9 left hand (note_seq Note.part) */
} pss_note;

typedef struct {
  double time;
  int32_t control_number, control_value;
} pss_cc;

typedef struct pss_seq pss_seq; /* owns a note sequence */

const char* pss_last_error(void);
int pss_version(void);

int pss_parse_midi(const uint8_t* data, size_t len, pss_seq** out);
int pss_from_notes(const pss_note* notes, int n_notes, const pss_cc* ccs, int n_cc, double total_time, pss_seq** out);
void pss_free(pss_seq* seq);

/* sizes, then copy-out (either array may be NULL) */
int pss_info(const pss_seq* seq, int* n_notes, int* n_cc, double* total_time, int* has_fingering);
int pss_get(const pss_seq* seq, pss_note* notes, pss_cc* ccs);

int pss_add_fingering(pss_seq* seq, const char* annotation_text);
int pss_trim_silence(pss_seq* seq);

/* Tables of T control steps: goal [T][89] (keys active at t, then the sustain target),
 * count [T], keys / fingers [T][max_notes] (pitch order, -1 padded). Call with goal == NULL
 * to get T only; otherwise T must be <= max_T. */
int pss_song_tables(const pss_seq* seq, double dt, double initial_buffer_time, int max_T, int max_notes,
                    float* goal, int32_t* count, int32_t* keys, int32_t* fingers, int* T);

/* MidiFile.stretch / MidiFile.transpose (midi_file.py:204-229), in place. note_seq is absent
 * here; the semantics of the two sequences_lib calls underneath are restated from upstream
 * knowledge, as pretty_midi's are above:
 *   stretch_note_sequence: every note start and end, every control-change time and total_time
 *     are multiplied by the factor (fp64); factor 1.0 is a no-op; factor <= 0 is an error.
 *   transpose_note_sequence(min 21, max 108): pitch += amount; a note that leaves the piano is
 *     removed, and when one was removed total_time becomes the last end of the notes that stay;
 *     amount 0 is a no-op. */
int pss_stretch(pss_seq* seq, double factor);
int pss_transpose(pss_seq* seq, int amount);

/* The per-episode MIDI augmentations (suite/variations.py; ps_set_augmentations of pianosim.h).
 * A song in the form the device builder reads: notes (pitch, start, end, part) as fp64, stably
 * sorted by start time; the CC64 events (time, value) in sequence order; total_time; a bit per
 * MIDI pitch that occurs (word p / 32, bit p % 32). pss_flatten writes it (notes [n_notes][4],
 * ccs [n_cc64][2]; either may be NULL to get the sizes) and refuses a song the builder cannot
 * take: no notes, a pitch off the piano, a velocity <= 0, a negative time, a part outside -1..61. */
typedef struct {
  const double* notes;
  const double* ccs;
  int32_t n_notes, n_cc;
  double total_time;
  uint32_t pitch_mask[4];
} pss_flat_song;
typedef struct {
  int32_t kind; /* 1 MidiSelect, 2 MidiTemporalStretch, 3 MidiPitchShift, 4 MidiOctaveShift */
  double prob, range;
} pss_variation;
int pss_flatten(const pss_seq* seq, double* notes, double* ccs, int* n_cc64, double* total_time,
                uint32_t* pitch_mask);
/* The device builder's own code (csrc/song_build.h) on the host: the tables of `song` stretched
 * by factor and transposed by shift, equal to pss_song_tables(pss_transpose(pss_stretch(seq)))
 * with max_notes 16. goal [T_cap][89], count [T_cap], keys / fingers [T_cap][16]; rows >= *T are
 * left alone. When the result would have more than T_cap rows or more than 16 keys in a row,
 * the tables are those of the song as given and *fell_back is 1. */
int pss_build_tables(const pss_flat_song* song, double factor, int shift, double dt, double initial_buffer_time,
                     int T_cap, float* goal, int32_t* count, int32_t* keys, int32_t* fingers, int* T,
                     int* fell_back);
/* The builder's draw of (seed, global env, episode) over a bank whose song 0 is the task's own
 * (variations.draw in Python is its specification). */
int pss_draw_augmentation(uint64_t seed, uint32_t env, uint32_t episode, const pss_variation* vars, int n_vars,
                          const pss_flat_song* bank, int n_songs, int* song, double* factor, int* shift);

/* The sequence as a Standard MIDI File (the reference exports through note_seq's
 * note_sequence_to_midi_file, midi_file.py:186-188): format 0, one track, 1000 ticks per quarter
 * note and one tempo event of 500000 us per quarter note, i.e. 2000 ticks per second - a time on
 * the 5 ms physics grid is a whole number of ticks. Times are rounded to the nearest tick; events
 * are sorted by tick, at one tick note-offs before control changes before note-ons (a re-strike
 * of a pitch at the tick its previous note ends reads back as two notes); a note shorter than
 * a tick lasts one; channel 0; control values as given. Returns the file's size in bytes and,
 * when out is not NULL, writes it (capacity must be at least the size). < 0: a pitch, velocity,
 * controller number or value outside 0..127, a negative or non-finite time (total_time
 * included), a buffer too small. */
int64_t pss_write_smf(const pss_seq* seq, uint8_t* out, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif
