"""Generate tests/golden/augment.json: the reference's trajectories of stretched and
transposed songs.

Like make_golden.py (whose stubs and loader it uses) this runs only where the reference
checkout is present. note_seq is absent, so ``MidiFile.stretch`` / ``.transpose``
(midi_file.py:204-229) cannot run; the few lines of ``_stretch`` / ``_transpose`` below RESTATE
note_seq's ``stretch_note_sequence`` / ``transpose_note_sequence`` on the stub sequences (they
are this generator's own, not the repo's native code), and the reference's unmodified
``NoteTrajectory.seq_to_trajectory`` is then run on the result. The fixture stores T and the
non-empty note and sustain steps only; Guren is left out to keep it small.

Usage: python tests/golden/make_augment_golden.py
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402

FACTORS = (0.5, 0.8, 1.0, 1.3, 1.5)
SHIFTS = (-2, 0, 3)


def _copy(seq):
    out = mg.NoteSequence()
    for n in seq.notes:
        out.notes.add(pitch=n.pitch, start_time=n.start_time, end_time=n.end_time, velocity=n.velocity, part=n.part)
    for c in seq.control_changes:
        out.control_changes.add(time=c.time, control_number=c.control_number, control_value=c.control_value)
    out.total_time = seq.total_time
    return out


def _stretch(seq, factor):
    """note_seq.sequences_lib.stretch_note_sequence, restated: 1.0 is a no-op, otherwise every
    note / control-change time and total_time are multiplied by the factor."""
    out = _copy(seq)
    if factor == 1.0:
        return out
    for n in out.notes:
        n.start_time *= factor
        n.end_time *= factor
    for c in out.control_changes:
        c.time *= factor
    out.total_time *= factor
    return out


def _transpose(seq, amount, lo=21, hi=108):
    """note_seq.sequences_lib.transpose_note_sequence(min 21, max 108), restated: notes that
    leave the range are removed; when one was, total_time is the last end of those that stay."""
    out = mg.NoteSequence()
    end = 0.0
    for n in seq.notes:
        if lo <= n.pitch + amount <= hi:
            out.notes.add(pitch=n.pitch + amount, start_time=n.start_time, end_time=n.end_time,
                          velocity=n.velocity, part=n.part)
            end = max(end, n.end_time)
    for c in seq.control_changes:
        out.control_changes.add(time=c.time, control_number=c.control_number, control_value=c.control_value)
    out.total_time = seq.total_time if len(out.notes) == len(seq.notes) else end
    return out


def _songs(lib):
    """name -> (stub sequence, dt): the three reference test MIDIs (midi_file_test.py:109-177,
    piano_with_shadow_hands_test.py:29-52), Twinkle, Crossing Field (repo parse + trim)."""
    out = {"twinkle": (lib.twinkle_twinkle_little_star_one_hand().seq, 0.05)}
    seq = mg.NoteSequence()
    seq.notes.add(start_time=0.01, end_time=0.02, velocity=80, pitch=84, part=-1)
    seq.notes.add(start_time=0.02, end_time=0.05, velocity=80, pitch=84, part=-1)
    seq.total_time = 0.05
    out["test_restrike"] = (seq, 0.01)
    seq = mg.NoteSequence()
    seq.notes.add(start_time=0.0, end_time=0.01, velocity=80, pitch=84, part=-1)
    seq.control_changes.add(time=0.0, control_number=64, control_value=64)
    seq.control_changes.add(time=0.03, control_number=64, control_value=0)
    seq.notes.add(start_time=0.05, end_time=0.06, velocity=80, pitch=84, part=-1)
    seq.total_time = 0.06
    out["test_sustain"] = (seq, 0.01)
    seq = mg.NoteSequence()
    seq.notes.add(start_time=0.0, end_time=0.02, velocity=80, pitch=84, part=1)
    seq.notes.add(start_time=0.02, end_time=0.03, velocity=80, pitch=79, part=0)
    seq.total_time = 0.03
    out["test_task"] = (seq, 0.01)
    cf = mg.our_music.trim_silence(mg.our_music.parse_midi(mg.REF / "midi_files_cut/Crossing Field Cut 10s.mid"))
    out["crossing_field"] = (mg._to_ref_seq(cf), 0.05)
    return out


def main():
    mg._install_stubs()
    mg._load("robopianist.music.constants", mg.REF / "robopianist/music/constants.py")
    mg._load("robopianist.music.piano_roll", mg.REF / "robopianist/music/piano_roll.py")
    mf = mg._load("robopianist.music.midi_file", mg.REF / "robopianist/music/midi_file.py")
    lib = mg._load("robopianist.music.library", mg.REF / "robopianist/music/library.py")
    rec = {"source": "reference seq_to_trajectory on sequences stretched / transposed by this generator's "
                     "restatement of note_seq", "factors": FACTORS, "shifts": SHIFTS, "cases": []}
    for name, (seq, dt) in _songs(lib).items():
        for f in FACTORS:
            for s in SHIFTS:
                notes, sustains = mf.NoteTrajectory.seq_to_trajectory(_transpose(_stretch(seq, f), s), dt)
                rec["cases"].append({
                    "song": name, "dt": dt, "factor": f, "shift": s, "T": len(notes),
                    # sparse: [t, [[key, finger], ...]] of the non-empty steps, the steps with the pedal down
                    "notes": [[t, [[int(n.key), int(n.fingering)] for n in step]] for t, step in enumerate(notes) if step],
                    "sustained": [t for t, v in enumerate(sustains) if v],
                })
    out = mg.OUT / "augment.json"
    out.write_text(json.dumps(rec, separators=(",", ":")))
    print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
