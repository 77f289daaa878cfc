"""The sound module's host side (no GPU): music.events_from_activations - the specification the
device recorder is held to (tests/test_gpu_midi_record.py) - against the reference's own
MidiModule (tests/golden/midi_module.json, written by make_midi_module_golden.py from the
reference's unmodified code); the event word; messages -> NoteSequence; the Standard MIDI File
writer (pss_write_smf) through the parser it closes the loop with, and once under the address
and undefined-behaviour sanitizers in a stand-alone program."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def fixture_arrays(seq):
    act = np.zeros((len(seq["active_keys"]), 88), bool)
    for s, keys in enumerate(seq["active_keys"]):
        act[s, keys] = True
    return act, np.array(seq["sustain"], bool)


def test_fixture_has_the_cases(golden):
    g = golden["midi_module"]
    seqs = g["sequences"]
    assert g["kinds"] == {"NOTE_ON": 0, "NOTE_OFF": 1, "SUSTAIN_ON": 2, "SUSTAIN_OFF": 3}
    assert seqs["silent"]["messages"] == []
    per_substep = np.bincount([m[2] for m in seqs["all_switch"]["messages"]])
    assert per_substep.max() == 89  # all 88 keys and the pedal in one substep
    assert all(seqs[k]["control_values"] in ([], [[64, 0]], [[64, 64]], [[64, 0], [64, 64]]) for k in seqs)


@pytest.mark.parametrize("name", ["sparse", "dense", "all_switch", "silent", "word_edges"])
def test_events_from_activations_is_the_reference_module(dp, golden, name):
    g = golden["midi_module"]
    dt = g["timestep"]
    act, sus = fixture_arrays(g["sequences"][name])
    want = g["sequences"][name]["messages"]  # [kind, note, ordinal, time] in the module's order
    got = dp.music.events_from_activations(act, sus, dt)
    assert [[int(m.event_type), getattr(m, "note", 0), round(m.time / dt)] for m in got] == [m[:3] for m in want]
    for m, w in zip(got, want):
        assert m.time == w[2] * dt and abs(m.time - w[3]) < 1e-12
    words = dp.music.events_from_activations(act, sus, dt, words=True)
    note, kind, ordinal = dp.music.event_fields(words)
    assert np.column_stack([kind, note, ordinal]).tolist() == [m[:3] for m in want] or not want
    assert [(type(a), a) for a in dp.music.decode_events(words, len(words), dt)] == [(type(a), a) for a in got]
    # the reference's message fields: velocity 127, CC64 with 64 for on and 0 for off
    for m in got:
        if m.event_type == dp.music.EventType.NOTE_ON:
            assert m.velocity == 127
        elif m.event_type == dp.music.EventType.SUSTAIN_ON:
            assert (m.control, m.value) == (64, 64)
        elif m.event_type == dp.music.EventType.SUSTAIN_OFF:
            assert (m.control, m.value) == (64, 0)


def test_pack_activations_layout(dp):
    act = np.zeros((3, 88), bool)
    act[0, [0, 31]] = True
    act[1, [32, 63, 64]] = True
    act[2, 87] = True
    rows = dp.music.pack_activations(act, [False, True, True])
    assert rows.dtype == np.uint32
    assert rows.tolist() == [[0x80000001, 0, 0], [0, 0x80000001, 1 | 1 << 24], [0, 0, 1 << 23 | 1 << 24]]


def test_event_word_field_limits(dp):
    m = dp.music
    w = m.encode_event(108, 3, 2 ** 22 - 1)
    assert w == 108 | 3 << 8 | (2 ** 22 - 1) << 10 and w < 2 ** 32
    # the device tensor holds it as int32: the top ordinal bit is the sign bit
    as_i32 = np.array([w], np.uint32).view(np.int32)
    assert as_i32[0] < 0
    note, kind, ordinal = m.event_fields(as_i32)
    assert (int(note[0]), int(kind[0]), int(ordinal[0])) == (108, 3, 2 ** 22 - 1)
    assert [tuple(int(x[0]) for x in m.event_fields([m.encode_event(*f)])) for f in [(0, 0, 0), (21, 1, 1), (255, 2, 7)]] == \
        [(0, 0, 0), (21, 1, 1), (255, 2, 7)]
    for bad in [(256, 0, 0), (21, 4, 0), (21, 0, 2 ** 22), (-1, 0, 0)]:
        with pytest.raises(ValueError):
            m.encode_event(*bad)
    msgs = m.decode_events(as_i32, 1, 0.005)
    assert isinstance(msgs[0], m.SustainOff) and msgs[0].time == (2 ** 22 - 1) * 0.005
    assert m.decode_events(as_i32, 0, 0.005) == []


def test_sequence_from_messages(dp):
    m = dp.music
    msgs = [m.NoteOn(60, 127, 0.005), m.SustainOn(0.005), m.NoteOn(64, 127, 0.010), m.NoteOff(60, 0.020),
            m.NoteOn(60, 127, 0.020), m.SustainOff(0.030), m.NoteOff(60, 0.035), m.NoteOff(72, 0.040)]
    seq = m.sequence_from_messages(msgs, 0.050)
    assert [(n.pitch, n.start_time, n.end_time, n.velocity) for n in seq.notes] == \
        [(60, 0.005, 0.020, 127), (64, 0.010, 0.050, 127), (60, 0.020, 0.035, 127)]  # 64 hangs: closed at the end
    assert [(c.time, c.control_number, c.control_value) for c in seq.control_changes] == [(0.005, 64, 64), (0.030, 64, 0)]
    assert seq.total_time == 0.050
    empty = m.sequence_from_messages([], 0.0)
    assert empty.notes == [] and empty.control_changes == [] and empty.total_time == 0.0


def _roundtrip_sequence(m):
    seq = m.NoteSequence(title="round trip")
    for p in (48, 52, 55):  # a chord
        seq.notes.append(m.Note(p, 0.005, 0.105, 127, 0))
    seq.notes.append(m.Note(60, 0.010, 0.050, 90, 0))
    seq.notes.append(m.Note(60, 0.050, 0.075, 100, 0))  # re-struck at the tick the last one ends
    seq.notes.append(m.Note(60, 0.075, 0.080, 1, 0))    # and again
    for p in (21, 108, 64):  # another chord, the piano's ends
        seq.notes.append(m.Note(p, 0.200, 1.005, 127, 0))
    seq.control_changes = [m.ControlChange(0.005, 64, 64), m.ControlChange(0.150, 64, 0),
                           m.ControlChange(0.150, 64, 64), m.ControlChange(1.000, 64, 0)]
    seq.total_time = 1.005
    return seq


def test_to_smf_round_trip(dp, tmp_path):
    m = dp.music
    seq = _roundtrip_sequence(m)
    data = m.to_smf(seq)
    assert data[:4] == b"MThd" and data[4:8] == (6).to_bytes(4, "big")
    assert int.from_bytes(data[8:10], "big") == 0      # format 0
    assert int.from_bytes(data[10:12], "big") == 1     # one track
    assert int.from_bytes(data[12:14], "big") == 1000  # ticks per quarter note
    assert data[14:18] == b"MTrk" and int.from_bytes(data[18:22], "big") == len(data) - 22
    assert data[22:29] == bytes([0, 0xFF, 0x51, 3, 0x07, 0xA1, 0x20])  # 500000 us per quarter note
    path = tmp_path / "out.mid"
    m.write_midi(seq, path)
    assert path.read_bytes() == data
    back = m.parse_midi(path)
    key = lambda n: (n.start_time, n.pitch)
    want, got = sorted(seq.notes, key=key), sorted(back.notes, key=key)
    assert len(got) == len(want)
    for a, b in zip(want, got):
        assert (a.pitch, a.velocity) == (b.pitch, b.velocity)
        assert abs(a.start_time - b.start_time) <= 1e-9 and abs(a.end_time - b.end_time) <= 1e-9
    assert len(back.control_changes) == len(seq.control_changes)
    for a, b in zip(seq.control_changes, back.control_changes):
        assert (a.control_number, a.control_value) == (b.control_number, b.control_value) and abs(a.time - b.time) <= 1e-9
    assert abs(back.total_time - 1.005) <= 1e-9


def test_to_smf_refuses_out_of_range_values(dp):
    m = dp.music
    for note in (m.Note(128, 0.0, 0.1, 80), m.Note(-1, 0.0, 0.1, 80), m.Note(60, 0.0, 0.1, 128),
                 m.Note(60, -0.1, 0.1, 80)):
        seq = m.NoteSequence(notes=[note], total_time=0.1)
        with pytest.raises(ValueError, match="pss_write_smf"):
            m.to_smf(seq)
    for cc in (m.ControlChange(0.0, 64, 128), m.ControlChange(0.0, 128, 0)):
        with pytest.raises(ValueError, match="outside 0..127"):
            m.to_smf(m.NoteSequence(control_changes=[cc]))
    for total in (-1.0, float("nan"), 1e12):  # total_time is held to the rule of every other time
        with pytest.raises(ValueError, match="total_time"):
            m.to_smf(m.NoteSequence(total_time=total))
    assert m.to_smf(m.NoteSequence())[:4] == b"MThd"  # an empty performance is a valid file
    assert m.SustainOn(0.0).value == m.SUSTAIN_ON_CC_VALUE == 64 and m.SustainOn(0.0).control == 64


def test_recorded_fixture_becomes_a_midi_file(dp, golden, tmp_path):
    """The whole host path on the reference's messages: messages -> NoteSequence -> .mid -> parse."""
    m = dp.music
    g = golden["midi_module"]
    act, sus = fixture_arrays(g["sequences"]["sparse"])
    dt = g["timestep"]
    seq = m.sequence_from_messages(m.events_from_activations(act, sus, dt), len(act) * dt)
    m.write_midi(seq, tmp_path / "sparse.mid")
    back = m.parse_midi(tmp_path / "sparse.mid")
    # the piano roll of the file is the activation matrix: key k sounds in substep s iff a note
    # of pitch k + 21 has start <= s dt < end (a note starts at the end of its first active substep)
    roll = np.zeros_like(act)
    for n in back.notes:
        roll[round(n.start_time / dt) - 1:round(n.end_time / dt) - 1, n.pitch - 21] = True
    # (a key still down after the last substep has its note closed there: the last row is open)
    np.testing.assert_array_equal(roll[:-1], act[:-1])
    assert sorted(n.pitch - 21 for n in seq.notes if n.end_time == len(act) * dt) == np.flatnonzero(act[-1]).tolist()
    assert len(back.notes) == len(seq.notes)


def test_smf_writer_under_sanitizers(tmp_path):
    """tools/smf_write_check.cpp + csrc/song.cpp, g++ -fsanitize=address,undefined, run once."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds libpianosong.so too)"
    exe = tmp_path / "smf_write_check"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tools" / "smf_write_check.cpp"),
                    str(ROOT / "diffusion-piano_amd" / "csrc" / "song.cpp")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "" and p.stdout.startswith("ok "), (p.returncode, p.stdout, p.stderr)


def test_versions(dp):
    import importlib
    lib = importlib.import_module("diffusion-piano_amd._lib")
    assert lib.load().ps_version() >= 6 and lib.load_song().pss_version() >= 2
