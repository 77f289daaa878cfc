"""Per-episode MIDI augmentations, host side: music.stretch / transpose against the reference's
trajectories (tests/golden/augment.json), the reference's own tests of them restated, the
variations and their counter-based draw, and the device builder's code (csrc/song_build.h, run
on the host through pss_build_tables) against the host path it has to equal."""
import importlib
import random

import numpy as np
import pytest

from helpers import song

TABLES = ("goal", "count", "keys", "fingers")


@pytest.fixture(scope="module")
def V():
    return importlib.import_module("diffusion-piano_amd.variations")


@pytest.fixture(scope="module")
def songs(dp):
    """name -> (sequence, dt): the golden file's songs, and Guren for the builder sweeps."""
    m = dp.music
    restrike = m.NoteSequence(notes=[m.Note(84, 0.01, 0.02, 80, -1), m.Note(84, 0.02, 0.05, 80, -1)], total_time=0.05)
    sustain = m.NoteSequence(notes=[m.Note(84, 0.0, 0.01, 80, -1), m.Note(84, 0.05, 0.06, 80, -1)],
                             control_changes=[m.ControlChange(0.0, 64, 64), m.ControlChange(0.03, 64, 0)],
                             total_time=0.06)
    return {"twinkle": (song(dp, "twinkle"), 0.05), "test_restrike": (restrike, 0.01), "test_sustain": (sustain, 0.01),
            "test_task": (m.test_midi(0.01), 0.01),
            "crossing_field": (m.trim_silence(song(dp, "crossing_field")), 0.05),
            "guren": (m.trim_silence(song(dp, "guren")), 0.05)}


def two_chords(m):
    """Two 9-note chords of distinct pitches at 0.0 s and 0.06 s, 0.04 s long: frames 0 and 1 at
    dt 0.05; at factor 0.5 both fall into frame 0 - 18 keys, more than a row holds."""
    seq = m.NoteSequence(title="two chords", total_time=0.1)
    for i in range(9):
        seq.notes.append(m.Note(40 + i, 0.0, 0.04, 80, 0))
    for i in range(9):
        seq.notes.append(m.Note(60 + i, 0.06, 0.1, 80, 0))
    return seq


def same_tables(a, b):
    assert a.T == b.T
    for k in TABLES:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


# ------------------------------------------------------------------ golden
def test_stretch_transpose_match_reference_trajectories(dp, golden, songs):
    g = golden["augment"]
    assert len(g["cases"]) == 5 * len(g["factors"]) * len(g["shifts"])
    m = dp.music
    for c in g["cases"]:
        seq, dt = songs[c["song"]]
        assert dt == c["dt"]
        notes, sustains = m.note_trajectory(m.transpose(m.stretch(seq, c["factor"]), c["shift"]), dt)
        what = (c["song"], c["factor"], c["shift"])
        assert len(notes) == c["T"], what
        want = [[] for _ in range(c["T"])]
        for t, step in c["notes"]:
            want[t] = [tuple(x) for x in step]
        assert notes == want, what
        assert [t for t, v in enumerate(sustains) if v] == c["sustained"], what


# ------------------------------------------------------------------ midi_file_test.py:30-57
def test_temporal_stretch(dp):
    m = dp.music
    seq = song(dp, "twinkle")
    for factor in (0.5, 1.0, 2.0, 1.3):
        out = m.stretch(seq, factor)
        assert len(out.notes) == len(seq.notes)
        assert out.total_time == seq.total_time * factor
        for a, b in zip(seq.notes, out.notes):
            assert (b.start_time, b.end_time, b.pitch) == (a.start_time * factor, a.end_time * factor, a.pitch)
    same = m.stretch(seq, 1.0)
    assert [(n.pitch, n.start_time, n.end_time, n.velocity, n.part) for n in same.notes] == \
        [(n.pitch, n.start_time, n.end_time, n.velocity, n.part) for n in seq.notes]
    for bad in (-1.0, 0.0):
        with pytest.raises(ValueError):
            m.stretch(seq, bad)


def test_transpose(dp):
    m = dp.music
    seq = song(dp, "twinkle")
    for amount in (-2, 0, 2, 12):
        out = m.transpose(seq, amount)
        assert len(out.notes) == len(seq.notes)
        assert [n.pitch for n in out.notes] == [n.pitch + amount for n in seq.notes]
        assert out.total_time == seq.total_time
    # Twinkle spans 60..69: 40 up leaves 60..68 on the piano (the 69s go), total_time = last end kept
    out = m.transpose(seq, 40)
    assert [n.pitch for n in out.notes] == [n.pitch + 40 for n in seq.notes if n.pitch + 40 <= 108]
    assert len(out.notes) == len(seq.notes) - 2 and out.total_time == 8.0
    assert m.transpose(seq, 60).notes == [] and m.transpose(seq, 60).total_time == 0.0


def test_load_takes_stretch_and_shift(dp):
    import inspect
    p = inspect.signature(dp.load).parameters
    assert p["stretch"].default == 1.0 and p["shift"].default == 0


# ------------------------------------------------------------------ variations_test.py
def test_variation_arguments(dp, V):
    with pytest.raises(ValueError):
        V.MidiPitchShift(1.0, 1.5)
    with pytest.raises(ValueError):
        V.MidiOctaveShift(1.0, 0.5)
    with pytest.raises(ValueError):
        V.MidiSelect([])
    with pytest.raises(TypeError):
        V.MidiSelect([3])
    with pytest.raises(ValueError):
        V.check([V.MidiPitchShift(1.0, 1), V.MidiPitchShift(0.5, 2)])
    with pytest.raises(TypeError):
        V.check([lambda initial_value, random_state: initial_value])
    assert dp.MidiTemporalStretch is V.MidiTemporalStretch and dp.MidiSelect is V.MidiSelect
    assert dp.TaskConfig().augmentations is None
    assert len(dp.TaskConfig(augmentations=[V.MidiOctaveShift(0.5, 1)]).augmentations) == 1


def test_prob_zero_and_range_zero_are_identity(dp, V):
    tw = song(dp, "twinkle")
    for augs in ([V.MidiTemporalStretch(0.0, 0.5), V.MidiPitchShift(0.0, 5), V.MidiOctaveShift(0.0, 2)],
                 [V.MidiTemporalStretch(1.0, 0.0), V.MidiPitchShift(1.0, 0), V.MidiOctaveShift(1.0, 0)]):
        for env in range(200):
            assert V.draw(7, env, env % 3, augs, [tw]) == (0, 1.0, 0)
    # u == 0 is not > prob 0: the gate passes once in 2**24 draws, never here
    out = V.apply([tw], 0, 1.0, 0)
    assert [(n.pitch, n.start_time, n.end_time) for n in out.notes] == \
        [(n.pitch, n.start_time, n.end_time) for n in tw.notes]


def test_draw_properties(dp, V, songs):
    tw, cf = songs["twinkle"][0], songs["crossing_field"][0]
    bank = [tw, cf, songs["guren"][0]]
    augs = [V.MidiSelect(bank[1:]), V.MidiTemporalStretch(1.0, 0.5), V.MidiPitchShift(1.0, 7)]
    seen = set()
    for env in range(600):
        s, f, sh = V.draw(99, env, env % 4, augs, bank)
        seen.add(s)
        assert s in (1, 2) and 0.5 <= f <= 1.5 and -7 <= sh <= 7
        ps = [n.pitch + sh for n in bank[s].notes]
        assert min(ps) >= 21 and max(ps) <= 108
    assert seen == {1, 2}
    # a song at the top of the piano: the pitch shift is truncated, never leaves it
    m = dp.music
    top = m.NoteSequence(notes=[m.Note(106, 0.0, 0.1, 80, 0), m.Note(50, 0.1, 0.2, 80, 1)], total_time=0.2)
    shifts = {V.draw(5, env, 0, [V.MidiPitchShift(1.0, 6)], [top])[2] for env in range(400)}
    assert shifts == set(range(-6, 3))
    octs = {V.draw(5, env, 0, [V.MidiOctaveShift(1.0, 2)], [tw])[2] for env in range(400)}
    assert octs == {-24, -12, 0, 12, 24}
    # the gate at prob 0.5 over envs 0..4095 of episode 0, seed 12345: within 6 sigma of 2048
    # (sigma = sqrt(4096 / 4) = 32)
    hits = sum(V.draw(12345, env, 0, [V.MidiTemporalStretch(0.5, 0.25)], [tw])[1] != 1.0 for env in range(4096))
    assert abs(hits - 2048) <= 192, hits
    # the order is honoured: a shift before MidiSelect is dropped with the song it was drawn for
    assert all(V.draw(3, env, 0, [V.MidiPitchShift(1.0, 5), V.MidiSelect([cf])], [tw, cf])[1:] == (1.0, 0)
               for env in range(50))


def test_native_draw_is_the_python_draw(dp, V, songs):
    """song_build.h's draw (the device code, on the host) against variations.draw, bit for bit."""
    m = dp.music
    bank = [songs["test_task"][0], songs["twinkle"][0], songs["crossing_field"][0], songs["guren"][0]]
    flats = [m.FlatSong.of(s) for s in bank]
    lists = ([V.MidiSelect(bank[1:]), V.MidiTemporalStretch(0.7, 0.5), V.MidiOctaveShift(0.5, 3), V.MidiPitchShift(0.9, 5)],
             [V.MidiPitchShift(1.0, 3), V.MidiTemporalStretch(1.0, 0.1)], [V.MidiOctaveShift(1.0, 4)], [])
    for augs in lists:
        b, f = (bank, flats) if augs and augs[0].kind == V.SELECT else (bank[1:2], flats[1:2])
        for env in range(0, 3000, 3):
            seed = 12345 + ((env % 5) << 32)
            assert V.draw_native(seed, 2 ** 31 + env, env % 7, augs, f) == V.draw(seed, 2 ** 31 + env, env % 7, augs, b)


# ------------------------------------------------------------------ the builder's code on the host
def test_build_tables_equals_host_path(dp, songs):
    """pss_build_tables (the device builder's code) == song_tables(transpose(stretch(seq))) for
    2000 seeded (song, factor, shift) draws, Guren included; shifts inside the piano and - every
    third - beyond it, where transpose drops notes and shortens the song."""
    m = dp.music
    names = ("test_task", "twinkle", "crossing_field", "guren", "test_restrike", "test_sustain")
    flats = {k: m.FlatSong.of(songs[k][0]) for k in names}
    rng = random.Random(0)
    for it in range(2000):
        name = names[rng.randrange(len(names))]
        seq, dt = songs[name]
        ps = flats[name].pitches()
        f = 1.0 if it % 11 == 0 else rng.uniform(0.5, 1.5)
        sh = rng.randint(21 - min(ps), 108 - max(ps)) if it % 3 else rng.randint(-45, 45)
        buf = rng.choice((0.0, 0.0, 0.5, 0.075))
        host = m.song_tables(m.transpose(m.stretch(seq, f), sh), dt, buf)
        dev, fell_back = m.build_tables(flats[name], f, sh, dt, buf)
        assert not fell_back, (name, f, sh)
        same_tables(host, dev)


def test_fallback_and_cap(dp, songs):
    m = dp.music
    seq = two_chords(m)
    plain = m.song_tables(seq, 0.05)
    assert plain.T == 3 and list(plain.count) == [9, 9, 0]
    dev, fell_back = m.build_tables(seq, 1.0, 0, 0.05)
    assert not fell_back
    same_tables(plain, dev)
    with pytest.raises(ValueError):  # the host path refuses the 18-key frame
        m.song_tables(m.stretch(seq, 0.5), 0.05)
    dev, fell_back = m.build_tables(seq, 0.5, 0, 0.05)
    assert fell_back
    same_tables(plain, dev)  # never a truncated table: the song as given
    # more rows than T_cap: the song as given again
    tw = songs["twinkle"][0]
    plain = m.song_tables(tw, 0.05)
    dev, fell_back = m.build_tables(tw, 1.5, 0, 0.05, T_cap=plain.T + 10)
    assert fell_back
    same_tables(plain, dev)
    # the songs of the GPU tests stay within 16 keys a frame over the stretch range
    rng = random.Random(1)
    for name in ("twinkle", "crossing_field", "guren"):
        flat = m.FlatSong.of(songs[name][0])
        for _ in range(100):
            tab, fell_back = m.build_tables(flat, rng.uniform(0.5, 1.5), 0, 0.05)
            assert not fell_back and tab.count.max() <= 8
    with pytest.raises(ValueError):
        m.FlatSong.of(m.NoteSequence())
    with pytest.raises(ValueError):
        m.FlatSong.of(m.NoteSequence(notes=[m.Note(110, 0.0, 0.1, 80, 0)], total_time=0.1))
