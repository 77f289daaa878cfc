"""Per-episode MIDI augmentations (``robopianist/suite/variations.py``), as descriptions.

The reference's variations are callables over a ``MidiFile`` that ``PianoWithShadowHands``
applies, in list order and starting from its initial (trimmed) song, at the start of every
episode (``piano_with_shadow_hands.py:151-157,169-174``). Here the episode starts on the GPU
(auto-reset after LAST), so the classes below only describe the variation; the draw and the
new song tables are made on the device, per env, by ``song_build_kernel``
(``ps_set_augmentations`` of include/pianosim.h). ``TaskConfig(augmentations=[...])`` takes them.

The reference draws from numpy's ``RandomState``; that stream cannot be reproduced on the
device. The draw is counter-based instead, and :func:`draw` states it in Python integers and
floats - it is the specification the device code (``csrc/song_build.h``) is held to, bit for
bit:

* Philox4x32-10 keyed by the handle's seed; variation ``i`` of the list takes the counter
  ``(episode, global env id, 0x6d696469, i)`` and the words ``c0, c1`` of its output.
* gate ``u = (c0 >> 8) * 2**-24``; the variation is skipped when ``u > prob``
  (``variations.py:73,112,163``). ``MidiSelect`` has no gate.
* a choice among ``n``: ``(c1 * n) >> 32``.
* the stretch factor: ``1.0 + (2.0 * (c1 * 2**-32) - 1.0) * stretch_range`` in fp64, in that
  operation order.
* the pitch shift is uniform on ``[low, high]`` with ``low = max(21 - min_pitch, -r)``,
  ``high = min(108 - max_pitch, r)`` (``variations.py:124-133``); the octave shift is uniform on
  ``[low // 12, high // 12]`` (Python floor division, ``variations.py:175-184``), times 12.
  The pitch bounds are those of the running song: the selected song, with the shifts so far,
  without the notes a shift has pushed off the piano (``MidiFile.transpose`` removes them).
"""

from __future__ import annotations

from pathlib import Path
from typing import List, Optional, Sequence, Tuple

from . import music

SELECT, STRETCH, PITCH, OCTAVE = 1, 2, 3, 4  # pss_variation.kind
DRAW_TAG = 0x6D696469  # "midi"
_M32 = 0xFFFFFFFF


class MidiSelect:
    """Every episode plays one of ``midis`` (NoteSequences or MIDI file paths), chosen
    uniformly. The songs are used as given (the reference trims only the constructor's midi);
    its name registry and PIG set are absent, so names are not accepted."""

    kind = SELECT

    def __init__(self, midis: Sequence = ()) -> None:
        self.midis = []
        for m in midis:
            if isinstance(m, music.NoteSequence):
                self.midis.append(m)
            elif isinstance(m, (str, Path)):
                self.midis.append(music.parse_midi(m))
            else:
                raise TypeError(f"MidiSelect takes NoteSequences or MIDI paths, got {type(m)!r}")
        if not self.midis:
            raise ValueError("MidiSelect needs at least one song.")
        self.prob, self.range = 1.0, float(len(self.midis))


class MidiTemporalStretch:
    """With probability ``prob``, stretch by a factor uniform on
    ``[1 - stretch_range, 1 + stretch_range]``."""

    kind = STRETCH

    def __init__(self, prob: float, stretch_range: float) -> None:
        self.prob, self.range = float(prob), float(stretch_range)
        if not 0.0 <= self.range < 1.0:
            raise ValueError("`stretch_range` must be in [0, 1): the factor has to stay positive.")


class MidiPitchShift:
    """With probability ``prob``, transpose by up to ``shift_range`` semitones, truncated to
    what keeps every note on the piano."""

    kind = PITCH

    def __init__(self, prob: float, shift_range: int) -> None:
        if not isinstance(shift_range, int):
            raise ValueError("`shift_range` must be an integer.")
        if shift_range < 0:
            raise ValueError("`shift_range` must not be negative.")
        self.prob, self.range = float(prob), float(shift_range)


class MidiOctaveShift:
    """With probability ``prob``, transpose by up to ``octave_range`` octaves."""

    kind = OCTAVE

    def __init__(self, prob: float, octave_range: int) -> None:
        if not isinstance(octave_range, int):
            raise ValueError("`octave_range` must be an integer.")
        if octave_range < 0:
            raise ValueError("`octave_range` must not be negative.")
        self.prob, self.range = float(prob), float(octave_range)


_KINDS = (MidiSelect, MidiTemporalStretch, MidiPitchShift, MidiOctaveShift)


def check(augmentations) -> List:
    """The list form of ``TaskConfig.augmentations``: at most one variation of each kind."""
    out = list(augmentations)
    for v in out:
        if not isinstance(v, _KINDS):
            raise TypeError(f"augmentations takes MidiSelect / MidiTemporalStretch / MidiPitchShift / "
                            f"MidiOctaveShift, got {type(v)!r}")
    if len({v.kind for v in out}) != len(out):
        raise ValueError("augmentations: at most one variation of each kind")
    return out


def bank(initial: music.NoteSequence, augmentations) -> List[music.NoteSequence]:
    """Song 0 is the task's initial song; then MidiSelect's songs."""
    songs = [initial]
    for v in augmentations:
        if v.kind == SELECT:
            songs += v.midis
    return songs


def max_stretch(augmentations) -> float:
    return max([1.0] + [1.0 + v.range for v in augmentations if v.kind == STRETCH])


# ------------------------------------------------------------------------------ the draw
def philox4x32_10(c: Sequence[int], k0: int, k1: int) -> Tuple[int, int, int, int]:
    c0, c1, c2, c3 = c
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def _bounds(pitches, shift) -> Optional[Tuple[int, int]]:
    kept = [p + shift for p in pitches
            if music.MIN_MIDI_PITCH_PIANO <= p + shift <= music.MAX_MIDI_PITCH_PIANO]
    return (min(kept), max(kept)) if kept else None


def draw(seed: int, env: int, episode: int, augmentations, songs) -> Tuple[int, float, int]:
    """-> ``(song, factor, shift)`` of global env ``env`` in its episode ``episode`` (0: the
    first reset): the index into ``songs`` (= :func:`bank`: the initial song, then MidiSelect's),
    the stretch factor and the transposition in semitones. ``songs`` may hold NoteSequences or
    lists of MIDI pitches."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    pitches = [sorted({n.pitch for n in s.notes}) if isinstance(s, music.NoteSequence) else list(s) for s in songs]
    song, factor, shift = 0, 1.0, 0
    for i, v in enumerate(augmentations):
        c0, c1, _, _ = philox4x32_10((episode & _M32, env & _M32, DRAW_TAG, i), k0, k1)
        u = float(c0 >> 8) * 2.0 ** -24
        if v.kind == SELECT:
            if len(songs) > 1:
                song = 1 + ((c1 * (len(songs) - 1)) >> 32)
            factor, shift = 1.0, 0
            continue
        if u > v.prob:
            continue
        if v.kind == STRETCH:
            factor = 1.0 + (2.0 * (float(c1) * 2.0 ** -32) - 1.0) * v.range
            continue
        r = int(v.range)
        b = _bounds(pitches[song], shift)
        if r == 0 or b is None:
            continue
        if v.kind == PITCH:
            low, high = max(music.MIN_MIDI_PITCH_PIANO - b[0], -r), min(music.MAX_MIDI_PITCH_PIANO - b[1], r)
            if high >= low:
                shift += low + ((c1 * (high - low + 1)) >> 32)
        else:
            low = max(music.MIN_MIDI_PITCH_PIANO - b[0], -12 * r)
            high = min(music.MAX_MIDI_PITCH_PIANO - b[1], 12 * r)
            lo, hi = low // 12, high // 12
            if hi >= lo:
                shift += 12 * (lo + ((c1 * (hi - lo + 1)) >> 32))
    return song, factor, shift


def apply(songs, song: int, factor: float, shift: int) -> music.NoteSequence:
    """The host form of a draw: ``transpose(stretch(songs[song], factor), shift)``, as
    ``music.load(stretch=, shift=)`` orders them (music/__init__.py:92)."""
    return music.transpose(music.stretch(songs[song], factor), shift)


def as_structs(augmentations):
    """-> ctypes array of ``pss_variation`` / ``ps_variation``."""
    arr = (music.Variation * max(1, len(augmentations)))()
    for i, v in enumerate(augmentations):
        arr[i] = music.Variation(v.kind, v.prob, v.range)
    return arr


def draw_native(seed: int, env: int, episode: int, augmentations, flat_songs) -> Tuple[int, float, int]:
    """The device code's draw run on the host (``pss_draw_augmentation``), for the tests that
    hold it to :func:`draw`."""
    import ctypes as C

    from . import _lib
    bank_arr = (music.FlatSong * len(flat_songs))()
    for i, f in enumerate(flat_songs):
        C.memmove(C.addressof(bank_arr[i]), C.addressof(f), C.sizeof(music.FlatSong))
    s, f, sh = C.c_int(), C.c_double(), C.c_int()
    music._check(_lib.load_song().pss_draw_augmentation(seed, env, episode, as_structs(augmentations),
                                                        len(augmentations), bank_arr, len(flat_songs),
                                                        C.byref(s), C.byref(f), C.byref(sh)))
    return s.value, f.value, sh.value
