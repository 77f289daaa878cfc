"""Song ingestion for the batched piano environment (host precompute, init-time only).

The reference's music pipeline (note_seq / pretty_midi in Python, both absent on the GPU
box) restated natively in ``libpianosong.so`` (``csrc/song.cpp``, C-ABI
``include/pianosong.h``); this module is its Python face and keeps the reference's data
classes:

* Standard MIDI File parsing with pretty_midi's note-pairing semantics
  (used by ``note_seq.midi_io.midi_file_to_note_sequence``, called at
  ``robopianist/music/midi_file.py:179`` and ``data_processing/add_fingering_to_midi.py:68``).
* ``MidiFile.trim_silence`` (``robopianist/music/midi_file.py:231-237``) with
  ``note_seq.sequences_lib.extract_subsequence`` semantics.
* ``NoteTrajectory.seq_to_trajectory`` (``robopianist/music/midi_file.py:315-362``) over the
  piano roll of ``robopianist/music/piano_roll.py:59-204`` (onset_window=0).
* ``add_fingering_from_annotation_file`` (``data_processing/add_fingering_to_midi.py:26-83``).
* ``twinkle_twinkle_little_star_one_hand`` (``robopianist/music/library.py:69-97``).

The product of this module is a :class:`SongTables` object: the dense per-control-step
goal table ``[T, 89]`` plus per-step (key, finger) lists that the GPU kernel reads.
Malformed input raises ``ValueError`` with the library's message.
"""

from __future__ import annotations

import ctypes as C
import enum
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from . import _lib

MIN_MIDI_PITCH_PIANO = 21  # robopianist/music/constants.py:21
MAX_MIDI_PITCH_PIANO = 108
NUM_KEYS = 88
MAX_VELOCITY = 127
SUSTAIN_PEDAL_CC_NUMBER = 64  # robopianist/music/constants.py:54
MAX_CC_VALUE = 127
SUSTAIN_ON_CC_VALUE = 64  # the value of the reference's SustainOn message (midi_message.py:82-90)

# Maximum number of simultaneous notes per control step the device tables hold.
MAX_NOTES_PER_STEP = 16


@dataclass
class Note:
    pitch: int
    start_time: float
    end_time: float
    velocity: int = 80
    part: int = 0  # protobuf default: 0 (fingering is stored in `part`).


@dataclass
class ControlChange:
    time: float
    control_number: int
    control_value: int


@dataclass
class NoteSequence:
    notes: List[Note] = field(default_factory=list)
    control_changes: List[ControlChange] = field(default_factory=list)
    total_time: float = 0.0
    title: str = ""

    def has_fingering(self) -> bool:
        """``MidiFile.has_fingering`` (robopianist/music/midi_file.py:252-261)."""
        parts = {n.part for n in self.notes}
        return len(parts) > 1 and any(p != 0 for p in parts)


# ---------------------------------------------------------------------------------------
# libpianosong.so (include/pianosong.h)
# ---------------------------------------------------------------------------------------


class _PssNote(C.Structure):
    _fields_ = [("pitch", C.c_int32), ("start_time", C.c_double), ("end_time", C.c_double),
                ("velocity", C.c_int32), ("part", C.c_int32)]


class _PssCC(C.Structure):
    _fields_ = [("time", C.c_double), ("control_number", C.c_int32), ("control_value", C.c_int32)]


def _check(rc: int) -> None:
    if rc != 0:
        msg = _lib.load_song().pss_last_error()
        raise ValueError(msg.decode() if msg else f"pianosong error {rc}")


class _Seq:
    """Owns a pss_seq handle."""

    def __init__(self, h: C.c_void_p):
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) is not None and self.h.value:
            _lib.load_song().pss_free(self.h)
            self.h = None

    @classmethod
    def parse(cls, data: bytes) -> "_Seq":
        h = C.c_void_p()
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        _check(_lib.load_song().pss_parse_midi(buf, len(data), C.byref(h)))
        return cls(h)

    @classmethod
    def of(cls, seq: NoteSequence) -> "_Seq":
        notes = (_PssNote * max(1, len(seq.notes)))(*[_PssNote(n.pitch, n.start_time, n.end_time, n.velocity, n.part)
                                                      for n in seq.notes])
        ccs = (_PssCC * max(1, len(seq.control_changes)))(
            *[_PssCC(c.time, c.control_number, c.control_value) for c in seq.control_changes])
        h = C.c_void_p()
        _check(_lib.load_song().pss_from_notes(notes, len(seq.notes), ccs, len(seq.control_changes),
                                               float(seq.total_time), C.byref(h)))
        return cls(h)

    def sequence(self, title: str) -> NoteSequence:
        L = _lib.load_song()
        nn, nc, tt = C.c_int(), C.c_int(), C.c_double()
        _check(L.pss_info(self.h, C.byref(nn), C.byref(nc), C.byref(tt), None))
        notes = (_PssNote * max(1, nn.value))()
        ccs = (_PssCC * max(1, nc.value))()
        _check(L.pss_get(self.h, notes, ccs))
        seq = NoteSequence(title=title, total_time=tt.value)
        seq.notes = [Note(n.pitch, n.start_time, n.end_time, n.velocity, n.part) for n in notes[:nn.value]]
        seq.control_changes = [ControlChange(c.time, c.control_number, c.control_value) for c in ccs[:nc.value]]
        return seq


# ---------------------------------------------------------------------------------------
# The reference's functions
# ---------------------------------------------------------------------------------------


def parse_midi(path) -> NoteSequence:
    """Parses a type-0/1 SMF into a :class:`NoteSequence` (``pss_parse_midi``).

    Note pairing follows pretty_midi ``PrettyMIDI._load_instruments``: a note-off (or a
    note-on with velocity 0) closes every open note of that (channel, pitch) that started
    at an earlier tick; an open note started at the same tick stays open. Instruments are
    keyed by (track, channel, program) in first-seen order and their notes are appended
    instrument by instrument, which is the order note_seq copies them into the sequence.
    Ticks map to seconds through the merged tempo map (default 120 qpm).
    """
    return _Seq.parse(Path(path).read_bytes()).sequence(Path(path).stem)


def trim_silence(seq: NoteSequence) -> NoteSequence:
    """``MidiFile.trim_silence``: ``extract_subsequence(seq, notes[0].start, notes[-1].end)``
    (``pss_trim_silence``): notes starting inside ``[start, end)`` shifted by ``-start``, ends
    clipped to ``end``; control changes inside the window shifted; a sustain pedal held at
    ``start`` re-emitted at time 0."""
    s = _Seq.of(seq)
    _check(_lib.load_song().pss_trim_silence(s.h))
    return s.sequence(seq.title)


def stretch(seq: NoteSequence, factor: float) -> NoteSequence:
    """``MidiFile.stretch`` (midi_file.py:204-214) over ``stretch_note_sequence``
    (``pss_stretch``): every note and control-change time and ``total_time`` times ``factor``;
    1.0 is a no-op, a factor <= 0 raises."""
    s = _Seq.of(seq)
    _check(_lib.load_song().pss_stretch(s.h, float(factor)))
    return s.sequence(seq.title)


def transpose(seq: NoteSequence, amount: int) -> NoteSequence:
    """``MidiFile.transpose`` (midi_file.py:216-229) over ``transpose_note_sequence``
    (``pss_transpose``): notes that leave MIDI 21..108 are removed; 0 is a no-op."""
    s = _Seq.of(seq)
    _check(_lib.load_song().pss_transpose(s.h, int(amount)))
    return s.sequence(seq.title)


class FlatSong(C.Structure):
    """``pss_flat_song``: a song as the per-episode builder reads it (``pss_flatten``)."""
    _fields_ = [("notes", C.c_void_p), ("ccs", C.c_void_p), ("n_notes", C.c_int32), ("n_cc", C.c_int32),
                ("total_time", C.c_double), ("pitch_mask", C.c_uint32 * 4)]

    @classmethod
    def of(cls, seq: NoteSequence) -> "FlatSong":
        L = _lib.load_song()
        s = _Seq.of(seq)
        ncc, tt = C.c_int(), C.c_double()
        mask = (C.c_uint32 * 4)()
        _check(L.pss_flatten(s.h, None, None, C.byref(ncc), C.byref(tt), mask))
        notes = np.zeros((len(seq.notes), 4), np.float64)
        ccs = np.zeros((max(1, ncc.value), 2), np.float64)
        _check(L.pss_flatten(s.h, notes.ctypes.data, ccs.ctypes.data, None, None, None))
        out = cls(notes.ctypes.data, ccs.ctypes.data, len(seq.notes), ncc.value, tt.value, mask)
        out._arrays = (notes, ccs)  # kept alive with the struct
        return out

    def pitches(self) -> List[int]:
        return [p for p in range(128) if (self.pitch_mask[p >> 5] >> (p & 31)) & 1]


class Variation(C.Structure):
    """``pss_variation`` (kind 1 select, 2 stretch, 3 pitch shift, 4 octave shift)."""
    _fields_ = [("kind", C.c_int32), ("prob", C.c_double), ("range", C.c_double)]


def build_tables(song, factor: float, shift: int, dt: float, initial_buffer_time: float = 0.0,
                 T_cap: Optional[int] = None, name: str = ""):
    """The device builder's code on the host (``pss_build_tables``): ``(SongTables, fell_back)``
    of ``song`` (a NoteSequence or FlatSong) stretched by ``factor`` and transposed by ``shift``.
    ``T_cap``: rows the tables may take (default: as many as this draw needs)."""
    flat = song if isinstance(song, FlatSong) else FlatSong.of(song)
    if T_cap is None:
        T_cap = int(flat.total_time * max(float(factor), 1.0) / dt) + int(round(initial_buffer_time / dt)) + 3
    goal = np.zeros((T_cap, NUM_KEYS + 1), np.float32)
    count = np.zeros(T_cap, np.int32)
    keys = np.full((T_cap, MAX_NOTES_PER_STEP), -1, np.int32)
    fingers = np.full((T_cap, MAX_NOTES_PER_STEP), -1, np.int32)
    T, fb = C.c_int(), C.c_int()
    _check(_lib.load_song().pss_build_tables(C.addressof(flat), float(factor), int(shift), float(dt),
                                             float(initial_buffer_time), int(T_cap), goal.ctypes.data,
                                             count.ctypes.data, keys.ctypes.data, fingers.ctypes.data,
                                             C.byref(T), C.byref(fb)))
    n = T.value
    has_f = len({int(x) for x in flat._arrays[0][:, 3]}) > 1 and bool((flat._arrays[0][:, 3] != 0).any())
    return SongTables(name, goal[:n], count[:n], keys[:n], fingers[:n], has_f), bool(fb.value)


_NOTE_VALUES = {
    "C": 0, "C#": 1, "Db": 1, "D": 2, "D#": 3, "Eb": 3, "E": 4, "F": 5, "F#": 6,
    "Gb": 6, "G": 7, "G#": 8, "Ab": 8, "A": 9, "A#": 10, "Bb": 10, "B": 11,
}


def parse_pitch_to_midi_number(pitch_str: str) -> int:
    """``data_processing/add_fingering_to_midi.py:7-24``."""
    m = re.match(r"([A-G][#b]?)(\d+)", pitch_str)
    if not m or m.group(1) not in _NOTE_VALUES:
        raise ValueError(f"Invalid pitch format: {pitch_str}")
    note, octave = m.groups()
    return _NOTE_VALUES[note] + (int(octave) + 1) * 12


def add_fingering_from_annotation_file(midi_path, annotation_path) -> NoteSequence:
    """``data_processing/add_fingering_to_midi.py:26-83`` (``pss_add_fingering``).

    Each sequence note takes the finger of the first annotation line whose start and end
    times are within 10 ms and whose pitch is equal.
    """
    s = _Seq.parse(Path(midi_path).read_bytes())
    _check(_lib.load_song().pss_add_fingering(s.h, Path(annotation_path).read_bytes()))
    return s.sequence(Path(midi_path).stem)


def twinkle_twinkle_little_star_one_hand() -> NoteSequence:
    """``robopianist/music/library.py:69-97``."""
    spec = [(60, 0.0, 0.5, 0), (60, 0.5, 1.0, 0), (67, 1.0, 1.5, 2), (67, 1.5, 2.0, 2),
            (69, 2.0, 2.5, 3), (69, 2.5, 3.0, 3), (67, 3.0, 4.0, 2), (65, 4.0, 4.5, 3),
            (65, 4.5, 5.0, 3), (64, 5.0, 5.5, 2), (64, 5.5, 6.0, 2), (62, 6.0, 6.5, 1),
            (62, 6.5, 7.0, 1), (60, 7.0, 8.0, 0)]
    seq = NoteSequence(title="Twinkle Twinkle (one hand)")
    for p, s, e, f in spec:
        seq.notes.append(Note(p, s, e, 80, f))
    seq.total_time = 8.0
    return seq


# ---------------------------------------------------------------------------------------
# NoteTrajectory / device tables.
# ---------------------------------------------------------------------------------------


@dataclass
class SongTables:
    """Dense per-control-step song tables, the device-side form of a NoteTrajectory.

    ``goal[t, k]`` is 1 for keys active at step t, ``goal[t, 88]`` the sustain target.
    ``keys[t, :count[t]]`` / ``fingers[t, :count[t]]`` hold the step's notes in pitch
    order (fingers 0-4 right hand, 5-9 left hand, -1 unknown).
    """

    name: str
    goal: np.ndarray  # [T, 89] float32
    count: np.ndarray  # [T] int32
    keys: np.ndarray  # [T, MAX_NOTES_PER_STEP] int32
    fingers: np.ndarray  # [T, MAX_NOTES_PER_STEP] int32
    has_fingering: bool

    @property
    def T(self) -> int:
        return int(self.goal.shape[0])


def _tables(seq: NoteSequence, dt: float, initial_buffer_time: float, max_notes: int):
    L = _lib.load_song()
    s = _Seq.of(seq)
    T = C.c_int()
    _check(L.pss_song_tables(s.h, float(dt), float(initial_buffer_time), 0, max_notes, None, None, None, None,
                             C.byref(T)))
    n = T.value
    goal = np.zeros((n, NUM_KEYS + 1), np.float32)
    count = np.zeros(n, np.int32)
    keys = np.full((n, max_notes), -1, np.int32)
    fingers = np.full((n, max_notes), -1, np.int32)
    _check(L.pss_song_tables(s.h, float(dt), float(initial_buffer_time), n, max_notes, goal.ctypes.data,
                             count.ctypes.data, keys.ctypes.data, fingers.ctypes.data, C.byref(T)))
    return goal, count, keys, fingers


def note_trajectory(seq: NoteSequence, dt: float):
    """``NoteTrajectory.seq_to_trajectory`` (robopianist/music/midi_file.py:315-362).

    Returns ``notes[T]`` as lists of ``(key, fingering)`` in increasing MIDI pitch order and
    ``sustains[T]``. Frame semantics are those of ``sequence_to_pianoroll``
    (robopianist/music/piano_roll.py:59-204) with ``onset_window=0``: a note occupies
    frames ``[int(s*fps), max(start+1, ceil(e*fps)))``; a note whose onset frame re-strikes
    a key that was active in the previous frame is dropped from that frame.
    """
    goal, count, keys, fingers = _tables(seq, dt, 0.0, NUM_KEYS)
    notes: List[List[Tuple[int, int]]] = [[(int(keys[t, i]), int(fingers[t, i])) for i in range(count[t])]
                                          for t in range(len(count))]
    return notes, [int(x) for x in goal[:, NUM_KEYS]]


def song_tables(seq: NoteSequence, dt: float, initial_buffer_time: float = 0.0,
                name: Optional[str] = None) -> SongTables:
    """``PianoWithShadowHands._reset_trajectory`` (piano_with_shadow_hands.py:159-165), with
    ``NoteTrajectory.add_initial_buffer_time`` (midi_file.py:388-401)."""
    goal, count, keys, fingers = _tables(seq, dt, initial_buffer_time, MAX_NOTES_PER_STEP)
    return SongTables(name or seq.title, goal, count, keys, fingers, seq.has_fingering())


def test_midi(dt: float = 0.01) -> NoteSequence:
    """``_get_test_midi`` of robopianist/suite/tasks/piano_with_shadow_hands_test.py:29-52."""
    seq = NoteSequence(title="test")
    seq.notes.append(Note(84, 0.0, 2 * dt, 80, 1))  # C6, right index.
    seq.notes.append(Note(79, 2 * dt, 3 * dt, 80, 0))  # G5, right thumb.
    seq.total_time = 3 * dt
    return seq


# ---------------------------------------------------------------------------------------
# The piano's sound module: what an env played (models/piano/midi_module.py) -> messages ->
# NoteSequence -> Standard MIDI File.
# ---------------------------------------------------------------------------------------


class EventType(enum.IntEnum):
    """The kind field of a recorded event word (PS_MIDI_* of include/pianosim.h); the names are
    those of ``robopianist/music/midi_message.py:25-32``."""
    NOTE_ON = 0
    NOTE_OFF = 1
    SUSTAIN_ON = 2
    SUSTAIN_OFF = 3


@dataclass
class NoteOn:
    note: int
    velocity: int
    time: float
    event_type = EventType.NOTE_ON


@dataclass
class NoteOff:
    note: int
    time: float
    event_type = EventType.NOTE_OFF


@dataclass
class SustainOn:
    """CC64 with the reference's value for "on", 64 (midi_message.py:82-90)."""
    time: float
    control: int = SUSTAIN_PEDAL_CC_NUMBER
    value: int = SUSTAIN_ON_CC_VALUE
    event_type = EventType.SUSTAIN_ON


@dataclass
class SustainOff:
    time: float
    control: int = SUSTAIN_PEDAL_CC_NUMBER
    value: int = 0
    event_type = EventType.SUSTAIN_OFF


EVENT_NOTE_BITS, EVENT_KIND_BITS = 8, 2  # then the substep ordinal, 22 bits
EVENT_ORDINAL_SHIFT = EVENT_NOTE_BITS + EVENT_KIND_BITS
EVENT_ORDINAL_MAX = (1 << 22) - 1


def encode_event(note: int, kind: int, ordinal: int) -> int:
    """The recorder's event word: note number | kind << 8 | substep ordinal << 10."""
    if not (0 <= note < 1 << EVENT_NOTE_BITS and 0 <= kind < 1 << EVENT_KIND_BITS and 0 <= ordinal <= EVENT_ORDINAL_MAX):
        raise ValueError(f"event field out of range: note {note}, kind {kind}, ordinal {ordinal}")
    return note | kind << EVENT_NOTE_BITS | ordinal << EVENT_ORDINAL_SHIFT


def event_fields(words) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (note, kind, ordinal) arrays of event words (any integer dtype; int32 words are taken
    as the uint32 they hold)."""
    w = np.asarray(words)
    w = w.view(np.uint32) if w.dtype == np.int32 else w.astype(np.uint32)
    return ((w & 0xFF).astype(np.int64), ((w >> EVENT_NOTE_BITS) & 3).astype(np.int64),
            (w >> EVENT_ORDINAL_SHIFT).astype(np.int64))


def _message(note: int, kind: int, time: float):
    if kind == EventType.NOTE_ON:
        return NoteOn(note, MAX_VELOCITY, time)  # the reference's constant (midi_module.py:67-69)
    if kind == EventType.NOTE_OFF:
        return NoteOff(note, time)
    return SustainOn(time) if kind == EventType.SUSTAIN_ON else SustainOff(time)


def decode_events(words, count: int, timestep: float) -> list:
    """The first ``count`` event words as messages; time = ordinal * timestep."""
    note, kind, ordinal = event_fields(np.asarray(words)[:int(count)])
    return [_message(int(n), int(k), int(o) * timestep) for n, k, o in zip(note, kind, ordinal)]


def events_from_activations(act, sustain, timestep: float, words: bool = False):
    """``MidiModule.after_substep`` (models/piano/midi_module.py:47-98) over a whole episode:
    ``act`` [S, 88] bool and ``sustain`` [S] bool are the activations after substeps 1 .. S, all
    off before the first. Per substep: the NoteOns by ascending key, the NoteOffs by ascending
    key, SustainOn, SustainOff, each stamped ``ordinal * timestep``. ``words``: the event words
    (uint32 array) instead of messages. This is the specification of the device recorder."""
    act = np.asarray(act, dtype=bool).reshape(-1, NUM_KEYS)
    sustain = np.asarray(sustain, dtype=bool).reshape(-1)
    if len(sustain) != len(act):
        raise ValueError("act and sustain differ in length")
    prev, prev_s = np.zeros(NUM_KEYS, bool), False
    out = []
    for s in range(len(act)):
        o = s + 1
        changed = act[s] ^ prev
        out += [(MIN_MIDI_PITCH_PIANO + int(k), EventType.NOTE_ON, o) for k in np.flatnonzero(changed & act[s])]
        out += [(MIN_MIDI_PITCH_PIANO + int(k), EventType.NOTE_OFF, o) for k in np.flatnonzero(changed & ~act[s])]
        if bool(sustain[s]) != prev_s:
            out.append((0, EventType.SUSTAIN_ON if sustain[s] else EventType.SUSTAIN_OFF, o))
        prev, prev_s = act[s].copy(), bool(sustain[s])
    if words:
        return np.array([encode_event(n, int(k), min(o, EVENT_ORDINAL_MAX)) for n, k, o in out], np.uint32)
    return [_message(n, k, o * timestep) for n, k, o in out]


def pack_activations(act, sustain) -> np.ndarray:
    """[S, 88] bool, [S] bool -> [S, 3] uint32 rows as ``ps_midi_push`` takes them: key k is bit
    k % 32 of word k // 32, the sustain activation bit 24 of word 2."""
    act = np.asarray(act, dtype=bool).reshape(-1, NUM_KEYS)
    bits = np.zeros((len(act), 96), bool)
    bits[:, :NUM_KEYS] = act
    bits[:, NUM_KEYS] = np.asarray(sustain, dtype=bool).reshape(-1)
    weights = (1 << np.arange(32, dtype=np.uint64))
    return (bits.reshape(len(act), 3, 32).astype(np.uint64) * weights).sum(-1).astype(np.uint32)


def sequence_from_messages(messages, end_time: float, title: str = "") -> NoteSequence:
    """Messages in time order -> a NoteSequence: a NoteOn opens its pitch (velocity as recorded),
    the next NoteOff of the pitch closes it, a note still on at the end is closed at
    ``end_time``; the pedal messages become CC64 control changes with their values (64 / 0).
    Notes in order of their starts; ``total_time`` = ``end_time``."""
    seq = NoteSequence(title=title, total_time=float(end_time))
    open_notes = {}
    order = []
    for m in messages:
        if m.event_type == EventType.NOTE_ON:
            if m.note in open_notes:  # (a re-strike without a NoteOff: the sounding note ends here)
                open_notes.pop(m.note).end_time = m.time
            n = Note(m.note, m.time, float(end_time), m.velocity, 0)
            open_notes[m.note] = n
            order.append(n)
        elif m.event_type == EventType.NOTE_OFF:
            if m.note in open_notes:
                open_notes.pop(m.note).end_time = m.time
        else:
            seq.control_changes.append(ControlChange(m.time, m.control, m.value))
    seq.notes = order
    return seq


def to_smf(seq: NoteSequence) -> bytes:
    """The sequence as a Standard MIDI File (``pss_write_smf``): format 0, 1000 ticks per quarter
    note at 120 qpm = 2000 ticks per second, so times on the 5 ms physics grid are exact.
    Raises ValueError on a pitch, velocity or controller value outside 0..127."""
    L = _lib.load_song()
    s = _Seq.of(seq)
    size = L.pss_write_smf(s.h, None, 0)
    if size < 0:
        _check(-1)
    buf = (C.c_uint8 * size)()
    if L.pss_write_smf(s.h, buf, size) != size:
        _check(-1)
    return bytes(buf)


def write_midi(seq: NoteSequence, path) -> None:
    """``MidiFile.save`` (midi_file.py:191-195): ``to_smf(seq)`` into ``path``."""
    Path(path).write_bytes(to_smf(seq))
