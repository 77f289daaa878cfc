"""Generate tests/golden/midi_module.json from the reference's own sound module.

Runs only where the reference checkout is present (``make_golden.REF``; see make_golden.py, whose
stub helpers this imports unchanged). robopianist/music/midi_message.py and robopianist/models/piano/midi_module.py are
loaded by path and executed unmodified; ``dm_control.mjcf`` is a two-line stub (the module only
names ``mjcf.Physics`` in annotations). ``MidiModule.after_substep`` is driven as piano.py:154-162
drives it, once per physics substep with the key and sustain activations, with a stand-in physics
whose ``data.time`` is the time after that substep, ordinal * 0.005 s.

The fixture holds data only: per sequence the active keys and the sustain activation of every
substep, and the reference's messages (kind, note, ordinal, time) from get_all_midi_messages().

Usage: python tests/golden/make_midi_module_golden.py
"""

from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as G  # noqa: E402  (stubs and the by-path loader)

DT = 0.005
KINDS = {"NOTE_ON": 0, "NOTE_OFF": 1, "SUSTAIN_ON": 2, "SUSTAIN_OFF": 3}


def sequences():
    rng = np.random.RandomState(20231)
    out = {}
    # keys and pedal flipping now and then (a played passage)
    act, sus = np.zeros(88, bool), False
    rows, pedal = [], []
    for _ in range(43):
        act = act ^ (rng.uniform(size=88) < 0.03)
        sus = sus ^ bool(rng.uniform() < 0.2)
        rows.append(act.copy())
        pedal.append(sus)
    out["sparse"] = (np.array(rows), np.array(pedal))
    # every key re-drawn every substep: ons and offs in the same substep, in both lane halves
    out["dense"] = (rng.uniform(size=(27, 88)) < 0.5, rng.uniform(size=27) < 0.5)
    # all 88 keys and the pedal switch in one substep, hold, and switch back in one
    a = np.zeros((5, 88), bool)
    a[1:4] = True
    out["all_switch"] = (a, np.array([False, True, True, True, False]))
    out["silent"] = (np.zeros((12, 88), bool), np.zeros(12, bool))
    # the first and last key of each 32-bit word and of the two lane halves, one substep each
    edge = [0, 31, 32, 63, 64, 87]
    a = np.zeros((len(edge) + 1, 88), bool)
    for s, k in enumerate(edge):
        a[s, k] = True
    out["word_edges"] = (a, np.zeros(len(edge) + 1, bool))
    return out


def main():
    G._install_stubs()
    dmc = types.ModuleType("dm_control")
    dmc.mjcf = types.ModuleType("dm_control.mjcf")
    dmc.mjcf.Physics = object
    sys.modules.update({"dm_control": dmc, "dm_control.mjcf": dmc.mjcf})
    for name in ("robopianist.models", "robopianist.models.piano"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    R = G.REF / "robopianist"
    G._load("robopianist.music.constants", R / "music/constants.py")
    G._load("robopianist.music.piano_roll", R / "music/piano_roll.py")
    G._load("robopianist.music.midi_file", R / "music/midi_file.py")
    G._load("robopianist.music.midi_message", R / "music/midi_message.py")
    G._load("robopianist.models.piano.piano_constants", R / "models/piano/piano_constants.py")
    mm = G._load("robopianist.models.piano.midi_module", R / "models/piano/midi_module.py")

    rec = {"source": "reference models/piano/midi_module.py MidiModule.after_substep, unmodified", "timestep": DT,
           "kinds": KINDS, "sequences": {}}
    for name, (act, sus) in sequences().items():
        module = mm.MidiModule()
        physics = types.SimpleNamespace(data=types.SimpleNamespace(time=0.0))
        module.initialize_episode(physics)
        ordinal_of = {}
        for s in range(len(act)):
            physics.data.time = (s + 1) * DT
            ordinal_of[physics.data.time] = s + 1
            module.after_substep(physics, act[s].copy(), np.array([sus[s]], dtype=bool))
        msgs = [[KINDS[m.event_type.name], int(getattr(m, "note", 0)) if m.event_type.name.startswith("NOTE") else 0,
                 ordinal_of[m.time], m.time] for m in module.get_all_midi_messages()]
        values = sorted({(m.control, m.value) for m in module.get_all_midi_messages()
                         if not m.event_type.name.startswith("NOTE")})
        rec["sequences"][name] = {"active_keys": [np.flatnonzero(r).tolist() for r in act],
                                  "sustain": [int(x) for x in sus], "messages": msgs,
                                  "control_values": [list(v) for v in values]}
    (G.OUT / "midi_module.json").write_text(json.dumps(rec))
    print({k: len(v["messages"]) for k, v in rec["sequences"].items()})


if __name__ == "__main__":
    main()
