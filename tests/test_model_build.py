"""The host-only model compiler (csrc/model_build.h: ps_model_desc -> DevModel, and what ps_create
refuses before it touches the device) through its stand-alone driver tools/model_build_check - no
GPU, no HIP. Valid descriptors of every collider set / action space / hand_side compile, twice to
the same bytes; every refusal of the header is reached by a case of the table below (the header is
read for its messages, so a refusal added without a case fails here)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "diffusion-piano_amd" / "csrc" / "model_build.h"
DRIVER = ROOT / "tools" / "model_build_check"

# TaskConfig.primitive_fingertip_collisions of the three collider sets bench.py runs (its HANDS)
COLLIDERS = {"hull": False, "primitive": True, "authored": None}
NG, NX, NGT = 20, 12, 40  # PS_HAND_NGEOM, PS_HAND_NXGEOM, capsules of both hands
GEOM_BOX, GEOM_HULL = 1, 2


def run_driver(tmp_path, tc, md, song=None, n_envs=4, want_model=False):
    """-> (return code, message, DevModel bytes or None). song = (T, goal [T][89] f32, count [T] i32):
    with it every argument rule of ps_create runs, without it the hand_side rules only."""
    blob = bytes(tc) + bytes(md)
    if song is not None:
        T, goal, count = song
        blob += np.array([n_envs, T], np.int32).tobytes() + np.ascontiguousarray(goal, np.float32).tobytes()
        blob += np.ascontiguousarray(count, np.int32).tobytes()
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    out.unlink(missing_ok=True)
    p = subprocess.run([str(DRIVER), str(src)] + ([str(out)] if want_model else []), capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)  # (and no sanitizer report)
    rc, _, msg = p.stdout.rstrip("\n").partition(" ")
    return int(rc), msg, out.read_bytes() if out.exists() else None


@pytest.fixture(scope="module")
def compiled(dp):
    """(collider set, reduced_action_space, hand_side) -> (ps_model_desc, SongTables, ps_task_cfg), each built once."""
    cache = {}
    seq = dp.music.twinkle_twinkle_little_star_one_hand()

    def get(hand="hull", reduced=False, side=None):
        key = (hand, reduced, side)
        if key not in cache:
            task = dp.TaskConfig(primitive_fingertip_collisions=COLLIDERS[hand], reduced_action_space=reduced,
                                 hand_side=side)
            cache[key] = dp.compile_task(seq, task, canonical_actions=False)
        return cache[key]

    return get


def song_of(st):
    return int(st.T), np.asarray(st.goal, np.float32), np.asarray(st.count, np.int32)


@pytest.mark.parametrize("side", [None, "right", "left"])
@pytest.mark.parametrize("reduced", [False, True])
@pytest.mark.parametrize("hand", list(COLLIDERS))
def test_valid_descriptor_compiles_deterministically(compiled, tmp_path, hand, reduced, side):
    md, st, tc = compiled(hand, reduced, side)
    rc, msg, first = run_driver(tmp_path, tc, md, song_of(st), want_model=True)
    assert (rc, msg) == (0, "")
    rc, msg, second = run_driver(tmp_path, tc, md, want_model=True)  # (the driver's short input)
    assert (rc, msg) == (0, "")
    assert first is not None and len(first) > 100000 and first == second


# ---------------------------------------------------------------------------- refusals
def header_refusals():
    """The refusals of model_build.h, each as a regex over its message: the string literals of a
    `return refuse(err, ...)` in order, anything (the numbers and names put between them) between."""
    text, found, pos = HEADER.read_text(), [], 0
    while (pos := text.find("return refuse(err,", pos)) >= 0:
        pos += len("return refuse(err,")
        depth, lits = 1, []
        while depth:
            c = text[pos]
            if c == '"':
                end = text.index('"', pos + 1)  # (no message has an escaped quote)
                lits.append(text[pos + 1:end])
                pos = end
            depth += (c == "(") - (c == ")")
            pos += 1
        assert lits, text[pos - 80:pos]
        found.append(".*".join(re.escape(s) for s in lits))
    return sorted(set(found))


# Refusals that no descriptor of the fixed array extents reaches (and why). Nothing else belongs here.
UNREACHABLE = {
    re.escape("too many bodies in one level"): "PS_NHAND * PS_HAND_NBODY = 50 bodies in all; the limit per level is 64",
}


def _first_x(md, h, kind):
    return next(i for i in range(NX) if md.xgeom_type[h][i] == kind)


def _chain(md):
    for b in range(25):
        md.body_parent[0][b] = b - 1


def _star(md):
    for b in range(1, 25):
        md.body_parent[0][b] = 0


def _two_dofs_on_one_body(md):  # contiguous, so the body of the last dof is left with none
    md.dof_body[0][25] = md.dof_body[0][24]


def _swap_parent_child_dofs(md):
    j = next(j for j in range(2, 25)
             if md.body_parent[0][md.dof_body[0][j + 1]] == md.dof_body[0][j])
    md.dof_body[0][j], md.dof_body[0][j + 1] = md.dof_body[0][j + 1], md.dof_body[0][j]


def _deep_dof_tree(md):
    """Hand 0 as a legal body tree 8 levels deep whose root carries 3 slides: 3 + 7 dofs on one
    chain, over MAXDEP = 9. Body 1 is a second root without dofs, bodies 2 .. 8 the chain, the rest
    hang off bodies 0, 9, 10, 11 (at most 5 children each); dofs 0 .. 2 on body 0, then one hinge
    per body 2 .. 24 in order."""
    parent = [-1, -1, 0] + list(range(2, 8)) + [0] * 4 + [9] * 5 + [10] * 5 + [11] * 2
    for b in range(25):
        md.body_parent[0][b] = parent[b]
    for j in range(26):
        md.dof_body[0][j] = 0 if j < 3 else j - 1
        md.dof_type[0][j] = 1 if j < 3 else 0


def _same_target(md):
    a, b = [a for a in range(22) if md.act_kind[0][a] == 0][:2]
    md.act_target[0][b] = md.act_target[0][a]


def _unused_in_xpair(md):
    b = md.xpair[0][1] - NGT
    md.xgeom_type[b // NX][b % NX] = 0


def _unused_in_cappair(md):
    g = md.cappair[0][0]
    md.geom_body[g // NG][g % NG] = -1


def _goal_17_keys(song):
    song["goal"][1] = 0.0
    song["goal"][1, :17] = 1.0


def _set(name, value, *index):
    """One field of the descriptor (or, with 'tc.' / 'song.' / 'n_envs', of the other arguments) set to a value."""
    def apply(md, tc, song):
        if name == "n_envs" or name.startswith("song."):
            key = name.split(".")[-1]
            if index:
                song[key][index] = value
            else:
                song[key] = value
            return
        obj, field = (tc, name[3:]) if name.startswith("tc.") else (md, name)
        if not index:
            setattr(obj, field, value)
            return
        a = getattr(obj, field)
        for i in index[:-1]:
            a = a[i]
        if isinstance(value, (list, tuple)):
            for k, v in enumerate(value):
                a[index[-1]][k] = v
        else:
            a[index[-1]] = value
    return apply


def _md(f):
    return lambda md, tc, song: f(md)


# id: (base descriptor (collider set, reduced, hand_side), the change, a substring of the message)
TWO, RED, ONE = ("hull", False, None), ("authored", True, None), ("hull", True, "right")
REFUSALS = {
    # build_dev_model
    "n_substeps": (TWO, _set("n_substeps", 0), "n_substeps must be >= 1"),
    "keys_unsorted": (TWO, _set("key_pos", -9.0, 40, 1), "keys are not sorted along y"),
    "body_order": (TWO, _set("body_parent", 3, 0, 3), "bodies must be in tree order"),
    "body_depth": (TWO, _md(_chain), "body tree too deep"),
    "children": (TWO, _md(_star), "too many children"),
    "frictionloss": (TWO, _set("dof_frictionloss", -1.0, 1, 3), "negative dof_frictionloss"),
    "frictionloss_nan": (TWO, _set("dof_frictionloss", float("nan"), 0, 0), "negative dof_frictionloss"),
    "dofs_contiguous": (TWO, _set("dof_body", 0, 0, 5), "dofs of a body must be contiguous"),
    "n_obs_joints": (TWO, _set("n_obs_joints", 27, 0), "n_obs_joints out of range"),
    "obs_order": (TWO, _set("dof_obs_order", 26, 1, 0), "dof_obs_order out of range"),
    "obs_locked": (TWO, lambda md, tc, song: _set("dof_locked", 1, 0, md.dof_obs_order[0][0])(md, tc, song),
                   "joints_pos lists a locked dof"),
    "one_hinge": (TWO, _md(_two_dofs_on_one_body), "non-root bodies need exactly one hinge"),
    "hinges": (TWO, _set("dof_type", 1, 0, 5), "non-root dofs must be hinges"),
    "slides": (TWO, _set("dof_type", 0, 0, 0), "root dofs must be slides"),
    "dof_order": (TWO, _md(_swap_parent_child_dofs), "dofs are not in tree order"),
    "dof_depth": (TWO, _md(_deep_dof_tree), "dof tree too deep"),
    "n_action": (TWO, _set("n_action", 46), "n_action out of range"),
    "act_column_range": (RED, _set("act_column", 38, 0, 0), "act_column out of range"),
    "act_column_twice": (RED, lambda md, tc, song: _set("act_column", md.act_column[0][0], 0, 1)(md, tc, song),
                         "two actuators in one action column"),
    "act_two_on_a_dof": (TWO, _md(_same_target), "a dof may be driven by at most one actuator"),
    # (tests/test_gpu_task_kwargs.py::test_action_column_gap_is_rejected: columns 0..37 used, 38 not, 39 = sustain)
    "act_column_gap": (RED, _set("n_action", 40), "act_column must fill columns 0 .. n_action - 2 (38 actuator columns "
                                                  "for n_action 40)"),
    "capsule_body": (TWO, _set("geom_body", 25, 0, 0), "capsule body out of range"),
    "x_type": (TWO, _set("xgeom_type", 7, 1, 0), "unknown extra collider type"),
    "x_body": (TWO, lambda md, tc, song: _set("xgeom_body", 25, 0, _first_x(md, 0, GEOM_BOX))(md, tc, song),
               "extra collider body out of range"),
    "x_quat": (TWO, lambda md, tc, song: _set("xgeom_quat", [0.0] * 4, 0, _first_x(md, 0, GEOM_HULL))(md, tc, song),
               "extra collider quaternion is zero"),
    "hull_range": (TWO, lambda md, tc, song: _set("xgeom_vert", 3, 0, _first_x(md, 0, GEOM_HULL), 1)(md, tc, song),
                   "hull vertex range out of bounds"),
    "hull_range_end": (TWO, lambda md, tc, song: _set("xgeom_vert", 381, 0, _first_x(md, 0, GEOM_HULL), 0)(md, tc, song),
                       "hull vertex range out of bounds"),
    "box_size": (TWO, lambda md, tc, song: _set("xgeom_size", 0.0, 0, _first_x(md, 0, GEOM_BOX), 2)(md, tc, song),
                 "box half sizes must be positive"),
    "n_xpairs": (TWO, _set("n_xpairs", 1025), "bad n_xpairs"),
    "xpair_range": (TWO, _set("xpair", 64, 0, 1), "extra pair index out of range"),
    "xpair_unused": (TWO, _md(_unused_in_xpair), "extra pair names an unused collider"),
    "n_cappairs": (TWO, _set("n_cappairs", -1), "bad n_cappairs"),
    "cappair_range": (TWO, _set("cappair", 40, 0, 0), "capsule pair index out of range"),
    # (the all-capsule hand: no extra pair names the capsule, which would be refused first)
    "cappair_unused": (("authored", False, None), _md(_unused_in_cappair), "capsule pair names an unused slot"),
    # ps_create's hand_side rules (hand_side "right": the left hand, h = 1, has to be detached)
    "hand_side_value": (TWO, _set("tc.hand_side", 3), "hand_side must be PS_HAND_BOTH, PS_HAND_RIGHT or PS_HAND_LEFT"),
    "one_randomize": (ONE, _set("tc.randomize_hand_positions", 1), "randomize_hand_positions is an option of the two-hand"),
    "one_dof": (ONE, _set("dof_locked", 0, 1, 3), "the left hand is not detached (dof 3 is not locked)"),
    "one_capsule": (ONE, _set("geom_body", 0, 1, 2), "the left hand is not detached (capsule 2)"),
    "one_x": (ONE, _set("xgeom_type", GEOM_BOX, 1, 4), "the left hand is not detached (box / hull collider 4)"),
    "one_full_row": (ONE, _set("n_action", 0), "the left hand is not detached (the model has the full action row)"),
    "one_actuator": (ONE, _set("act_column", 0, 1, 5), "the left hand is not detached (actuator 5)"),
    "one_cappair": (ONE, _set("cappair", NG, 0, 1), "the left hand is not detached (capsule pair 0 names it)"),
    "one_xpair": (ONE, _set("xpair", NGT + NX, 0, 1), "the left hand is not detached (collider pair 0 names it)"),
    "other_side": (ONE, _set("tc.hand_side", 2), "the right hand is not detached (dof 0 is not locked)"),
    # ps_create's other argument rules
    "struct_size": (TWO, _set("tc.struct_size", 8), "rebuild against include/pianosim.h"),
    "n_envs": (TWO, _set("n_envs", 0), "n_envs must be positive"),
    "empty_song": (TWO, _set("song.T", 0), "empty song"),
    "lookahead": (TWO, _set("tc.n_steps_lookahead", -1), "negative lookahead"),
    "max_contacts": (TWO, _set("tc.max_contacts", 25), "max_contacts out of range"),
    "solver_iterations": (TWO, _set("tc.solver_iterations", -1), "negative solver_iterations"),
    "solver_refine": (TWO, _set("tc.solver_refine", 3), "solver_refine must be 0, 1 or 2"),
    "solver": (TWO, _set("tc.solver", 2), "unknown solver"),
    "note_count": (TWO, _set("song.count", 17, 1), "bad note count"),
    "goal_keys": (TWO, lambda md, tc, song: _goal_17_keys(song), "step 1 has 17 goal keys; at most 16 are supported"),
}


def refusal_inputs(compiled, name):
    """-> (ps_task_cfg, ps_model_desc, song, n_envs) of a case: copies of its base with its change applied."""
    base, change, _ = REFUSALS[name]
    md0, st, tc0 = compiled(*base)
    md, tc = type(md0).from_buffer_copy(md0), type(tc0).from_buffer_copy(tc0)
    T, goal, count = song_of(st)
    song = {"T": T, "goal": goal.copy(), "count": count.copy(), "n_envs": 4}
    change(md, tc, song)
    T = song["T"]
    return tc, md, (T, song["goal"][:max(T, 0)], song["count"][:max(T, 0)]), song["n_envs"]


@pytest.fixture(scope="module")
def refused(compiled, tmp_path_factory):
    """Every case run once: id -> (return code, message)."""
    tmp = tmp_path_factory.mktemp("refusals")
    out = {}
    for name in REFUSALS:
        tc, md, song, n_envs = refusal_inputs(compiled, name)
        out[name] = run_driver(tmp, tc, md, song, n_envs, want_model=True)
    return out


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal(refused, name):
    rc, msg, model = refused[name]
    assert rc == -1 and model is None and REFUSALS[name][2] in msg, (rc, msg)


def test_every_refusal_of_the_header_has_a_case(refused):
    patterns = header_refusals()
    assert len(patterns) >= 50 and set(UNREACHABLE) <= set(patterns)
    messages = [msg for _, msg, _ in refused.values()]
    missing = [p for p in patterns if p not in UNREACHABLE and not any(re.fullmatch(p, m) for m in messages)]
    assert not missing, missing
