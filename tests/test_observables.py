"""TaskConfig.observables / ps_task_cfg.observables without a GPU: the layout contract of the wider
row on the Python side (names -> bits, obs_layout, abi.obs_dim), on the C side (ps_obs_dim, and the
handle's widths as ps_create computes them, through the model compiler's stand-alone driver), and
the argument rules (unknown and refused names, unknown bits)."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tools" / "model_build_check"

PIANO = [("piano/joints_pos", 88), ("piano/activation", 88), ("piano/sustain_activation", 1)]
HAND = ["joints_pos_cos_sin", "joints_vel", "actuators_force", "actuators_velocity", "actuators_power",
        "fingertip_positions", "position"]
NAMES = [n for n, _ in PIANO] + HAND

# model options -> (nj, na) per kept hand: the full hand, the reduced action space (THJ5, THJ1, LFJ5
# and their actuators gone), one forearm slide (forearm_ty and its actuator gone), both
MODELS = {
    "two": (dict(), 26, 22),
    "right": (dict(hand_side="right"), 26, 22),
    "left": (dict(hand_side="left"), 26, 22),
    "reduced": (dict(reduced_action_space=True), 23, 19),
    "tx": (dict(forearm_dofs=("forearm_tx",)), 25, 21),
    "reduced_tx_left": (dict(reduced_action_space=True, forearm_dofs=("forearm_tx",), hand_side="left"), 22, 18),
}


@pytest.fixture(scope="module")
def compiled(dp):
    seq = dp.music.twinkle_twinkle_little_star_one_hand()
    return {k: dp.compile_task(seq, dp.TaskConfig(**kw), canonical_actions=False) for k, (kw, _, _) in MODELS.items()}


def expected_layout(side, fingering, lookahead, nj, na, names):
    """The row as the issue states it, written out here: the default part, then the extras in their
    fixed order. side: 0 both hands, 1 right, 2 left. -> [(key, width)]"""
    hands = ["rh_shadow_hand", "lh_shadow_hand"]
    out = [("goal", (lookahead + 1) * 89)]
    if fingering:
        out.append(("fingering", 5 if side else 10))
    out += [("piano/state", 88), ("piano/sustain_state", 1)]
    kept = hands if not side else [hands[side - 1]]
    out += [(h + "/joints_pos", nj) for h in kept]
    if side:
        out.append((kept[0] + "/position", 3))
    n_default = len(out)
    out += [(n, w) for n, w in PIANO if n in names]
    widths = dict(joints_pos_cos_sin=2 * nj, joints_vel=nj, actuators_force=na, actuators_velocity=na,
                  actuators_power=na, fingertip_positions=15, position=0 if side else 3)
    for h in kept:
        out += [(h + "/" + n, widths[n]) for n in HAND if n in names and widths[n]]
    return out, n_default


def subsets():
    for r in range(len(NAMES) + 1):
        yield from itertools.combinations(NAMES, r)


def test_names_and_bits(dp):
    abi = dp.abi
    assert list(abi.OBSERVABLES) == NAMES and abi.OBS_ALL == 0x3ff
    assert abi.obs_mask(None) == 0 and abi.obs_mask([]) == 0
    for i, n in enumerate(NAMES):
        assert abi.obs_mask([n]) == 1 << i
    # order and duplicates do not matter
    assert abi.obs_mask(["position", "joints_vel", "position", "piano/activation"]) == (1 << 9) | (1 << 4) | (1 << 1)
    header = (ROOT / "include" / "pianosim.h").read_text()
    for i, macro in enumerate(["PIANO_JOINTS_POS", "PIANO_ACTIVATION", "PIANO_SUSTAIN_ACTIVATION", "JOINTS_POS_COS_SIN",
                               "JOINTS_VEL", "ACTUATORS_FORCE", "ACTUATORS_VELOCITY", "ACTUATORS_POWER",
                               "FINGERTIP_POSITIONS", "POSITION"]):
        assert f"#define PS_OBS_{macro} (1u << {i})" in header
    assert C.sizeof(abi.TaskCfg) == abi.TaskCfg().struct_size and abi.TaskCfg.observables.size == 4


@pytest.mark.parametrize("model", list(MODELS))
def test_layout_of_every_subset(dp, compiled, model):
    md, _, tc0 = compiled[model]
    _, nj, na = MODELS[model]
    tc = type(tc0).from_buffer_copy(tc0)
    checked = 0
    for fingering, lookahead in itertools.product((0, 1), (0, 2)):
        tc.fingering_reward, tc.n_steps_lookahead = fingering, lookahead
        tc.observables = 0
        default = dp.obs_layout(tc, md)
        for names in subsets():
            tc.observables = dp.abi.obs_mask(reversed(names))  # (the order of request does not matter)
            lay = dp.obs_layout(tc, md)
            exp, n_default = expected_layout(tc.hand_side, fingering, lookahead, nj, na, names)
            assert [(k, s.stop - s.start) for k, s in lay.items()] == exp, names
            o = 0
            for s in lay.values():  # contiguous, in order
                assert s.start == o and s.stop > s.start and s.step is None
                o = s.stop
            assert o == dp.abi.obs_dim(tc, md)
            assert list(lay.items())[:n_default] == list(default.items()) and len(default) == n_default
            assert dp.abi.obs_base_dim(tc, md) == list(default.values())[-1].stop
            checked += 1
    assert checked == 4 * 1024


def test_ps_obs_dim_of_every_mask(dp):
    """The library's full-hand width (no model) against abi.obs_dim, for every mask, side, fingering, lookahead."""
    L = dp._lib.load()
    for side, fingering, lookahead in itertools.product((0, 1, 2), (0, 1), (0, 2)):
        cfg = dp.abi.TaskCfg(n_steps_lookahead=lookahead, fingering_reward=fingering, hand_side=side)
        for mask in range(dp.abi.OBS_ALL + 1):
            cfg.observables = mask
            assert L.ps_obs_dim(C.byref(cfg)) == dp.abi.obs_dim(cfg), (side, fingering, lookahead, mask)
    cfg.observables = dp.abi.OBS_ALL
    cfg.hand_side = 0
    cfg.fingering_reward, cfg.n_steps_lookahead = 1, 1
    assert L.ps_obs_dim(C.byref(cfg)) == 329 + 177 + 2 * (52 + 26 + 3 * 22 + 15 + 3)


def run_driver(tmp_path, tc, md):
    """-> (return code, message, row) of ps_create's host part; row = (default width, source codes
    of tc.observables' extras, extras' width per mask 0 .. OBS_ALL), None when refused."""
    src, out, dims = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "dims.txt"
    src.write_bytes(bytes(tc) + bytes(md))
    dims.unlink(missing_ok=True)
    p = subprocess.run([str(DRIVER), str(src), str(out), str(dims)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
    rc, _, msg = p.stdout.rstrip("\n").partition(" ")
    row = None
    if dims.exists():
        base, codes, widths = dims.read_text().split("\n")[:3]
        row = (int(base), [int(c) for c in codes.split()], [int(w) for w in widths.split()])
    return int(rc), msg, row


# DevModel::obsx source kinds (csrc/devmodel.h OX_*), in the order of the observables that use them
OX = dict(KQ=0, KACT=1, SUSACT=2, COS=3, SIN=4, V=5, ACTF=6, ACTV=7, ACTP=8, TIP=9, ROOT=10)


@pytest.mark.parametrize("model", list(MODELS))
def test_handle_row_from_the_model_compiler(dp, compiled, tmp_path, model):
    """What ps_create gives a handle (obs_base_dim and build_obs_extras of csrc/model_build.h on the
    compiled model) against the Python side: the default width, the extras' width for every mask,
    and for all extras at once where each entry's value comes from."""
    md, _, tc0 = compiled[model]
    _, nj, na = MODELS[model]
    tc = type(tc0).from_buffer_copy(tc0)
    tc.observables = dp.abi.OBS_ALL
    rc, msg, (base, codes, widths) = run_driver(tmp_path, tc, md)
    assert (rc, msg) == (0, "")
    assert base == dp.abi.obs_base_dim(tc, md) and len(widths) == dp.abi.OBS_ALL + 1
    for mask in range(dp.abi.OBS_ALL + 1):
        tc.observables = mask
        assert widths[mask] == dp.abi.obs_dim(tc, md) - base, mask
    tc.observables = dp.abi.OBS_ALL
    assert len(codes) == widths[-1] == dp.abi.obs_dim(tc, md) - base
    # the sources, entry by entry, restated from the model description
    want = [(OX["KQ"], k) for k in range(88)] + [(OX["KACT"], k) for k in range(88)] + [(OX["SUSACT"], 0)]
    for h in ((0, 1) if not tc.hand_side else (tc.hand_side - 1,)):
        dofs = [26 * h + md.dof_obs_order[h][i] for i in range(md.n_obs_joints[h] or 26)]
        col = (lambda a: md.act_column[h][a]) if md.n_action > 0 else (lambda a: 22 * h + a)
        acts = [22 * h + a for a in sorted([a for a in range(22) if col(a) >= 0], key=col)]
        assert (len(dofs), len(acts)) == (nj, na)
        want += [(OX["COS"], d) for d in dofs] + [(OX["SIN"], d) for d in dofs] + [(OX["V"], d) for d in dofs]
        want += [(kind, a) for kind in (OX["ACTF"], OX["ACTV"], OX["ACTP"]) for a in acts]
        want += [(OX["TIP"], 15 * h + i) for i in range(15)]
        if not tc.hand_side:
            want += [(OX["ROOT"], 3 * h + i) for i in range(3)]
    assert [(c >> 8, c & 255) for c in codes] == want


def test_mask_zero_is_the_default_row(dp):
    """Nothing requested: the widths of the three benchmark songs are what they were."""
    from helpers import song
    want = {"twinkle": 329, "crossing_field": 319, "guren": 329}
    for name, width in want.items():
        md, st, tc = dp.compile_task(song(dp, name), dp.TaskConfig(), canonical_actions=False)
        assert tc.observables == 0 and dp.abi.obs_dim(tc, md) == width == dp.abi.obs_base_dim(tc, md)
        assert dp._lib.load().ps_obs_dim(C.byref(tc)) == width
        md, st, tc2 = dp.compile_task(st, dp.TaskConfig(observables=[]), canonical_actions=False)
        assert bytes(tc2) == bytes(tc)


def test_argument_rules(dp, compiled, tmp_path):
    seq = dp.music.twinkle_twinkle_little_star_one_hand()
    with pytest.raises(ValueError, match="unknown observable 'joint_vel'.*known: piano/joints_pos.*joints_vel.*position"):
        dp.compile_task(seq, dp.TaskConfig(observables=["joint_vel"]))
    for name in ("joints_torque", "fingertip_force"):
        with pytest.raises(ValueError, match=f"{name}.*not modelled"):
            dp.compile_task(seq, dp.TaskConfig(observables=["joints_vel", name]))
    with pytest.raises(TypeError):
        dp.compile_task(seq, dp.TaskConfig(observables="joints_vel"))
    # `position` in the one-hand task is in the row already: naming it adds nothing
    md, _, tc = dp.compile_task(seq, dp.TaskConfig(hand_side="right", observables=["position"]))
    assert dp.abi.obs_dim(tc, md) == dp.abi.obs_base_dim(tc, md)
    assert list(dp.obs_layout(tc, md))[-1] == "rh_shadow_hand/position"
    # an unknown bit: refused by the model compiler (ps_create's and ps_obs_dim's rule) with its message
    md, _, tc0 = compiled["two"]
    tc = type(tc0).from_buffer_copy(tc0)
    tc.observables = dp.abi.OBS_ALL | 1 << 10 | 1 << 31
    rc, msg, row = run_driver(tmp_path, tc, md)
    assert rc == -1 and row is None
    assert msg == f"observables: unknown PS_OBS_* bits {1 << 10 | 1 << 31} (PS_OBS_ALL is 1023)"
    L = dp._lib.load()
    assert L.ps_obs_dim(C.byref(tc)) < 0 and b"unknown PS_OBS_* bits" in L.ps_last_error()
    assert L.ps_version() >= 7


def test_public_surface_carries_the_mask(dp):
    """TaskConfig -> ps_task_cfg -> from_compiled's TaskConfig; load(task_kwargs=) takes the field."""
    import dataclasses
    assert "observables" in [f.name for f in dataclasses.fields(dp.TaskConfig)]
    seq = dp.music.twinkle_twinkle_little_star_one_hand()
    _, _, tc = dp.compile_task(seq, dp.TaskConfig(observables=("joints_vel", "piano/activation", "joints_vel")))
    assert tc.observables == (1 << 4) | (1 << 1)
