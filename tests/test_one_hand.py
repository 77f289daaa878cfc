"""The one-hand task (PianoWithOneShadowHand, TaskConfig(hand_side=...)) on the host: the
detached-hand model description, the observation layout and the argument checks, and the
fp64 checker - unchanged - stepping that model (a detached hand is locked dofs, unused collider
slots and absent actuators, all of which it already honours)."""
import numpy as np
import pytest

from helpers import song

SIDES = (("right", 0), ("left", 1))


def _two_hand(dp, **kw):
    return dp.model.build_model(**kw)


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "reduced"])
@pytest.mark.parametrize("side,keep", SIDES)
@pytest.mark.parametrize("hull", [False, True], ids=["capsule", "hull"])
def test_detached_hand_model(dp, side, keep, reduced, hull):
    abi = dp.abi
    hand = dp.mjcf.box_hull_hand() if hull else None
    two = _two_hand(dp, hand=hand, reduced_action_space=reduced)
    md = dp.model.build_model(hand=hand, reduced_action_space=reduced, hand_side=side)
    gone = 1 - keep
    # locked dofs, empty collider slots
    assert all(md.dof_locked[gone][j] == 1 for j in range(abi.HAND_NDOF))
    assert [md.dof_locked[keep][j] for j in range(abi.HAND_NDOF)] == [two.dof_locked[keep][j]
                                                                      for j in range(abi.HAND_NDOF)]
    assert all(md.geom_body[gone][g] == -1 for g in range(abi.HAND_NGEOM))
    assert all(md.xgeom_type[gone][i] == abi.GEOM_NONE for i in range(abi.HAND_NXGEOM))
    assert [md.geom_body[keep][g] for g in range(abi.HAND_NGEOM)] == [two.geom_body[keep][g]
                                                                     for g in range(abi.HAND_NGEOM)]
    assert [md.xgeom_type[keep][i] for i in range(abi.HAND_NXGEOM)] == [two.xgeom_type[keep][i]
                                                                       for i in range(abi.HAND_NXGEOM)]
    # no pair names a detached collider; the kept hand's same-hand pairs are the two-hand model's
    hand_of = dp.model.collider_hand
    pairs = [tuple(md.cappair[i]) for i in range(md.n_cappairs)]
    xpairs = [tuple(md.xpair[i]) for i in range(md.n_xpairs)]
    assert pairs and all(hand_of(a) == keep and hand_of(b) == keep for a, b in pairs + xpairs)
    assert pairs == [p for p in (tuple(two.cappair[i]) for i in range(two.n_cappairs))
                     if hand_of(p[0]) == keep and hand_of(p[1]) == keep]
    assert xpairs == [p for p in (tuple(two.xpair[i]) for i in range(two.n_xpairs))
                      if hand_of(p[0]) == keep and hand_of(p[1]) == keep]
    assert bool(xpairs) == hull
    # actuators and the action row
    assert all(md.act_column[gone][a] == -1 for a in range(abi.HAND_NACT))
    assert md.n_action == (20 if reduced else 23) == dp.model.action_dim(md)
    cols = [md.act_column[keep][a] for a in range(abi.HAND_NACT) if md.act_column[keep][a] >= 0]
    assert cols == list(range(md.n_action - 1))
    lo, hi = dp.model.action_spec(md)
    lo2, hi2 = dp.model.action_spec(two)
    kept2 = [c for h, a, c in dp.model.action_columns(two) if h == keep]
    np.testing.assert_array_equal(lo, np.append(lo2[kept2], 0.0))
    np.testing.assert_array_equal(hi, np.append(hi2[kept2], 1.0))
    # M is block diagonal over the hands: the kept hand's and the keys' inverse weights are the
    # two-hand model's, exactly
    for name in ("body_invweight", "dof_invweight"):
        assert list(getattr(md, name)[keep]) == list(getattr(two, name)[keep]), name
    assert list(md.key_body_invweight) == list(two.key_body_invweight)
    assert list(md.key_dof_invweight) == list(two.key_dof_invweight)
    # n_obs_joints does not encode the missing joints_pos (0 means 26 there)
    assert md.n_obs_joints[gone] == 0 and md.n_obs_joints[keep] == two.n_obs_joints[keep]


@pytest.mark.parametrize("side,name", [("right", "rh"), ("left", "lh")])
def test_obs_layout(dp, side, name):
    md, st, tc = dp.compile_task(song(dp, "twinkle"), dp.TaskConfig(hand_side=side))
    assert tc.hand_side == (1 if side == "right" else 2) and tc.fingering_reward == 1
    lay = dp.obs_layout(tc, md)
    assert list(lay) == ["goal", "fingering", "piano/state", "piano/sustain_state",
                         f"{name}_shadow_hand/joints_pos", f"{name}_shadow_hand/position"]
    widths = [s.stop - s.start for s in lay.values()]
    assert widths == [178, 5, 88, 1, 26, 3]
    assert [s.start for s in lay.values()] == list(np.cumsum([0] + widths[:-1]))
    assert dp.abi.obs_dim(tc, md) == 301 == list(lay.values())[-1].stop
    # no fingering: no 'fingering' key; reduced: 23 joints; lookahead 3
    md, st, tc = dp.compile_task(song(dp, "twinkle"), dp.TaskConfig(hand_side=dp.HandSide(side), n_steps_lookahead=3,
                                                                    disable_fingering_reward=True,
                                                                    reduced_action_space=True))
    lay = dp.obs_layout(tc, md)
    assert "fingering" not in lay and dp.abi.obs_dim(tc, md) == 4 * 89 + 88 + 1 + 23 + 3
    # the two-hand layout is untouched
    md, st, tc = dp.compile_task(song(dp, "twinkle"), dp.TaskConfig())
    assert tc.hand_side == 0 and dp.abi.obs_dim(tc, md) == 178 + 10 + 88 + 1 + 52


def test_argument_errors(dp):
    seq = song(dp, "twinkle")
    with pytest.raises(ValueError, match="randomize_hand_positions"):
        dp.compile_task(seq, dp.TaskConfig(hand_side="right", randomize_hand_positions=True))
    with pytest.raises(ValueError, match="hand_side"):
        dp.compile_task(seq, dp.TaskConfig(hand_side="both"))
    with pytest.raises(ValueError, match="hand_side"):
        dp.model.build_model(hand_side="middle")


@pytest.mark.parametrize("side,keep", SIDES)
def test_checker_steps_the_one_hand_model(dp, ref, side, keep):
    n = 4
    md, st, tc = dp.compile_task(song(dp, "twinkle"), dp.TaskConfig(hand_side=side), canonical_actions=False)
    o = ref.OracleEnv(md, st, tc, n)
    assert o.action_dim == 23
    o.reset()
    lo, hi = dp.model.action_spec(md)
    rng = np.random.RandomState(5)
    gone = 1 - keep
    slots = slice(88 + 26 * gone, 88 + 26 * gone + 26)
    ncon = 0
    for _ in range(20):
        o.step(rng.uniform(lo, hi, (n, 23)).astype(np.float32))
        s = o.get_state()
        for k in ("qpos", "qvel", "qacc_ws", "ctrl"):
            assert np.isfinite(s[k]).all(), k
        for k in ("qpos", "qvel", "qacc_ws"):
            assert np.abs(s[k][:, slots]).max() == 0.0, k
        assert np.abs(s["ctrl"][:, 22 * gone:22 * gone + 22]).max() == 0.0
        for i in range(n):
            for kind, key, g1, g2, dist in o.contacts(i):
                ncon += 1
                assert dp.model.collider_hand(g2) == keep and (g1 < 0 or dp.model.collider_hand(g1) == keep)
    assert np.abs(s["qpos"][:, 88 + 26 * keep:88 + 26 * keep + 26]).max() > 0.0
    assert ncon > 0
