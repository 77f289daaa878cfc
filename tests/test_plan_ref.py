"""tests/plan_ref.py (the float64 reference of the planner's kernels) pinned on hand-worked cases;
the built libraries export the snapshot and planner symbols; PredictiveSampler's argument checks
raise before any GPU call. No GPU."""
import importlib
import types

import numpy as np
import pytest

import plan_ref
import rl_ref

NAN = float("nan")


def test_single_knot_is_held_over_the_horizon():
    k = np.array([[[0.25, -0.5]]])  # N = 1, P = 1, A = 2
    for H in (1, 4):
        for h in range(H):
            for mode in (plan_ref.ZERO, plan_ref.LINEAR):
                assert np.array_equal(plan_ref.action(k, H, h, mode), [[0.25, -0.5]])


def test_a_knot_per_step_is_the_knot():
    k = np.arange(8, dtype=np.float64).reshape(1, 4, 2)  # P = H = 4
    for h in range(4):
        for mode in (plan_ref.ZERO, plan_ref.LINEAR):
            assert np.array_equal(plan_ref.action(k, 4, h, mode), k[:, h])


def test_knot_times_and_interpolation():
    # P = 3 over H = 7: knots at steps 0, 3, 6
    k = np.array([[[0.0], [3.0], [-3.0]]])
    zero = [plan_ref.action(k, 7, h, plan_ref.ZERO)[0, 0] for h in range(7)]
    assert zero == [0, 0, 0, 3, 3, 3, -3]
    lin = [plan_ref.action(k, 7, h, plan_ref.LINEAR)[0, 0] for h in range(7)]
    assert np.allclose(lin, [0, 1, 2, 3, 1, -1, -3], rtol=0, atol=1e-15)
    assert lin[0] == 0 and lin[3] == 3 and lin[6] == -3  # the knot itself at a knot's step
    # P = 2 over H = 2: knots at steps 0, 1
    k2 = np.array([[[1.0], [2.0]]])
    assert [plan_ref.action(k2, 2, h, plan_ref.LINEAR)[0, 0] for h in range(2)] == [1, 2]


def test_perturb_candidate_zero_clamp_and_noise_layout():
    G, C, P, A = 2, 3, 2, 2
    nominal = np.array([[[0.5, 2.0], [-2.0, 0.0]], [[0.1, 0.2], [0.3, 0.4]]])
    knots, z = plan_ref.perturb(nominal, 0.5, -1.0, 1.0, C, seed=5, offset=9)
    assert knots.shape == (G * C, P, A)
    assert np.array_equal(knots[0], [[0.5, 1.0], [-1.0, 0.0]])  # candidate 0: clamp(nominal)
    assert np.array_equal(knots[3], nominal[1])
    want = rl_ref.gauss_noise(5, 9, G * C, P * A)  # row = global candidate, column = p * A + a
    assert np.array_equal(z[4], want[4].reshape(P, A)) and np.array_equal(z[0], np.zeros((P, A)))
    assert np.array_equal(knots[4], np.clip(nominal[1] + 0.5 * want[4].reshape(P, A), -1, 1))
    assert not np.array_equal(plan_ref.perturb(nominal, 0.5, -1.0, 1.0, C, seed=5, offset=10)[0], knots)


def test_accumulate_stops_at_last_and_at_discount_zero():
    M, L, F = plan_ref.MID, plan_ref.LAST, plan_ref.FIRST
    # env 0: plain; env 1: LAST at step 1, then the next episode's FIRST and large rewards;
    # env 2: discount 0 at step 0; env 3: a NaN reward after its LAST
    r = np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 2.0, 5.0, 2.0], [4.0, 1e6, 5.0, NAN], [8.0, 1e6, 5.0, NAN]])
    d = np.array([[1.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    st = np.array([[M, M, M, M], [M, L, M, L], [M, F, M, F], [M, M, M, M]])
    ret, mag, ws = plan_ref.accumulate(r, d, st, 0.5)
    assert ret.tolist() == [1 + 1 + 1 + 1, 1 + 1, 1, 1 + 1]
    assert mag.tolist() == ret.tolist()
    assert ws[:, 0].tolist() == [0.5, 0.25, 0.125, 0.0625] and ws[1:, 1].tolist() == [0, 0, 0]
    assert ws[:, 2].tolist() == [0, 0, 0, 0]


def test_select_ties_nan_and_copies():
    G, C, P, A, H = 2, 4, 2, 1, 3
    knots = np.arange(G * C * P * A, dtype=np.float64).reshape(G * C, P, A)
    ret = np.array([1.0, 3.0, 3.0, 2.0, NAN, -5.0, NAN, -7.0])
    best, best_ret, nominal, chosen = plan_ref.select(ret, knots, G, C, H, plan_ref.ZERO, 0)
    assert best.tolist() == [1, 1] and best_ret.tolist() == [3.0, -5.0]  # the tie to the lowest index; no NaN
    assert np.array_equal(nominal, knots[[1, 5]]) and np.array_equal(chosen, knots[[1, 5], 0])
    best, best_ret, _, _ = plan_ref.select([NAN] * 4 + [NAN, NAN, NAN, 0.0], knots, G, C, H, plan_ref.ZERO, 0)
    assert best.tolist() == [0, 3] and np.isnan(best_ret[0]) and best_ret[1] == 0.0
    best, _, _, _ = plan_ref.select([-np.inf, NAN, -np.inf, NAN] * 2, knots, G, C, H, plan_ref.ZERO, 0)
    assert best.tolist() == [0, 0]


def test_shift_resamples_one_step_later_and_holds_the_last_knot():
    # one group, one candidate; P = 3 over H = 5: knots at steps 0, 2, 4
    knots = np.array([[[0.0], [2.0], [6.0]]])
    _, _, nominal, chosen = plan_ref.select([0.0], knots, 1, 1, 5, plan_ref.LINEAR, 1)
    assert np.allclose(nominal[0, :, 0], [1.0, 4.0, 6.0], rtol=0, atol=1e-15)  # steps 1, 3 and the held last knot
    assert chosen[0, 0] == 0.0  # the first action is the unshifted plan's
    _, _, nominal, _ = plan_ref.select([0.0], knots, 1, 1, 5, plan_ref.ZERO, 1)
    assert nominal[0, :, 0].tolist() == [0.0, 2.0, 6.0]  # zero-order: step 1 is still knot 0's
    # a knot per step: the plan moves up by one knot
    k4 = np.array([[[1.0], [2.0], [3.0], [4.0]]])
    for mode in (plan_ref.ZERO, plan_ref.LINEAR):
        assert plan_ref.select([0.0], k4, 1, 1, 4, mode, 1)[2][0, :, 0].tolist() == [2.0, 3.0, 4.0, 4.0]
    k1 = np.array([[[7.0, 8.0]]])
    assert np.array_equal(plan_ref.select([0.0], k1, 1, 1, 3, plan_ref.LINEAR, 1)[2], k1)


def test_libraries_export_the_new_symbols():
    lib = importlib.import_module("diffusion-piano_amd._lib")
    L, R = lib.load(), lib.load_rl()
    for name in ("ps_snapshot_create", "ps_snapshot_bytes", "ps_snapshot_save", "ps_snapshot_restore",
                 "ps_snapshot_destroy"):
        assert hasattr(L, name) and name in lib.EXPORTS, name
    for name in ("prl_plan_perturb", "prl_plan_action", "prl_plan_accumulate", "prl_plan_select"):
        assert hasattr(R, name) and name in lib.RL_EXPORTS, name
    assert L.ps_version() >= 8 and R.prl_version() >= 3
    # argument validation happens before any device call
    assert L.ps_snapshot_create(None, 0, None) < 0 and b"null" in L.ps_last_error()
    assert L.ps_snapshot_save(None, None, None) < 0 and L.ps_snapshot_restore(None, None, None, None, None) < 0
    assert L.ps_snapshot_bytes(None) == 0
    assert R.prl_plan_perturb(None, None, None, None, 1, 1, 1, 1, 0, 0, None, None) < 0
    assert b"null" in R.prl_last_error()
    assert R.prl_plan_action(1, 4, 3, 2, 2, 0, 0, 1, None) < 0  # more knots than steps
    assert b"knots" in R.prl_last_error()
    assert R.prl_plan_action(1, 4, 2, 2, 2, 2, 0, 1, None) < 0  # step outside the horizon
    assert R.prl_plan_action(1, 4, 2, 2, 2, 0, 7, 1, None) < 0  # unknown interpolation
    assert R.prl_plan_select(1, 1, 0, 4, 1, 1, 1, 0, 0, 1, 1, 1, 1, None) < 0  # no groups


@pytest.mark.parametrize("kw,what", [(dict(groups=3, horizon=4, knots=2), "multiple"),
                                     (dict(groups=2, horizon=3, knots=4), "knots"),
                                     (dict(groups=2, horizon=3, knots=2, interpolation="cubic"), "interpolation")])
def test_predictive_sampler_refuses_bad_arguments(dp, kw, what):
    env = types.SimpleNamespace(num_envs=10)  # refused before the env is touched
    with pytest.raises(ValueError, match=what):
        dp.PredictiveSampler(env, sigma=0.1, **kw)
