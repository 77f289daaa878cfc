"""The planner's kernels (csrc/plan.inc, prl_plan_*) against tests/plan_ref.py at their edge
shapes, through the C-ABI on torch tensors.

Bounds. The noise of prl_plan_perturb is held to the rule tests/test_gpu_ppo_kernels.py applies to
prl_gauss_sample's (its ``check``: against the float64 Box-Muller of the same Philox words, within
4 x the float32 evaluation's own error). The linear interpolation is k0 + f (k1 - k0) in float32
with three roundings of relative size u = 2^-24 each - f = fl(rem / den) = f (1 + e1), d = fl(k1 -
k0) = (k1 - k0)(1 + e2), v = fl(f d + k0) = (f d + k0)(1 + e3), one fused multiply-add - so with M =
max(|k0|, |k1|), |k1 - k0| <= 2 M, f < 1 and |f d + k0| <= M (1 + 4u):
|v - exact| <= 2 M (2 u + u^2) + M (1 + 4u) u < 6 u M; the kernel then keeps v inside [min(k0, k1),
max(k0, k1)], where the exact value lies, which cannot move it away. The return is held to the
issue's H 2^-24 sum |w r|."""
import importlib

import numpy as np
import pytest

import plan_ref
from test_gpu_ppo_kernels import check, dev, empty, ptr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("diffusion-piano_amd._lib")


@pytest.fixture(scope="module")
def R(lib):
    return lib.load_rl()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def lerp_bound(knots, num, den):
    """6 u max(|k0|, |k1|) per entry of evaluate(knots [..., P, A], num / den); 0 where the result is a knot"""
    P = knots.shape[-2]
    j, rem = divmod(num, den) if P > 1 else (0, 0)
    if P == 1 or j >= P - 1 or rem == 0:
        return np.zeros(knots.shape[:-2] + knots.shape[-1:])
    return 6 * U * np.maximum(np.abs(knots[..., j, :]), np.abs(knots[..., j + 1, :]))


# ------------------------------------------------------------------------------- prl_plan_perturb
def run_perturb(R, lib, nominal, sigma, lo, hi, G, C, P, A, seed, offset):
    knots = empty(G * C, P, A)
    t = [dev(x) for x in (nominal, sigma, lo, hi)]
    lib.check_rl(R.prl_plan_perturb(*(ptr(x) for x in t), G, C, P, A, seed, offset, ptr(knots), None))
    torch.cuda.synchronize()
    return knots.cpu().numpy()


@pytest.mark.parametrize("A", [1, 45])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("G,C", [(1, 1), (1, 65), (3, 2)])
def test_perturb(R, lib, G, C, P, A):
    rng = np.random.RandomState(100 * G + 10 * C + P + A)
    seed, offset = 0xC0FFEE0012345678, (9 << 32) | 77
    nominal = (rng.randint(-8, 9, (G, P, A)) / 8).astype(np.float32)
    sigma = rng.uniform(0.05, 0.5, A).astype(np.float32)
    wide = np.full(A, 100, np.float32)
    got = run_perturb(R, lib, nominal, sigma, -wide, wide, G, C, P, A, seed, offset)
    ref64, z64 = plan_ref.perturb(nominal, sigma, -wide, wide, C, seed, offset)
    ref32, _ = plan_ref.perturb(nominal, sigma, -wide, wide, C, seed, offset, np.float32)
    assert np.array_equal(bits(got[::C]), bits(nominal))  # candidate 0: the nominal plan itself
    if C > 1:
        rep = np.repeat(nominal.astype(np.float64), C, axis=0)
        unz = lambda k: np.delete((k.astype(np.float64) - rep) / sigma, np.s_[::C], axis=0)
        check(f"plan_perturb G={G} C={C} P={P} A={A}", "z", unz(got), np.delete(z64, np.s_[::C], axis=0), unz(ref32))
    # the same seed and offset repeat bit for bit; another offset (either word) or seed does not
    assert np.array_equal(bits(got), bits(run_perturb(R, lib, nominal, sigma, -wide, wide, G, C, P, A, seed, offset)))
    if C > 1:
        for s2, o2 in ((seed, offset + 1), (seed, offset + (1 << 32)), (seed + 1, offset)):
            assert not np.array_equal(got, run_perturb(R, lib, nominal, sigma, -wide, wide, G, C, P, A, s2, o2))
    # sigma = 10 against bounds of +-1 (and a clamped nominal): inside, and exactly on the bound where clamped
    lo = np.full(A, -1, np.float32)
    nominal[0, 0, 0] = 3.0
    big = np.full(A, 10, np.float32)
    got = run_perturb(R, lib, nominal, big, lo, -lo, G, C, P, A, seed, offset)
    raw = np.repeat(nominal.astype(np.float64), C, axis=0) + 10.0 * z64
    assert (got >= -1).all() and (got <= 1).all()
    assert (got[raw > 1 + 1e-3] == 1).all() and (got[raw < -1 - 1e-3] == -1).all()
    assert got[0, 0, 0] == 1
    if C > 1:
        assert (np.abs(raw) > 1 + 1e-3).sum() > raw.size // 4


# ------------------------------------------------------------------------------- prl_plan_action
@pytest.mark.parametrize("H,P", [(1, 1), (2, 1), (2, 2), (7, 1), (7, 2), (7, 3)])
def test_action(R, lib, H, P):
    N, A = 3, 5
    rng = np.random.RandomState(10 * H + P)
    knots = rng.uniform(-1, 1, (N, P, A)).astype(np.float32)
    dk, action = dev(knots), empty(N, A)
    for mode in (plan_ref.ZERO, plan_ref.LINEAR):
        for h in range(H):
            lib.check_rl(R.prl_plan_action(ptr(dk), N, P, A, H, h, mode, ptr(action), None))
            torch.cuda.synchronize()
            got = action.cpu().numpy()
            want = plan_ref.action(knots, H, h, mode)
            bound = lerp_bound(knots.astype(np.float64), h * (P - 1), H - 1) if mode == plan_ref.LINEAR else 0 * want
            err = np.abs(got.astype(np.float64) - want)
            print(f"\nplan_action H={H} P={P} mode={mode} h={h} err={err.max():.3e} bound={bound.max():.3e}", end="")
            assert (err <= bound).all()
            if not bound.any():  # zero-order, and linear at a knot's step: the knot, bitwise
                assert np.array_equal(bits(got), bits(want.astype(np.float32)))
                assert any(np.array_equal(bits(got), bits(knots[:, p])) for p in range(P))
    if P > 1:  # knot p's step is p (H - 1) / (P - 1): whole for every knot of these shapes
        assert (H - 1) % (P - 1) == 0
        for p in range(P):
            lib.check_rl(R.prl_plan_action(ptr(dk), N, P, A, H, p * (H - 1) // (P - 1), plan_ref.LINEAR, ptr(action),
                                           None))
            torch.cuda.synchronize()
            assert np.array_equal(bits(action.cpu().numpy()), bits(knots[:, p]))


# ------------------------------------------------------------------------------- prl_plan_accumulate
def run_accumulate(R, lib, r, d, st, gamma):
    H, N = r.shape
    ret, w = empty(N), empty(N)
    dr, dd, ds = dev(r), dev(d), dev(st, torch.uint8)
    for h in range(H):
        lib.check_rl(R.prl_plan_accumulate(ptr(dr[h]), ptr(dd[h]), ptr(ds[h]), N, gamma, int(h == 0), ptr(ret), ptr(w),
                                           None))
    torch.cuda.synchronize()
    return ret.cpu().numpy(), w.cpu().numpy()


def test_accumulate(R, lib):
    H, N, gamma = 7, 320, 0.99  # (rows of 320 floats stay 64-byte aligned; two workgroups)
    rng = np.random.RandomState(3)
    r = rng.uniform(-1, 1, (H, N)).astype(np.float32)
    d = rng.choice(np.array([1, 1, 1, 0.5], np.float32), (H, N))
    st = np.full((H, N), plan_ref.MID, np.uint8)
    ended = np.arange(N) % 3 == 0  # LAST at step 2, then the next episode: FIRST and rewards of 1e6
    st[2, ended], st[3, ended] = plan_ref.LAST, plan_ref.FIRST
    r[3:, ended] = 1e6
    dead = np.arange(N) % 5 == 1   # discount 0 at step 1
    d[1, dead] = 0
    g32 = float(np.float32(gamma))  # the kernel takes gamma as a float
    ret, w = run_accumulate(R, lib, r, d, st, gamma)
    want, mag, ws = plan_ref.accumulate(r, d, st, g32)
    err = np.abs(ret.astype(np.float64) - want)
    bound = H * U * mag
    print(f"\nplan_accumulate err/bound max {np.max(err / bound):.3f}, err max {err.max():.3e}", end="")
    assert (err <= bound).all()
    assert (np.abs(want[ended]) < 4).all() and (w[ended] == 0).all() and (w[dead] == 0).all()
    np.testing.assert_allclose(w, ws[-1], rtol=2 * H * U, atol=0)
    # the excluded rewards add exactly nothing: other values there, NaN among them, the same bits
    r2 = r.copy()
    r2[3:, ended] = NAN
    r2[2:, dead & ~ended] = -1e30
    ret2, _ = run_accumulate(R, lib, r2, d, st, gamma)
    assert np.array_equal(bits(ret2), bits(ret))


# ------------------------------------------------------------------------------- prl_plan_select
def run_select(R, lib, ret, knots, G, C, P, A, H, mode, shift):
    best, best_ret = empty(G, dtype=torch.int32), empty(G)
    nominal, chosen = empty(G, P, A), empty(G, A)
    dr, dk = dev(ret), dev(knots)
    lib.check_rl(R.prl_plan_select(ptr(dr), ptr(dk), G, C, P, A, H, mode, shift, ptr(best), ptr(best_ret),
                                   ptr(nominal), ptr(chosen), None))
    torch.cuda.synchronize()
    return best.cpu().numpy(), best_ret.cpu().numpy(), nominal.cpu().numpy(), chosen.cpu().numpy()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", [1, 64, 65, 4097])
def test_select(R, lib, C, G):
    P, A, H = 3, 5, 6
    rng = np.random.RandomState(C + G)
    knots = rng.uniform(-1, 1, (G * C, P, A)).astype(np.float32)
    base = rng.uniform(0, 1, (G, C)).astype(np.float32)
    spots = sorted({p for p in (0, 63, 64, C - 1) if p < C})
    cases = []
    for i, pos in enumerate(spots):
        ret = base.copy()
        for g in range(G):  # each group's maximum at another of the spots
            ret[g, spots[(i + g) % len(spots)]] = 2
        cases.append(ret)
    if C > 1:
        tie = base.copy()
        tie[:, C // 2], tie[:, C - 1] = 2, 2  # a tie: the lowest index
        one_nan = base.copy()
        one_nan[:, 0] = NAN                   # a NaN is never chosen, wherever the wave reduction meets it
        one_nan[:, C - 1] = NAN
        most_nan = np.full((G, C), NAN, np.float32)
        most_nan[:, C - 1] = -np.inf          # ... even against -inf
        cases += [tie, one_nan, most_nan]
    cases.append(np.full((G, C), NAN, np.float32))  # all NaN: candidate 0
    for ret in cases:
        for mode, shift in ((plan_ref.ZERO, 0), (plan_ref.ZERO, 1), (plan_ref.LINEAR, 1)):
            best, best_ret, nominal, chosen = run_select(R, lib, ret, knots, G, C, P, A, H, mode, shift)
            wb, wr, wn, wc = plan_ref.select(ret, knots, G, C, H, mode, shift)
            assert np.array_equal(best, wb), (best, wb)
            assert np.array_equal(best_ret, wr.astype(np.float32), equal_nan=True)
            win = knots.reshape(G, C, P, A)[np.arange(G), wb]
            assert np.array_equal(bits(chosen), bits(win[:, 0]))
            if not shift:
                assert np.array_equal(bits(nominal), bits(win))
            elif mode == plan_ref.ZERO:
                assert np.array_equal(bits(nominal), bits(wn.astype(np.float32)))
            else:
                for p in range(P):
                    bound = lerp_bound(win.astype(np.float64), p * (H - 1) + (P - 1), H - 1)
                    assert (np.abs(nominal[:, p].astype(np.float64) - wn[:, p]) <= bound).all()
                assert np.array_equal(bits(nominal[:, P - 1]), bits(win[:, P - 1]))  # the held last knot
    if C > 1:
        assert (plan_ref.select(tie, knots, G, C, H, 0, 0)[0] == C // 2).all()
        assert (plan_ref.select(most_nan, knots, G, C, H, 0, 0)[0] == C - 1).all()
