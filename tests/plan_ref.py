"""float64 numpy restatement of the planner's kernels (csrc/plan.inc: prl_plan_perturb / _action /
_accumulate / _select), the reference of tests/test_gpu_plan_kernels.py and test_gpu_plan.py.
test_plan_ref.py pins it on hand-worked cases. The noise is rl_ref.gauss_noise, the float64
Box-Muller of the Philox words the kernel draws.

Layout: N = G * C candidates, group g = envs [g C, (g + 1) C); a plan is P knots of A actions over
H steps, knot p at step p (H - 1) / (P - 1) (P = 1: one knot at step 0)."""
import numpy as np

import rl_ref  # oracle/, on the path through conftest.py

FIRST, MID, LAST = 0, 1, 2
ZERO, LINEAR = 0, 1


def perturb(nominal, sigma, lo, hi, C, seed, offset, dtype=np.float64):
    """knots [G * C, P, A]: candidate 0 of a group clamp(nominal), the others clamp(nominal + sigma z),
    z = gauss_noise(seed, offset, N, P * A) at row = global candidate, column = p * A + a.
    ``dtype`` float32: the rounding floor (the kernel's arithmetic on the CPU)."""
    f = np.dtype(dtype).type
    nominal = np.asarray(nominal, dtype)
    G, P, A = nominal.shape
    N = G * C
    z = rl_ref.gauss_noise(seed, offset, N, P * A, dtype).reshape(N, P, A)
    z[::C] = 0
    sigma, lo, hi = (np.broadcast_to(np.asarray(x, dtype), (A,)) for x in (sigma, lo, hi))
    x = np.repeat(nominal, C, axis=0) + sigma * z
    x[::C] = np.repeat(nominal, C, axis=0)[::C]
    assert x.dtype == f
    return np.minimum(np.maximum(x, lo), hi), z


def evaluate(knots, num, den, interpolation):
    """The plans ``knots`` [..., P, A] at knot-unit time num / den (integers): past the last knot the
    last knot; zero-order the knot at or before the time; linear k0 + (rem / den) (k1 - k0)."""
    knots = np.asarray(knots, np.float64)
    P = knots.shape[-2]
    if P == 1:
        return knots[..., 0, :].copy()
    j, rem = divmod(num, den)
    if j >= P - 1:
        return knots[..., P - 1, :].copy()
    k0 = knots[..., j, :]
    if interpolation == ZERO or rem == 0:
        return k0.copy()
    k1 = knots[..., j + 1, :]
    return k0 + (rem / den) * (k1 - k0)


def action(knots, H, h, interpolation):
    """[N, A]: every candidate's action at horizon step h."""
    P = np.asarray(knots).shape[-2]
    assert 1 <= P <= H and 0 <= h < H
    return evaluate(knots, h * (P - 1), H - 1, interpolation)


def accumulate(rewards, discounts, step_types, gamma):
    """rewards / discounts / step_types [H, N] -> (ret [N], sum |w r| [N], w after every step [H, N]).
    ret += w r; w *= gamma discount; w = 0 from a LAST on. A weight of 0 adds nothing at all."""
    rewards, discounts = np.asarray(rewards, np.float64), np.asarray(discounts, np.float64)
    H, N = rewards.shape
    ret, mag, w, ws = np.zeros(N), np.zeros(N), np.ones(N), np.zeros((H, N))
    for h in range(H):
        live = w != 0
        ret[live] += w[live] * rewards[h][live]
        mag[live] += np.abs(w[live] * rewards[h][live])
        w = np.where(np.asarray(step_types[h]) == LAST, 0.0, w * (float(gamma) * discounts[h]))
        ws[h] = w
    return ret, mag, ws


def select(ret, knots, G, C, H, interpolation, shift):
    """-> best [G] (index in the group: the largest ret, ties to the lowest index, NaN never unless
    all are, then 0), best_ret [G], nominal_out [G, P, A] (the winner's knots; shift: its plan one
    control step after every knot's step, the last knot held), chosen [G, A] (its first action)."""
    ret = np.asarray(ret, np.float64).reshape(G, C)
    knots = np.asarray(knots, np.float64)
    N, P, A = knots.shape
    assert N == G * C
    best = np.zeros(G, np.int64)
    for g in range(G):
        ok = ~np.isnan(ret[g])
        if ok.any():
            best[g] = int(np.flatnonzero(ok & (ret[g] == ret[g][ok].max()))[0])
    win = knots.reshape(G, C, P, A)[np.arange(G), best]
    best_ret = ret[np.arange(G), best]
    if shift:
        nominal = np.stack([evaluate(win, p * (H - 1) + (P - 1), H - 1, interpolation) for p in range(P)], axis=1)
    else:
        nominal = win.copy()
    return best, best_ret, nominal, win[:, 0, :].copy()
