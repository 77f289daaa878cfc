"""Every PPO kernel of libpianorl.so against the float64 restatement (oracle/rl_ref.py) at its
edge shapes, called through the C-ABI (include/pianorl.h) on torch tensors.

Tolerance rule (``check``): for each compared tensor the metric is max|x - ref64| / max|ref64|.
The same reference function evaluated in float32 on the CPU gives the rounding floor of that
tensor, measured against the reference (not against the kernel), and the kernel must satisfy

    err_kernel <= min(4 * max(floor, 8 * 2**-23), cap)

The factor 4 covers the kernels' summation orders (16-lane DPP rows, tile order, k-ordered MFMA,
128-row chunks), which differ from the CPU's; 8 * 2**-23 covers tensors the CPU happens to
compute exactly; cap is what tests/test_gpu_ppo.py already grants (2e-4 of the tensor's maximum,
2e-5 for logged means), so an ill-conditioned floor can never loosen a check past it. An
indexing, mask, scale or bias-correction error is 1e-2 .. 1 on this metric. The six logged means
are compared entry by entry, each error divided by the mean magnitude of the terms that entry
averages (rl_ref.mlp_step's log_scale): a mean of signed rows may cancel, and its rounding error
is bounded relative to that scale, not to the remainder. Each check prints ``parity <case>
<tensor> err floor ratio`` (pytest -s; the MI355X run is kept in profiles/ppo_kernel_parity.txt).
fp64 statistics compare at 1e-12 relative.

The floor is computed at test time by the host's float32 torch and so depends on that host's
summation order, most on small tensors whose every entry carries the one rounding error of a
row's importance ratio; the kernel's side is deterministic. In the whole-step cases the floor is
therefore the largest over three float32 evaluations with the minibatch rows in different orders
(``mlp_case``), which steadies it without leaving the reference's own error.

Inputs are seeded and built so that no discontinuity is decided by rounding, and the builders
(``lnrelu_case``, ``actor_case``, ``mlp_case``: CPU only, also run by tests/test_rl_ref.py)
assert that on the reference alone: every float64 pre-activation the test controls is exactly 0
or at least 1e-3 in magnitude (multiples of 1/64, or of 1/512 at the first layer of the whole
step), every importance ratio is 1e-3 (relative) away from 1 +- clip, and in the whole-step
cases no deeper pre-activation is within 1e-5 of 0, so no row is excluded from any comparison.

The column of log_std slightly below -20 (sd = e^-20) has mean and action both exactly 0
(Z = -bias, act = 0): any other choice makes (a - mu)^2 / sd^2 ~ 1e16 and the ratio
meaningless in float32. Its log_std gradient is exactly 0 (clamped) either way.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rl_ref  # noqa: E402  (oracle/, on the path through conftest.py)

FLOOR_MIN = 8 * 2.0 ** -23
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("diffusion-piano_amd._lib")


@pytest.fixture(scope="module")
def R(lib):
    return lib.load_rl()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to("cuda:0", dtype).contiguous()


def empty(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan") if dtype.is_floating_point else -1, dtype=dtype, device="cuda:0")


def ptr(t):
    if t is None:
        return None
    assert t.is_contiguous() and t.data_ptr() % 64 == 0
    return t.data_ptr()


def metric(x, ref, scale=None):
    """max|x - ref| / max|ref|; with ``scale`` (one positive number per entry) max(|x - ref| / scale)."""
    x, ref = (torch.as_tensor(np.asarray(v.cpu()) if isinstance(v, torch.Tensor) else np.asarray(v)).to(F64)
              for v in (x, ref))
    assert x.shape == ref.shape, (x.shape, ref.shape)
    assert bool(torch.isfinite(x).all()), "non-finite values"
    if scale is not None:
        scale = torch.as_tensor(np.asarray(scale)).to(F64)
        assert bool((scale > 0).all())
        return float(((x - ref).abs() / scale).max())
    scale = float(ref.abs().max())
    diff = float((x - ref).abs().max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale


CAP, CAP_LOG = 2e-4, 2e-5  # what test_gpu_ppo.py grants gradients / logged means: never wider than that


def check(case, name, got, ref64, ref32, cap=CAP, scale=None):
    """ref32: one float32 evaluation or several (other summation orders): the floor is their largest."""
    err = metric(got, ref64, scale)
    floor = max(metric(r, ref64, scale) for r in (ref32 if isinstance(ref32, (list, tuple)) else [ref32]))
    bound = min(4 * max(floor, FLOOR_MIN), cap)
    # (a leading newline: the line must not share pytest's progress line)
    print(f"\nparity {case} {name} err={err:.3e} floor={floor:.3e} ratio={err / max(floor, FLOOR_MIN):.2f}", end="")
    assert err <= bound, (f"{case} {name}: kernel error {err:.3e} above min(4 x max(floor {floor:.3e}, "
                          f"{FLOOR_MIN:.3e}), cap {cap:.0e})")


def sixtyfourths(rng, lo, hi, size):
    return rng.randint(lo, hi + 1, size=size).astype(np.float32) / 64


# ------------------------------------------------------------------------------- prl_lnrelu_*
LN_EPS = 1e-5
BIG_STEP = (3 << 32) | 0x89ABCDEF  # a dropout step counter above 2^32: its high word is keyed
LN_SEED = 0xFEEDFACE12345678
LN_MODES = ((0.0, 0), (0.1, 0), (0.5, 2))  # (p, layer)


@functools.lru_cache(maxsize=None)
def lnrelu_case(H, B, p, layer):
    rng = np.random.RandomState(1000 * H + 10 * B + layer)
    Z = sixtyfourths(rng, -128, 128, (B, H))
    bias = sixtyfourths(rng, -64, 64, H)
    Z[0, ::7] = -bias[::7]  # exact-zero pre-activations (ReLU input 0: gradient 0)
    if B > 1:
        Z[1] = -bias  # a whole row of them: variance 0, rstd = 1 / sqrt(eps)
    gamma = rng.uniform(0.5, 1.5, H).astype(np.float32)
    beta = rng.uniform(6.0, 7.0, H).astype(np.float32)
    dY = rng.randn(B, H).astype(np.float32)
    keep = rl_ref.dropout_keep(LN_SEED, BIG_STEP, layer, B, H, p)
    out = {}
    for dt in (F64, F32):
        Y, xhat, rstd = rl_ref.lnrelu(Z, bias, gamma, beta, LN_EPS, keep, p, dt)
        dZ, dye, dyx = rl_ref.lnrelu_bwd(Z, bias, gamma, beta, LN_EPS, keep, p, dY, dt)
        out[dt] = dict(Y=Y, xhat=xhat, rstd=rstd, dZ=dZ, dyx=dyx, dye=dye)
    # margins, on the reference alone
    pre = torch.as_tensor(Z).to(F64) + torch.as_tensor(bias).to(F64)
    assert bool(((pre == 0) | (pre.abs() >= 1e-3)).all())
    assert bool((pre[0, ::7] == 0).all()) and (B == 1 or bool((pre[1] == 0).all()))
    assert bool((out[F64]["dZ"][pre == 0] == 0).all())
    kept = torch.as_tensor(keep)
    assert bool((out[F64]["Y"][kept].abs() > 1e-3).all()), "a kept Y near 0: move beta"
    assert p == 0.0 or bool((out[F64]["Y"][~kept] == 0).all())
    return dict(Z=Z, bias=bias, gamma=gamma, beta=beta, dY=dY, keep=keep, ref=out)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [256, 64, 1024, 1000, 250, 65, 63, 16, 1])
def test_lnrelu_fwd_bwd_match_fp64(R, lib, H, B):
    step = dev(np.array([BIG_STEP], np.uint64).view(np.int64), torch.int64)
    for p, layer in LN_MODES:
        c = lnrelu_case(H, B, p, layer)
        Z, bias, gamma, beta, dY = (dev(c[k]) for k in ("Z", "bias", "gamma", "beta", "dY"))
        Y, xhat, rstd = empty(B, H), empty(B, H), empty(B)
        lib.check_rl(R.prl_lnrelu_fwd(ptr(Z), ptr(bias), ptr(gamma), ptr(beta), B, H, LN_EPS, p, LN_SEED, ptr(step),
                                      layer, ptr(Y), ptr(xhat), ptr(rstd), None))
        dZ, dyx, dye = empty(B, H), empty(B, H), empty(B, H)
        lib.check_rl(R.prl_lnrelu_bwd(ptr(dY), ptr(Z), ptr(bias), ptr(xhat), ptr(rstd), ptr(gamma), B, H, p, LN_SEED,
                                      ptr(step), layer, ptr(dZ), ptr(dyx), ptr(dye), None))
        torch.cuda.synchronize()
        got = dict(Y=Y, xhat=xhat, rstd=rstd, dZ=dZ, dyx=dyx, dye=dye)
        for k, v in got.items():
            check(f"lnrelu H={H} B={B} p={p} layer={layer}", k, v, c["ref"][F64][k], c["ref"][F32][k])
        # dropped exactly where the Python mask says, and nowhere else
        assert np.array_equal(Y.cpu().numpy() == 0, ~c["keep"] if p > 0 else np.zeros((B, H), bool))
        pre0 = (c["Z"] + c["bias"]) == 0
        assert bool((dZ.cpu().numpy()[pre0] == 0).all())
    assert int(step.item()) == np.int64(np.uint64(BIG_STEP))  # read only


def test_lnrelu_dropout_mask_rate_and_keys(R, lib):
    B, H = 64, 1024
    rng = np.random.RandomState(2)
    Z, bias = dev(sixtyfourths(rng, -128, 128, (B, H))), dev(sixtyfourths(rng, -64, 64, H))
    gamma, beta = dev(np.ones(H)), dev(np.full(H, 9.0))

    def mask(p, seed, step_value, layer):
        step = dev(np.array([step_value], np.uint64).view(np.int64), torch.int64)
        Y, xhat, rstd = empty(B, H), empty(B, H), empty(B)
        lib.check_rl(R.prl_lnrelu_fwd(ptr(Z), ptr(bias), ptr(gamma), ptr(beta), B, H, LN_EPS, p, seed, ptr(step),
                                      layer, ptr(Y), ptr(xhat), ptr(rstd), None))
        torch.cuda.synchronize()
        m = Y.cpu().numpy() != 0
        assert np.array_equal(m, rl_ref.dropout_keep(seed, step_value, layer, B, H, p))
        return m

    for p in (0.1, 0.5):
        m = mask(p, LN_SEED, BIG_STEP, 0)
        se = np.sqrt(p * (1 - p) / (B * H))
        assert abs(m.mean() - (1 - p)) < 4 * se, (p, m.mean())
    base = mask(0.5, LN_SEED, BIG_STEP, 0)
    for other in (mask(0.5, LN_SEED, BIG_STEP, 2),             # layer
                  mask(0.5, LN_SEED, BIG_STEP + 1, 0),         # step, low word
                  mask(0.5, LN_SEED, BIG_STEP + (1 << 32), 0),  # step, high word
                  mask(0.5, LN_SEED + 1, BIG_STEP, 0),         # seed, low word
                  mask(0.5, LN_SEED ^ (1 << 40), BIG_STEP, 0)):  # seed, high word
        assert 0.4 < (base != other).mean() < 0.6


def test_lnrelu_refuses_bad_arguments(R):
    t = dev(np.zeros(2048))
    step = dev(np.zeros(1), torch.int64)
    a = ptr(t)
    for H, p, st in ((1025, 0.0, ptr(step)), (0, 0.0, ptr(step)), (64, 0.1, None)):
        assert R.prl_lnrelu_fwd(a, a, a, a, 1, H, LN_EPS, p, 1, st, 0, a, a, a, None) < 0
        assert b"prl_lnrelu_fwd" in R.prl_last_error()
        assert R.prl_lnrelu_bwd(a, a, a, a, a, a, 1, H, p, 1, st, 0, a, a, a, None) < 0
        assert b"prl_lnrelu_bwd" in R.prl_last_error()
    torch.cuda.synchronize()
    assert bool((t == 0).all())  # nothing was launched


# ------------------------------------------------------------------------------- prl_actor_head
CLIP, ENT_COEF = 0.2, 0.01
# (ratio target, advantage): the four clip quadrants, then inside with adv = 0, then the rest
RATIO_ADV = [(0.5, 0.7), (1.5, -1.3), (0.5, -1.3), (1.5, 0.7), (1.1, 0.0), (0.9, 0.7), (1.0, -1.3), (1.1, 0.7),
             (0.9, -1.3), (1.0, 0.7), (1.1, -1.3), (0.5, 0.0), (1.5, 0.0), (0.9, 0.0), (1.0, 0.0)]


def ratio_margin_ok(ratio, clip):
    r = np.asarray(ratio, np.float64)
    return bool(((np.abs(r / (1 - clip) - 1) >= 1e-3) & (np.abs(r / (1 + clip) - 1) >= 1e-3)).all())


def targets(n):
    t = np.array([RATIO_ADV[r % len(RATIO_ADV)] for r in range(n)], np.float64)
    return t[:, 0], t[:, 1].astype(np.float32)


@functools.lru_cache(maxsize=None)
def actor_case(A, B):
    rng = np.random.RandomState(100 * A + B)
    Z = sixtyfourths(rng, -96, 96, (B, A))
    bias = sixtyfourths(rng, -32, 32, A)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    log_std = rng.uniform(-0.7, 0.5, A).astype(np.float32)
    if A >= 3:
        log_std[1] = 2.5                    # above 2: clamped, sd = e^2
        log_std[2] = np.float32(-20.0001)   # slightly below -20: clamped, sd = e^-20 (module docstring)
        Z[:, 2], act[:, 2] = -bias[2], 0.0
    tgt, adv = targets(B)
    old_lp = (rl_ref.actor_log_prob(Z, bias, log_std, act).numpy() - np.log(tgt)).astype(np.float32)
    ref = {dt: rl_ref.actor_head(Z, bias, log_std, act, old_lp, adv, CLIP, ENT_COEF, dt) for dt in (F64, F32)}
    ratio = ref[F64]["ratio"].numpy()
    assert ratio_margin_ok(ratio, CLIP)
    assert np.abs(ratio / tgt - 1).max() < 1e-4  # old_lp's rounding moved no ratio off its target
    if B >= 5:
        lo, hi = ratio < 1 - CLIP, ratio > 1 + CLIP
        for sel in (lo & (adv > 0), lo & (adv < 0), hi & (adv > 0), hi & (adv < 0), ~lo & ~hi, adv == 0):
            assert sel.any()
    if A >= 3:
        assert float(log_std[2]) < -20 and bool((ref[F64]["dls"][:, 1:3] == 0).all())
        ls_c = np.clip(log_std.astype(np.float64), -20, 2)
        assert abs(float(ref[F64]["ent_rows"][0]) - (0.5 + 0.5 * np.log(2 * np.pi) + ls_c.mean())) < 1e-12
    return dict(Z=Z, bias=bias, log_std=log_std, act=act, old_lp=old_lp, adv=adv, ref=ref)


@pytest.mark.parametrize("B", [1, 4, 5, 67])
@pytest.mark.parametrize("A", [45, 23, 39, 64, 1])
def test_actor_head_matches_fp64(R, lib, A, B):
    c = actor_case(A, B)
    Z, bias, log_std, act, old_lp, adv = (dev(c[k]) for k in ("Z", "bias", "log_std", "act", "old_lp", "adv"))
    dZ, dls, stats, ent = empty(B, A), empty(B, A), empty(B), empty(B)
    lib.check_rl(R.prl_actor_head(ptr(Z), ptr(bias), ptr(log_std), ptr(act), ptr(old_lp), ptr(adv), B, A, CLIP,
                                  ENT_COEF, ptr(dZ), ptr(dls), ptr(stats), ptr(ent), None))
    torch.cuda.synchronize()
    for k, v in (("dZ", dZ), ("dls", dls), ("rows", stats), ("ent_rows", ent)):
        check(f"actor_head A={A} B={B}", k, v, c["ref"][F64][k], c["ref"][F32][k])
    if A >= 3:
        assert bool((dls[:, 1:3] == 0).all())  # the clamped columns, exactly


def test_actor_head_refuses_wide_action(R):
    t = dev(np.zeros(256))
    a = ptr(t)
    for A in (0, 65):
        assert R.prl_actor_head(a, a, a, a, a, a, 1, A, CLIP, ENT_COEF, a, a, a, a, None) < 0
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ------------------------------------------------------------------------------- prl_critic_head
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_critic_head_matches_fp64(R, lib, B):
    rng = np.random.RandomState(B)
    Z, bias, ret = rng.randn(B).astype(np.float32), np.array([0.375], np.float32), rng.randn(B).astype(np.float32)
    dZ, v, sq = empty(B), empty(B), empty(B)
    dZin, dbias, dret = dev(Z), dev(bias), dev(ret)  # (held: a temporary's memory is reused by the next one)
    lib.check_rl(R.prl_critic_head(ptr(dZin), ptr(dbias), ptr(dret), B, ptr(dZ), ptr(v), ptr(sq), None))
    torch.cuda.synchronize()
    ref = {dt: rl_ref.critic_head(Z, bias, ret, dt) for dt in (F64, F32)}
    for k, g in (("dZ", dZ), ("v", v), ("sq", sq)):
        check(f"critic_head B={B}", k, g, ref[F64][k], ref[F32][k])


# ------------------------------------------------------------------------------- prl_colsums
COLS = (1, 45, 127, 128, 129, 256)


def run_colsums(R, srcs, scale, B, scratch, scratch_floats=None):
    n = len(srcs)
    dsts = [empty(s.shape[1]) for s in srcs]
    src_a = (C.c_void_p * n)(*[ptr(s) for s in srcs])
    dst_a = (C.c_void_p * n)(*[ptr(d) for d in dsts])
    cols_a = (C.c_int * n)(*[s.shape[1] for s in srcs])
    scale_a = (C.c_float * n)(*scale) if scale is not None else None
    rc = R.prl_colsums(n, src_a, cols_a, scale_a, dst_a, B, ptr(scratch),
                       scratch.numel() if scratch_floats is None else scratch_floats, None)
    torch.cuda.synchronize()
    return rc, dsts


@pytest.mark.parametrize("n", [1, 32])
@pytest.mark.parametrize("B", [1, 127, 128, 129, 300])
def test_colsums_match_fp64(R, lib, B, n):
    """The entries are drawn with mean 1, so that a one-column entry's sum (the whole tensor,
    hence the metric's scale) is not the remainder of a cancellation. With zero-mean entries the
    B = 127, one-column entry measured err 6.7e-6 against a floor of 7.8e-7: the kernel adds a
    column's rows one by one in row order (error growing with the row count, up to 128 per
    chunk), the CPU pairwise, and both were divided by a sum that had cancelled to a few units.
    That is conditioning of the input, not of the kernel, so the inputs changed and the rule did
    not."""
    rng = np.random.RandomState(B * 40 + n)
    cols = [int(c) for c in rng.choice(COLS, n)] if n > 1 else [129]
    if n > 1:
        cols[:len(COLS)] = COLS  # every width at least once
    X = [(rng.randn(B, c) + 1.0).astype(np.float32) for c in cols]
    srcs = [dev(x) for x in X]
    need = -(-B // 128) * sum(cols)
    scratch = empty(max(need, 1))
    for scale in (None, [float(np.float32(s)) for s in rng.uniform(0.5, 2.0, n)]):
        rc, dsts = run_colsums(R, srcs, scale, B, scratch, need)  # the documented size, exactly
        lib.check_rl(rc)
        rc2, dsts2 = run_colsums(R, srcs, scale, B, scratch, need)
        lib.check_rl(rc2)
        worst = (0.0, 0.0)
        for i, (x, d, d2) in enumerate(zip(X, dsts, dsts2)):
            assert torch.equal(d, d2)  # deterministic
            s = 1.0 if scale is None else scale[i]
            r64, r32 = rl_ref.colsums(x, s, F64), rl_ref.colsums(x, np.float32(s), F32)
            err, floor = metric(d, r64), metric(r32, r64)
            assert err <= 4 * max(floor, FLOOR_MIN), (i, cols[i], err, floor)
            worst = max(worst, (err / max(floor, FLOOR_MIN), err))
        print(f"\nparity colsums B={B} n={n} scale={'given' if scale else 'NULL'} worst entry err={worst[1]:.3e} "
              f"ratio={worst[0]:.2f}", end="")


def test_colsums_refuse_small_scratch_and_too_many_entries(R):
    B = 129
    srcs = [dev(np.ones((B, 45)))]
    scratch = empty(2 * 45)
    rc, dsts = run_colsums(R, srcs, None, B, scratch, 2 * 45 - 1)
    assert rc < 0 and b"scratch" in R.prl_last_error()
    assert bool(torch.isnan(dsts[0]).all()) and bool(torch.isnan(scratch).all())  # nothing launched
    srcs = [dev(np.ones((4, 3))) for _ in range(33)]
    rc, dsts = run_colsums(R, srcs, None, 4, scratch)
    assert rc < 0
    assert all(bool(torch.isnan(d).all()) for d in dsts)


# ------------------------------------------------------------------------------- prl_gather_minibatch
@pytest.mark.parametrize("adim", [1, 45])
@pytest.mark.parametrize("sdim", [1, 329, 600])
def test_gather_minibatch_is_bitwise(R, lib, sdim, adim):
    rng = np.random.RandomState(sdim + adim)
    N, B = 50, 37
    S, A = dev(rng.randn(N, sdim)), dev(rng.randn(N, adim))
    lp, adv, ret = dev(rng.randn(N)), dev(rng.randn(N)), dev(rng.randn(N))
    ix = rng.randint(0, N, B)
    ix[3], ix[4], ix[-1] = N - 1, ix[5], N - 1  # the last row, and repeats
    idx = dev(ix, torch.int64)
    step0 = (1 << 32) - 1  # the increment carries into the high word
    for step in (dev(np.array([step0], np.int64), torch.int64), None):
        oS, oA, olp, oadv, oret = empty(B, sdim), empty(B, adim), empty(B), empty(B), empty(B)
        lib.check_rl(R.prl_gather_minibatch(ptr(S), sdim, ptr(A), adim, ptr(lp), ptr(adv), ptr(ret), ptr(idx), B,
                                            ptr(oS), ptr(oA), ptr(olp), ptr(oadv), ptr(oret), ptr(step), None))
        torch.cuda.synchronize()
        for got, src in ((oS, S), (oA, A), (olp, lp), (oadv, adv), (oret, ret)):
            assert torch.equal(got, src.index_select(0, idx))
        if step is not None:
            assert int(step.item()) == step0 + 1


# ------------------------------------------------------------------------------- prl_gauss_sample
@pytest.mark.parametrize("n,a", [(1, 1), (5, 64), (7, 23), (1000, 45)])
def test_gauss_sample_matches_philox_box_muller(R, lib, n, a):
    """Pins the sampler's Philox keying (column, row, offset lo / hi; seed lo / hi): the noise is
    the float64 Box-Muller of the same two words."""
    rng = np.random.RandomState(7 * n + a)
    seed, offset = 0xC0FFEE0012345678, (9 << 32) | 77
    mean = (rng.randint(-8, 9, (n, a)) / 8).astype(np.float32)
    log_std = rng.uniform(-0.7, 0.5, a).astype(np.float32)
    if a >= 3:
        log_std[1] = 3.0     # clamped to 2
        log_std[2] = -25.0   # clamped to -20: sd = e^-20, so the mean is 0 to keep sd * z visible
        mean[:, 2] = 0.0
    action, logp = empty(n, a), empty(n)
    dmean, dls = dev(mean), dev(log_std)
    lib.check_rl(R.prl_gauss_sample(ptr(dmean), ptr(dls), n, a, seed, offset, ptr(action), ptr(logp), None))
    torch.cuda.synchronize()
    act = action.cpu().numpy()
    sd = np.exp(np.clip(log_std.astype(np.float64), -20, 2))
    z64 = rl_ref.gauss_noise(seed, offset, n, a)
    z_gpu = (act.astype(np.float64) - mean) / sd
    # the floor: the float32 Box-Muller of the same words, through the same mean + sd * z
    z32 = rl_ref.gauss_noise(seed, offset, n, a, np.float32)
    act32 = mean + np.exp(np.clip(log_std, np.float32(-20), np.float32(2))) * z32
    assert act32.dtype == np.float32
    check(f"gauss_sample n={n} a={a}", "z", z_gpu, z64, (act32.astype(np.float64) - mean) / sd)
    want = rl_ref.gauss_logp(mean, log_std, act)
    np.testing.assert_allclose(logp.cpu().numpy(), want, rtol=1e-5, atol=1e-4)
    # another offset / seed word gives other noise
    for s2, o2 in ((seed, offset + 1), (seed, offset + (1 << 32)), (seed + 1, offset), (seed ^ (1 << 33), offset)):
        assert np.abs(rl_ref.gauss_noise(s2, o2, n, a) - z64).max() > 1e-3


def test_gauss_sample_refuses_wide_action(R):
    t = dev(np.zeros(256))
    assert R.prl_gauss_sample(ptr(t), ptr(t), 2, 65, 1, 0, ptr(t), ptr(t), None) < 0
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ------------------------------------------------------------------------------- prl_clip_adam
BETAS, ADAM_EPS, MAX_NORM = (0.9, 0.999), 1e-5, 0.5
LRS = [float(np.float32(x)) for x in (1e-2, 2e-2, 3e-2, 4e-2)]  # distinct per segment


def seg_ends(n, nseg):
    """Segment ends inside a block (no multiple of 256), one segment empty at nseg = 4."""
    def inside(x):
        x = max(1, min(n, int(x)))
        return x + 1 if (x % 256 == 0 and x < n) else x
    if nseg == 1:
        return [n]
    if nseg == 2:
        return [inside(0.37 * n), n]
    a, b = inside(0.21 * n), inside(0.58 * n)
    return [a, a, max(a, b), n]  # segment 1 is empty


def adam_inputs(n, nseg, seed):
    rng = np.random.RandomState(seed)
    ends = seg_ends(n, nseg)
    p = rng.uniform(-1, 1, n).astype(np.float32)
    m = (rng.randn(n) * 0.1).astype(np.float32)
    v = (rng.rand(n) * 0.01).astype(np.float32)
    return ends, p, m, v, rng


def adam_grad(rng, n, ends, k):
    """Clipping active in the even segments (norm > MAX_NORM), inactive in the odd ones."""
    g = np.zeros(n, np.float32)
    lo, live = 0, 0
    for hi in ends:
        if hi > lo:
            x = rng.randn(hi - lo)
            x[0] += 1.0  # (a one-element segment with a zero gradient has no norm)
            norm = (3.0 + k) if live % 2 == 0 else 0.1 / (1 + k)
            g[lo:hi] = (x * norm / np.sqrt((x * x).sum())).astype(np.float32)
            live += 1
        lo = hi
    return g


@pytest.mark.parametrize("nseg", [1, 2, 4])
@pytest.mark.parametrize("n", [300_000, 1024 + 3, 255, 1, 2_300_000])
def test_clip_adam_matches_fp64(R, lib, n, nseg):
    """n = 2 300 000 is the only size that enters clip_adam_kernel's grid-stride tail loop
    (above 2048 blocks x 256 threads x 4 elements = 2 097 152); the others end in the unrolled
    first pass. Each call starts from the device's own state, so each step is held to the
    reference on its own."""
    ends, p, m, v, rng = adam_inputs(n, nseg, 17 * n + nseg)
    P, M, V = dev(p), dev(m), dev(v)
    step = dev(np.zeros(nseg))
    lr = dev(LRS[:nseg])
    scratch = empty(256 * 4, dtype=torch.float64)
    seg = (C.c_int64 * nseg)(*ends)
    for k in range(3):
        g = adam_grad(rng, n, ends, k)
        p0, m0, v0, s0 = P.cpu().numpy(), M.cpu().numpy(), V.cpu().numpy(), step.cpu().numpy()
        G = dev(g)
        lib.check_rl(R.prl_clip_adam(ptr(P), ptr(G), ptr(M), ptr(V), seg, nseg, ptr(lr), ptr(step), BETAS[0],
                                     BETAS[1], ADAM_EPS, MAX_NORM, ptr(scratch), None, None))
        torch.cuda.synchronize()
        r64 = rl_ref.clip_adam(p0, g, m0, v0, ends, LRS, s0, BETAS, ADAM_EPS, MAX_NORM)
        r32 = rl_ref.clip_adam(p0, g, m0, v0, ends, LRS, s0, BETAS, ADAM_EPS, MAX_NORM, np.float32)
        live = [s for s in range(nseg) if ends[s] > (ends[s - 1] if s else 0)]
        for j, s in enumerate(live):  # on the reference: clipping on / off in neighbouring segments
            assert (r64[4][s] > MAX_NORM + 0.05) if j % 2 == 0 else (r64[4][s] < MAX_NORM - 0.05)
        case = f"clip_adam n={n} nseg={nseg} call={k + 1}"
        check(case, "param", P, r64[0], r32[0])
        check(case, "exp_avg", M, r64[1], r32[1])
        check(case, "exp_avg_sq", V, r64[2], r32[2])
        assert step.cpu().tolist() == [float(k + 1)] * nseg
        # the fp64 statistic: the norm pass's partials per segment
        sums = scratch.cpu().numpy().reshape(256, 4)[:min(256, -(-n // 256))].sum(0)
        np.testing.assert_allclose(sums[:nseg], r64[4] ** 2, rtol=1e-12)


def test_clip_adam_max_norm_zero_and_guard(R, lib):
    n, nseg = 1027, 2
    ends, p, m, v, rng = adam_inputs(n, nseg, 5)
    g = adam_grad(rng, n, ends, 0)
    P, M, V, G = dev(p), dev(m), dev(v), dev(g)
    step, lr = dev(np.zeros(nseg)), dev(LRS[:nseg])
    scratch = empty(256 * 4, dtype=torch.float64)
    seg = (C.c_int64 * nseg)(*ends)
    guard = dev(np.array([3]), torch.int32)
    lib.check_rl(R.prl_clip_adam(ptr(P), ptr(G), ptr(M), ptr(V), seg, nseg, ptr(lr), ptr(step), *BETAS, ADAM_EPS,
                                 MAX_NORM, ptr(scratch), ptr(guard), None))
    torch.cuda.synchronize()
    for t, x in ((P, p), (M, m), (V, v), (G, g), (step, np.zeros(nseg, np.float32))):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))  # bitwise unchanged
    guard.zero_()
    for max_norm in (0.0, -1.0):  # no clipping
        P, M, V, step = dev(p), dev(m), dev(v), dev(np.zeros(nseg))
        lib.check_rl(R.prl_clip_adam(ptr(P), ptr(G), ptr(M), ptr(V), seg, nseg, ptr(lr), ptr(step), *BETAS, ADAM_EPS,
                                     max_norm, ptr(scratch), ptr(guard), None))
        torch.cuda.synchronize()
        r64 = rl_ref.clip_adam(p, g, m, v, ends, LRS, np.zeros(nseg), BETAS, ADAM_EPS, max_norm)
        r32 = rl_ref.clip_adam(p, g, m, v, ends, LRS, np.zeros(nseg), BETAS, ADAM_EPS, max_norm, np.float32)
        assert r64[4][0] > MAX_NORM  # (it would have been clipped)
        for name, t, j in (("param", P, 0), ("exp_avg", M, 1), ("exp_avg_sq", V, 2)):
            check(f"clip_adam max_norm={max_norm}", name, t, r64[j], r32[j])
    bad = (C.c_int64 * 2)(5, 3)
    assert R.prl_clip_adam(ptr(P), ptr(G), ptr(M), ptr(V), bad, 2, ptr(lr), ptr(step), *BETAS, ADAM_EPS, MAX_NORM,
                           ptr(scratch), None, None) < 0
    assert R.prl_clip_adam(ptr(P), ptr(G), ptr(M), ptr(V), seg, 5, ptr(lr), ptr(step), *BETAS, ADAM_EPS, MAX_NORM,
                           ptr(scratch), None, None) < 0


@pytest.mark.parametrize("nparts", [1, 4, 257])
def test_clip_adam_parts_matches_clip_adam(R, lib, nparts):
    """The per-segment sums of squares arrive split over nparts rows; 257 rows exceed the
    block's 256 threads, so the strided fold of the partials runs."""
    n, nseg = 300_000, 2
    ends, p, m, v, rng = adam_inputs(n, nseg, 23)
    g = adam_grad(rng, n, ends, 0)
    g64 = g.astype(np.float64)
    tot = np.array([(g64[:ends[0]] ** 2).sum(), (g64[ends[0]:] ** 2).sum()])
    w = rng.rand(nparts, 1) + 0.1
    parts = np.zeros((nparts, 4))
    parts[:, :2] = (w / w.sum()) * tot
    parts[:, 2:] = 1e30  # (the unused segments' columns are not read into any result)
    seg = (C.c_int64 * nseg)(*ends)
    lr = dev(LRS[:nseg])
    steps = np.array([3.0, 7.0], np.float32)  # already advanced by the caller
    P, M, V, step = dev(p), dev(m), dev(v), dev(steps)
    G, parts_d = dev(g), dev(parts, torch.float64)
    lib.check_rl(R.prl_clip_adam_parts(ptr(P), ptr(G), ptr(M), ptr(V), seg, nseg, ptr(lr), ptr(step), *BETAS,
                                       ADAM_EPS, MAX_NORM, ptr(parts_d), nparts, None, None))
    torch.cuda.synchronize()
    assert step.cpu().tolist() == [3.0, 7.0]  # not advanced here
    r64 = rl_ref.clip_adam(p, g, m, v, ends, LRS, steps - 1, BETAS, ADAM_EPS, MAX_NORM, sumsq=parts[:, :2].sum(0))
    r32 = rl_ref.clip_adam(p, g, m, v, ends, LRS, steps - 1, BETAS, ADAM_EPS, MAX_NORM, np.float32,
                           sumsq=parts[:, :2].sum(0))
    # prl_clip_adam from the same state: the same numbers to the same rule
    P2, M2, V2, step2 = dev(p), dev(m), dev(v), dev(steps - 1)
    scratch = empty(256 * 4, dtype=torch.float64)
    lib.check_rl(R.prl_clip_adam(ptr(P2), ptr(G), ptr(M2), ptr(V2), seg, nseg, ptr(lr), ptr(step2), *BETAS,
                                 ADAM_EPS, MAX_NORM, ptr(scratch), None, None))
    torch.cuda.synchronize()
    assert step2.cpu().tolist() == [3.0, 7.0]
    for name, t, t2, j in (("param", P, P2, 0), ("exp_avg", M, M2, 1), ("exp_avg_sq", V, V2, 2)):
        check(f"clip_adam_parts nparts={nparts}", name, t, r64[j], r32[j])
        check(f"clip_adam_parts nparts={nparts} (prl_clip_adam)", name, t2, r64[j], r32[j])
    assert R.prl_clip_adam_parts(ptr(P), ptr(G), ptr(M), ptr(V), seg, nseg, ptr(lr), ptr(step), *BETAS, ADAM_EPS,
                                 MAX_NORM, None, nparts, None, None) < 0


# ------------------------------------------------------------------------------- prl_mlp_step*
MLP_SEED = 0x0DDBA11C0DE5EED5
MLP_STEP0 = (2 << 32) | 41
CRITIC_P = (0.1, 0.1, 0.0)  # the agent's critic (ppo.Critic)

# name: hidden widths, sdim, A, B, critic / actor dropout (pc / pa), entry point (mode), nseg (norm),
# reseed: the seed offset at which no row of the float64 reference sits within 1e-5 of a ReLU kink
MLP_CASES = {
    "suite-shape":   dict(h=(256, 256, 256), sdim=64, A=45, B=512, reseed=18),
    "agent-512-idx": dict(h=(256, 256, 256), sdim=329, A=45, B=512, pc=CRITIC_P, mode="idx", reseed=48),
    "tiny-all-1":    dict(h=(16, 16, 16), sdim=1, A=1, B=1),
    "48-32-16-drop": dict(h=(48, 32, 16), sdim=3, A=23, B=15, pc=CRITIC_P),
    "256-128-64":    dict(h=(256, 128, 64), sdim=15, A=39, B=16),
    "actor-drop":    dict(h=(128, 256, 128), sdim=16, A=64, B=17, pa=(0.0, 0.25, 0.0)),
    "norm-nseg2":    dict(h=(16, 16, 16), sdim=17, A=45, B=33, mode="norm", nseg=2),
    "widest-nseg1":  dict(h=(48, 32, 16), sdim=400, A=23, B=33, mode="norm", nseg=1, pc=CRITIC_P, reseed=1),
    "A1-512-drop":   dict(h=(256, 128, 64), sdim=64, A=1, B=512, pc=CRITIC_P, reseed=1),
    "329-B15":       dict(h=(128, 256, 128), sdim=329, A=39, B=15),
    "B1-wide":       dict(h=(256, 256, 256), sdim=329, A=64, B=1, pc=CRITIC_P, mode="idx"),
    "B16-A23":       dict(h=(16, 16, 16), sdim=16, A=23, B=16),
}
# the column-split rows kernel (B <= 256, hidden 128 / 256, state width 32..384)
SPLIT_CASES = {
    "split-s32-B1":    dict(h=(128, 128, 128), sdim=32, A=45, B=1),
    "split-s384-B16":  dict(h=(256, 128, 256), sdim=384, A=23, B=16, noguard=True),
    "split-s32-B40":   dict(h=(256, 128, 256), sdim=32, A=39, B=40, pc=CRITIC_P),
    "split-s384-B256": dict(h=(128, 128, 128), sdim=384, A=64, B=256, mode="idx"),
}


def test_mlp_cases_cover_every_listed_value():
    c = MLP_CASES.values()
    assert {x["h"] for x in c} == {(16, 16, 16), (48, 32, 16), (256, 128, 64), (128, 256, 128), (256, 256, 256)}
    assert {x["sdim"] for x in c} == {1, 3, 15, 16, 17, 64, 329, 400}
    assert {x["A"] for x in c} == {1, 23, 39, 45, 64}
    assert {x["B"] for x in c} == {1, 15, 16, 17, 33, 512}
    assert sum(1 for x in c if "pc" in x) >= 3 and sum(1 for x in c if "pa" in x) >= 1
    assert sum(1 for x in c if x.get("mode") in ("idx", "norm")) >= 2
    assert {x.get("nseg") for x in c if x.get("mode") == "norm"} == {1, 2}
    s = SPLIT_CASES.values()
    assert {x["sdim"] for x in s} == {32, 384} and {x["B"] for x in s} == {1, 16, 40, 256}
    assert {x["h"] for x in s} == {(128, 128, 128), (256, 128, 256)}


def all_cases():
    return {**MLP_CASES, **SPLIT_CASES}


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    """Inputs, float64 reference, float32 floor and the margin assertions of one whole-step case
    (CPU only).

    The returns are drawn with mean 1.5. The critic's output-bias gradient is ONE number,
    (2 / B) sum_r (v_r - ret_r), and with no dropout on layer 2 the whole of critic.dbeta2 is that
    number times the output weights. With zero-mean returns its terms cancel, and the metric
    divides the float32 error of the values v_r (three LayerNorm layers deep, ~1e-6 of |v|) by the
    remainder, while the floor of a one-number tensor is a single draw of the same noise: the
    case split-s384-B16 measured critic.db3 9.5e-6 / floor 2.5e-6 and critic.dbeta2 9.9e-6 /
    2.2e-6 (4.59 x), every other tensor of it below 2.3 x. That is the conditioning of the input,
    not the kernel's arithmetic, so the input changed and the rule did not."""
    cfg = all_cases()[name]
    h, sdim, A, B = cfg["h"], cfg["sdim"], cfg["A"], cfg["B"]
    mode = cfg.get("mode", "direct")
    rng = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + cfg.get("reseed", 0))
    N = B if mode == "direct" else 3 * B
    nets = []
    for i, (out, p) in enumerate(((A, cfg.get("pa", (0.0,) * 3)), (1, cfg.get("pc", (0.0,) * 3)))):
        widths = [sdim, *h, out]
        W, b = [], []
        for l in range(4):
            if l == 0:  # multiples of 1/64 (states: of 1/8): the first pre-activation is exact
                W.append(sixtyfourths(rng, -24, 24, (widths[1], widths[0])))
                b.append(sixtyfourths(rng, -32, 32, widths[1]))
            else:
                W.append((rng.randn(widths[l + 1], widths[l]) * (1.3 / np.sqrt(widths[l]))).astype(np.float32))
                b.append((rng.randn(widths[l + 1]) * 0.3).astype(np.float32))
        net = dict(W=W, b=b, gamma=[rng.uniform(0.5, 1.5, w).astype(np.float32) for w in h],
                   beta=[(rng.randn(w) * 0.3).astype(np.float32) for w in h], p=list(p))
        if i == 0:
            net["log_std"] = rng.uniform(-0.7, 0.5, A).astype(np.float32)
            if A >= 3:
                net["log_std"][1] = 2.5  # clamped: gradient exactly 0
        nets.append(net)
    S = (rng.randint(-16, 17, (N, sdim)) / 8).astype(np.float32)
    act = rng.uniform(-1, 1, (N, A)).astype(np.float32)
    ret = (rng.randn(N) + 1.5).astype(np.float32)
    idx = None
    if mode != "direct":
        idx = rng.randint(0, N, B)
        idx[0], idx[B // 2] = N - 1, idx[B - 1]  # the last row, a repeat
    step_eff = MLP_STEP0 + (0 if idx is None else 1)
    keeps = [[rl_ref.dropout_keep(MLP_SEED, step_eff, l, B, h[l], net["p"][l]) if net["p"][l] > 0 else None
              for l in range(3)] for net in nets]
    tgt, adv = targets(N)
    zeros = np.zeros(N, np.float32)
    # the new log-prob of every rollout row, to place its ratio (actor dropout only in direct
    # cases, where rollout row = minibatch row = mask row; the critic plays no part in it)
    assert idx is None or not any(nets[0]["p"])
    lp = rl_ref.mlp_step([nets[0], dict(nets[1], p=[0.0] * 3)], S, act, zeros, adv, ret, None, CLIP, ENT_COEF, LN_EPS,
                         [keeps[0], [None] * 3], F64)["lp"]
    old_lp = (lp.numpy() - np.log(tgt)).astype(np.float32)
    ref = {F64: rl_ref.mlp_step(nets, S, act, old_lp, adv, ret, idx, CLIP, ENT_COEF, LN_EPS, keeps, F64)}
    # the float32 floor over three orders of the minibatch rows (as given, reversed, shuffled):
    # every compared tensor is a sum over the rows, so each order is another float32 evaluation of
    # the same numbers, and their largest error depends less on one host's summation order
    ref[F32] = []
    for perm in (np.arange(B), np.arange(B)[::-1].copy(), np.random.RandomState(B).permutation(B)):
        kp = [[None if k is None else k[perm] for k in net_keeps] for net_keeps in keeps]
        if idx is None:
            args = (S[perm], act[perm], old_lp[perm], adv[perm], ret[perm], None)
        else:
            args = (S, act, old_lp, adv, ret, idx[perm])
        ref[F32].append(rl_ref.mlp_step(nets, *args, CLIP, ENT_COEF, LN_EPS, kp, F32))
    # margins, on the float64 reference alone
    r64 = ref[F64]
    assert ratio_margin_ok(r64["ratio"].numpy(), CLIP), name
    excluded = torch.zeros(B, dtype=torch.bool)
    for i in range(2):
        z0 = r64["preact"][i][0]
        assert bool(((z0 == 0) | (z0.abs() >= 1e-3)).all()), name
        for l in (1, 2):
            excluded |= (r64["preact"][i][l].abs() < 1e-5).any(1)
    assert int(excluded.sum()) == 0, f"{name}: rows {excluded.nonzero().flatten().tolist()} sit on a ReLU kink; reseed"
    return dict(cfg=cfg, nets=nets, S=S, act=act, old_lp=old_lp, adv=adv, ret=ret, idx=idx, ref=ref, N=N)


class DeviceNets:
    """The networks on the device: parameters as separate tensors, every gradient in one flat
    buffer (critic first, then actor, as FlatAdam), each on a 64-byte boundary."""

    def __init__(self, lib, nets, nseg):
        self.keep = []
        sizes = []
        for i in (1, 0):
            net = nets[i]
            for l in range(4):
                sizes += [(i, "dW", l, net["W"][l].shape), (i, "db", l, net["b"][l].shape)]
            for l in range(3):
                sizes += [(i, "dgamma", l, net["gamma"][l].shape), (i, "dbeta", l, net["beta"][l].shape)]
            if i == 0:
                sizes.append((0, "dlog_std", 0, net["log_std"].shape))
        off, self.slots, critic_end = 0, {}, 0
        for i, kind, l, shape in sizes:
            n = int(np.prod(shape))
            self.slots[(i, kind, l)] = (off, n, tuple(shape))
            off += -(-n // 16) * 16
            if i == 1:
                critic_end = off
        self.flat = torch.full((off,), float("nan"), dtype=torch.float32, device="cuda:0")
        for o, n, _ in self.slots.values():  # (the alignment padding stays out of every sum)
            self.flat[o + n:o + -(-n // 16) * 16] = 0
        self.seg_end = [off] if nseg == 1 else [critic_end, off]
        self.c = (lib.PrlNet * 2)()
        for i, net in enumerate(nets):
            self.c[i].nlayers, self.c[i].head = 4, i
            for l in range(4):
                L = self.c[i].layer[l]
                L.out, L.in_ = net["W"][l].shape
                L.W, L.b = self._p(net["W"][l]), self._p(net["b"][l])
                L.dW, L.db = self._g(i, "dW", l), self._g(i, "db", l)
                if l < 3:
                    L.gamma, L.beta = self._p(net["gamma"][l]), self._p(net["beta"][l])
                    L.dgamma, L.dbeta = self._g(i, "dgamma", l), self._g(i, "dbeta", l)
                    L.dropout = float(net["p"][l])
        self.c[0].log_std = self._p(nets[0]["log_std"])
        self.c[0].dlog_std = self._g(0, "dlog_std", 0)

    def _p(self, x):
        t = dev(x)
        self.keep.append(t)
        return ptr(t)

    def _g(self, i, kind, l):
        o = self.slots[(i, kind, l)][0]
        assert o % 16 == 0
        return self.flat.data_ptr() + 4 * o

    def grad(self, i, kind, l=0):
        o, n, shape = self.slots[(i, kind, l)]
        return self.flat[o:o + n].reshape(shape)


def run_mlp(R, lib, name, split):
    c = mlp_case(name)
    cfg, nets = c["cfg"], c["nets"]
    sdim, A, B = cfg["sdim"], cfg["A"], cfg["B"]
    mode, nseg = cfg.get("mode", "direct"), cfg.get("nseg", 2)
    D = DeviceNets(lib, nets, nseg)
    S, act, old_lp, adv, ret = (dev(c[k]) for k in ("S", "act", "old_lp", "adv", "ret"))
    idx = dev(c["idx"], torch.int64) if c["idx"] is not None else None
    step = dev(np.array([MLP_STEP0], np.int64), torch.int64)
    log_row = empty(6)
    nwork = R.prl_mlp_step_work(D.c, sdim, B)
    assert nwork > 0, R.prl_last_error()
    work = torch.zeros(nwork, dtype=torch.float32, device="cuda:0")
    guard = None if cfg.get("noguard") else torch.zeros(1, dtype=torch.int32, device="cuda:0")
    if split:  # the host takes the split kernel only if all of this holds; else the test would not reach it
        groups = 2 * -(-B // 16)
        assert torch.cuda.get_device_properties(0).multi_processor_count >= 4 * groups
        exchange = groups * 6 * 4 * 16 * 64 * 2  # granules [groups][6 exchanges][4 members][16][64], 2 floats each
        assert nwork >= exchange + groups + 1, "no exchange region in the work space: not a split shape"
        assert all(w in (128, 256) for w in cfg["h"]) and 32 <= sdim <= 384 and B <= 256
    head = (D.c, ptr(S), sdim, ptr(act), A, ptr(old_lp), ptr(adv), ptr(ret))
    tail = (CLIP, ENT_COEF, LN_EPS, MLP_SEED, ptr(step), ptr(log_row), ptr(work), work.numel())
    adam_step = npart = None
    if mode == "direct":
        rc = R.prl_mlp_step(*head, B, *tail, ptr(guard), None)
    elif mode == "idx":
        rc = R.prl_mlp_step_idx(*head, ptr(idx), B, *tail, ptr(guard), None)
    else:
        nparts = R.prl_mlp_step_norm_parts(D.c, sdim, B)
        assert nparts > 0
        npart = torch.zeros(nparts, 4, dtype=torch.float64, device="cuda:0")
        adam_step = dev(np.full(nseg, 4.0))
        seg = (C.c_int64 * nseg)(*D.seg_end)
        norm_tail = (ptr(D.flat), seg, nseg, ptr(adam_step), ptr(npart), nparts)
        rc = R.prl_mlp_step_idx_norm(*head, ptr(idx), B, *tail, *norm_tail, ptr(guard), None)
    lib.check_rl(rc)
    torch.cuda.synchronize()
    if guard is None:  # the split kernel's error word: the guard, or without one the work space's last word
        assert int(work[-1:].view(torch.int32).item()) == 0
    else:
        assert int(guard.item()) == 0
    assert int(step.item()) == MLP_STEP0 + (0 if mode == "direct" else 1)  # advanced once with idx
    r64, r32 = c["ref"][F64], c["ref"][F32]
    # the six logged means entry by entry, each against the mean magnitude of the terms it averages
    # (a mean of signed rows can cancel; its rounding error is bounded relative to that scale)
    check(name, "log_row", log_row, r64["log"], [r["log"] for r in r32], CAP_LOG, r64["log_scale"])
    for i, net in enumerate(("actor", "critic")):
        for kind, count in (("dW", 4), ("db", 4), ("dgamma", 3), ("dbeta", 3)):
            for l in range(count):
                check(name, f"{net}.{kind}{l}", D.grad(i, kind, l), r64["grads"][i][kind][l],
                      [r["grads"][i][kind][l] for r in r32])
    check(name, "actor.dlog_std", D.grad(0, "dlog_std"), r64["grads"][0]["dlog_std"],
          [r["grads"][0]["dlog_std"] for r in r32])
    if cfg["A"] >= 3:
        assert float(D.grad(0, "dlog_std")[1]) == 0.0  # the clamped column
    if mode == "norm":
        assert adam_step.cpu().tolist() == [5.0] * nseg
        flat = D.flat.cpu().numpy().astype(np.float64)
        assert np.isfinite(flat).all()  # every gradient slot was written
        want = [(flat[lo:hi] ** 2).sum() for lo, hi in zip([0] + D.seg_end[:-1], D.seg_end)]
        np.testing.assert_allclose(npart.cpu().numpy().sum(0)[:nseg], want, rtol=1e-12)
        # a non-zero guard: the Adam step counts stay
        guard.fill_(2)
        lib.check_rl(R.prl_mlp_step_idx_norm(*head, ptr(idx), B, *tail, *norm_tail, ptr(guard), None))
        torch.cuda.synchronize()
        assert adam_step.cpu().tolist() == [5.0] * nseg


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_step_matches_fp64(R, lib, monkeypatch, name):
    """The one-workgroup-per-tile rows kernel + the gradient kernel against the float64 step:
    hidden widths below 256 (idle waves of gemm_xwt / gemm_dzw, row sums with N < 256), state
    widths below and off 16 (the clamped k-tail), output widths 1 .. 64, B < 16, and the critic's
    (and one actor layer's) gradients under dropout with the Python keep masks."""
    monkeypatch.setenv("PIANORL_MLP_SPLIT", "0")
    run_mlp(R, lib, name, split=False)


@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_mlp_split_step_matches_fp64(R, lib, monkeypatch, name):
    """The column-split rows kernel against the same float64 step; its error word stays 0.

    Regression: the three cases without idx call prl_mlp_step, which the agent never does at
    these shapes (it always passes idx). There the host hands the kernel no copy buffer for the
    gathered state rows (Sg = NULL), and mlp_split_kernel stored the rows through it all the
    same: "split-s32-B1" (hidden 128/128/128, state width 32, A = 45, B = 1) ended in an
    illegal memory access. The store is now under ``a.Sg`` as in mlp_rows_kernel."""
    monkeypatch.delenv("PIANORL_MLP_SPLIT", raising=False)
    run_mlp(R, lib, name, split=True)


def test_mlp_step_widest_state_is_400(R, lib, monkeypatch):
    """16 KS + 31824 floats of LDS <= 150 KB with KS = roundup16(sdim) + 4: sdim <= 400 (run by
    the "widest-nseg1" case); 401 is refused before any launch."""
    monkeypatch.setenv("PIANORL_MLP_SPLIT", "0")
    rng = np.random.RandomState(0)
    B, A, sdim = 4, 23, 401
    nets = []
    for out in (A, 1):
        w = [sdim, 16, 16, 16, out]
        nets.append(dict(W=[rng.randn(w[l + 1], w[l]).astype(np.float32) for l in range(4)],
                         b=[np.zeros(w[l + 1], np.float32) for l in range(4)],
                         gamma=[np.ones(16, np.float32)] * 3, beta=[np.zeros(16, np.float32)] * 3, p=[0.0] * 3,
                         log_std=np.zeros(A, np.float32)))
    D = DeviceNets(lib, nets, 2)
    nwork = R.prl_mlp_step_work(D.c, sdim, B)
    work = torch.zeros(nwork, dtype=torch.float32, device="cuda:0")
    S, act, v = dev(np.zeros((B, sdim))), dev(np.zeros((B, A))), dev(np.zeros(B))
    step, log_row = dev(np.zeros(1), torch.int64), empty(6)
    rc = R.prl_mlp_step(D.c, ptr(S), sdim, ptr(act), A, ptr(v), ptr(v), ptr(v), B, CLIP, ENT_COEF, LN_EPS, 1, ptr(step),
                        ptr(log_row), ptr(work), work.numel(), None, None)
    assert rc < 0 and b"too wide" in R.prl_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(log_row).all()) and bool((work == 0).all())


def test_mlp_step_refuses_misaligned_work_at_split_shapes(R, lib, monkeypatch):
    """The exchange granules need a 16-byte aligned work space (include/pianorl.h): checked by the
    host before any launch, whichever rows kernel it would go on to choose."""
    monkeypatch.delenv("PIANORL_MLP_SPLIT", raising=False)
    c = mlp_case("split-s32-B1")
    cfg = c["cfg"]
    D = DeviceNets(lib, c["nets"], 2)
    nwork = R.prl_mlp_step_work(D.c, cfg["sdim"], cfg["B"])
    work = torch.zeros(nwork + 4, dtype=torch.float32, device="cuda:0")
    S, act, old_lp, adv, ret = (dev(c[k]) for k in ("S", "act", "old_lp", "adv", "ret"))
    step, log_row = dev(np.zeros(1), torch.int64), empty(6)
    rc = R.prl_mlp_step(D.c, ptr(S), cfg["sdim"], ptr(act), cfg["A"], ptr(old_lp), ptr(adv), ptr(ret), cfg["B"], CLIP,
                        ENT_COEF, LN_EPS, 1, ptr(step), ptr(log_row), work.data_ptr() + 4, nwork, None, None)
    assert rc < 0 and b"16-byte aligned" in R.prl_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(log_row).all()) and bool((work == 0).all())
