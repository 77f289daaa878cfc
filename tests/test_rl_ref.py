"""CPU pins of the minibatch-step restatement in oracle/rl_ref.py (no GPU): the reference that
tests/test_gpu_ppo_kernels.py holds libpianorl.so to is itself held to torch's own modules,
autograd, clip_grad_norm_ and Adam in float64, and its Philox to the package's scalar one.
"""
import importlib
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import rl_ref  # noqa: E402  (oracle/, on the path through conftest.py)


def rel(x, ref):
    x, ref = (torch.as_tensor(v, dtype=torch.float64) for v in (x, ref))
    return float((x - ref).abs().max() / ref.abs().max())


def test_philox_matches_scalar_philox():
    var = importlib.import_module("diffusion-piano_amd.variations")
    rng = np.random.RandomState(11)
    w = rng.randint(0, 2**32, size=(300, 6), dtype=np.uint64)
    w[0] = 0
    w[1] = 0xFFFFFFFF
    got = np.stack(rl_ref.philox4x32_10(*(w[:, j] for j in range(6))), axis=1)
    assert got.dtype == np.uint32
    for r in range(w.shape[0]):
        want = var.philox4x32_10(tuple(int(x) for x in w[r, :4]), int(w[r, 4]), int(w[r, 5]))
        assert tuple(int(x) for x in got[r]) == want, r
    # the known-answer vectors of Random123 (kat_vectors: philox4x32 10)
    z = rl_ref.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = rl_ref.philox4x32_10(*[0xFFFFFFFF] * 6)
    assert [int(x) for x in f] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_dropout_keep_and_gauss_noise_key_words():
    """The counter / key words of the two draws, stated once more with the scalar Philox."""
    var = importlib.import_module("diffusion-piano_amd.variations")
    seed, step, layer, p = 0x123456789ABCDEF, (7 << 32) | 0xFEDCBA98, 2, 0.3
    keep = rl_ref.dropout_keep(seed, step, layer, 3, 5, p)
    for r in range(3):
        for c in range(5):
            c0 = var.philox4x32_10((c, r, (step & 0xFFFFFFFF) ^ (layer << 24), step >> 32), seed & 0xFFFFFFFF,
                                   seed >> 32)[0]
            assert bool(keep[r, c]) == bool(np.float32(c0) * np.float32(2.3283064e-10) >= np.float32(p))
    z = rl_ref.gauss_noise(seed, step, 3, 5)
    for r in range(3):
        for c in range(5):
            w = var.philox4x32_10((c, r, step & 0xFFFFFFFF, step >> 32), seed & 0xFFFFFFFF, seed >> 32)
            want = math.sqrt(-2 * math.log((w[0] + 1) / 2**32)) * math.cos(2 * math.pi * w[1] / 2**32)
            assert abs(z[r, c] - want) < 1e-12


def test_lnrelu_matches_torch_modules():
    torch.manual_seed(3)
    B, H = 7, 50
    mod = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.LayerNorm(H, eps=1e-5)).double()
    with torch.no_grad():
        mod[1].weight.uniform_(0.5, 1.5)
        mod[1].bias.uniform_(-1, 1)
    z = torch.randn(B, H, dtype=torch.float64)
    bias = torch.randn(H, dtype=torch.float64)
    dY = torch.randn(B, H, dtype=torch.float64)
    x = (z + bias).requires_grad_(True)
    want = mod(x)
    (want * dY).sum().backward()
    keep = np.ones((B, H), bool)
    y, xhat, rstd = rl_ref.lnrelu(z, bias, mod[1].weight.detach(), mod[1].bias.detach(), 1e-5, keep, 0.0)
    assert rel(y, want.detach()) < 1e-12
    dZ, dye, dyx = rl_ref.lnrelu_bwd(z, bias, mod[1].weight.detach(), mod[1].bias.detach(), 1e-5, keep, 0.0, dY)
    assert rel(dZ, x.grad) < 1e-12
    assert rel(dye.sum(0), mod[1].bias.grad) < 1e-12 and rel(dyx.sum(0), mod[1].weight.grad) < 1e-12
    # the mask and its 1 / (1 - p) scale
    keep = torch.rand(B, H) < 0.6
    y2, xhat2, _ = rl_ref.lnrelu(z, bias, mod[1].weight.detach(), mod[1].bias.detach(), 1e-5, keep.numpy(), 0.4)
    assert rel(y2, want.detach() * keep / 0.6) < 1e-12 and torch.equal(xhat2, xhat)


def _copy_net(module, log_std=None):
    lin = [m for m in module.network if isinstance(m, torch.nn.Linear)]
    ln = [m for m in module.network if isinstance(m, torch.nn.LayerNorm)]
    d = dict(W=[m.weight.detach().numpy() for m in lin], b=[m.bias.detach().numpy() for m in lin],
             gamma=[m.weight.detach().numpy() for m in ln], beta=[m.bias.detach().numpy() for m in ln], p=[0.0] * 3)
    if log_std is not None:
        d["log_std"] = log_std.detach().numpy()
    return d, lin, ln


def test_mlp_step_matches_autograd_through_the_agents_modules():
    ppo = importlib.import_module("diffusion-piano_amd.ppo")
    torch.manual_seed(5)
    sdim, adim, N, B, clip, ent_coef = 37, 23, 90, 40, 0.2, 0.01
    actor, critic = ppo.Actor(sdim, adim).double().eval(), ppo.Critic(sdim).double().eval()
    with torch.no_grad():  # away from the initial values (zero biases, unit LayerNorm, log_std -1)
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.1 * torch.randn_like(p))
        actor.log_std[0] = 2.5  # clamped: no gradient
    S = torch.randn(N, sdim, dtype=torch.float64)
    A = torch.randn(N, adim, dtype=torch.float64).clamp(-1, 1)
    with torch.no_grad():
        LP = actor(S).log_prob(A).sum(1) + 0.3 * torch.randn(N, dtype=torch.float64)
    ADV, RET = torch.randn(N, dtype=torch.float64), torch.randn(N, dtype=torch.float64)
    idx = torch.randint(0, N, (B,))
    # the agent's own loss expressions (PPOAgent._forward_backward, non-fused branch)
    b_s, b_a, b_lp, b_adv, b_ret = (x.index_select(0, idx) for x in (S, A, LP, ADV, RET))
    mean = actor.network(b_s)
    log_scale = torch.log(torch.exp(torch.clamp(actor.log_std, -20, 2)))
    var = torch.exp(torch.clamp(actor.log_std, -20, 2)) ** 2
    new_lp = (-((b_a - mean) ** 2) / (2 * var) - log_scale - ppo._LOG_SQRT_2PI).sum(1)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + log_scale).expand_as(mean).mean()
    ratio = torch.exp(new_lp - b_lp)
    surr1 = ratio * b_adv
    surr2 = torch.clamp(ratio, 1 - clip, 1 + clip) * b_adv
    actor_loss = -torch.min(surr1, surr2).mean() - ent_coef * entropy
    value_pred = critic(b_s).squeeze(-1)
    critic_loss = torch.nn.functional.mse_loss(value_pred, b_ret)
    critic_loss.backward()
    actor_loss.backward()
    want_log = torch.stack([actor_loss, critic_loss, entropy, value_pred.mean(), b_ret.mean(), b_adv.mean()]).detach()

    (na, alin, aln), (nc, clin, cln) = _copy_net(actor, actor.log_std), _copy_net(critic)
    out = rl_ref.mlp_step((na, nc), S, A, LP, ADV, RET, idx.numpy(), clip, ent_coef, 1e-5, None, torch.float64)
    assert rel(out["log"], want_log) < 1e-10
    for g, lin, ln in ((out["grads"][0], alin, aln), (out["grads"][1], clin, cln)):
        for l in range(4):
            assert rel(g["dW"][l], lin[l].weight.grad) < 1e-10 and rel(g["db"][l], lin[l].bias.grad) < 1e-10
        for l in range(3):
            assert rel(g["dgamma"][l], ln[l].weight.grad) < 1e-10 and rel(g["dbeta"][l], ln[l].bias.grad) < 1e-10
    assert rel(out["grads"][0]["dlog_std"], actor.log_std.grad) < 1e-10
    assert out["grads"][0]["dlog_std"][0] == 0 and out["grads"][0]["dlog_std"][1] != 0
    # the per-kernel restatements chain to the same numbers
    head = rl_ref.actor_head(out["preact"][0][0][:, :adim], np.zeros(adim), na["log_std"], b_a[:, :adim], b_lp, b_adv,
                             clip, ent_coef)
    assert head["dls"].shape == (B, adim) and torch.all(head["dls"][:, 0] == 0)
    z3 = torch.randn(B, dtype=torch.float64)
    ch = rl_ref.critic_head(z3, torch.tensor([0.25], dtype=torch.float64), b_ret)
    assert rel(ch["dZ"], 2 * (z3 + 0.25 - b_ret) / B) < 1e-14


def test_actor_head_matches_torch_distribution():
    torch.manual_seed(9)
    B, A = 6, 5
    Z = torch.randn(B, A, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(A, dtype=torch.float64)
    ls = torch.tensor([-0.5, 0.3, 2.5, -21.0, 1.0], dtype=torch.float64, requires_grad=True)
    act, adv = torch.randn(B, A, dtype=torch.float64), torch.randn(B, dtype=torch.float64)
    with torch.no_grad():  # sd = e^-20 on column 3: its mean and action are both exactly 0
        Z[:, 3], act[:, 3] = -bias[3], 0.0
    old = rl_ref.actor_log_prob(Z, bias, ls, act) + 0.3 * torch.randn(B, dtype=torch.float64)
    d = torch.distributions.Normal(torch.tanh(Z + bias), torch.exp(torch.clamp(ls, -20, 2)))
    ratio = torch.exp(d.log_prob(act).sum(1) - old)
    rows = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv) - 0.01 * d.entropy().mean()
    rows.mean().backward()
    h = rl_ref.actor_head(Z, bias, ls, act, old, adv, 0.2, 0.01)
    assert rel(h["rows"], rows.detach()) < 1e-12 and rel(h["dZ"], Z.grad) < 1e-12
    assert rel(h["dls"].sum(0), ls.grad) < 1e-12 and torch.all(h["dls"][:, 2:4] == 0)
    assert 0 < int(((h["ratio"] < 0.8) | (h["ratio"] > 1.2)).sum()) < B  # both sides of the clip occur
    assert rel(h["ent_rows"], d.entropy().mean().detach().expand(B)) < 1e-12
    assert rel(rl_ref.actor_log_prob(Z, bias, ls, act), d.log_prob(act).sum(1).detach()) < 1e-12


def test_clip_adam_matches_torch_clip_and_adam():
    torch.manual_seed(1)
    sizes, max_norm = (300, 170), 0.5
    lrs = tuple(float(np.float32(x)) for x in (2e-4, 1e-4))  # (the kernel reads them as float)
    params = [torch.nn.Parameter(torch.randn(n, dtype=torch.float64)) for n in sizes]
    opts = [torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-5) for p, lr in zip(params, lrs)]
    seg_end = np.cumsum(sizes)
    p = np.concatenate([q.detach().numpy() for q in params])
    m, v, step = np.zeros_like(p), np.zeros_like(p), np.zeros(2)
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-5))  # as the C-ABI receives them
    for o in opts:
        o.param_groups[0]["betas"], o.param_groups[0]["eps"] = (b1, b2), eps
    for k in range(3):
        # segment 0 clipped (norm > 0.5), segment 1 not
        grads = [torch.randn(sizes[0], dtype=torch.float64) * (1 + k), torch.randn(sizes[1], dtype=torch.float64) * 1e-3]
        for q, g, o in zip(params, grads, opts):  # each network clipped and stepped separately
            q.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([q], max_norm)
            o.step()
        g = np.concatenate([x.numpy() for x in grads])
        p, m, v, step, norms = rl_ref.clip_adam(p, g, m, v, seg_end, lrs, step, (0.9, 0.999), 1e-5, max_norm)
        assert norms[0] > max_norm > norms[1]
        assert list(step) == [k + 1, k + 1]
        want = np.concatenate([q.detach().numpy() for q in params])
        np.testing.assert_allclose(p, want, rtol=1e-12, atol=0)
        st = [o.state[q] for o, q in zip(opts, params)]
        np.testing.assert_allclose(m, np.concatenate([s["exp_avg"].numpy() for s in st]), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, np.concatenate([s["exp_avg_sq"].numpy() for s in st]), rtol=1e-12, atol=1e-300)
    # max_norm <= 0: no clipping
    p2, m2, _, _, _ = rl_ref.clip_adam(p, g, m, v, seg_end, lrs, step, (0.9, 0.999), 1e-5, 0.0)
    np.testing.assert_allclose(m2[:300], m[:300] + (1 - b1) * (g[:300] - m[:300]), rtol=1e-14)


def test_gpu_kernel_cases_keep_their_margins():
    """The inputs of tests/test_gpu_ppo_kernels.py, built here without a GPU: their builders
    assert on the float64 reference that no ReLU input and no importance ratio sits where
    rounding could decide a branch, with no row excluded."""
    k = importlib.import_module("test_gpu_ppo_kernels")
    k.test_mlp_cases_cover_every_listed_value()
    for name in k.all_cases():
        k.mlp_case(name)
    for A in (1, 23, 39, 45, 64):
        for B in (1, 4, 5, 67):
            k.actor_case(A, B)
    for H in (1, 16, 63, 64, 65, 250, 256, 1000, 1024):
        for B in (1, 3):
            for p, layer in k.LN_MODES:
                k.lnrelu_case(H, B, p, layer)
