"""CPU restatement of the PPO statistics of ppo_v2.py (TEST INFRASTRUCTURE ONLY).

Checker for libpianorl.so (include/pianorl.h): imported by tests/ only, never by the
product package. Plain numpy loops in fp64, following the reference line by line:

* running_norm  <- RunningMeanStd.__call__          ppo_v2.py:107-131
* gae           <- PPOAgent.update, returns + GAE   ppo_v2.py:234-253
* normalize     <- advantage normalisation          ppo_v2.py:256
* gauss_logp    <- Actor.forward + Normal.log_prob  ppo_v2.py:70-74, 216
* philox4x32_10, dropout_keep, gauss_noise, lnrelu(_bwd), actor_head, critic_head, colsums,
  clip_adam, mlp_step <- the minibatch step (ppo_v2.py:266-293) and the draws of pianorl.hip,
  in torch on the CPU (float64 the reference, float32 the rounding floor; autograd backward)

Pinned by tests/golden/ppo_v2.npz, produced by running the reference's own PPOAgent
(tests/golden/make_ppo_golden.py): the GAE advantages / TD returns it built and the
RunningMeanStd statistics after two update() calls.
"""

from __future__ import annotations

import numpy as np


def running_norm(stats, x):
    """stats = (mean, var, count) -> (new_stats, normalised x). ppo_v2.py:113-131."""
    mean, var, count = stats
    x = np.asarray(x, np.float64)
    batch_mean = np.mean(x, axis=0)
    batch_var = np.var(x, axis=0)
    batch_count = x.shape[0]
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m_a = var * count
    m_b = batch_var * batch_count
    M2 = m_a + m_b + np.square(delta) * count * batch_count / tot_count
    new_var = M2 / tot_count
    return (new_mean, new_var, tot_count), (x - new_mean) / np.sqrt(new_var + 1e-8)


def gae(rewards, values, next_values, dones, gamma=0.99, lam=0.95, returns_mode=0):
    """Arrays [T, E] (or [T]): the reference's recursion over axis 0 (ppo_v2.py:245-253).
    returns_mode 0: TD returns r + gamma * next_values * (1 - d) (:234-237); 1: adv + values."""
    r = np.asarray(rewards, np.float64)
    squeeze = r.ndim == 1
    r = r.reshape(r.shape[0], -1)
    v = np.asarray(values, np.float64).reshape(r.shape)
    nv = np.asarray(next_values, np.float64).reshape(r.shape)
    d = np.asarray(dones, np.float64).reshape(r.shape)
    T = r.shape[0]
    adv = np.zeros_like(r)
    g = np.zeros(r.shape[1])
    for t in reversed(range(T)):
        next_value = nv[t] if t == T - 1 else v[t + 1]
        delta = r[t] + gamma * next_value * (1 - d[t]) - v[t]
        g = delta + gamma * lam * (1 - d[t]) * g
        adv[t] = g
    ret = r + gamma * nv * (1 - d) if returns_mode == 0 else adv + v
    if squeeze:
        return adv[:, 0], ret[:, 0]
    return adv, ret


def normalize(x, eps=1e-8):
    """(x - mean) / (std + eps) with torch.std's unbiased estimator (ppo_v2.py:256)."""
    x = np.asarray(x, np.float64)
    return (x - x.mean()) / (x.std(ddof=1) + eps)


def gauss_logp(mean, log_std, action):
    """Normal(mean, exp(clamp(log_std, -20, 2))).log_prob(action).sum(1) (ppo_v2.py:70-74, 216)."""
    mean = np.asarray(mean, np.float64)
    ls = np.clip(np.asarray(log_std, np.float64), -20, 2)
    sd = np.exp(ls)
    a = np.asarray(action, np.float64)
    return (-((a - mean) ** 2) / (2 * sd * sd) - np.log(sd) - 0.5 * np.log(2 * np.pi)).sum(-1)


# ---------------------------------------------------------------------------------------------
# The minibatch step's kernels restated (tests/test_rl_ref.py pins these on the CPU,
# tests/test_gpu_ppo_kernels.py holds libpianorl.so to them). torch on the CPU with a dtype
# argument: float64 is the reference, float32 the rounding floor of the same expressions.
# Every backward is autograd's, so the kernels' hand-written backward is compared with
# something that does not share its derivation.

_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x).astype(np.uint64) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) vectorised over numpy arrays of 32-bit words (any
    broadcastable shapes; scalars allowed). Returns four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # both factors < 2^32: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def dropout_keep(seed, step, layer, B, H, p):
    """keep_elem of csrc/pianorl.hip over rows 0..B-1, columns 0..H-1 -> bool [B, H]: counter
    (col, row, lo32(step) ^ (layer << 24), hi32(step)), key (lo32(seed), hi32(seed)); keep iff
    float32(c0) * float32(2.3283064e-10) >= p, evaluated in float32."""
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    col = np.arange(H, dtype=np.uint64)[None, :]
    row = np.arange(B, dtype=np.uint64)[:, None]
    c0 = philox4x32_10(col, row, (step & 0xFFFFFFFF) ^ ((int(layer) << 24) & 0xFFFFFFFF), step >> 32,
                       seed & 0xFFFFFFFF, seed >> 32)[0]
    return c0.astype(np.float32) * np.float32(2.3283064e-10) >= np.float32(p)


def gauss_noise(seed, offset, n, a, dtype=np.float64):
    """The standard-normal draw z [n, a] of gauss_sample_kernel: counter (column, row,
    lo32(offset), hi32(offset)), key (lo32(seed), hi32(seed)); u1 = (c0 + 1) 2^-32 in (0, 1],
    u2 = c1 2^-32, z = sqrt(-2 ln u1) cos(2 pi u2). float64 from the same two words is the
    reference; dtype=np.float32 rounds as the kernel does (the words to float32 first)."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    col = np.arange(a, dtype=np.uint64)[None, :]
    row = np.arange(n, dtype=np.uint64)[:, None]
    c = philox4x32_10(col, row, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    f = np.dtype(dtype).type
    u1 = (c[0].astype(dtype) + f(1)) * f(2.0 ** -32)
    u2 = c[1].astype(dtype) * f(2.0 ** -32)
    return np.sqrt(f(-2) * np.log(u1)) * np.cos(f(2 * np.pi) * u2)


def _t(x, dtype):
    import torch
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", dtype).clone()
    return torch.as_tensor(np.asarray(x)).to(dtype).clone()


def lnrelu(z, bias, gamma, beta, eps, keep=None, p=0.0, dtype=None):
    """Y = Dropout_p(LayerNorm(ReLU(z + bias))) by rows, biased variance, with the given keep
    mask (bool [B, H]; None = all kept) -> (Y, xhat, rstd). The inputs are used as they are when
    they are tensors of ``dtype`` (autograd flows through them)."""
    import torch
    dtype = dtype or torch.float64
    z, bias, gamma, beta = (x if isinstance(x, torch.Tensor) and x.dtype == dtype else _t(x, dtype)
                            for x in (z, bias, gamma, beta))
    x = torch.relu(z + bias)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd
    y = xhat * gamma + beta
    if p > 0.0:
        y = y * _t(keep, dtype) / (1.0 - p)
    return y, xhat, rstd.squeeze(-1)


def lnrelu_bwd(z, bias, gamma, beta, eps, keep, p, dY, dtype=None):
    """-> (dZ by autograd of sum(Y * dY), dye = dY * keep / (1 - p), dyx = dye * xhat)."""
    import torch
    dtype = dtype or torch.float64
    z = _t(z, dtype).requires_grad_(True)
    dY = _t(dY, dtype)
    y, xhat, _ = lnrelu(z, _t(bias, dtype), _t(gamma, dtype), _t(beta, dtype), eps, keep, p, dtype)
    (y * dY).sum().backward()
    dye = dY * _t(keep, dtype) / (1.0 - p) if p > 0.0 else dY
    return z.grad, dye, dye * xhat.detach()


_HALF_LOG_2PI = 0.5 * float(np.log(2 * np.pi))


def _actor_rows(mean, ls_rows, act, old_lp, adv, clip, ent_coef):
    """Loss rows -min(surr1, surr2) - ent_coef * entropy, entropy rows and the importance ratio
    from the tanh mean [B, A] and per-row copies of log_std [B, A] (ppo_v2.py:70-74, 272-279)."""
    import torch
    ls = torch.clamp(ls_rows, -20, 2)
    var = torch.exp(ls) ** 2
    lp = (-((act - mean) ** 2) / (2 * var) - ls - _HALF_LOG_2PI).sum(1)
    ent = (0.5 + _HALF_LOG_2PI + ls).mean(1)
    ratio = torch.exp(lp - old_lp)
    s1 = ratio * adv
    s2 = torch.clamp(ratio, 1 - clip, 1 + clip) * adv
    return -torch.min(s1, s2) - ent_coef * ent, ent, ratio, lp


def actor_log_prob(Z, bias, log_std, act, dtype=None):
    """Normal(tanh(Z + bias), exp(clamp(log_std))).log_prob(act).sum(1) (to build old_lp from)."""
    import torch
    dtype = dtype or torch.float64
    Z, bias, log_std, act = (_t(x, dtype) for x in (Z, bias, log_std, act))
    z = torch.zeros(Z.shape[0], dtype=dtype)
    return _actor_rows(torch.tanh(Z + bias), log_std.expand(Z.shape).clone(), act, z, z, 0.2, 0.0)[3]


def actor_head(Z, bias, log_std, act, old_lp, adv, clip, ent_coef, dtype=None):
    """prl_actor_head: -> dict(rows, ent_rows, ratio, dZ, dls). dZ and the per-row log_std terms
    dls [B, A] are autograd's for rows.mean() (log_std enters as a [B, A] broadcast copy, so
    dls.sum(0) is log_std.grad)."""
    import torch
    dtype = dtype or torch.float64
    Z, bias, log_std, act, old_lp, adv = (_t(x, dtype) for x in (Z, bias, log_std, act, old_lp, adv))
    Z.requires_grad_(True)
    ls_rows = log_std.expand(Z.shape).clone().requires_grad_(True)
    rows, ent, ratio, _ = _actor_rows(torch.tanh(Z + bias), ls_rows, act, old_lp, adv, clip, ent_coef)
    rows.mean().backward()
    return dict(rows=rows.detach(), ent_rows=ent.detach(), ratio=ratio.detach(), dZ=Z.grad, dls=ls_rows.grad)


def critic_head(Z, bias, ret, dtype=None):
    """prl_critic_head: v = Z + bias, (v - ret)^2, dZ = d mean((v - ret)^2) / dZ (autograd)."""
    import torch
    dtype = dtype or torch.float64
    Z, bias, ret = (_t(x, dtype) for x in (Z, bias, ret))
    Z.requires_grad_(True)
    v = Z + bias
    sq = (v - ret) ** 2
    sq.mean().backward()
    return dict(v=v.detach(), sq=sq.detach(), dZ=Z.grad)


def colsums(x, scale=1.0, dtype=None):
    import torch
    return _t(x, dtype or torch.float64).sum(0) * scale


def clip_adam(param, grad, m, v, seg_end, lr, step, betas=(0.9, 0.999), eps=1e-5, max_norm=0.5, dtype=np.float64,
              sumsq=None):
    """clip_grad_norm_(max_norm) + torch.optim.Adam.step per segment [seg_end[s-1], seg_end[s]) of
    flat buffers, in float64 (dtype=np.float32: the same expressions rounded to float32, the
    rounding floor) -> (param, m, v, step, norms). sumsq: the segments' sums of squared gradients
    given instead of computed (prl_clip_adam_parts). coef = min(1, max_norm / (norm +
    1e-6)) (max_norm <= 0: no clipping); step incremented before the bias corrections;
    m.lerp(g, 1 - b1); v = b2 v + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)."""
    f = np.dtype(dtype).type
    p, g, m, v = (np.array(x, dtype=dtype) for x in (param, grad, m, v))
    step = np.array(step, dtype=np.float64) + 1.0
    b1, b2, eps = (f(np.float32(x)) for x in (*betas, eps))  # the C-ABI takes them as float
    norms = []
    lo = 0
    for s, hi in enumerate(int(e) for e in seg_end):
        gs = g[lo:hi]
        norm = f(np.sqrt((gs * gs).sum() if sumsq is None else sumsq[s]))
        norms.append(float(norm))
        coef = min(f(1), f(np.float32(max_norm)) / (norm + f(1e-6))) if max_norm > 0 else f(1)
        gs = gs * coef
        m[lo:hi] = m[lo:hi] + (f(1) - b1) * (gs - m[lo:hi])
        v[lo:hi] = b2 * v[lo:hi] + (f(1) - b2) * gs * gs
        bc1, bc2 = 1 - float(b1) ** step[s], 1 - float(b2) ** step[s]
        p[lo:hi] -= f(float(np.float32(lr[s])) / bc1) * m[lo:hi] / (np.sqrt(v[lo:hi]) / f(np.sqrt(bc2)) + eps)
        lo = hi
    return p, m, v, step, np.array(norms)


LOG_KEYS = ("actor_loss", "critic_loss", "entropy", "value_predictions", "returns", "advantages")


def mlp_step(nets, S, A, old_lp, adv, ret, idx=None, clip=0.2, ent_coef=0.01, ln_eps=1e-5, keeps=None, dtype=None):
    """One PPO minibatch step (ppo_v2.py:266-293, as PPOAgent._forward_backward's non-fused branch
    states it) for arbitrary layer widths and per-layer dropout on either network.

    nets = (actor, critic), each a dict: W [4 arrays [out, in]], b [4], gamma [3], beta [3],
    p [3 floats] and (actor) log_std. keeps[net][layer] = bool [B, out] keep mask (needed where
    p > 0). idx selects the minibatch rows of S / A / old_lp / adv / ret (None: all rows).
    Returns dict(log = the six logged means (LOG_KEYS), grads = per network dict(dW [4], db [4],
    dgamma [3], dbeta [3], dlog_std), preact = per network the 3 hidden pre-activations z + b,
    ratio, lp = the new log-probs, log_scale = per logged mean the mean magnitude of its terms)."""
    import torch
    dtype = dtype or torch.float64
    S, A, old_lp, adv, ret = (_t(x, dtype) for x in (S, A, old_lp, adv, ret))
    if idx is not None:
        ix = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
        S, A, old_lp, adv, ret = (x.index_select(0, ix) for x in (S, A, old_lp, adv, ret))
    leaves, outs, preact = [], [], []
    for i, net in enumerate(nets):
        P = dict(W=[_t(w, dtype).requires_grad_(True) for w in net["W"]],
                 b=[_t(w, dtype).requires_grad_(True) for w in net["b"]],
                 gamma=[_t(w, dtype).requires_grad_(True) for w in net["gamma"]],
                 beta=[_t(w, dtype).requires_grad_(True) for w in net["beta"]])
        x, pre = S, []
        for l in range(3):
            z = x @ P["W"][l].t()
            pre.append((z + P["b"][l]).detach())
            p = float(net["p"][l])
            x, _, _ = lnrelu(z, P["b"][l], P["gamma"][l], P["beta"][l], ln_eps,
                             keeps[i][l] if p > 0.0 else None, p, dtype)
        outs.append(x @ P["W"][3].t() + P["b"][3])
        leaves.append(P)
        preact.append(pre)
    log_std = _t(nets[0]["log_std"], dtype).requires_grad_(True)
    rows, ent, ratio, lp = _actor_rows(torch.tanh(outs[0]), log_std.expand(outs[0].shape), A, old_lp, adv, clip,
                                       ent_coef)
    actor_loss = rows.mean()
    value = outs[1].squeeze(-1)
    critic_loss = ((value - ret) ** 2).mean()
    critic_loss.backward()
    actor_loss.backward()
    grads = []
    for P in leaves:
        grads.append(dict(dW=[w.grad for w in P["W"]], db=[w.grad for w in P["b"]],
                          dgamma=[w.grad for w in P["gamma"]], dbeta=[w.grad for w in P["beta"]]))
    grads[0]["dlog_std"] = log_std.grad
    log = torch.stack([actor_loss, critic_loss, ent.mean(), value.mean(), ret.mean(), adv.mean()]).detach()
    # each logged mean's own scale: the mean magnitude of the terms it averages
    log_scale = torch.stack([rows.abs().mean(), ((value - ret) ** 2).mean(), ent.abs().mean(), value.abs().mean(),
                             ret.abs().mean(), adv.abs().mean()]).detach()
    return dict(log=log, log_scale=log_scale, grads=grads, preact=preact, ratio=ratio.detach(), lp=lp.detach())
