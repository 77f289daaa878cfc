"""Predictive-sampling MPC on the batched simulator (the RoboPianist paper's non-learning
baseline): fork the current state into C candidates, roll each out H control steps under a
perturbed action spline, keep the best.

The env's N envs are G groups of C = N / G: group g owns envs [g C, (g + 1) C) and env g C is
its leader - the real env; the others are its scratch copies. One ``plan()`` is

    snapshot.save -> restore(src = leader) -> prl_plan_perturb
    -> H x (prl_plan_action, env.step, prl_plan_accumulate) -> prl_plan_select
    -> restore(src = leader)

all on the current stream with no host synchronisation: the snapshot rows never leave the
device (ps_snapshot_*, include/pianosim.h) and the planner's own kernels are libpianorl.so's
prl_plan_* (include/pianorl.h). The model is the world: a candidate's rollout is bitwise the
steps the leader would take under the same actions.
"""

from __future__ import annotations

import numpy as np

from . import _lib

INTERPOLATIONS = {"zero": 0, "linear": 1}  # PRL_PLAN_ZERO / PRL_PLAN_LINEAR


def check_plan_args(num_envs: int, groups: int, horizon: int, knots: int, interpolation: str) -> int:
    """The argument checks of :class:`PredictiveSampler` (no GPU needed) -> candidates per group."""
    if groups < 1 or num_envs % groups:
        raise ValueError(f"num_envs ({num_envs}) must be a multiple of groups ({groups})")
    if horizon < 1:
        raise ValueError(f"horizon must be at least 1, got {horizon}")
    if not 1 <= knots <= horizon:
        raise ValueError(f"knots must be in 1 .. horizon ({horizon}), got {knots}")
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation is 'zero' or 'linear', not {interpolation!r}")
    return num_envs // groups


class PredictiveSampler:
    """``PredictiveSampler(env, groups, horizon, knots, sigma)``: ``plan()`` -> the chosen first
    action of every group [G, A]; ``act()`` plans, then steps every env with its group's action.

    ``sigma`` (a number or [A]) scales the standard-normal perturbation of every knot, in action
    units; candidate 0 of a group always rolls out the unperturbed nominal plan, so a plan's
    return never falls below the nominal's. Actions are clamped to the env's bounds
    (``action_lo / action_hi``, or [-1, 1] with canonical actions). The nominal plan of the next
    call is the winner's, shifted by one control step. ``gamma`` discounts the rollout's rewards
    besides the env's own discount; a candidate's return stops at its episode's LAST step. The
    draws are Philox-keyed by ``seed`` and the plan counter, which advances by one per plan."""

    def __init__(self, env, groups: int, horizon: int, knots: int, sigma, interpolation: str = "zero",
                 gamma: float = 1.0, seed: int = 0):
        self.candidates = check_plan_args(env.num_envs, groups, horizon, knots, interpolation)
        self.env, self.groups, self.horizon, self.knots = env, int(groups), int(horizon), int(knots)
        self.interpolation, self.gamma, self.seed = INTERPOLATIONS[interpolation], float(gamma), int(seed)
        self.counter = 0
        torch = env._torch
        self._R = _lib.load_rl()
        N, G, C, P, A = env.num_envs, self.groups, self.candidates, self.knots, env.action_dim
        sig = np.asarray(sigma, np.float32)
        if sig.ndim == 0:
            sig = np.full(A, sig, np.float32)
        if sig.shape != (A,) or not (sig >= 0).all():
            raise ValueError(f"sigma is a non-negative number or [{A}] vector")
        if env.canonical_actions:
            lo, hi = -np.ones(A, np.float32), np.ones(A, np.float32)
        else:
            lo, hi = np.asarray(env.action_lo, np.float32), np.asarray(env.action_hi, np.float32)
        f32 = dict(device=env.device, dtype=torch.float32)
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(**f32).contiguous()
        self.sigma, self.lo, self.hi = dev(sig), dev(lo), dev(hi)
        self.nominal = torch.zeros(G, P, A, **f32)
        self._nominal_next = torch.zeros(G, P, A, **f32)
        self.plan_knots = torch.zeros(N, P, A, **f32)
        self.action = torch.zeros(N, A, **f32)
        self.ret = torch.zeros(N, **f32)
        self.weight = torch.zeros(N, **f32)
        self.best = torch.zeros(G, device=env.device, dtype=torch.int32)
        self.best_ret = torch.zeros(G, **f32)
        self.chosen = torch.zeros(G, A, **f32)
        self.leader = (torch.arange(N, device=env.device, dtype=torch.int32) // C) * C
        self._snap = env.snapshot()

    def close(self) -> None:
        self._snap.close()

    def plan(self):
        """-> chosen [G, A] (the planner's tensor, overwritten by the next plan). The env is left
        as it was, with every follower again its leader's copy; ``best`` [G], ``best_ret`` [G],
        ``ret`` [N] and ``plan_knots`` [N, P, A] hold the plan's record."""
        env, R, ck = self.env, self._R, _lib.check_rl
        N, G, C, P, A, H = env.num_envs, self.groups, self.candidates, self.knots, env.action_dim, self.horizon
        s = env.stream
        p = lambda t: t.data_ptr()
        self._snap.save()
        env.restore(self._snap, self.leader)
        ck(R.prl_plan_perturb(p(self.nominal), p(self.sigma), p(self.lo), p(self.hi), G, C, P, A, self.seed,
                              self.counter, p(self.plan_knots), s))
        self.counter += 1
        for h in range(H):
            ck(R.prl_plan_action(p(self.plan_knots), N, P, A, H, h, self.interpolation, p(self.action), s))
            env.step(self.action)
            ck(R.prl_plan_accumulate(p(env.reward), p(env.discount), p(env.step_type), N, self.gamma, int(h == 0),
                                     p(self.ret), p(self.weight), s))
        ck(R.prl_plan_select(p(self.ret), p(self.plan_knots), G, C, P, A, H, self.interpolation, 1, p(self.best),
                             p(self.best_ret), p(self._nominal_next), p(self.chosen), s))
        self.nominal, self._nominal_next = self._nominal_next, self.nominal
        env.restore(self._snap, self.leader)
        return self.chosen

    def act(self):
        """``plan()``, then one step of all N envs, each with its group's chosen action -> the
        leaders' (obs [G, .], reward [G], discount [G], step_type [G])."""
        chosen = self.plan()
        C = self.candidates
        obs, reward, discount, step_type = self.env.step(chosen.repeat_interleave(C, dim=0))
        return obs[::C], reward[::C], discount[::C], step_type[::C]
