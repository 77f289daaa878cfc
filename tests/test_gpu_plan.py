"""The predictive-sampling planner (planning.PredictiveSampler) on the simulator: a plan leaves the
env where it was, the winner's return is what the env really pays for its actions, the step after
the plan is the rollout's first step (the model is the world), the plans are deterministic in the
seed, and episode ends inside a horizon are survived. Twinkle, G = 2 groups of C = 5, H = 3 steps,
P = 2 knots, both interpolations."""
import numpy as np
import pytest

import plan_ref
from helpers import song
from test_gpu_snapshot import assert_env_equal, record, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G, C, H, P = 2, 5, 3, 2
N = G * C
U = 2.0 ** -24
MODES = {"zero": plan_ref.ZERO, "linear": plan_ref.LINEAR}


def make(dp, name="twinkle", seed=0, **task):
    env = dp.BatchedPianoEnv(N, song(dp, name), dp.TaskConfig(**task), device="cuda:0", seed=seed)
    env.reset()
    return env


def sampler(dp, env, mode, seed=0):
    return dp.PredictiveSampler(env, groups=G, horizon=H, knots=P, sigma=0.3, interpolation=mode, seed=seed)


def warm(env, steps=2):
    """a few random steps, every follower stepping with its leader's action: the groups are copies"""
    rng = np.random.RandomState(4)
    for _ in range(steps):
        a = rng.uniform(-1, 1, (G, env.action_dim)).astype(np.float32)
        env.step(torch.as_tensor(np.repeat(a, C, axis=0)).cuda())


@pytest.mark.parametrize("mode", list(MODES))
def test_plan_leaves_the_env_as_it_was_and_its_return_is_real(dp, mode):
    env = make(dp)
    warm(env)
    ps = sampler(dp, env, mode)
    before = record(env, False)
    snap = env.snapshot()
    chosen = ps.plan().cpu().numpy()
    after = record(env, False)
    for e in range(N):
        assert_env_equal(after, before, e, e, "after plan()")
    best, best_ret = ps.best.cpu().numpy(), ps.best_ret.cpu().numpy()
    ret, knots = ps.ret.cpu().numpy(), ps.plan_knots.cpu().numpy()
    assert (best >= 0).all() and (best < C).all()
    win = knots.reshape(G, C, P, -1)[np.arange(G), best]
    assert same(chosen, win[:, 0])
    assert same(best_ret, ret.reshape(G, C)[np.arange(G), best])
    assert (best_ret >= ret.reshape(G, C)[:, 0]).all()  # candidate 0 rolls out the nominal plan
    assert (np.abs(knots) <= 1).all() and len({knots[n].tobytes() for n in range(N)}) == N - G + 1
    # the winner's actions, stepped from the pre-plan state: the rewards the planner summed
    env.restore(snap)
    rs, ds, sts = [], [], []
    for h in range(H):
        a = plan_ref.action(win, H, h, MODES[mode]).astype(np.float32)
        r, d, st = env.step(torch.as_tensor(np.repeat(a, C, axis=0)).cuda())[1:]
        rs.append(r.cpu().numpy()[::C]), ds.append(d.cpu().numpy()[::C]), sts.append(st.cpu().numpy()[::C])
    want, mag, _ = plan_ref.accumulate(np.stack(rs), np.stack(ds), np.stack(sts), 1.0)
    err = np.abs(best_ret.astype(np.float64) - want)
    print(f"\nplan {mode}: best {best} best_ret {best_ret} stepped {want} err {err} bound {H * U * mag}", end="")
    assert (err <= H * U * mag).all()
    ps.close(), snap.close(), env.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_act_steps_the_rollouts_first_step(dp, mode):
    env = make(dp)
    warm(env)
    ps = sampler(dp, env, mode)
    seen, step = [], env.step

    def spy(action):
        out = step(action)
        seen.append(out[1].clone())
        return out

    env.step = spy
    obs, reward, discount, step_type = ps.act()
    assert len(seen) == H + 1  # the horizon's steps, then the real one
    best = ps.best.cpu().numpy()
    first = seen[0].cpu().numpy().reshape(G, C)[np.arange(G), best]
    assert same(reward.cpu().numpy(), first)
    assert same(obs.cpu().numpy(), env.obs.cpu().numpy()[::C])
    state = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    for k, v in state.items():
        for e in range(N):
            assert same(v[e], v[e // C * C]), f"{k}: follower {e} is not its leader's copy"
    ps.close(), env.close()


def test_plans_are_deterministic_in_the_seed(dp):
    runs = {}
    for name, seed in (("a", 3), ("b", 3), ("c", 4)):
        env = make(dp)
        ps = sampler(dp, env, "linear", seed=seed)
        acts = []
        for _ in range(5):
            ps.act()
            acts.append(ps.chosen.cpu().numpy().copy())
        assert ps.counter == 5
        runs[name] = np.stack(acts)
        ps.close(), env.close()
    assert same(runs["a"], runs["b"])
    assert not same(runs["a"][0], runs["c"][0])
    assert not same(runs["a"][0], runs["a"][1])  # the plan counter moves the draws on


@pytest.mark.parametrize("randomize", [False, True])
def test_episode_ends_inside_the_horizon(dp, randomize):
    env = make(dp, "test_task", seed=9, randomize_hand_positions=randomize)
    ps = sampler(dp, env, "zero")
    lasts = distinct = 0
    for _ in range(7):  # T = 4: every horizon of 3 steps crosses an episode end sooner or later
        step_type = ps.act()[3]
        lasts += int((step_type == 2).sum())
        assert torch.isfinite(ps.ret).all() and torch.isfinite(env.obs).all()
        distinct = max(distinct, len(set(env.hand_offset()[0].cpu().numpy().tolist())))
    assert lasts >= G
    if randomize:  # the followers reset with their own draws ...
        assert distinct > G
    ps.plan()      # ... and are their leaders' copies again after the next plan
    now = record(env, False)
    for e in range(N):
        assert_env_equal(now, now, e, e // C * C, "after plan()")
    ps.close(), env.close()
