"""The one-hand task (PianoWithOneShadowHand, TaskConfig(hand_side=...)) on the GPU: physics
parity against the fp64 checker (which steps the detached-hand model unchanged), the task layer
against numpy / fp64 restatements of piano_with_one_shadow_hand.py written here, the episode
semantics, the one-hand task's physics against the two-hand task's on the same model (bitwise),
and per-episode augmentations."""
import math

import numpy as np
import pytest

from helpers import Floor, assert_parity, song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEYS = ("qpos", "qvel", "qacc_ws", "ctrl", "sustain", "t_idx", "last")
HANDS = {"capsule": {}, "hull": dict(primitive_fingertip_collisions=False)}
SIDES = {"right": 0, "left": 1}


def both_hands_song(dp):
    """A short song with notes for fingers 0-9: steps of both hands' notes, of the right hand's
    only, of the left hand's only, mixed again, and silent ones."""
    m = dp.music
    seq = m.NoteSequence(title="both hands")
    spec = [(60, 0.0, 0.25, 0), (64, 0.0, 0.25, 2), (40, 0.0, 0.25, 5), (36, 0.0, 0.25, 9),
            (62, 0.25, 0.5, 1), (65, 0.25, 0.5, 3), (69, 0.25, 0.5, 4),
            (45, 0.5, 0.75, 6), (47, 0.5, 0.75, 7), (50, 0.5, 0.75, 8),
            (72, 0.75, 1.0, 4), (43, 0.75, 1.0, 5), (67, 0.75, 1.0, 2)]
    for p, s, e, f in spec:
        seq.notes.append(m.Note(p, s, e, 80, f))
    seq.total_time = 1.1
    return seq


def _song(dp, name):
    return both_hands_song(dp) if name == "both" else song(dp, name)


def _gs(g):
    return {k: v.cpu().numpy() for k, v in g.get_state().items()}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def assert_reward_is_sum(rew, terms):
    """reward == the sum of the stored terms, to fp32 rounding: the kernel adds the five terms in
    fp32 and may fuse the energy term's product into the sum, so it and this fp64 sum of the
    stored fp32 terms differ by at most the 4 roundings of the partial sums and the product's,
    each half an ulp of a value no larger than S = sum |terms|: 5 * 2^-24 * S."""
    t = terms.astype(np.float64)
    bound = 5.0 * 2.0 ** -24 * np.maximum(np.abs(t).sum(axis=1), 1.0)
    assert (np.abs(rew.astype(np.float64) - t.sum(axis=1)) <= bound).all(), (rew, t.sum(axis=1))


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", ["twinkle", "both"])
@pytest.mark.parametrize("hand", list(HANDS))
@pytest.mark.parametrize("side", list(SIDES))
def test_parity_teacher_forced(dp, ref, side, hand, name):
    """qpos by helpers.assert_parity; key_press, sustain and energy against the checker's within
    the two-hand term tests' bound (p99 < 1e-3). The checker has no one-hand task layer: its
    fingering / forearm slots are the two-hand task's and are not compared."""
    n, steps = 16, 20
    seq = _song(dp, name)
    task = dp.TaskConfig(hand_side=side, **HANDS[hand])
    md, st, tc = dp.compile_task(seq, task, canonical_actions=False)
    g = dp.BatchedPianoEnv(n, seq, task, device="cuda:0", canonical_actions=False)
    assert g.action_dim == 23 and g.obs_dim == 301
    o, o2 = ref.OracleEnv(md, st, tc, n), Floor(ref, md, st, tc, n)
    lo, hi = dp.model.action_spec(md)
    rng, prng = np.random.RandomState(23), np.random.RandomState(3)
    g.reset()
    o.reset()
    errs, fl, terr = [], [], []
    gone = 1 - SIDES[side]
    for _ in range(steps):
        a = rng.uniform(lo, hi, (n, 23)).astype(np.float32)
        s = {k: v for k, v in _gs(g).items() if k in KEYS}
        if s["last"].any():  # (the both-hands song is 23 steps long; twinkle 161)
            break
        o.set_state(s)
        o2.set_state(s, prng)
        g.step(_cuda(a))
        o.step(a)
        o2.step(a)
        qg = _gs(g)["qpos"]
        errs.append(np.abs(qg - o.get_state()["qpos"]).max(axis=1))
        fl.append(o2.dev(o.get_state()["qpos"]))
        terr.append(np.abs(g.reward_terms().cpu().numpy()[:, :3] - o.reward_terms()[:, :3]))
        assert np.abs(qg[:, 88 + 26 * gone:88 + 26 * gone + 26]).max() == 0.0
    assert len(errs) == steps
    assert_parity(np.concatenate(errs), np.concatenate(fl), f"one hand {side} {hand} {name}")
    t = np.concatenate(terr)
    print("terms |gpu - checker| p99", np.percentile(t, 99, axis=0), "max", t.max(axis=0))
    assert np.percentile(t, 99) < 1e-3, t.max()


# ---------------------------------------------------------------- 2. observation row
def _root_position(md, h, qpos):
    """World position of hand h's root body in fp64: its pose plus the slide axes times q."""
    quat = dp_quat_to_mat(list(md.body_quat[h][0]))
    p = np.tile(np.array(list(md.body_pos[h][0]), np.float64), (len(qpos), 1))
    for j in range(26):
        if md.dof_body[h][j] == 0 and not md.dof_locked[h][j]:
            assert md.dof_type[h][j] == 1
            p += np.outer(qpos[:, 88 + 26 * h + j].astype(np.float64), quat @ np.array(list(md.dof_axis[h][j])))
    return p


def dp_quat_to_mat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _expected_obs_head(st, L, t, side):
    """goal rows t .. t + L (zero past the end) and the kept hand's 5-wide fingering of step t."""
    goal = np.zeros((L + 1, 89), np.float32)
    for j in range(L + 1):
        if t + j < st.T:
            goal[j] = st.goal[t + j]
    fing = np.zeros(5, np.float32)
    for i in range(st.count[t]):
        f = int(st.fingers[t, i])
        if side == "right" and f < 5:
            fing[f] = 1.0  # (a negative f indexes from the end, as the reference's numpy row does)
        elif side == "left" and f >= 5:
            fing[f - 5] = 1.0
    return goal.ravel(), fing


@pytest.mark.parametrize("side", list(SIDES))
def test_observation_row(dp, side):
    n, L = 4, 2
    seq = both_hands_song(dp)
    task = dp.TaskConfig(hand_side=side, n_steps_lookahead=L)
    g = dp.BatchedPianoEnv(n, seq, task, device="cuda:0", canonical_actions=False)
    md, st, lay = g.model_desc, g.song, g.obs_slices
    h, name = SIDES[side], ("rh", "lh")[SIDES[side]] + "_shadow_hand"
    assert list(lay) == ["goal", "fingering", "piano/state", "piano/sustain_state", name + "/joints_pos",
                         name + "/position"]
    assert g.obs_dim == 3 * 89 + 5 + 88 + 1 + 26 + 3
    lo, hi = dp.model.action_spec(md)
    rng = np.random.RandomState(8)
    obs = g.reset().cpu().numpy()
    empty = 0
    for t in range(st.T):  # obs shows step t; the last step's obs is stale (t = T - 1 again)
        tt = min(t, st.T - 1)
        goal, fing = _expected_obs_head(st, L, tt, side)
        np.testing.assert_array_equal(obs[0, lay["goal"]], goal)
        for e in range(n):
            np.testing.assert_array_equal(obs[e, lay["fingering"]], fing)
        empty += st.count[tt] > 0 and not fing.any()  # notes, all of the other hand: all zeros
        s = _gs(g)
        order = [md.dof_obs_order[h][i] for i in range(26)]
        np.testing.assert_array_equal(obs[:, lay[name + "/joints_pos"]], s["qpos"][:, [88 + 26 * h + j for j in order]])
        # fp32 kinematics of a position below 1 m (ulp 6e-8), a handful of operations: 1e-6
        np.testing.assert_allclose(obs[:, lay[name + "/position"]], _root_position(md, h, s["qpos"]), rtol=0, atol=1e-6)
        if t == 0:  # at reset: the root pose itself
            np.testing.assert_allclose(obs[0, lay[name + "/position"]], list(md.body_pos[h][0]), rtol=0, atol=1e-7)
        a = rng.uniform(lo, hi, (n, 23)).astype(np.float32)
        obs = g.step(_cuda(a))[0].cpu().numpy()
    assert empty > 0
    goal, fing = _expected_obs_head(st, L, st.T - 1, side)  # after the LAST step: the stale rows of T - 1
    np.testing.assert_array_equal(obs[0, lay["goal"]], goal)
    np.testing.assert_array_equal(obs[0, lay["fingering"]], fing)
    moved =np.abs(_root_position(md, h, _gs(g)["qpos"]) - np.array(list(md.body_pos[h][0]))).max()
    assert moved > 1e-3  # the position follows the forearm slides


# ---------------------------------------------------------------- 3. fingering term
def _tolerance(x, hi, margin):
    """dm_control rewards.tolerance, bounds (0, hi), gaussian, value_at_margin 0.1, x >= 0."""
    if x <= hi:
        return 1.0
    scale = math.sqrt(-2.0 * math.log(0.1))
    return math.exp(-0.5 * ((x - hi) / margin * scale) ** 2)


def _fingering_term(md, st, t, side, tips, qkeys):
    """piano_with_one_shadow_hand.py:244-275 in fp64 for one env: the mean gaussian tolerance of
    the kept hand's fingertip-to-key distances over its fingered notes of step t; 0.0 with none."""
    h = SIDES[side]
    rews = []
    for i in range(st.count[t]):
        f, k = int(st.fingers[t, i]), int(st.keys[t, i])
        if (f < 5) != (side == "right"):
            continue
        finger = (f + 5 if f < 0 else f) if f < 5 else f - 5
        half, pos, anc = (np.array(list(x[k]), np.float64) for x in (md.key_half, md.key_pos, md.key_anchor))
        c, s = math.cos(float(qkeys[k])), math.sin(float(qkeys[k]))
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        centre = pos + anc + R @ (-anc)
        centre[0] += 0.35 * half[0]
        centre[2] += 0.5 * half[2]
        rews.append(_tolerance(float(np.linalg.norm(centre - tips[h, finger].astype(np.float64))), 0.01, 0.1))
    return float(np.mean(rews)) if rews else 0.0


@pytest.mark.parametrize("side", list(SIDES))
def test_fingering_term(dp, side):
    """The kernel's fp32 term against the fp64 restatement on the handle's own fingertips and key
    angles, within the existing reward-term tests' 1e-3 (tests/test_gpu_parity.py, held here on
    every sample, not the p99); exactly 0 on a step without a note of the kept hand."""
    n = 8
    seq = both_hands_song(dp)
    g = dp.BatchedPianoEnv(n, seq, dp.TaskConfig(hand_side=side), device="cuda:0", canonical_actions=False)
    md, st = g.model_desc, g.song
    lo, hi = dp.model.action_spec(md)
    rng = np.random.RandomState(12)
    g.reset()
    err, zeros, nonzero = 0.0, 0, 0
    for t in range(st.T - 1):
        _, rew, _, _ = g.step(_cuda(rng.uniform(lo, hi, (n, 23))))
        terms, tips, q = g.reward_terms().cpu().numpy(), g.fingertips().cpu().numpy(), _gs(g)["qpos"]
        for e in range(n):
            exp = _fingering_term(md, st, t, side, tips[e], q[e, :88])
            err = max(err, abs(float(terms[e, 3]) - exp))
            if exp == 0.0:
                assert terms[e, 3] == 0.0
                zeros += 1
            else:
                nonzero += 1
        assert (terms[:, 4] == 0.0).all()
        assert_reward_is_sum(rew.cpu().numpy(), terms)
    print("fingering term max |fp32 - fp64|", err)
    assert zeros > 0 and nonzero > 0
    assert err < 1e-3, err


def test_no_fingering_reward_has_no_fourth_term(dp):
    n = 4
    seq = both_hands_song(dp)
    g = dp.BatchedPianoEnv(n, seq, dp.TaskConfig(hand_side="right", disable_fingering_reward=True), device="cuda:0",
                           canonical_actions=False)
    assert g.task_cfg.fingering_reward == 0 and "fingering" not in g.obs_slices and g.obs_dim == 296
    lo, hi = dp.model.action_spec(g.model_desc)
    rng = np.random.RandomState(2)
    g.reset()
    for _ in range(6):
        _, rew, _, _ = g.step(_cuda(rng.uniform(lo, hi, (n, 23))))
        terms = g.reward_terms().cpu().numpy()
        assert (terms[:, 3:] == 0.0).all() and (terms[:, 0] > 0.0).all()
        assert_reward_is_sum(rew.cpu().numpy(), terms)


# ---------------------------------------------------------------- 4. episode semantics
def test_episode_semantics(dp):
    seq = song(dp, "test_task")
    g = dp.BatchedPianoEnv(2, seq, dp.TaskConfig(hand_side="right", control_timestep=0.01), device="cuda:0",
                           canonical_actions=False)
    T = g.song.T
    zero = torch.zeros(2, 23, device="cuda:0")
    g.reset()
    for i in range(T):
        _, r, d, s = g.step(zero)
        assert int(s[0]) == (dp.abi.LAST if i == T - 1 else dp.abi.MID) and float(d[0]) == 1.0
    _, r, d, s = g.step(zero)  # auto-reset
    assert int(s[0]) == dp.abi.FIRST and float(r[0]) == 0.0 and float(d[0]) == 1.0
    with pytest.raises(ValueError, match="action"):
        g.step(torch.zeros(2, 45, device="cuda:0"))
    # the single-env facade and the VecEnv surface carry the one-hand specs
    env = dp.load("RoboPianist-debug-TwinkleTwinkleLittleStar-v0", task_kwargs=dict(hand_side="left"))
    assert env.action_spec().shape == (23,)
    ts = env.reset()
    assert list(ts.observation)[-2:] == ["lh_shadow_hand/joints_pos", "lh_shadow_hand/position"]
    assert env.step(np.zeros(23, np.float32)).observation["lh_shadow_hand/position"].shape == (3,)
    vec = dp.VectorizedPianoEnv(2, song(dp, "twinkle"), hand_side="right")
    assert vec.envs[1].action_spec().shape == (23,)
    assert vec.envs[0].observation_spec()["rh_shadow_hand/position"].shape == (3,)
    assert vec.reset()["fingering"].shape == (2, 5)


def test_wrong_press_termination(dp):
    """piano_with_one_shadow_hand.py:167-174: a key that should not sound ends the episode with
    discount 0 (the key held down through qfrc_applied, as piano_with_shadow_hands_test.py:239)."""
    seq = song(dp, "test_task")
    g = dp.BatchedPianoEnv(2, seq, dp.TaskConfig(hand_side="right", control_timestep=0.01,
                                                 wrong_press_termination=True), device="cuda:0",
                           canonical_actions=False)
    g.reset()
    f = np.zeros((2, 140), np.float32)
    f[1, 10] = 5.0  # env 1: a key outside the song, pressed
    g.set_applied(f)
    zero = torch.zeros(2, 23, device="cuda:0")
    for _ in range(g.song.T):
        _, r, d, s = g.step(zero)
        if int(s[1]) == dp.abi.LAST:
            break
    assert int(s[1]) == dp.abi.LAST and float(d[1]) == 0.0
    assert int(s[0]) == dp.abi.MID and float(d[0]) == 1.0


def test_create_refusals(dp):
    import ctypes as C
    import importlib
    lib = importlib.import_module("diffusion-piano_amd._lib").load()
    seq = song(dp, "twinkle")
    md, st, tc = dp.compile_task(seq, dp.TaskConfig(), canonical_actions=False)  # both hands attached
    sd = dp.abi.SongDesc.from_tables(st)
    h = C.c_void_p()
    tc.hand_side = dp.abi.HAND_RIGHT
    assert lib.ps_create(C.addressof(md), C.addressof(sd), C.addressof(tc), 2, 0, 1, C.byref(h)) < 0
    assert b"not detached" in lib.ps_last_error()
    md, st, tc = dp.compile_task(seq, dp.TaskConfig(hand_side="left"), canonical_actions=False)
    tc.randomize_hand_positions = 1
    assert lib.ps_create(C.addressof(md), C.addressof(sd), C.addressof(tc), 2, 0, 1, C.byref(h)) < 0
    assert b"randomize_hand_positions" in lib.ps_last_error()
    tc.randomize_hand_positions = 0
    tc.hand_side = dp.abi.HAND_RIGHT  # the model keeps the left hand
    assert lib.ps_create(C.addressof(md), C.addressof(sd), C.addressof(tc), 2, 0, 1, C.byref(h)) < 0
    assert b"not detached" in lib.ps_last_error()
    assert lib.ps_version() >= 5


# ---------------------------------------------------------------- 5. the one-hand task's physics is the two-hand one's
@pytest.mark.parametrize("n,steps", [(64, 10), (1024, 10), (2304, 4)], ids=["64", "1024", "2304"])
@pytest.mark.parametrize("hand", list(HANDS))
def test_one_hand_task_equals_two_hand_task_bitwise(dp, hand, n, steps, monkeypatch):
    """The same detached-hand model and action stream with hand_side = 1 and with hand_side = 0 (to
    which it is a model with locked dofs): the step kernels are shared and only the task layer
    branches on the hand side, so after every step qpos, qvel, qacc_ws, ctrl and the key_press /
    sustain / energy terms are bitwise equal. 64 envs: the one-wave instantiation; 1024 and 2304:
    the two-wave one, 2304 being more envs than resident wave slots. A one-hand handle steps
    monolithic at every env count (csrc/pianosim.hip launch()); a two-hand
    handle above 2048 envs is time-sliced by default, so at 2304 envs the hand_side = 0 handle is
    created with PIANOSIM_CHUNKS=0 and both legs run the monolithic step."""
    seq = song(dp, "crossing_field")
    md, st, tc = dp.compile_task(seq, dp.TaskConfig(hand_side="right", trim_silence=True, **HANDS[hand]),
                                 canonical_actions=False)
    tc0 = dp.abi.TaskCfg.from_buffer_copy(tc)
    tc0.hand_side = dp.abi.HAND_BOTH
    A = dp.BatchedPianoEnv.from_compiled(n, md, st, tc, device="cuda:0")
    if n > 2048:
        monkeypatch.setenv("PIANOSIM_CHUNKS", "0")
    B = dp.BatchedPianoEnv.from_compiled(n, md, st, tc0, device="cuda:0")
    assert A.obs_dim == 301 - 5 * (1 - tc.fingering_reward) and B.obs_dim == A.obs_dim - 3 + 26 + 5 * tc.fingering_reward
    assert A.action_dim == B.action_dim == 23 and A.task.hand_side == "right" and B.task.hand_side is None
    lo, hi = dp.model.action_spec(md)
    gen = torch.Generator(device="cuda:0").manual_seed(31)
    tlo, thi = _cuda(lo), _cuda(hi)
    A.reset()
    B.reset()
    ncon = 0
    for i in range(steps):
        a = tlo + (thi - tlo) * torch.rand(n, 23, device="cuda:0", generator=gen)
        A.step(a)
        B.step(a)
        sa, sb = A.get_state(), B.get_state()
        for k in ("qpos", "qvel", "qacc_ws", "ctrl"):
            assert torch.equal(sa[k], sb[k]), (k, i)
        assert torch.equal(A.reward_terms()[:, :3], B.reward_terms()[:, :3]), i
        ncon += int(A.contact_count().sum())
    assert ncon > 0 and float(sa["qpos"][:, 88:114].abs().max()) > 0.0


@pytest.mark.parametrize("hand", list(HANDS))
@pytest.mark.parametrize("side", list(SIDES))
def test_task_layer_on_the_time_sliced_step(dp, side, hand, monkeypatch):
    """The one-hand task layer at the end of a time-sliced step (PIANOSIM_CHUNKS=6: the queue kernel,
    2304 envs on 2048 workgroups), checked against each env's OWN returned state, so that it holds
    whatever the physics of the step did: the detached slots at 0, joints_pos and `position` from
    the returned qpos, the 5-wide fingering row and the goal row of the env's step, the fingering
    term from the env's own fingertips and key angles (fp64 restatement, within 1e-3 as
    test_fingering_term), no forearm term, reward = the sum of the terms. The envs are staggered
    over the song so every kind of step (own notes, the other hand's only, silence) occurs."""
    n, steps = 2304, 4
    monkeypatch.setenv("PIANOSIM_CHUNKS", "6")
    seq = both_hands_song(dp)
    g = dp.BatchedPianoEnv(n, seq, dp.TaskConfig(hand_side=side, **HANDS[hand]), device="cuda:0",
                           canonical_actions=False)
    md, st, lay = g.model_desc, g.song, g.obs_slices
    h, gone = SIDES[side], 1 - SIDES[side]
    name = ("rh", "lh")[h] + "_shadow_hand"
    lo, hi = dp.model.action_spec(md)
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    tlo, thi = _cuda(lo), _cuda(hi)
    g.reset()
    g.set_state({"t_idx": (np.arange(n) % (st.T - steps - 1)).astype(np.int32)})  # no env reaches LAST
    order = [88 + 26 * h + md.dof_obs_order[h][i] for i in range(26)]
    heads = [_expected_obs_head(st, 1, t, side) for t in range(st.T)]
    err, zeros, nonzero = 0.0, 0, 0
    for _ in range(steps):
        t_cur = _gs(g)["t_idx"]
        obs, rew, _, stype = g.step(tlo + (thi - tlo) * torch.rand(n, 23, device="cuda:0", generator=gen))
        obs, s = obs.cpu().numpy(), _gs(g)
        terms, tips = g.reward_terms().cpu().numpy(), g.fingertips().cpu().numpy()
        assert (stype.cpu().numpy() == dp.abi.MID).all()
        np.testing.assert_array_equal(s["t_idx"], t_cur + 1)
        for k in ("qpos", "qvel", "qacc_ws"):
            assert np.abs(s[k][:, 88 + 26 * gone:88 + 26 * gone + 26]).max() == 0.0, k
        assert np.abs(s["ctrl"][:, 22 * gone:22 * gone + 22]).max() == 0.0
        np.testing.assert_array_equal(obs[:, lay[name + "/joints_pos"]], s["qpos"][:, order])
        np.testing.assert_allclose(obs[:, lay[name + "/position"]], _root_position(md, h, s["qpos"]), rtol=0, atol=1e-6)
        np.testing.assert_array_equal(obs[:, lay["goal"]], np.stack([heads[t][0] for t in s["t_idx"]]))
        np.testing.assert_array_equal(obs[:, lay["fingering"]], np.stack([heads[t][1] for t in s["t_idx"]]))
        for e in range(n):
            exp = _fingering_term(md, st, int(t_cur[e]), side, tips[e], s["qpos"][e, :88])
            err = max(err, abs(float(terms[e, 3]) - exp))
            zeros += exp == 0.0 and terms[e, 3] == 0.0
            nonzero += exp != 0.0
        assert (terms[:, 4] == 0.0).all()
        assert_reward_is_sum(rew.cpu().numpy(), terms)
    print("fingering term max |fp32 - fp64|", err, "zero steps", zeros, "others", nonzero)
    assert zeros > 0 and nonzero > 0 and zeros + nonzero == n * steps
    assert err < 1e-3, err


# ---------------------------------------------------------------- 6. augmentations
def test_augmented_one_hand_handle(dp):
    n = 8
    seq = both_hands_song(dp)
    task = dp.TaskConfig(hand_side="left", augmentations=[dp.MidiPitchShift(1.0, 2)])
    g = dp.BatchedPianoEnv(n, seq, task, device="cuda:0", canonical_actions=False, seed=5)
    lay = g.obs_slices
    lo, hi = dp.model.action_spec(g.model_desc)
    rng = np.random.RandomState(6)
    obs = g.reset().cpu().numpy()
    resets, shifts = 0, set()
    t = np.zeros(n, np.int64)
    for _ in range(2 * g.song.T + 4):
        tab = {k: v.cpu().numpy() for k, v in g.song_tables().items()}
        aug = {k: v.cpu().numpy() for k, v in g.augmentation().items()}
        shifts |= set(aug["shift"].tolist())
        for e in range(n):
            row = min(t[e], aug["T"][e] - 1)
            np.testing.assert_array_equal(obs[e, lay["goal"]][:89], tab["goal"][e, row])
            fing = np.zeros(5, np.float32)
            for i in range(tab["count"][e, row]):
                if tab["fingers"][e, row, i] >= 5:
                    fing[tab["fingers"][e, row, i] - 5] = 1.0
            np.testing.assert_array_equal(obs[e, lay["fingering"]], fing)
        o, _, _, s = g.step(_cuda(rng.uniform(lo, hi, (n, 23))))
        obs, s = o.cpu().numpy(), s.cpu().numpy()
        t = np.where(s == dp.abi.FIRST, 0, t + 1)
        resets += int((s == dp.abi.FIRST).sum())
    assert resets >= n and len(shifts) > 1
