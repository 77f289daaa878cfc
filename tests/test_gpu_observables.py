"""TaskConfig.observables on the GPU: the extras the step kernel appends to the observation row.

1. the default part of the row, the rewards and the state are bitwise those of a handle without
   extras; 2. the extras that restate an export of the kernel equal it bitwise; 3. cos/sin, the
   actuator velocity and force, the energy identity and the two-hand `position` against fp64
   restatements written here (and the one-hand row's own `position` column); 4. reset rows (reset,
   masked reset, auto-reset); 5. the one-wave / two-wave instantiations and the time-sliced step
   give the same bits.

8 envs and 6 random-action steps from random states unless stated."""
import numpy as np
import pytest

from helpers import random_states, song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, STEPS = 8, 6
HANDS = {"capsule": None, "hull": False}  # TaskConfig.primitive_fingertip_collisions
HAND_NAMES = ("rh_shadow_hand", "lh_shadow_hand")


def _np(t):
    return t.cpu().numpy().copy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _all(dp):
    return list(dp.abi.OBSERVABLES)


def _make(dp, seq, n=N, observables=None, **kw):
    return dp.BatchedPianoEnv(n, seq, dp.TaskConfig(observables=observables, **kw), device="cuda:0",
                              canonical_actions=False)


def _kept(g):
    return (0, 1) if not g.task_cfg.hand_side else (g.task_cfg.hand_side - 1,)


def _zero_locked(md, x):
    """(a detached or removed dof's slot is held at 0: random_states fills it)"""
    for h in range(2):
        for j in range(26):
            if md.dof_locked[h][j]:
                x[:, 88 + 26 * h + j] = 0.0
    return x


def _record(g):
    s = {k: _np(v) for k, v in g.get_state().items()}
    return dict(obs=_np(g.obs), reward=_np(g.reward), discount=_np(g.discount), step_type=_np(g.step_type),
                tips=_np(g.fingertips()), terms=_np(g.reward_terms()), **s)


def _rollout(g, seed, steps=STEPS, applied=None):
    """reset row, then `steps` random-action steps from random states -> [records]; [0] is the reset."""
    rng = np.random.RandomState(seed)
    md = g.model_desc
    g.reset()
    out = [_record(g)]
    q, v = random_states(md, g.num_envs, rng)
    g.set_state({"qpos": _zero_locked(md, q), "qvel": _zero_locked(md, v)})
    if applied is not None:
        g.set_applied(applied)
    lo, hi = g.action_lo, g.action_hi
    for _ in range(steps):
        a = rng.uniform(lo, hi, (g.num_envs, g.action_dim)).astype(np.float32)
        g.step(_cuda(a))
        out.append(_record(g))
    return out


# ---------------------------------------------------------------- 1. the default part is untouched
CASES = {
    "capsule_twinkle_L0": ("capsule", "twinkle", dict(n_steps_lookahead=0)),
    "hull_twinkle_L2": ("hull", "twinkle", dict(n_steps_lookahead=2)),
    "capsule_crossing_L2": ("capsule", "crossing_field", dict(n_steps_lookahead=2)),
    "hull_crossing_L0": ("hull", "crossing_field", dict(n_steps_lookahead=0)),
    "capsule_right_L2": ("capsule", "twinkle", dict(hand_side="right", n_steps_lookahead=2)),
    "hull_left_L0": ("hull", "twinkle", dict(hand_side="left", n_steps_lookahead=0)),
    "capsule_narrowest": ("capsule", "twinkle", dict(reduced_action_space=True, forearm_dofs=("forearm_tx",))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_default_part_is_bitwise_the_default_row(dp, case):
    hand, name, kw = CASES[case]
    seq = song(dp, name)
    kw = dict(kw, primitive_fingertip_collisions=HANDS[hand])
    plain = _make(dp, seq, **kw)
    full = _make(dp, seq, observables=_all(dp), **kw)
    base = plain.obs_dim
    assert list(full.obs_slices)[:len(plain.obs_slices)] == list(plain.obs_slices)
    assert full.obs_dim > base and list(full.obs_slices.values())[len(plain.obs_slices) - 1].stop == base
    assert ("fingering" in plain.obs_slices) == (name == "twinkle")
    a, b = _rollout(plain, 3), _rollout(full, 3)
    plain.close(), full.close()
    for t, (ra, rb) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(_bits(ra["obs"]), _bits(rb["obs"][:, :base]), err_msg=f"step {t} obs")
        for k in ra:
            if k != "obs":
                np.testing.assert_array_equal(_bits(ra[k]), _bits(rb[k]), err_msg=f"step {t} {k}")
    assert np.abs(b[-1]["qvel"]).max() > 0 and np.abs(b[-1]["obs"][:, base:]).max() > 0


# ---------------------------------------------------------------- the model description, restated
def _obs_dofs(md, h):
    """qpos / qvel columns of hand h's joints_pos entries, in their order."""
    nj = md.n_obs_joints[h] or 26
    return [88 + 26 * h + md.dof_obs_order[h][i] for i in range(nj)]


def _actuators(md, h):
    """Hand h's actuators the reference has, in the order of their action columns."""
    col = (lambda a: md.act_column[h][a]) if md.n_action > 0 else (lambda a: 22 * h + a)
    return sorted([a for a in range(22) if col(a) >= 0], key=col)


def _transmission(md, h, a):
    """[(qpos column, coefficient)] of actuator a's length: its joint, or its fixed tendon's two."""
    tg = md.act_target[h][a]
    if md.act_kind[h][a] == 0:
        return [(88 + 26 * h + tg, 1.0)]
    return [(88 + 26 * h + md.tendon_dof[h][tg][i], float(np.float32(md.tendon_coef[h][tg][i]))) for i in range(2)]


def _length(md, h, acts, x):
    """-> (sum c x, sum |c x|) [n, len(acts)] in fp64 of the fp32 values x (qpos or qvel)."""
    x = x.astype(np.float64)
    s = np.stack([sum(c * x[:, d] for d, c in _transmission(md, h, a)) for a in acts], axis=1)
    m = np.stack([sum(np.abs(c * x[:, d]) for d, c in _transmission(md, h, a)) for a in acts], axis=1)
    return s, m


def actuator_force_fp64(md, h, acts, qpos, ctrl):
    """clip(kp (clip(ctrl, ctrlrange) - length(qpos)), forcerange) in fp64 -> (force, clipped?, kp (|ctrl| + |length|))."""
    length, _ = _length(md, h, acts, qpos)
    kp = np.array([md.act_kp[h][a] for a in acts])
    cr = np.array([list(md.act_ctrlrange[h][a]) for a in acts])
    fr = np.array([list(md.act_forcerange[h][a]) for a in acts])
    lim = np.array([bool(md.act_forcelimited[h][a]) for a in acts])
    c = np.clip(ctrl[:, [22 * h + a for a in acts]].astype(np.float64), cr[:, 0], cr[:, 1])
    raw = kp * (c - length)
    f = np.where(lim, np.clip(raw, fr[:, 0], fr[:, 1]), raw)
    return f, f != raw, kp * (np.abs(c) + np.abs(length))


def _root_position(md, h, qpos, dy):
    """World position of hand h's root body in fp64: its pose, the episode's y offset, the slides."""
    w, x, y, z = np.asarray(list(md.body_quat[h][0]), np.float64) / np.linalg.norm(list(md.body_quat[h][0]))
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (y * y + x * x)]])
    p = np.tile(np.array(list(md.body_pos[h][0]), np.float64), (len(qpos), 1))
    p[:, 1] += np.asarray(dy, np.float64)
    for j in range(26):
        if md.dof_body[h][j] == 0 and not md.dof_locked[h][j]:
            p += np.outer(qpos[:, 88 + 26 * h + j].astype(np.float64), R @ np.array(list(md.dof_axis[h][j])))
    return p


# ---------------------------------------------------------------- 2. identities with the kernel's exports
@pytest.fixture(scope="module")
def full_rollouts(dp):
    """The all-extras rollout of three handles, computed once and left unchanged: the two-hand task
    (hull hand), the narrowest hand, the left hand alone. Three keys are pushed down by an applied
    force so both activations occur. -> {name: (layout, model, kept hands, records)}"""
    out = {}
    for name, kw in (("two", dict(primitive_fingertip_collisions=False)),
                     ("narrowest", dict(reduced_action_space=True, forearm_dofs=("forearm_tx",))),
                     ("left", dict(hand_side="left"))):
        g = _make(dp, song(dp, "twinkle"), observables=_all(dp), **kw)
        f = np.zeros((N, 140), np.float32)
        f[:, [10, 40, 41]] = 5.0
        out[name] = (g.obs_slices, g.model_desc, _kept(g), _rollout(g, 5, applied=f))
        g.close()
    return out


@pytest.mark.parametrize("name", ["two", "narrowest", "left"])
def test_extras_equal_the_exports_bitwise(dp, full_rollouts, name):
    lay, md, kept, recs = full_rollouts[name]
    lo = np.array([md.key_range[k][0] for k in range(88)], np.float32)
    hi = np.array([md.key_range[k][1] for k in range(88)], np.float32)
    acts_seen, sus_seen = set(), set()
    for t, r in enumerate(recs):
        obs, q = r["obs"], r["qpos"]
        eq = lambda key, want: np.testing.assert_array_equal(_bits(obs[:, lay[key]]), _bits(np.ascontiguousarray(want, np.float32)),
                                                             err_msg=f"step {t} {key}")
        eq("piano/joints_pos", q[:, :88])
        act = np.abs(np.clip(q[:, :88], lo, hi) - hi) <= np.float32(dp.abi.KEY_THRESHOLD)
        assert act.dtype == bool and q.dtype == np.float32
        eq("piano/activation", act)
        eq("piano/sustain_activation", (r["sustain"] >= 0.5)[:, None])
        acts_seen |= set(np.unique(obs[:, lay["piano/activation"]]))
        sus_seen |= set(np.unique(obs[:, lay["piano/sustain_activation"]]))
        for h in kept:
            hn = HAND_NAMES[h]
            eq(hn + "/joints_vel", r["qvel"][:, _obs_dofs(md, h)])
            eq(hn + "/fingertip_positions", r["tips"][:, h].reshape(N, 15))
            f, v = obs[:, lay[hn + "/actuators_force"]], obs[:, lay[hn + "/actuators_velocity"]]
            eq(hn + "/actuators_power", np.abs(f) * np.abs(v))
            assert f.shape[1] == len(_actuators(md, h)) and v.dtype == np.float32
    assert acts_seen == {0.0, 1.0} and sus_seen == {0.0, 1.0}
    pw = recs[-1]["obs"][:, lay[HAND_NAMES[kept[0]] + "/actuators_power"]]
    assert (pw > 0).any()


# ---------------------------------------------------------------- 3. against fp64
@pytest.mark.parametrize("name", ["two", "narrowest", "left"])
def test_cos_sin_velocity_and_energy(dp, full_rollouts, name):
    lay, md, kept, recs = full_rollouts[name]
    coef = dp.TaskConfig().energy_penalty_coef
    for t, r in enumerate(recs):
        obs, power = r["obs"], 0.0
        for h in kept:
            hn = HAND_NAMES[h]
            # numpy fp64 of the exported fp32 angles; sinf / cosf are good to ~2 ulp (2.4e-7 at 1): 1e-6
            q = r["qpos"][:, _obs_dofs(md, h)].astype(np.float64)
            cs = obs[:, lay[hn + "/joints_pos_cos_sin"]].astype(np.float64)
            err = np.abs(cs - np.hstack([np.cos(q), np.sin(q)])).max()
            print(f"{name} step {t} {hn}: cos/sin max error {err:.2e}")
            assert err <= 1e-6
            # the transmission's coefficients times the exported qvel, within 4 ulp of sum |c v|
            want, mag = _length(md, h, _actuators(md, h), r["qvel"])
            verr = np.abs(obs[:, lay[hn + "/actuators_velocity"]].astype(np.float64) - want)
            print(f"{name} step {t} {hn}: actuator velocity max error / ulp {np.max(verr / np.spacing(np.maximum(mag, 1e-30).astype(np.float32))):.2f}")
            assert (verr <= 4 * np.spacing(mag.astype(np.float32))).all()
            power = power + obs[:, lay[hn + "/actuators_power"]].astype(np.float64).sum(axis=1)
        if t > 0:  # (44 non-negative fp32 terms summed in another order)
            np.testing.assert_allclose(-coef * power, r["terms"][:, 2], rtol=1e-5, atol=0)
    assert np.abs(recs[-1]["terms"][:, 2]).min() > 0


def force_case(dp, seed=0):
    """The single-substep handle's inputs: (task kwargs, qpos, qvel, action) - plain numpy."""
    kw = dict(control_timestep=0.005, physics_timestep=0.005)
    md, _, _ = dp.compile_task(song(dp, "twinkle"), dp.TaskConfig(**kw), canonical_actions=False)
    rng = np.random.RandomState(seed)
    q, v = random_states(md, N, rng)
    lo, hi = dp.model.action_spec(md)
    a = rng.uniform(lo, hi, (N, 45)).astype(np.float32)
    return kw, md, q.astype(np.float32), v.astype(np.float32), a


def test_force_case_has_both_populations(dp):
    """(no GPU work: the seed of test_actuators_force gives clipped and unclipped actuators)"""
    _, md, q, _, a = force_case(dp)
    for h in range(2):
        _, clipped, _ = actuator_force_fp64(md, h, _actuators(md, h), q, a[:, :44])
        assert clipped.any() and (~clipped).any()


def test_actuators_force(dp):
    """One substep per control step: the reported force is that substep's actuation force, from the
    state the step started at."""
    kw, md0, q, v, a = force_case(dp)
    g = _make(dp, song(dp, "twinkle"), observables=["actuators_force"], **kw)
    md, lay = g.model_desc, g.obs_slices
    assert md.n_substeps == 1 and bytes(md) == bytes(md0)
    g.reset()
    g.set_state({"qpos": q, "qvel": v})
    obs = _np(g.step(_cuda(a))[0])
    ctrl = _np(g.get_state()["ctrl"])
    g.close()
    np.testing.assert_array_equal(ctrl, a[:, :44])
    n_clip = n_free = 0
    for h in range(2):
        want, clipped, scale = actuator_force_fp64(md, h, _actuators(md, h), q, ctrl)
        err = np.abs(obs[:, lay[HAND_NAMES[h] + "/actuators_force"]].astype(np.float64) - want)
        print(f"{HAND_NAMES[h]}: force max error / (2^-23 kp (|ctrl| + |len|)) {np.max(err / (2.0 ** -23 * scale)):.2f}")
        assert (err <= 4 * 2.0 ** -23 * scale).all()
        n_clip, n_free = n_clip + clipped.sum(), n_free + (~clipped).sum()
    assert n_clip > 0 and n_free > 0


def test_two_hand_position(dp):
    seq = song(dp, "twinkle")
    g = _make(dp, seq, observables=["position"], randomize_hand_positions=True)
    md, lay = g.model_desc, g.obs_slices
    recs = _rollout(g, 9)
    dy = _np(g.hand_offset()[0])
    g.close()
    assert np.abs(dy).max() > 1e-3
    for t, r in enumerate(recs):
        for h in range(2):
            # the one-hand row's tolerance: fp32 kinematics of a position below 1 m, a handful of operations
            np.testing.assert_allclose(r["obs"][:, lay[HAND_NAMES[h] + "/position"]], _root_position(md, h, r["qpos"], dy),
                                       rtol=0, atol=1e-6, err_msg=f"step {t} hand {h}")
    moved = np.abs(_root_position(md, 0, recs[-1]["qpos"], dy) - _root_position(md, 0, recs[0]["qpos"], dy)).max()
    assert moved > 1e-3  # the position follows the forearm slides
    # ... and against the one-hand row's own `position` column (held to the closed form by
    # tests/test_gpu_one_hand.py). The fp64 checker has no one-hand row - it steps the detached-hand
    # model as the two-hand task - so the pin is on the kernel: the same detached-hand model under
    # the two-hand task with `position` requested steps the same physics, and its kept hand's extra
    # must be that column, bit for bit.
    for side, h in (("right", 0), ("left", 1)):
        md1, st1, tc1 = dp.compile_task(seq, dp.TaskConfig(hand_side=side), canonical_actions=False)
        tc0 = dp.abi.TaskCfg.from_buffer_copy(tc1)
        tc0.hand_side, tc0.observables = dp.abi.HAND_BOTH, dp.abi.obs_mask(["position"])
        one = dp.BatchedPianoEnv.from_compiled(N, md1, st1, tc1, device="cuda:0")
        two = dp.BatchedPianoEnv.from_compiled(N, md1, st1, tc0, device="cuda:0")
        assert two.task.observables == ["position"] and one.task.observables is None
        key = HAND_NAMES[h] + "/position"
        a, b = _rollout(one, 4), _rollout(two, 4)
        one.close(), two.close()
        for t, (ra, rb) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(_bits(ra["qpos"]), _bits(rb["qpos"]))
            np.testing.assert_array_equal(_bits(ra["obs"][:, one.obs_slices[key]]), _bits(rb["obs"][:, two.obs_slices[key]]),
                                          err_msg=f"{side} step {t}")
        assert np.abs(a[-1]["obs"][:, one.obs_slices[key]] - a[0]["obs"][:, one.obs_slices[key]]).max() > 1e-3


# ---------------------------------------------------------------- 4. resets
def _short_song(dp):
    m = dp.music
    seq = m.NoteSequence(title="chunk test")
    for p, s, e in [(60, 0.0, 0.15), (64, 0.05, 0.2), (67, 0.1, 0.3), (48, 0.15, 0.4), (72, 0.25, 0.4)]:
        seq.notes.append(m.Note(p, s, e, 80, 0))
    seq.total_time = 0.4
    return seq


def _reset_force(md, h):
    """clip(kp (clamp(0, ctrlrange) - 0), forcerange) as the fp32 the kernel computes (one product)."""
    out = []
    for a in _actuators(md, h):
        c = np.clip(np.float32(0), np.float32(md.act_ctrlrange[h][a][0]), np.float32(md.act_ctrlrange[h][a][1]))
        f = np.float32(md.act_kp[h][a]) * c
        if md.act_forcelimited[h][a]:
            f = np.clip(f, np.float32(md.act_forcerange[h][a][0]), np.float32(md.act_forcerange[h][a][1]))
        out.append(f)
    return np.array(out, np.float32)


def test_reset_rows(dp):
    seq = _short_song(dp)
    fresh = _make(dp, seq, n=2, observables=_all(dp))
    row = _np(fresh.reset())[0]
    fresh.close()
    g = _make(dp, seq, n=N, observables=_all(dp))
    md, lay, T = g.model_desc, g.obs_slices, g.song.T
    assert 4 <= T <= 12
    obs = _np(g.reset())
    for e in range(N):
        np.testing.assert_array_equal(_bits(obs[e]), _bits(row))
    # the reset row: mj_forward at the reset pose with ctrl 0
    for h in range(2):
        hn = HAND_NAMES[h]
        assert not row[lay[hn + "/joints_vel"]].any() and not row[lay[hn + "/actuators_velocity"]].any()
        assert not row[lay[hn + "/actuators_power"]].any()
        np.testing.assert_array_equal(row[lay[hn + "/actuators_force"]], _reset_force(md, h))
        np.testing.assert_allclose(row[lay[hn + "/position"]], list(md.body_pos[h][0]), rtol=0, atol=1e-7)
        np.testing.assert_array_equal(row[lay[hn + "/joints_pos_cos_sin"]], np.r_[np.ones(26), np.zeros(26)].astype(np.float32))
    assert not row[lay["piano/joints_pos"]].any() and not row[lay["piano/activation"]].any()
    # staggered episodes: the auto-reset row inside a step is the fresh handle's reset row
    g.set_state({"t_idx": (np.arange(N) % T).astype(np.int32)})
    rng = np.random.RandomState(2)
    firsts = 0
    for _ in range(12):
        a = rng.uniform(g.action_lo, g.action_hi, (N, 45)).astype(np.float32)
        obs, _, _, stype = g.step(_cuda(a))
        obs, stype = _np(obs), _np(stype)
        for e in np.nonzero(stype == dp.abi.FIRST)[0]:
            np.testing.assert_array_equal(_bits(obs[e]), _bits(row))
            firsts += 1
        assert np.abs(obs[stype != dp.abi.FIRST][:, lay["rh_shadow_hand/joints_vel"]]).max() > 0
    assert firsts >= N
    # a masked reset rewrites the masked rows only
    before = _np(g.obs)
    mask = np.arange(N) % 3 == 0
    after = _np(g.reset(mask))
    g.close()
    for e in range(N):
        np.testing.assert_array_equal(_bits(after[e]), _bits(row if mask[e] else before[e]))
    assert (before[mask] != row).any()


# ---------------------------------------------------------------- 5. paths
def _path_rollout(dp, monkeypatch, env, n, steps, hand):
    for k in ("PIANOSIM_ONE_WAVE_MAX", "PIANOSIM_CHUNKS", "PIANOSIM_STEP_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = _make(dp, _short_song(dp), n=n, observables=_all(dp), primitive_fingertip_collisions=HANDS[hand])
    T = g.song.T
    g.reset()
    g.set_state({"t_idx": (np.arange(n) % T).astype(np.int32)})
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    out = []
    for _ in range(steps):
        a = torch.rand(n, g.action_dim, device="cuda:0", generator=gen) * 2 - 1
        o, r, d, s = g.step(a)
        out.append(dict(obs=_np(o), reward=_np(r), discount=_np(d), step_type=_np(s)))
    g.close()
    kinds = np.concatenate([o["step_type"] for o in out])
    assert (kinds == 0).any() and (kinds == 2).any(), "no auto-reset / terminal step in the window"
    return out


def _assert_same(a, b, what):
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in ra:
            np.testing.assert_array_equal(_bits(ra[k]), _bits(rb[k]), err_msg=f"{what}: step {t}, {k}")


@pytest.mark.parametrize("hand", list(HANDS))
def test_one_wave_and_two_wave_builds_agree(dp, monkeypatch, hand):
    """8 envs run the one-wave (no-scratch) instantiation; PIANOSIM_ONE_WAVE_MAX=0 the two-wave one."""
    a = _path_rollout(dp, monkeypatch, {}, N, 12, hand)
    b = _path_rollout(dp, monkeypatch, {"PIANOSIM_ONE_WAVE_MAX": "0"}, N, 12, hand)
    _assert_same(a, b, f"{hand}: one wave vs two waves")


@pytest.mark.parametrize("hand", list(HANDS))
def test_time_sliced_step_carries_the_extras(dp, monkeypatch, hand):
    """40 envs on 8 workgroups, 3 chunks of substeps: the actuator force crosses chunks in the park row."""
    a = _path_rollout(dp, monkeypatch, {"PIANOSIM_CHUNKS": "0"}, 40, 12, hand)
    b = _path_rollout(dp, monkeypatch, {"PIANOSIM_CHUNKS": "3", "PIANOSIM_STEP_GRID": "8"}, 40, 12, hand)
    _assert_same(a, b, f"{hand}: monolithic vs 3 chunks")


# ---------------------------------------------------------------- the Python surfaces
def test_surfaces_carry_the_extras(dp):
    """obs_dict / observation_spec, VectorizedPianoEnv, Environment and load(task_kwargs=) read obs_layout."""
    names = ["joints_vel", "piano/activation"]
    env = dp.load("RoboPianist-debug-TwinkleTwinkleLittleStar-v0", task_kwargs=dict(observables=names))
    ts = env.reset()
    assert list(ts.observation)[-3:] == ["piano/activation", "rh_shadow_hand/joints_vel", "lh_shadow_hand/joints_vel"]
    assert env.observation_spec()["lh_shadow_hand/joints_vel"].shape == (26,)
    ts = env.step(np.full(45, 0.5, np.float32))
    assert ts.observation["piano/activation"].shape == (88,) and np.abs(ts.observation["rh_shadow_hand/joints_vel"]).max() > 0
    vec = dp.VectorizedPianoEnv(2, song(dp, "twinkle"), observables=names, reduced_action_space=True)
    assert vec.reset()["rh_shadow_hand/joints_vel"].shape == (2, 23)
    assert vec.envs[0].observation_spec()["piano/activation"].shape == (88,)
    core = vec.core
    assert core.obs_dict()["lh_shadow_hand/joints_vel"].shape == (2, 23) and core.obs_dim == 329 - 6 + 88 + 46
    again = dp.BatchedPianoEnv.from_compiled(2, core.model_desc, core.song, core.task_cfg, device="cuda:0")
    assert again.obs_slices == core.obs_slices and again.task.observables == ["piano/activation", "joints_vel"]
    again.close()
