"""Per-episode MIDI augmentations on the GPU (csrc/augment.inc song_build_kernel): every env
draws its variations when its episode starts and rebuilds its own song tables on the device.
The draw is held to variations.draw (bitwise), the tables to the host path
song_tables(transpose(stretch(song))) (bitwise), and a step on per-env tables to the step of a
plain handle created from the same host-augmented song (bitwise)."""
import importlib

import numpy as np
import pytest

from helpers import song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TABLES = ("goal", "count", "keys", "fingers")
SEED = 12345


@pytest.fixture(scope="module")
def V():
    return importlib.import_module("diffusion-piano_amd.variations")


@pytest.fixture(scope="module")
def S(dp):
    m = dp.music
    return {"twinkle": song(dp, "twinkle"), "guren": m.trim_silence(song(dp, "guren")),
            "crossing_field": m.trim_silence(song(dp, "crossing_field"))}


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _aug(g):
    return {k: v.cpu().numpy() for k, v in g.augmentation().items()}


def _check_draws_and_tables(dp, V, g, seed, env0=0, min_episode=0):
    """augmentation() == variations.draw and song_tables() == the host tables of that draw, for
    every env; -> the episodes (resets so far) per env."""
    a = _aug(g)
    tab = {k: v.cpu().numpy() for k, v in g.song_tables().items()}
    episodes = g.hand_offset()[1].cpu().numpy()
    assert (episodes >= 1 + min_episode).any()
    assert (a["fallbacks"] == 0).all()
    host = {}
    for e in range(g.num_envs):
        want = V.draw(seed, env0 + e, int(episodes[e]) - 1, g.augmentations, g.songs)
        got = (int(a["song"][e]), float(a["factor"][e]), int(a["shift"][e]))
        assert got == want, (e, episodes[e], got, want)  # the factor bitwise: == on fp64
        if want not in host:
            host[want] = dp.music.song_tables(V.apply(g.songs, *want), g.task.control_timestep,
                                              g.task.initial_buffer_time)
        st = host[want]
        assert a["T"][e] == st.T, (e, want)
        for k in TABLES:
            np.testing.assert_array_equal(_bits(tab[k][e, :st.T]), _bits(getattr(st, k)), err_msg=f"env {e} {want} {k}")
    return episodes, a


def test_draws_and_tables(dp, V, S):
    short = dp.music.test_midi(0.05)
    augs = [V.MidiSelect([short, S["twinkle"], S["guren"]]), V.MidiTemporalStretch(1.0, 0.5), V.MidiPitchShift(1.0, 3)]
    g = dp.BatchedPianoEnv(32, short, dp.TaskConfig(augmentations=augs), device="cuda:0", seed=SEED)
    g.reset()
    episodes, a = _check_draws_and_tables(dp, V, g, SEED)
    assert (episodes == 1).all() and set(a["song"]) == {1, 2, 3} and len(set(a["factor"])) == 32
    zero = torch.zeros(32, g.action_dim, device="cuda:0")
    for _ in range(7):
        g.step(zero)
    # the 2-5-frame song has ended and restarted with a new draw (episode >= 1)
    episodes, _ = _check_draws_and_tables(dp, V, g, SEED, min_episode=1)
    assert (episodes[a["song"] == 1] >= 2).all()
    g.close()


def _two_chords(m, dt):
    seq = m.NoteSequence(title="two chords", total_time=2 * dt)
    for i in range(9):
        seq.notes.append(m.Note(40 + i, 0.0, 0.8 * dt, 80, 0))
    for i in range(9):
        seq.notes.append(m.Note(60 + i, 1.2 * dt, 2 * dt, 80, 0))
    return seq


def test_forced_edge_cases(dp, V):
    m = dp.music
    dt = 0.01
    restrike = m.NoteSequence(notes=[m.Note(84, 0.01, 0.02, 80, -1), m.Note(84, 0.02, 0.05, 80, -1)], total_time=0.05)
    sustain = m.NoteSequence(notes=[m.Note(84, 0.0, 0.01, 80, -1), m.Note(84, 0.05, 0.06, 80, -1)],
                             control_changes=[m.ControlChange(0.0, 64, 64), m.ControlChange(0.03, 64, 0)],
                             total_time=0.06)
    edge = m.NoteSequence(notes=[m.Note(30, 0.0, 0.02, 80, 0), m.Note(90, 0.01, 0.04, 80, 0)], total_time=0.04)
    chords = _two_chords(m, dt)
    augs = [V.MidiSelect([restrike, sustain, edge, chords]), V.MidiTemporalStretch(1.0, 0.5)]
    g = dp.BatchedPianoEnv(8, restrike, dp.TaskConfig(augmentations=augs, control_timestep=dt), device="cuda:0")
    #        identity     restrike            sustain             key 87      key 0       18 keys in frame 0
    forced = [(0, 1.0, 0), (1, 0.5, 0), (1, 1.5, 0), (2, 0.5, 0), (2, 1.5, 0), (3, 1.0, 18), (3, 1.0, -9), (4, 0.5, 0)]
    g.set_augmentation(*(np.array(x) for x in zip(*forced)))
    a = _aug(g)
    tab = {k: v.cpu().numpy() for k, v in g.song_tables().items()}
    np.testing.assert_array_equal(a["fallbacks"], [0, 0, 0, 0, 0, 0, 0, 1])
    for e, (s, f, sh) in enumerate(forced):
        want = (s, 1.0, 0) if e == 7 else (s, f, sh)  # the fallback: the song as given
        assert (int(a["song"][e]), float(a["factor"][e]), int(a["shift"][e])) == want
        st = m.song_tables(V.apply(g.songs, *want), dt)
        assert a["T"][e] == st.T
        for k in TABLES:
            np.testing.assert_array_equal(_bits(tab[k][e, :st.T]), _bits(getattr(st, k)), err_msg=f"env {e} {k}")
    plain = g.song  # what a plain handle of the same song uploads
    assert a["T"][0] == plain.T
    for k in TABLES:
        np.testing.assert_array_equal(_bits(tab[k][0, :plain.T]), _bits(getattr(plain, k)))
    assert tab["keys"][5, :a["T"][5]].max() == 87 and (tab["keys"][6, :a["T"][6]] == 0).any()
    assert tab["goal"][1, :a["T"][1], :88].sum(axis=1).min() == 0  # the re-strike's gap survives the stretch
    g.close()


def _rollout(dp, init, augs, forced, steps=12, **task_kw):
    """The augmented handle with every env forced to its own draw, then `steps` seeded actions."""
    n = len(forced)
    g = dp.BatchedPianoEnv(n, init, dp.TaskConfig(augmentations=augs, **task_kw), device="cuda:0", seed=SEED)
    g.reset()
    g.set_augmentation(*(np.array(x) for x in zip(*forced)))
    out = _steps(g, n, steps)
    songs = g.songs
    g.close()
    return out, songs


def _steps(g, n, steps):
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    out = []
    for _ in range(steps):
        act = torch.rand(n, g.action_dim, device="cuda:0", generator=gen) * 2 - 1
        o, r, d, s = g.step(act)
        rec = dict(obs=o, reward=r, discount=d, step_type=s, terms=g.reward_terms(), qpos=g.get_state()["qpos"])
        out.append({k: v.cpu().numpy().copy() for k, v in rec.items()})
    return out


def _assert_env_equals_plain(dp, V, out, songs, forced, **task_kw):
    n = len(forced)
    for e, draw in enumerate(forced):
        p = dp.BatchedPianoEnv(n, V.apply(songs, *draw), dp.TaskConfig(**task_kw), device="cuda:0", seed=SEED)
        p.reset()
        ref = _steps(p, n, len(out))
        p.close()
        for t, (a, b) in enumerate(zip(out, ref)):
            for k in a:
                np.testing.assert_array_equal(_bits(a[k][e]), _bits(b[k][e]), err_msg=f"env {e} {draw}: step {t}, {k}")


FORCED = [(1, 1.3, 2), (0, 0.8, -1), (0, 1.0, 0), (1, 0.6, -3)]  # song 0 Guren (fingering reward), 1 Twinkle


def _guren_case(V, S):
    return S["guren"], [V.MidiSelect([S["twinkle"]]), V.MidiTemporalStretch(1.0, 0.5), V.MidiPitchShift(1.0, 3)]


def test_step_equals_plain_handle_of_the_augmented_song(dp, V, S):
    init, augs = _guren_case(V, S)
    out, songs = _rollout(dp, init, augs, FORCED)
    assert out[0]["obs"].shape[1] == 89 * 2 + 10 + 89 + 52  # the fingering observation is on
    assert len({o["reward"].tobytes() for o in out}) == len(out)
    _assert_env_equals_plain(dp, V, out, songs, FORCED)


def test_step_equals_plain_handle_ot_reward(dp, V, S):
    augs = [V.MidiTemporalStretch(1.0, 0.5), V.MidiPitchShift(1.0, 3)]
    forced = [(0, 1.2, 1)]
    out, songs = _rollout(dp, S["crossing_field"], augs, forced, disable_fingering_reward=True)
    _assert_env_equals_plain(dp, V, out, songs, forced, disable_fingering_reward=True)


def test_queue_path_is_bitwise_the_monolithic_launch(dp, V, S, monkeypatch):
    init, augs = _guren_case(V, S)
    monkeypatch.setenv("PIANOSIM_CHUNKS", "0")
    mono, _ = _rollout(dp, init, augs, FORCED)
    monkeypatch.setenv("PIANOSIM_CHUNKS", "2")
    monkeypatch.setenv("PIANOSIM_STEP_GRID", "2")  # 4 envs x 2 chunks on 2 workgroups
    sliced, _ = _rollout(dp, init, augs, FORCED)
    for t, (a, b) in enumerate(zip(mono, sliced)):
        for k in a:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"step {t}, {k}")


def test_sharded_handle_draws_its_global_envs(dp, V, S):
    short = dp.music.test_midi(0.05)
    augs = [V.MidiSelect([short, S["twinkle"]]), V.MidiTemporalStretch(1.0, 0.5), V.MidiOctaveShift(1.0, 1)]
    whole = dp.BatchedPianoEnv(16, short, dp.TaskConfig(augmentations=augs), device="cuda:0", seed=SEED)
    shard = dp.BatchedPianoEnv(8, short, dp.TaskConfig(augmentations=augs), device="cuda:0", seed=SEED, env_offset=8)
    for g in (whole, shard):
        g.reset()
        for _ in range(6):
            g.step(torch.zeros(g.num_envs, g.action_dim, device="cuda:0"))
    _check_draws_and_tables(dp, V, shard, SEED, env0=8, min_episode=1)
    a, b = _aug(whole), _aug(shard)
    ta, tb = whole.song_tables(), shard.song_tables()
    for k in a:
        np.testing.assert_array_equal(a[k][8:], b[k], err_msg=k)
    for e in range(8):
        for k in TABLES:
            T = b["T"][e]
            assert torch.equal(ta[k][8 + e, :T], tb[k][e, :T]), (e, k)
    whole.close()
    shard.close()


def test_teacher_forced_step_against_the_checker(dp, V, S, ref):
    """One control step from the reset state on per-env tables against the fp64 checker built
    from the host-augmented SongTables. Tolerances: those of tests/test_gpu_parity.py for a
    Twinkle step - step type, discount, goal and fingering observations exact; reward and reward
    terms within 1e-3; qpos within 1e-4 (its p99 bound there; 2 envs here, so the maximum)."""
    augs = [V.MidiSelect([S["guren"]]), V.MidiTemporalStretch(1.0, 0.5), V.MidiPitchShift(1.0, 3)]
    forced = [(0, 1.25, 2), (1, 0.75, -1)]
    task = dp.TaskConfig(augmentations=augs)
    g = dp.BatchedPianoEnv(2, S["twinkle"], task, device="cuda:0", canonical_actions=False)
    g.reset()
    g.set_augmentation(*(np.array(x) for x in zip(*forced)))
    lo, hi = dp.model.action_spec(g.model_desc)
    rng = np.random.RandomState(3)
    a = rng.uniform(lo, hi, (2, 45)).astype(np.float32)
    og, rg, dg, sg = (x.cpu().numpy() for x in g.step(torch.from_numpy(a).cuda()))
    tg, qg = g.reward_terms().cpu().numpy(), g.get_state()["qpos"].cpu().numpy()
    lay = dp.obs_layout(g.task_cfg)
    for e, draw in enumerate(forced):
        md, st, tc = dp.compile_task(V.apply(g.songs, *draw), dp.TaskConfig(), canonical_actions=False)
        o = ref.OracleEnv(md, st, tc, 2)
        o.reset()
        oo, ro, do, so = o.step(a)
        assert sg[e] == so[e] and dg[e] == do[e]
        np.testing.assert_array_equal(og[e, lay["goal"]], oo[e, lay["goal"]])
        np.testing.assert_array_equal(og[e, lay["fingering"]], oo[e, lay["fingering"]])
        assert og[e, lay["goal"]].sum() > 0
        assert abs(rg[e] - ro[e]) < 1e-3 and np.abs(tg[e] - o.reward_terms()[e]).max() < 1e-3
        assert np.abs(qg[e] - o.get_state()["qpos"][e]).max() < 1e-4
        assert np.abs(og[e] - oo[e]).max() < 1e-3
    g.close()


def test_surfaces(dp, V, S):
    ev = importlib.import_module("diffusion-piano_amd.evaluation")
    augs = [V.MidiTemporalStretch(1.0, 0.3), V.MidiPitchShift(1.0, 2)]
    venv = ev.MidiEvaluationWrapper(dp.VectorizedPianoEnv(8, S["twinkle"], return_numpy=True, seed=SEED,
                                                          augmentations=augs), deque_size=8)
    obs = venv.reset()
    assert obs["goal"].shape == (8, 178) and obs["goal"].dtype == np.float64
    a = _aug(venv.core)
    T = a["T"]
    assert len(set(T)) > 1 and (a["fallbacks"] == 0).all()
    length = np.zeros(8, int)
    act = np.zeros((8, 45), np.float32)
    for t in range(1, int(T.max()) + 1):
        obs, rewards, dones = venv.step(act)
        assert isinstance(rewards, np.ndarray) and np.isfinite(rewards).all()
        length[dones & (length == 0)] = t
    np.testing.assert_array_equal(length, T)  # every env's episode is as long as its own song
    m = venv.get_musical_metrics()
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in m.values())
    with pytest.raises(dp.PianosimError):
        dp.BatchedPianoEnv(2, S["twinkle"], dp.TaskConfig(augmentations=augs, augmentation_max_bytes=1000),
                           device="cuda:0")
    with pytest.raises(ValueError):  # Crossing Field has no fingering, Twinkle has
        dp.BatchedPianoEnv(2, S["twinkle"], dp.TaskConfig(augmentations=[V.MidiSelect([S["crossing_field"]])]),
                           device="cuda:0")
    with pytest.raises(dp.PianosimError):
        dp.BatchedPianoEnv(2, S["twinkle"], device="cuda:0").augmentation()
