"""The MIDI recorder on the device (ps_record_midi: the step kernel's per-substep capture and
midi_events_kernel, csrc/midi_events.inc) against its specification,
music.events_from_activations, which tests/test_midi_record.py holds to the reference's
MidiModule.

1 compaction alone, through ps_midi_push, on the fixture's sequences (all 88 keys and the pedal
  in one substep included) in slices of 1, 3 and 10 rows, and into banks too small;
2 known-answer physics: keys pushed by an applied force, the expected events from the fp64
  checker stepped substep by substep (its margin to the activation boundary asserted first);
3 after every step of a random-action rollout the notes sounding by the events are the keys
  active in the state the library returns; monolithic and time-sliced legs agree bitwise;
4 a recording handle returns bitwise what a plain one does;
5 episodes and the two banks, also where LAST steps and auto-resets run on the time-sliced step;
6 the refusals."""
import importlib

import numpy as np
import pytest

import helpers

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _snapshot(env, which="current"):
    ev = env.midi_events(which)
    torch.cuda.synchronize()
    return {k: (_words(v) if k == "events" else v.cpu().numpy()) for k, v in ev.items()}


def _queue(monkeypatch, chunks, grid):
    """The forced time-sliced step, as tests/test_gpu_chunked.py forces it (read at create)."""
    if chunks is None:
        monkeypatch.delenv("PIANOSIM_CHUNKS", raising=False)
        monkeypatch.delenv("PIANOSIM_STEP_GRID", raising=False)
    else:
        monkeypatch.setenv("PIANOSIM_CHUNKS", str(chunks))
        monkeypatch.setenv("PIANOSIM_STEP_GRID", str(grid))


# ------------------------------------------------------------------ 1 compaction
def _fixture_rows(golden):
    """Three envs' activation sequences, padded to one length by holding the last row (no event)."""
    seqs = golden["midi_module"]["sequences"]

    def arrays(*names):
        act = np.concatenate([np.array([[k in s for k in range(88)] for s in map(set, seqs[n]["active_keys"])], bool)
                              .reshape(-1, 88) for n in names])
        return act, np.concatenate([np.array(seqs[n]["sustain"], bool) for n in names])

    envs = [arrays("dense"), arrays("sparse"), arrays("all_switch", "silent", "word_edges")]
    S = max(len(a) for a, _ in envs)
    return [(np.concatenate([a, np.repeat(a[-1:], S - len(a), 0)]), np.concatenate([s, np.repeat(s[-1:], S - len(s))]))
            for a, s in envs], S


@pytest.fixture(scope="module")
def push_env(dp):
    env = dp.BatchedPianoEnv(3, dp.music.twinkle_twinkle_little_star_one_hand(), dp.TaskConfig(), device=DEV)
    yield env
    env.close()


def _push_all(dp, env, envs, S, k):
    bits = np.stack([dp.music.pack_activations(a, s) for a, s in envs])  # [3, S, 3]
    for i in range(0, S, k):
        env.midi_push(torch.from_numpy(np.ascontiguousarray(bits[:, i:i + k]).view(np.int32)).to(DEV))


@pytest.mark.parametrize("k", [1, 3, 10])
def test_compaction_is_the_specification(dp, golden, push_env, k):
    envs, S = _fixture_rows(golden)
    push_env.record_midi(0)
    push_env.record_midi(2048)
    _push_all(dp, push_env, envs, S, k)
    got = _snapshot(push_env)
    for e, (a, s) in enumerate(envs):
        want = dp.music.events_from_activations(a, s, 0.005, words=True)
        assert got["count"][e] == len(want) and got["dropped"][e] == 0 and got["substeps"][e] == S
        np.testing.assert_array_equal(got["events"][e, :len(want)], want, err_msg=f"env {e}, slices of {k}")
        assert not got["events"][e, len(want):].any()
    assert got["count"][0] > 1000 and got["count"][2] >= 2 * 89  # (the dense and the all-at-once sequences)
    prev = _snapshot(push_env, "previous")
    assert not prev["count"].any() and not prev["events"].any() and not prev["substeps"].any()


def _gather_guarded(env, which, M):
    """ps_midi_events into arrays with a guard row behind them (it must stay as it is)."""
    guard = -1515870811  # 0xA5A5A5A5
    ev = torch.full((4, M), guard, dtype=torch.int32, device=DEV)
    cnt, drp, sub = (torch.full((4,), guard, dtype=torch.int32, device=DEV) for _ in range(3))
    lib = importlib.import_module("diffusion-piano_amd._lib")
    lib.check(lib.load().ps_midi_events(env._h, which, ev.data_ptr(), cnt.data_ptr(), drp.data_ptr(), sub.data_ptr(),
                                        env.stream))
    torch.cuda.synchronize()
    for t in (ev, cnt, drp, sub):
        assert (t[3] == guard).all()
    return _words(ev)[:3], cnt.cpu().numpy()[:3], drp.cpu().numpy()[:3], sub.cpu().numpy()[:3]


def test_a_full_bank_drops_and_writes_nothing_past_it(dp, golden, push_env):
    """Banks of 100 events. The memory behind a full bank is made observable: the banks lie as
    [env][bank][100], so what follows env e's bank 0 is its bank 1, and what follows its bank 1 is
    env e + 1's bank 0. Both are overflowed while the bank behind holds a finished episode - known
    words that ps_midi_events returns (count > 0) - and those must stay as they were."""
    envs, S = _fixture_rows(golden)
    M = 100
    spec = [dp.music.events_from_activations(a, s, 0.005, words=True) for a, s in envs]
    assert len(spec[0]) > 1000 + M and min(len(w) for w in spec) > M  # every env overflows

    def overflow_and_check(what):
        _push_all(dp, push_env, envs, S, 10)
        words, cnt, drp, sub = _gather_guarded(push_env, 0, M)
        for e in range(3):
            assert cnt[e] == M and drp[e] == len(spec[e]) - M and sub[e] == S, what
            np.testing.assert_array_equal(words[e], spec[e][:M], err_msg=f"{what}, env {e}")
        return words

    push_env.record_midi(0)
    push_env.record_midi(M)
    # a short finished episode in bank 0 of every env: env e holds e + 1 NoteOns, then a reset
    first = np.zeros((3, 1, 88), bool)
    for e in range(3):
        first[e, 0, [5 + e, 40, 87][:e + 1]] = True
    push_env.midi_push(torch.from_numpy(np.stack([dp.music.pack_activations(a, [False]) for a in first])
                                        .view(np.int32)).to(DEV))
    short = [dp.music.events_from_activations(a, [False], 0.005, words=True) for a in first]
    push_env.reset()

    def previous_is(want, what, full=False):
        words, cnt, drp, sub = _gather_guarded(push_env, 1, M)
        for e in range(3):
            assert cnt[e] == len(want[e]) > 0 and drp[e] == (len(spec[e]) - M if full else 0), what
            np.testing.assert_array_equal(words[e, :cnt[e]], want[e], err_msg=f"{what}, env {e}")

    previous_is(short, "before the overflow")
    # bank 1 runs and overflows: behind env e's bank 1 lies env e + 1's bank 0, the short episodes
    kept = overflow_and_check("bank 1 running")
    previous_is(short, "behind the overflowed bank 1")
    # swap again: bank 0 runs and overflows, and behind it lies the same env's full bank 1
    push_env.reset()
    previous_is(list(kept), "after the second reset", full=True)
    overflow_and_check("bank 0 running")
    previous_is(list(kept), "behind the overflowed bank 0", full=True)


# ------------------------------------------------------------------ 2 known-answer physics
PUSHED = [0, 1, 30, 31, 39, 40, 63, 64, 65, 87]
_KNOWN = {}


def _applied():
    f = np.zeros((4, 140), np.float32)
    for i, scale in enumerate([0.5, 1.0, 2.0, 3.0]):
        for j, k in enumerate(PUSHED):
            f[i, k] = scale * (1 + 0.13 * j)
    return f


def _checker_events(dp, ref):
    """The fp64 checker stepped by physics_substep() with the same force: (event words per env,
    smallest distance of any key from the activation boundary over the 60 substeps)."""
    if "checker" not in _KNOWN:
        song = dp.music.twinkle_twinkle_little_star_one_hand()
        md, st, tc = dp.compile_task(song, dp.TaskConfig(), canonical_actions=False)
        assert md.n_substeps == 10
        o = ref.OracleEnv(md, st, tc, 4)
        o.reset()
        rng_ = np.array(md.key_range, np.float64).reshape(88, 2)
        act, margin = [], np.inf
        for phase in (_applied().astype(np.float64), None):
            o.set_applied(phase)
            for _ in range(30):
                o.physics_substep()
                q = o.get_state()["qpos"][:, :88]
                d = np.abs(np.clip(q, rng_[:, 0], rng_[:, 1]) - rng_[:, 1])
                margin = min(margin, float(np.abs(d - dp.abi.KEY_THRESHOLD).min()))
                act.append(d <= dp.abi.KEY_THRESHOLD)
        act = np.array(act)  # [60, 4, 88]
        words = [dp.music.events_from_activations(act[:, i], np.zeros(60, bool), md.timestep, words=True) for i in range(4)]
        _KNOWN["checker"] = (words, margin)
    return _KNOWN["checker"]


def test_known_answer_margin(dp, ref):
    """From the checker alone: no key comes nearer than 1e-4 rad (the teacher-forced parity
    ceiling) to the activation boundary, the NoteOns fall inside the first control step and the
    NoteOffs inside the fourth (they cross chunk boundaries of the time-sliced leg)."""
    words, margin = _checker_events(dp, ref)
    print(f"known-answer scenario: smallest distance from the activation boundary {margin:.3e} rad")
    assert margin >= 1e-4
    for w in words:
        note, kind, ordinal = dp.music.event_fields(w)
        assert sorted(note[kind == 0] - 21) == PUSHED and sorted(note[kind == 1] - 21) == PUSHED and len(w) == 20
        assert ordinal[kind == 0].min() >= 1 and ordinal[kind == 0].max() <= 10
        assert ordinal[kind == 1].min() >= 31 and ordinal[kind == 1].max() <= 40


@pytest.mark.parametrize("sliced", [False, True], ids=["monolithic", "queue_6_chunks"])
def test_known_answer_physics(dp, ref, monkeypatch, sliced):
    want, margin = _checker_events(dp, ref)
    assert margin >= 1e-4
    _queue(monkeypatch, 6 if sliced else None, 2)
    env = dp.BatchedPianoEnv(4, dp.music.twinkle_twinkle_little_star_one_hand(), dp.TaskConfig(), device=DEV,
                             canonical_actions=False)
    env.record_midi()
    env.reset()
    zero = torch.zeros(4, env.action_dim, device=DEV)
    env.set_applied(_applied())
    contacts = 0
    for t in range(6):
        if t == 3:
            env.set_applied(None)
        env.step(zero)
        contacts += int(env.contact_count().sum())
    got = _snapshot(env)
    assert contacts == 0  # no hand contact after any of the six steps
    env.close()
    for i in range(4):
        assert got["count"][i] == len(want[i]) and got["dropped"][i] == 0 and got["substeps"][i] == 60
        np.testing.assert_array_equal(got["events"][i, :len(want[i])], want[i], err_msg=f"env {i}")


# ------------------------------------------------------------------ 3, 4 rollouts
STEPS = 30
LEGS = {"monolithic64": (64, None, None), "queue96": (96, 6, 16)}
_ROLL = {}


def _rollout(dp, monkeypatch, leg, record):
    """30 random-action steps of Crossing Field (computed once per leg and kind, shared, never
    modified): per step the outputs and state and, recording, the running episode's events."""
    key = (leg, record)
    if key in _ROLL:
        return _ROLL[key]
    n, chunks, grid = LEGS[leg]
    _queue(monkeypatch, chunks, grid)
    env = dp.BatchedPianoEnv(n, helpers.song(dp, "crossing_field"), dp.TaskConfig(trim_silence=True), device=DEV, seed=7)
    if record:
        env.record_midi()
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2024)
    out = []
    for t in range(STEPS):
        a = (torch.rand(96, env.action_dim, device=DEV, generator=gen) * 2 - 1)[:n]
        o, r, d, s = env.step(a)
        st = env.get_state()
        rec = dict(obs=o, reward=r, discount=d, step_type=s, **st)
        if record:
            rec.update({"midi_" + k: v for k, v in env.midi_events().items()})
        out.append({k: v.cpu().numpy().copy() for k, v in rec.items()})
    _ROLL[key] = (out, np.array(env.model_desc.key_range, np.float32).reshape(88, 2))
    env.close()
    return _ROLL[key]


def _check_against_state(dp, out, key_range, n):
    """Replays every env's running episode step by step: the notes sounding by the events are
    the keys active in the returned state (key_state2's rule in fp32), likewise the pedal; an
    env's auto-reset step (FIRST) starts an empty episode and moves the one it had, as it was,
    to "previous" (where the rollout kept it). Returns (events seen, finished episodes with events)."""
    sounding, pedal = np.zeros((n, 88), bool), np.zeros(n, bool)
    seen, sub, total, finished = np.zeros(n, int), np.zeros(n, int), 0, 0
    lo, hi, thr = key_range[:, 0], key_range[:, 1], np.float32(dp.abi.KEY_THRESHOLD)
    for t, o in enumerate(out):
        assert not o["midi_dropped"].any()
        words = o["midi_events"].view(np.uint32)
        for e in range(n):
            if o["step_type"][e] == dp.abi.FIRST:
                assert o["midi_count"][e] == 0, f"step {t} env {e}: events in a new episode"
                sounding[e], pedal[e], seen[e], sub[e] = False, False, 0, 0
                if t and "midi_prev_events" in o:
                    for k in ("events", "count", "dropped", "substeps"):
                        np.testing.assert_array_equal(o["midi_prev_" + k][e], out[t - 1]["midi_" + k][e],
                                                      err_msg=f"step {t} env {e}: previous {k}")
                    finished += int(o["midi_prev_count"][e] > 0)
            else:
                sub[e] += 10
            note, kind, ordinal = dp.music.event_fields(words[e, seen[e]:o["midi_count"][e]])
            assert ((ordinal > sub[e] - 10) & (ordinal <= sub[e])).all(), f"step {t} env {e}: ordinals"
            for p, k in zip(note, kind):
                if k < 2:
                    assert sounding[e, p - 21] == (k == 1), f"step {t} env {e}: a repeated NoteOn / NoteOff"
                    sounding[e, p - 21] = k == 0
                else:
                    assert pedal[e] == (k == 3)
                    pedal[e] = k == 2
            total += o["midi_count"][e] - seen[e]
            seen[e] = o["midi_count"][e]
        np.testing.assert_array_equal(o["midi_substeps"], sub, err_msg=f"step {t}")
        q = o["qpos"][:, :88].astype(np.float32)
        active = np.abs(np.clip(q, lo, hi) - hi) <= thr  # key_state2's rule, in fp32
        np.testing.assert_array_equal(sounding, active, err_msg=f"step {t}")
        np.testing.assert_array_equal(pedal, o["sustain"] >= np.float32(dp.abi.SUSTAIN_THRESHOLD), err_msg=f"step {t}")
    return int(total), finished


@pytest.mark.parametrize("leg", list(LEGS))
def test_events_agree_with_the_returned_state(dp, monkeypatch, leg):
    out, key_range = _rollout(dp, monkeypatch, leg, True)
    n = LEGS[leg][0]
    total, _ = _check_against_state(dp, out, key_range, n)
    assert total == int(out[-1]["midi_count"].sum())
    print(f"{leg}: {total} events, {int((out[-1]['midi_count'] > 0).sum())} of {n} envs played")
    assert total > 0, "the rollout pressed no key: nothing was checked"


# episodes that end inside the window, on the monolithic and on the time-sliced step: a 9-step
# song with the episodes staggered as bench.py does (tests/test_gpu_chunked.py's shape: 40 envs
# on 8 workgroups, 3 chunks), so LAST steps and auto-resets of a recording handle run on
# pianosim_queue_kernel too
SHORT_N, SHORT_STEPS = 40, 24
_SHORT = {}


def _short_rollout(dp, monkeypatch, chunks):
    if chunks in _SHORT:
        return _SHORT[chunks]
    m = dp.music
    seq = m.NoteSequence(title="short")
    for p, s, e in [(60, 0.0, 0.15), (64, 0.05, 0.2), (67, 0.1, 0.3), (48, 0.15, 0.4), (72, 0.25, 0.4)]:
        seq.notes.append(m.Note(p, s, e, 80, 0))
    seq.total_time = 0.4
    _queue(monkeypatch, chunks, 8)
    env = dp.BatchedPianoEnv(SHORT_N, seq, dp.TaskConfig(), device=DEV, seed=9)
    T = env.song.T
    assert 4 <= T <= 12, T
    env.record_midi()
    env.reset()
    env.set_state({"t_idx": (np.arange(SHORT_N) % T).astype(np.int32)})  # bench.py stagger_episodes
    gen = torch.Generator(device=DEV).manual_seed(31)
    out = []
    for t in range(SHORT_STEPS):
        o, r, d, s = env.step(torch.rand(SHORT_N, env.action_dim, device=DEV, generator=gen) * 2 - 1)
        rec = dict(obs=o, reward=r, step_type=s, **env.get_state())
        rec.update({"midi_" + k: v for k, v in env.midi_events().items()})
        rec.update({"midi_prev_" + k: v for k, v in env.midi_events("previous").items()})
        out.append({k: v.cpu().numpy().copy() for k, v in rec.items()})
    _SHORT[chunks] = (out, np.array(env.model_desc.key_range, np.float32).reshape(88, 2))
    env.close()
    return _SHORT[chunks]


@pytest.mark.parametrize("chunks", [0, 3], ids=["monolithic", "queue_3_chunks"])
def test_episode_ends_and_auto_resets(dp, monkeypatch, chunks):
    out, key_range = _short_rollout(dp, monkeypatch, chunks)
    kinds = np.stack([o["step_type"] for o in out])
    assert ((kinds == dp.abi.LAST).sum(0) >= 2).all() and ((kinds == dp.abi.FIRST).sum(0) >= 2).all()
    total, finished = _check_against_state(dp, out, key_range, SHORT_N)
    print(f"short song, chunks {chunks}: {total} events, {finished} finished episodes with events")
    assert total > 0 and finished > 0, "no key pressed / no played episode finished: nothing was checked"


def test_time_sliced_resets_record_what_the_monolithic_step_records(dp, monkeypatch):
    a, _ = _short_rollout(dp, monkeypatch, 0)
    b, _ = _short_rollout(dp, monkeypatch, 3)
    for t in range(SHORT_STEPS):
        for k in a[t]:
            x, y = a[t][k], b[t][k]
            np.testing.assert_array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                                          y.view(np.int32) if y.dtype == np.float32 else y, err_msg=f"step {t}, {k}")


def test_legs_record_the_same_events(dp, monkeypatch):
    a, _ = _rollout(dp, monkeypatch, "monolithic64", True)
    b, _ = _rollout(dp, monkeypatch, "queue96", True)
    for t in range(STEPS):
        for k in ("midi_events", "midi_count", "midi_dropped", "midi_substeps"):
            np.testing.assert_array_equal(a[t][k], b[t][k][:64], err_msg=f"step {t}, {k}")


@pytest.mark.parametrize("leg", list(LEGS))
def test_recording_changes_nothing_else(dp, monkeypatch, leg):
    rec, _ = _rollout(dp, monkeypatch, leg, True)
    plain, _ = _rollout(dp, monkeypatch, leg, False)
    for t in range(20):
        for k in plain[t]:
            a, b = plain[t][k], rec[t][k]
            np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                          b.view(np.int32) if b.dtype == np.float32 else b, err_msg=f"step {t}, {k}")


# ------------------------------------------------------------------ 5 episodes and banks
def test_episodes_and_banks(dp, tmp_path):
    m = dp.music
    env = dp.BatchedPianoEnv(2, m.test_midi(0.01), dp.TaskConfig(control_timestep=0.01), device=DEV,
                             canonical_actions=False)
    assert env.song.T == 4 and env.model_desc.n_substeps == 2
    env.record_midi(64)
    env.reset()
    force = np.zeros((2, 140), np.float32)
    force[:, 40] = 3.0
    env.set_applied(force)
    zero = torch.zeros(2, env.action_dim, device=DEV)
    for t in range(4):
        _, _, _, st = env.step(zero)
    assert (st.cpu().numpy() == dp.abi.LAST).all()
    done = _snapshot(env)
    assert (done["count"] >= 1).all() and (done["substeps"] == 8).all()
    note, kind, ordinal = m.event_fields(done["events"][0, :done["count"][0]])
    assert (note[0], kind[0]) == (61, 0) and 1 <= ordinal[0] <= 8
    # the auto-reset: the finished episode moves to "previous", the running one is empty
    _, _, _, st = env.step(zero)
    assert (st.cpu().numpy() == dp.abi.FIRST).all()
    prev, cur = _snapshot(env, "previous"), _snapshot(env)
    for k in done:
        np.testing.assert_array_equal(prev[k], done[k], err_msg=k)
    assert not cur["count"].any() and not cur["substeps"].any() and not cur["events"].any()
    # the finished performance as a file
    seq = env.performance(0, "previous")
    msgs = env.midi_messages(0, "previous")
    assert len(msgs) == done["count"][0] and isinstance(msgs[0], m.NoteOn) and msgs[0].time == ordinal[0] * 0.005
    assert seq.total_time == 8 * 0.005 and len(seq.notes) == int((kind == 0).sum()) >= 1
    m.write_midi(seq, tmp_path / "episode.mid")
    back = m.parse_midi(tmp_path / "episode.mid")
    key = lambda x: (x.start_time, x.pitch)
    for a, b in zip(sorted(seq.notes, key=key), sorted(back.notes, key=key)):
        assert (a.pitch, a.velocity) == (b.pitch, b.velocity) == (61, 127)
        assert abs(a.start_time - b.start_time) <= 1e-9 and abs(a.end_time - b.end_time) <= 1e-9
    assert len(back.notes) == len(seq.notes)
    # a new episode under way, then a masked reset that leaves env 1 out
    env.step(zero)
    env.step(zero)
    before = _snapshot(env)
    assert (before["count"] >= 1).all() and (before["substeps"] == 4).all()
    before_prev = _snapshot(env, "previous")
    env.reset(mask=[1, 0])
    after, after_prev = _snapshot(env), _snapshot(env, "previous")
    for k in before:
        np.testing.assert_array_equal(after[k][1], before[k][1], err_msg=k)
        np.testing.assert_array_equal(after_prev[k][1], before_prev[k][1], err_msg=k)
        np.testing.assert_array_equal(after_prev[k][0], before[k][0], err_msg=k)
    assert after["count"][0] == 0 and after["substeps"][0] == 0
    # ... and a launch that skips an env adds nothing to it
    env.reset(mask=[0, 0])
    again = _snapshot(env)
    for k in after:
        np.testing.assert_array_equal(again[k], after[k], err_msg=k)
    env.close()


# ------------------------------------------------------------------ 6 refusals
def test_refusals(dp):
    lib = importlib.import_module("diffusion-piano_amd._lib")
    song = dp.music.twinkle_twinkle_little_star_one_hand()
    env = dp.BatchedPianoEnv(4, song, dp.TaskConfig(), device=DEV, seed=3)
    plain = dp.BatchedPianoEnv(4, song, dp.TaskConfig(), device=DEV, seed=3)
    with pytest.raises(lib.PianosimError, match="recording is off"):
        env.midi_events()
    with pytest.raises(lib.PianosimError, match="recording is off"):
        env.midi_push(torch.zeros(4, 1, 3, dtype=torch.int32, device=DEV))
    with pytest.raises(lib.PianosimError, match=r"needs \d+ B \(4 envs x \(2 banks x 2048 events"):
        env.record_midi(2048, max_bytes=1000)
    with pytest.raises(lib.PianosimError, match="max_events"):
        env.record_midi(-1)
    env.record_midi(16)
    with pytest.raises(lib.PianosimError, match="over the budget"):
        env.record_midi(2048, max_bytes=1000)  # refused: the handle goes on recording as it was
    assert env.midi_events()["events"].shape == (4, 16)
    with pytest.raises(lib.PianosimError, match=r"11 rows; one push takes 1 \.\. 10"):
        env.midi_push(torch.zeros(4, 11, 3, dtype=torch.int32, device=DEV))
    assert lib.load().ps_midi_push(env._h, torch.zeros(4, 1, 3, dtype=torch.int32, device=DEV).data_ptr(), 0, None) < 0
    assert b"0 rows" in lib.load().ps_last_error()
    with pytest.raises(ValueError):
        env.midi_events("next")
    assert lib.load().ps_midi_events(env._h, 2, None, None, None, None, None) < 0
    assert b"which" in lib.load().ps_last_error()
    assert lib.load().ps_midi_push(env._h, None, 1, None) < 0
    env.reset()
    plain.reset()
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = torch.rand(4, env.action_dim, device=DEV, generator=gen) * 2 - 1
    env.step(a)
    plain.step(a)
    assert (_snapshot(env)["substeps"] == 10).all()
    env.record_midi(0)  # off: the handle steps as a plain one
    with pytest.raises(lib.PianosimError, match="recording is off"):
        env.midi_events()
    for _ in range(2):
        o, r, _, _ = env.step(a)
        po, pr, _, _ = plain.step(a)
    torch.cuda.synchronize()
    assert torch.equal(o, po) and torch.equal(r, pr)
    assert torch.equal(env.get_state()["qpos"], plain.get_state()["qpos"])
    env.close()
    plain.close()
