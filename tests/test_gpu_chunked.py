"""The time-sliced step (csrc/kernel_v2.inc pianosim_queue_kernel): a launch of more envs than
resident wave slots runs each env-step as chunks of substeps that workgroups take off an
in-launch FIFO, the state live across a substep boundary handed over in the env's park row.
Every output must be bitwise the monolithic kernel's (PIANOSIM_CHUNKS=0, same library, same
seed), whatever the chunk count, the grid (PIANOSIM_STEP_GRID) or the order the items are
popped in. Both switches are read when the handle is created.

Shapes: 40 envs on 8 workgroups (every workgroup runs several envs, continuations change
workgroups), on 7 (40 x 3 items: the last pass is partial) and on the default grid; 2, 3 and 10
chunks of the 10 substeps; a 9-step song with the episodes staggered as bench.py does, so
auto-resets and terminal steps fall inside the 12-step window."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, STEPS = 40, 12
HANDS = {"hull": False, "capsule": None}  # TaskConfig.primitive_fingertip_collisions


def _short_song(dp):
    m = dp.music
    seq = m.NoteSequence(title="chunk test")
    for p, s, e in [(60, 0.0, 0.15), (64, 0.05, 0.2), (67, 0.1, 0.3), (48, 0.15, 0.4), (72, 0.25, 0.4)]:
        seq.notes.append(m.Note(p, s, e, 80, 0))
    seq.total_time = 0.4
    return seq


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _rollout(dp, monkeypatch, hand, chunks, grid=None, poison=False):
    monkeypatch.setenv("PIANOSIM_CHUNKS", str(chunks))
    if grid is None:
        monkeypatch.delenv("PIANOSIM_STEP_GRID", raising=False)
    else:
        monkeypatch.setenv("PIANOSIM_STEP_GRID", str(grid))
    task = dp.TaskConfig(primitive_fingertip_collisions=HANDS[hand])
    g = dp.BatchedPianoEnv(N, _short_song(dp), task, device="cuda:0")
    T = g.song.T
    assert 4 <= T <= STEPS, T
    g.reset()
    g.set_state({"t_idx": (np.arange(N) % T).astype(np.int32)})  # bench.py stagger_episodes
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    if poison:  # an applied force on every dof: the reset of the poisoned env has a row to clear
        g.set_applied((torch.rand(N, 140, device="cuda:0", generator=gen) - 0.5) * 1e-3)
    out = []
    for t in range(STEPS):
        a = torch.rand(N, g.action_dim, device="cuda:0", generator=gen) * 2 - 1
        if poison and t in (1, 2, 7):
            a[17, 3] = float("nan")  # mj_checkAcc: PS_RESET_PHYSICS in the step's first substep
        o, r, d, s = g.step(a)
        st = g.get_state()
        out.append(dict(obs=o, reward=r, discount=d, step_type=s, qpos=st["qpos"], qvel=st["qvel"],
                        qacc_warmstart=st["qacc_ws"], ctrl=st["ctrl"], t_idx=st["t_idx"], last=st["last"],
                        stats=g.solver_stats(), warnings=g.warnings()))
        out[-1] = {k: v.cpu().numpy().copy() for k, v in out[-1].items()}
    g.close()
    return out


_REF = {}


def _reference(dp, monkeypatch, hand, poison):
    """The monolithic rollout (computed once per hand and kind, shared, never modified)."""
    key = (hand, poison)
    if key not in _REF:
        ref = _rollout(dp, monkeypatch, hand, 0, poison=poison)
        kinds = np.concatenate([o["step_type"] for o in ref])
        assert (kinds == 0).any() and (kinds == 2).any(), "no auto-reset / terminal step in the window"
        assert max(o["stats"][:, 3].max() for o in ref) > 0, "no constraint rows: the solve was not exercised"
        if poison:
            assert ref[-1]["warnings"][17].sum() >= 2 and np.delete(ref[-1]["warnings"], 17, 0).sum() == 0
        _REF[key] = ref
    return _REF[key]


def _assert_bitwise(ref, got, what):
    for t, (a, b) in enumerate(zip(ref, got)):
        for k in a:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: step {t}, {k}")


@pytest.mark.parametrize("grid", [8, None], ids=["grid8", "default_grid"])
@pytest.mark.parametrize("chunks", [2, 3, 10])
@pytest.mark.parametrize("hand", list(HANDS))
def test_time_sliced_step_is_bitwise_the_monolithic_step(dp, monkeypatch, hand, chunks, grid):
    ref = _reference(dp, monkeypatch, hand, False)
    got = _rollout(dp, monkeypatch, hand, chunks, grid)
    _assert_bitwise(ref, got, f"{hand}, {chunks} chunks, grid {grid}")


@pytest.mark.parametrize("chunks", [3, 10])
@pytest.mark.parametrize("hand", list(HANDS))
def test_physics_reset_is_carried_across_chunks(dp, monkeypatch, hand, chunks):
    """A NaN in one env's action row: mj_checkAcc resets that env's physics in the first substep
    (ctrl and qfrc_applied stay cleared for the rest of the step, the warning is counted once):
    the chunks after it must see the cleared state."""
    ref = _reference(dp, monkeypatch, hand, True)
    got = _rollout(dp, monkeypatch, hand, chunks, 8, poison=True)
    _assert_bitwise(ref, got, f"{hand}, {chunks} chunks, poisoned env")


@pytest.mark.parametrize("hand", list(HANDS))
def test_partial_last_pass(dp, monkeypatch, hand):
    """7 workgroups for 40 x 3 items: the grid does not divide the item count."""
    ref = _reference(dp, monkeypatch, hand, False)
    got = _rollout(dp, monkeypatch, hand, 3, 7)
    _assert_bitwise(ref, got, f"{hand}, 3 chunks, grid 7")
