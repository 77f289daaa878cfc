"""The item loop of the time-sliced step (csrc/kernel_v2.inc pianosim_queue_kernel) taken many
times by one workgroup: 64 envs x 3 chunks on a grid of 8 workgroups, so every workgroup runs
about 24 (env, chunk) items back to back and what one trip leaves in registers meets the next
trip's env. The loop rebuilds everything the step body receives from an opaque pointer to the
kernel arguments at the top of every trip; a value wrongly carried from one item to the next
would show here as a difference from the monolithic kernel (PIANOSIM_CHUNKS=0, same library,
same seed, same handle inputs). Both switches (PIANOSIM_CHUNKS, PIANOSIM_STEP_GRID) are read
when the handle is created.

3 steps of a 9-step song with the episodes staggered as bench.py does: envs with t_idx = T - 1
end their episode on the first step and auto-reset on the second."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, STEPS, GRID, CHUNKS = 64, 3, 8, 3
HANDS = {"hull": False, "capsule": None}  # TaskConfig.primitive_fingertip_collisions
KEYS = ("obs", "reward", "discount", "step_type", "qpos", "qvel")


def _short_song(dp):
    m = dp.music
    seq = m.NoteSequence(title="queue loop test")
    for p, s, e in [(60, 0.0, 0.15), (64, 0.05, 0.2), (67, 0.1, 0.3), (48, 0.15, 0.4), (72, 0.25, 0.4)]:
        seq.notes.append(m.Note(p, s, e, 80, 0))
    seq.total_time = 0.4
    return seq


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _rollout(dp, monkeypatch, hand, chunks, grid):
    monkeypatch.setenv("PIANOSIM_CHUNKS", str(chunks))
    if grid is None:
        monkeypatch.delenv("PIANOSIM_STEP_GRID", raising=False)
    else:
        monkeypatch.setenv("PIANOSIM_STEP_GRID", str(grid))
    task = dp.TaskConfig(primitive_fingertip_collisions=HANDS[hand])
    g = dp.BatchedPianoEnv(N, _short_song(dp), task, device="cuda:0")
    T = g.song.T
    assert 4 <= T <= N, T
    g.reset()
    g.set_state({"t_idx": (np.arange(N) % T).astype(np.int32)})  # bench.py stagger_episodes
    gen = torch.Generator(device="cuda:0").manual_seed(23)
    out = []
    for _ in range(STEPS):
        o, r, d, s = g.step(torch.rand(N, g.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        st = g.get_state()
        row = dict(obs=o, reward=r, discount=d, step_type=s, qpos=st["qpos"], qvel=st["qvel"])
        out.append({k: v.cpu().numpy().copy() for k, v in row.items()})
    stats = g.solver_stats().cpu().numpy().copy()
    g.close()
    return out, stats


@pytest.mark.parametrize("hand", list(HANDS))
def test_many_items_per_workgroup_are_bitwise_the_monolithic_step(dp, monkeypatch, hand):
    ref, ref_stats = _rollout(dp, monkeypatch, hand, 0, None)
    kinds = np.stack([o["step_type"] for o in ref])
    assert (kinds[1:] == 0).any(), "no env auto-reset inside the window"
    assert (kinds == 2).any(), "no terminal step inside the window"
    assert ref_stats[:, 3].max() > 0, "no constraint rows: the solve was not exercised"
    got, _ = _rollout(dp, monkeypatch, hand, CHUNKS, GRID)
    for t, (a, b) in enumerate(zip(ref, got)):
        for k in KEYS:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{hand}: step {t}, {k}")
