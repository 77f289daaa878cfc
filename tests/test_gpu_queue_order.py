"""The time-sliced step's dispatch by slots known in advance (csrc/kernel_v2.inc
pianosim_queue_kernel): item (chunk c, rank r) lives at queue[c * n + r], tickets walk round 0
in rank order, round 1 in rank order, ...; a ticket that meets an unpublished slot leaves it to
its publisher and takes the next one. Who runs which chunk, and when, must not show in any
output: every case is compared bitwise with the monolithic kernel (PIANOSIM_CHUNKS=0, same
library, same seed, same handle inputs) over 3 steps, for both hands.

The construction is tests/test_gpu_queue_loop.py's: a 9-step song with the episodes staggered
as bench.py does, so in every launch some envs are due for their auto-reset (one chunk only:
their later slots are never published) and the others are not."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 3
HANDS = {"hull": False, "capsule": None}  # TaskConfig.primitive_fingertip_collisions
KEYS = ("obs", "reward", "discount", "step_type", "qpos", "qvel", "stats")
# (envs, chunks, workgroups, PIANOSIM_NO_ORDER)
CASES = {
    "items_cross_workgroups": (64, 3, 8, False),      # many tickets per workgroup
    "one_workgroup_drains_all": (64, 3, 1, False),    # every continuation is self-run
    "grid_is_the_env_count": (64, 3, 64, False),      # next-round slots mostly unpublished when reached
    "ten_chunks": (64, 10, 8, False),
    "unsorted": (64, 3, 8, True),
    "some_envs_due_for_reset": (64, 3, 16, False),    # (asserted below for every 64-env case)
    "odd_sizes": (5, 3, 4, False),
}


def _short_song(dp):
    m = dp.music
    seq = m.NoteSequence(title="queue order test")
    for p, s, e in [(60, 0.0, 0.15), (64, 0.05, 0.2), (67, 0.1, 0.3), (48, 0.15, 0.4), (72, 0.25, 0.4)]:
        seq.notes.append(m.Note(p, s, e, 80, 0))
    seq.total_time = 0.4
    return seq


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _rollout(dp, monkeypatch, hand, n, chunks, grid, no_order):
    monkeypatch.setenv("PIANOSIM_CHUNKS", str(chunks))
    if grid is None:
        monkeypatch.delenv("PIANOSIM_STEP_GRID", raising=False)
    else:
        monkeypatch.setenv("PIANOSIM_STEP_GRID", str(grid))
    if no_order:
        monkeypatch.setenv("PIANOSIM_NO_ORDER", "1")
    else:
        monkeypatch.delenv("PIANOSIM_NO_ORDER", raising=False)
    task = dp.TaskConfig(primitive_fingertip_collisions=HANDS[hand])
    g = dp.BatchedPianoEnv(n, _short_song(dp), task, device="cuda:0")
    T = g.song.T
    assert T >= 4, T
    g.reset()
    g.set_state({"t_idx": (np.arange(n) % T).astype(np.int32)})  # bench.py stagger_episodes
    gen = torch.Generator(device="cuda:0").manual_seed(23)
    out = []
    for _ in range(STEPS):
        o, r, d, s = g.step(torch.rand(n, g.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        st = g.get_state()
        row = dict(obs=o, reward=r, discount=d, step_type=s, qpos=st["qpos"], qvel=st["qvel"], stats=g.solver_stats())
        out.append({k: v.cpu().numpy().copy() for k, v in row.items()})
    g.close()
    return out


_REF = {}


def _reference(dp, monkeypatch, hand, n):
    """The monolithic rollout of (hand, n), computed once and shared by the cases."""
    if (hand, n) not in _REF:
        ref = _rollout(dp, monkeypatch, hand, n, 0, None, False)
        for o in ref:
            for v in o.values():
                v.setflags(write=False)
        _REF[hand, n] = ref
    return _REF[hand, n]


@pytest.mark.parametrize("hand", list(HANDS))
@pytest.mark.parametrize("case", list(CASES))
def test_slot_order_dispatch_is_bitwise_the_monolithic_step(dp, monkeypatch, hand, case):
    n, chunks, grid, no_order = CASES[case]
    ref = _reference(dp, monkeypatch, hand, n)
    if n == 64:
        kinds = np.stack([o["step_type"] for o in ref])
        # steps 1 and 2 each mix envs with one chunk (due for their auto-reset) and envs with all chunks
        last = kinds[:-1] == 2
        assert last.any(axis=1).all() and (~last).any(axis=1).all(), "a launch without both kinds of env"
        assert (kinds[1:] == 0).any(), "no env auto-reset inside the window"
        assert ref[-1]["stats"][:, 3].max() > 0, "no constraint rows: the solve was not exercised"
    got = _rollout(dp, monkeypatch, hand, n, chunks, grid, no_order)
    for t, (a, b) in enumerate(zip(ref, got)):
        for k in KEYS:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{hand} {case}: step {t}, {k}")
