"""The final-state collision pass on demand (csrc/kernel_v2.inc env_step, fore_near): without
contact recording a step runs the pass only for the envs whose forearm prefilter finds the two
hands' root-body colliders near each other, and leaves the contact counts to be materialised when
they are read (csrc/pianosim.hip materialise_ncon). Nothing a caller can read may depend on that:
a handle that reads the counts after every step, one that reads them once, and one with contact
recording on (the eager pass, every step) must agree bit for bit.

Shapes: 8 envs (16 on the time-sliced path), 20 steps of Crossing Field, random actions; the first
envs start with the forearms slid together (forearm_tx of both hands), so that the rollout holds
env-steps that run the pass and env-steps that skip it."""
import numpy as np
import pytest

from helpers import song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 20
HANDS = {"hull": dict(primitive_fingertip_collisions=False), "authored": {}}
TX = 88, 88 + 26  # qpos columns of forearm_tx: right hand, left hand (hand dof 0)
# forearm_tx of the right hand (the left hand's: the negative), by env: slid together until the root
# geoms overlap, nearly, and apart (these rollouts compare handles with each other, not with the
# checker: any mix of states that runs and skips the pass will do)
SLIDES = (-0.2, -0.16, -0.12, 0.0, 0.1, -0.18, 0.0, -0.14)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _slid(state, slides):
    q = np.array(state["qpos"], np.float32)
    for e in range(q.shape[0]):
        q[e, TX[0]], q[e, TX[1]] = slides[e % len(slides)], -slides[e % len(slides)]
    return dict(state, qpos=q)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def _rollout(dp, hand, n, counts, record=False, task_kw=None, steps=STEPS):
    """counts: 'every' step, or 'last' only. -> (per-step outputs, per-step counts or None)"""
    task = dp.TaskConfig(trim_silence=True, **dict(HANDS[hand], **(task_kw or {})))
    g = dp.BatchedPianoEnv(n, song(dp, "crossing_field"), task, device="cuda:0")
    if record:
        g.record_contacts(True)
    g.reset()
    if not task_kw:
        g.set_state(_slid(_np(g.get_state()), SLIDES))
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    out, ncon = [], []
    for t in range(steps):
        a = torch.rand(n, g.action_dim, device="cuda:0", generator=gen) * 2 - 1
        o, r, d, s = g.step(a)
        out.append(_np(dict(obs=o, reward=r, discount=d, step_type=s, terms=g.reward_terms())))
        ncon.append(g.contact_count().cpu().numpy().copy() if counts == "every" or t == steps - 1 else None)
    g.close()
    return out, ncon


def _assert_bitwise(a, b, what):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in x:
            np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=f"{what}: step {t}, {k}")


@pytest.mark.parametrize("hand", list(HANDS))
def test_lazy_counts_equal_eager(dp, hand):
    """A reads the counts after every step, B after the last one only, C records contacts."""
    A, nA = _rollout(dp, hand, 8, "every")
    B, nB = _rollout(dp, hand, 8, "last")
    C, nC = _rollout(dp, hand, 8, "every", record=True)
    _assert_bitwise(A, B, f"{hand}: counts every step vs once")
    _assert_bitwise(A, C, f"{hand}: lazy vs recording")
    for t in range(STEPS):
        np.testing.assert_array_equal(nA[t], nC[t], err_msg=f"{hand}: counts, step {t}")
    np.testing.assert_array_equal(nA[-1], nB[-1], err_msg=f"{hand}: final counts")
    fore = np.stack([o["terms"][:, 4] for o in A])
    assert (fore == 0.0).any() and (fore == 0.5).any(), "the rollout holds no forearm hit / only hits"
    assert np.stack(nA).max() > 0


@pytest.mark.parametrize("hand", list(HANDS))
def test_counts_survive_set_state(dp, hand):
    """Step, overwrite the state, then read the counts: those of the step's final state, as a
    twin handle read them straight after the step."""
    task = dp.TaskConfig(trim_silence=True, **HANDS[hand])
    gs = [dp.BatchedPianoEnv(8, song(dp, "crossing_field"), task, device="cuda:0") for _ in range(2)]
    got = []
    for i, g in enumerate(gs):
        g.reset()
        rest = _np(g.get_state())
        g.set_state(_slid(rest, SLIDES))
        g.step(torch.zeros(8, g.action_dim, device="cuda:0"))
        if i == 1:
            g.set_state(rest)  # (the reset state: no contact anywhere)
        got.append(g.contact_count().cpu().numpy().copy())
        g.close()
    assert got[0].max() > 0
    np.testing.assert_array_equal(got[0], got[1])


# States for the comparison with the fp64 checker: only ones whose outcome in the checker is far from
# the threshold, so that the fp32 step cannot legitimately land on the other side. One step with zero
# actions from forearm_tx = s / -s leaves, in the checker (both collider sets):
#   -0.2, -0.19: ONE contact in all, between the two root capsules, 2.3 mm and 1.3 mm deep;
#   -0.12: 16-20 finger and palm contacts, the root capsules 7 mm apart;
#   -0.25: the hands have passed each other: no contact, the root capsules' bounding spheres
#          still overlap (the pass runs and finds nothing);
#   0, 0.1: no contact, the hands 0.3 m and more apart (the pass is skipped).
# (-0.14 to -0.17 are not used: 9-20 interpenetrating contacts at the contact cap with the root
# contact among them, a state whose step moves by millimetres under rounding.)
FORE_SLIDES = (-0.2, -0.19, -0.12, 0.0, 0.1, -0.25, -0.2, 0.0)


@pytest.mark.parametrize("hand", list(HANDS))
def test_forearm_term_against_the_checker(dp, ref, hand):
    """One step with zero actions from FORE_SLIDES: terms[:, 4] equals the checker's in every env -
    0 where the root geoms touch (the first two envs), 0.5 elsewhere - on the lazy handle and on
    the recording one."""
    n = len(FORE_SLIDES)
    task = dp.TaskConfig(trim_silence=True, **HANDS[hand])
    md, st, tc = dp.compile_task(song(dp, "crossing_field"), task, canonical_actions=False)
    o = ref.OracleEnv(md, st, tc, n)
    o.reset()
    o.set_state(_slid(o.get_state(), FORE_SLIDES))
    o.step(np.zeros((n, 45), np.float32))
    want = np.asarray(o.reward_terms())[:, 4].astype(np.float32)
    assert (want[:2] == 0.0).all() and (want[2:6] == 0.5).all(), want  # touching / not touching
    got = {}
    for record in (False, True):
        g = dp.BatchedPianoEnv(n, song(dp, "crossing_field"), task, device="cuda:0", canonical_actions=False)
        g.record_contacts(record)
        g.reset()
        g.set_state(_slid(_np(g.get_state()), FORE_SLIDES))
        g.step(torch.zeros(n, 45, device="cuda:0"))
        got[record] = g.reward_terms().cpu().numpy()[:, 4]
        g.close()
    print(f"{hand}: checker {want}, lazy {got[False]}, recording {got[True]}")
    np.testing.assert_array_equal(got[False], got[True], err_msg=f"{hand}: lazy vs recording")
    np.testing.assert_array_equal(got[False], want, err_msg=f"{hand}: vs the checker")


@pytest.mark.parametrize("hand", list(HANDS))
def test_time_sliced_path(dp, monkeypatch, hand):
    """PIANOSIM_CHUNKS=3 (read at create) on 16 envs against the monolithic handle."""
    monkeypatch.setenv("PIANOSIM_CHUNKS", "0")
    M, nM = _rollout(dp, hand, 16, "every")
    monkeypatch.setenv("PIANOSIM_CHUNKS", "3")
    B, nB = _rollout(dp, hand, 16, "last")
    C, nC = _rollout(dp, hand, 16, "every", record=True)
    _assert_bitwise(M, B, f"{hand}: monolithic vs time-sliced")
    _assert_bitwise(M, C, f"{hand}: monolithic vs time-sliced, recording")
    for t in range(STEPS):
        np.testing.assert_array_equal(nM[t], nC[t], err_msg=f"{hand}: counts, step {t}")
    np.testing.assert_array_equal(nM[-1], nB[-1], err_msg=f"{hand}: final counts")
    assert np.stack(nM).max() > 0 and nM[-1].max() > 0, "no contact: the counts compare nothing"


@pytest.mark.parametrize("hand", list(HANDS))
def test_one_hand_handle(dp, hand):
    """The one-hand task has no forearm term: no step runs the pass, every count is materialised."""
    A, nA = _rollout(dp, hand, 8, "every", task_kw=dict(hand_side="right"))
    C, nC = _rollout(dp, hand, 8, "every", record=True, task_kw=dict(hand_side="right"))
    _assert_bitwise(A, C, f"{hand}: one hand, lazy vs recording")
    for t in range(STEPS):
        np.testing.assert_array_equal(nA[t], nC[t], err_msg=f"{hand}: one hand, counts, step {t}")
    assert np.stack(nA).max() > 0, "no contact: the counts compare nothing"


def _offset_rollout(dp, hand, record):
    """randomize_hand_positions on (the pass reads hand_dy). Per step: the outputs and the counts;
    after step 2 the hand offsets are overwritten (the counts read AFTER it on the lazy handle, before
    it on the recording one: those of the step either way); then a masked reset, a full reset, and
    steps across the end of the episode (LAST, then the auto-reset inside the next step)."""
    n = 8
    task = dp.TaskConfig(trim_silence=True, randomize_hand_positions=True, **HANDS[hand])
    g = dp.BatchedPianoEnv(n, song(dp, "crossing_field"), task, device="cuda:0", seed=3)
    g.record_contacts(record)
    g.reset()
    g.set_state(_slid(_np(g.get_state()), SLIDES))
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    out, ncon = [], []

    def step():
        a = torch.rand(n, g.action_dim, device="cuda:0", generator=gen) * 2 - 1
        o, r, d, s = g.step(a)
        out.append(_np(dict(obs=o, reward=r, discount=d, step_type=s, terms=g.reward_terms())))

    def count():
        ncon.append(g.contact_count().cpu().numpy().copy())

    for t in range(3):
        step()
        if t < 2:
            count()
    dy = torch.linspace(-0.05, 0.05, n, device="cuda:0")
    if record:
        count()
        g.set_hand_offset(dy)
    else:
        g.set_hand_offset(dy)
        count()
    step()
    count()
    mask = np.arange(n) % 2 == 0
    g.reset(mask)
    count()  # reset envs: the reset state's counts; the others keep the step's
    g.reset()
    count()
    T = g.song.T
    st = _slid(_np(g.get_state()), SLIDES)
    st["t_idx"] = np.where(np.arange(n) < 4, T - 2, 0).astype(np.int32)
    g.set_state(st)
    for t in range(4):
        step()
        count()
    kinds = np.stack([o["step_type"] for o in out[-4:]])
    g.close()
    return out, ncon, kinds


@pytest.mark.parametrize("hand", list(HANDS))
def test_hand_offset_and_resets(dp, hand):
    A, nA, kinds = _offset_rollout(dp, hand, False)
    C, nC, _ = _offset_rollout(dp, hand, True)
    _assert_bitwise(A, C, f"{hand}: randomized hands, lazy vs recording")
    assert len(nA) == len(nC) == 10
    for i, (a, c) in enumerate(zip(nA, nC)):
        np.testing.assert_array_equal(a, c, err_msg=f"{hand}: counts, read {i}")
    assert nA[2].max() > 0 and nA[3].max() > 0  # around set_hand_offset
    assert (nA[4][1::2] == nA[3][1::2]).all()  # the masked reset leaves the other envs' counts
    assert (kinds == 2).any() and (kinds == 0).any(), "no terminal step / auto-reset in the window"
