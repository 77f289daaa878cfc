"""ps_render (csrc/render.inc; BatchedPianoEnv.render) against the fp64 ray caster tests/render_ref.py
over the checker's world shapes (OracleEnv.shape): N = 3 envs, 24 x 40 images - partial 16 x 16
tiles on both axes - at helpers.random_states(seed 5), set on the env and on an OracleEnv.

A pixel is *unstable* when the fp64 caster alone returns another id for one of the four rays
shifted by +-1/128 pixel in x or y (render_ref.unstable; never from the GPU image). On stable pixels
the ids are equal, the depth is within DEPTH_GATE and rgb within one level; at most 2% of an image
may be unstable.

Unstable shares of the fp64 caster at 24 x 40, this seed, all six cameras (measured on the CPU):
capsule hand at most 1.46%, default hull fingertips at most 1.56%, box_hull_hand (the same
colliders through the MJCF path) at most 1.56%, the largest under topdown, whose rows run along
the key gaps (profiles/render_parity.txt has every image's). The floor and the base are part of
the scene, so their outlines count.

DEPTH_GATE: the largest |gpu - ref| over the stable finite pixels of all 18 cases x 3 envs was
measured on the MI355X, 3.711e-7 m (profiles/render_parity.txt), and the gate is 4 x that, never above 1e-3 m
(a renderer off by a key gap is wrong whatever was measured). The fp64 scene moved by 2e-6 m moves
stable depths by up to 3.8e-5 m, so that order is expected."""
import ctypes as C
import importlib

import numpy as np
import pytest

import render_ref as rr
from helpers import box_hull_hand, random_states, song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, H, W, SEED = 3, 24, 40, 5
T_IDX = (3, 9, 17)   # rows of the Twinkle tables with goal keys: the colorize path is live
UNSTABLE_CAP = 0.02
DEPTH_GATE = 4 * 3.711e-7  # metres: 4 x the measured maximum (below the 1e-3 cap); see the module docstring
HANDS = ("capsule", "hull", "box_hull")
CAMERAS = ("closeup", "left", "right", "back", "egocentric", "topdown")
BACKGROUND = [13, 13, 26]


def task_of(dp, hand, **kw):
    if hand == "capsule":
        return dp.TaskConfig(**kw)
    if hand == "hull":
        return dp.TaskConfig(primitive_fingertip_collisions=False, **kw)
    return dp.TaskConfig(hand_xml=dp.mjcf.hand_to_mjcf(box_hull_hand(dp)), **kw)


def ref_cam(dp, camera):
    c = dp.rendering.camera_of(camera)
    return rr.Cam(c.pos, c.x, c.y, c.fovy)


_PAIRS, _REFS = {}, {}


def pair(dp, ref, hand):
    """(env, oracle) of a hand at the test states, made once per hand."""
    if hand not in _PAIRS:
        seq = song(dp, "twinkle")
        task = task_of(dp, hand)
        env = dp.BatchedPianoEnv(N, seq, task, device="cuda:0")
        md, st, tc = dp.compile_task(seq, task)
        env.reset()
        q, v = random_states(md, N, np.random.RandomState(SEED))
        env.set_state(dict(qpos=q, qvel=v, t_idx=np.array(T_IDX, np.int32)))
        oracle = ref.OracleEnv(md, st, tc, N)
        oracle.reset()
        oracle.set_state({k: t.cpu().numpy() for k, t in env.get_state().items()})
        _PAIRS[hand] = (env, oracle, md, st, tc)
    return _PAIRS[hand]


def reference(dp, oracle, md, st, tc, camera, h=H, w=W, activation=False, colorize=True, key=None):
    """Per env the fp64 images and the unstable mask; shared by the tests of one (hand, camera)."""
    key = key or (id(oracle), camera, h, w, activation, colorize)
    if key not in _REFS:
        state = oracle.get_state()
        cam = ref_cam(dp, camera)
        out = []
        for i in range(oracle.n):
            col = rr.object_colors(md, tc, st, state["qpos"][i], state["t_idx"][i], activation, colorize)
            prims = rr.oracle_scene(oracle, i, md, col)
            img = rr.render(prims, cam, h, w)
            img["unstable"] = rr.unstable(prims, cam, h, w, img["seg"])
            out.append(img)
        _REFS[key] = out
    return _REFS[key]


def compare(gpu, refs, what, gate=DEPTH_GATE):
    """seg / depth / rgb tensors [n, h, w(, 3)] against the per-env reference images."""
    seg, depth, rgb = (t.cpu().numpy() for t in gpu)
    worst = 0.0
    for i, r in enumerate(refs):
        ok = ~r["unstable"]
        share = 1.0 - ok.mean()
        fin = ok & np.isfinite(r["depth"])
        err = float(np.abs(depth[i][fin] - r["depth"][fin]).max()) if fin.any() else 0.0
        lvl = float(np.abs(rgb[i][ok].astype(float) - r["rgb_f"][ok]).max()) if ok.any() else 0.0
        print(f"render_parity {what} env {i}: unstable {100 * share:.2f}% seg_mismatch "
              f"{int((seg[i][ok] != r['seg'][ok]).sum())} max_depth_err {err:.3e} max_rgb_err {lvl:.2f}")
        worst = max(worst, err)
    for i, r in enumerate(refs):
        ok = ~r["unstable"]
        assert 1.0 - ok.mean() <= UNSTABLE_CAP, f"{what} env {i}: {100 * (1 - ok.mean()):.2f}% unstable"
        assert np.array_equal(seg[i][ok], r["seg"][ok]), f"{what} env {i}: ids differ on stable pixels"
        fin = ok & np.isfinite(r["depth"])
        assert np.array_equal(np.isinf(depth[i][ok]), np.isinf(r["depth"][ok]))
        assert (depth[i][ok & ~fin] > 0).all()
        assert np.abs(depth[i][fin] - r["depth"][fin]).max(initial=0.0) <= gate, f"{what} env {i}: depth"
        # within one level of the reference shading (the unrounded level: rounding adds at most 1/2)
        assert np.abs(rgb[i][ok].astype(float) - r["rgb_f"][ok]).max(initial=0.0) <= 1.5, f"{what} env {i}: rgb"
        assert np.abs(rgb[i][ok].astype(int) - r["rgb"][ok].astype(int)).max(initial=0) <= 1, f"{what} env {i}: rgb"
    return worst


def images(env, camera, h=H, w=W, **kw):
    return (env.render(camera, h, w, segmentation=True, **kw), env.render(camera, h, w, depth=True, **kw),
            env.render(camera, h, w, **kw))


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("hand", HANDS)
def test_depth_seg_rgb_against_the_reference(dp, ref, hand, camera):
    env, oracle, md, st, tc = pair(dp, ref, hand)
    refs = reference(dp, oracle, md, st, tc, camera)
    gpu = images(env, camera)
    assert gpu[0].dtype == torch.int32 and gpu[1].dtype == torch.float32 and gpu[2].dtype == torch.uint8
    assert gpu[0].shape == (N, H, W) and gpu[1].shape == (N, H, W) and gpu[2].shape == (N, H, W, 3)
    compare(gpu, refs, f"{hand} {camera}")
    # the scene is there: hands, keys and the base or floor in at least one env's image
    ids = np.unique(gpu[0].cpu().numpy())
    assert (ids >= rr.SEG_KEY0).any() and ids.max() <= rr.SEG_FLOOR and ids.min() >= -1
    assert (ids[ids >= 0] < rr.SEG_KEY0).any()


def calm(dp, ref, **kw):
    """One env and its checker at the reset pose: the hands hover over a few keys, the others are seen."""
    seq = song(dp, "twinkle")
    task = dp.TaskConfig(**kw)
    env = dp.BatchedPianoEnv(1, seq, task, device="cuda:0")
    md, st, tc = dp.compile_task(seq, task)
    env.reset()
    oracle = ref.OracleEnv(md, st, tc, 1)
    oracle.reset()
    return env, oracle, md, st, tc


def set_both(env, oracle, **state):
    env.set_state(state)
    oracle.set_state({k: t.cpu().numpy() for k, t in env.get_state().items()})


def assert_lit(px, colour, what):
    """Pixels [n, 3] show `colour` under the headlight: one shading factor for the three channels,
    between full light and the darkest a key can get here - topdown at 60 x 100 sees the image
    corner 31 degrees off its axis and a key tilts by at most its travel (< 4 degrees), so the
    normal and the ray are less than 35 degrees apart."""
    want = np.asarray(colour) * 255
    s = px.sum(axis=1) / want.sum()
    lo = rr.AMBIENT + rr.DIFFUSE * np.cos(np.radians(35))
    assert (s >= lo - 0.01).all() and (s <= 1.01).all(), (what, s.min(), s.max())
    assert np.abs(px - want * s[:, None]).max() <= 1.5, (what, px[:3], want)


def key_pixels(seg, refs, k):
    m = (seg == rr.SEG_KEY0 + k) & ~refs[0]["unstable"]
    assert m.sum() >= 2, f"key {k} is not visible"
    return m


def test_activation_and_goal_colours(dp, ref):
    """topdown at 60 x 100 (a pixel is ~1 cm, a key ~2.3 cm). A key at its full travel shows the
    activation colour with change_color_on_activation; a goal key of the row just played shows its
    finger's colour with colorize, and its own colour without or with disable_colorization."""
    h, w = 60, 100
    env, oracle, md, st, tc = calm(dp, ref)
    t = next(t for t in range(st.T) if st.count[t] > 0 and 0 <= st.fingers[t, 0] < 10)
    goal, finger = int(st.keys[t, 0]), int(st.fingers[t, 0]) % 5
    q = env.get_state()["qpos"].cpu().numpy().astype(np.float64)
    # the seen keys: those the hands do not cover in the reference's image
    seg0 = rr.render(rr.oracle_scene(oracle, 0, md), ref_cam(dp, "topdown"), h, w)["seg"]
    seen = [k for k in range(88) if (seg0 == rr.SEG_KEY0 + k).sum() >= 4 and k % 12 not in rr.BLACK_KEYS]
    assert goal in seen, f"the goal key {goal} is hidden; seen {seen}"
    pressed = next(k for k in seen if abs(k - goal) > 2)
    q[0, pressed] = md.key_range[pressed][1]
    set_both(env, oracle, qpos=q, t_idx=np.array([t + 1], np.int32))
    for act, colz in ((True, True), (True, False), (False, True), (False, False)):
        refs = reference(dp, oracle, md, st, tc, "topdown", h, w, act, colz, key=("colour", act, colz))
        gpu = images(env, "topdown", h, w, change_color_on_activation=act, colorize=colz)
        compare(gpu, refs, f"colours act={act} colorize={colz}")
        seg, rgb = gpu[0][0].cpu().numpy(), gpu[2][0].cpu().numpy().astype(int)
        px = rgb[key_pixels(seg, refs, pressed)]
        assert_lit(px, rr.COLORS[rr.ACTIVATION if act else rr.WHITE], ("pressed", act, colz))
        px = rgb[key_pixels(seg, refs, goal)]
        assert_lit(px, rr.COLORS[rr.FINGER0 + finger if colz else rr.WHITE], ("goal", act, colz))
    # right after a reset (t_idx 0) no row has been played: no goal colour
    set_both(env, oracle, qpos=q, t_idx=np.array([0], np.int32))
    rgb = env.render("topdown", h, w, colorize=True)[0].cpu().numpy().astype(int)
    seg = env.render("topdown", h, w, segmentation=True)[0].cpu().numpy()
    assert_lit(rgb[seg == rr.SEG_KEY0 + goal], rr.COLORS[rr.WHITE], "goal after a reset")
    env.close()
    # disable_colorization turns the default off
    env, oracle, md, st, tc = calm(dp, ref, disable_colorization=True)
    set_both(env, oracle, qpos=q, t_idx=np.array([t + 1], np.int32))
    refs = reference(dp, oracle, md, st, tc, "topdown", h, w, False, False, key=("colour", "disabled"))
    gpu = images(env, "topdown", h, w)
    compare(gpu, refs, "colours disable_colorization")
    px = gpu[2][0].cpu().numpy().astype(int)[key_pixels(gpu[0][0].cpu().numpy(), refs, goal)]
    assert_lit(px, rr.COLORS[rr.WHITE], "goal with disable_colorization")
    on = env.render("topdown", h, w, colorize=True)[0].cpu().numpy().astype(int)
    assert_lit(on[key_pixels(gpu[0][0].cpu().numpy(), refs, goal)], rr.COLORS[rr.FINGER0 + finger], "goal, colorize asked for")
    env.close()


def test_fingertips_take_their_colour(dp, ref):
    """colorize paints the distal colliders: with it off every hand pixel has the hand's grey
    hue, with it on some have a finger's."""
    env, oracle, md, st, tc = pair(dp, ref, "capsule")
    seg = env.render("egocentric", 48, 64, segmentation=True).cpu().numpy()
    hand = (seg >= 0) & (seg < rr.SEG_KEY0)
    off = env.render("egocentric", 48, 64, colorize=False).cpu().numpy().astype(int)[hand]
    on = env.render("egocentric", 48, 64, colorize=True).cpu().numpy().astype(int)[hand]
    assert hand.sum() > 100 and (off.max(axis=1) - off.min(axis=1)).max() <= 1
    assert ((on.max(axis=1) - on.min(axis=1)) > 40).sum() > 5


@pytest.mark.parametrize("h, w", [(1, 1), (3, 17)])
def test_small_images(dp, ref, h, w):
    env, oracle, md, st, tc = pair(dp, ref, "hull")
    for camera in ("closeup", "topdown"):
        refs = reference(dp, oracle, md, st, tc, camera, h, w)
        # (a 1 x 1 image whose one pixel is unstable would say nothing: the cap does not apply here)
        gpu = images(env, camera, h, w)
        seg, depth, rgb = (t.cpu().numpy() for t in gpu)
        assert seg.shape == (N, h, w) and rgb.shape == (N, h, w, 3)
        for i, r in enumerate(refs):
            ok = ~r["unstable"]
            assert np.array_equal(seg[i][ok], r["seg"][ok])
            fin = ok & np.isfinite(r["depth"])
            assert np.abs(depth[i][fin] - r["depth"][fin]).max(initial=0.0) <= DEPTH_GATE
            assert np.abs(rgb[i][ok].astype(int) - r["rgb"][ok].astype(int)).max(initial=0) <= 1


def test_selection_and_bad_indices(dp, ref):
    env, *_ = pair(dp, ref, "hull")
    full = images(env, "left")
    pick = images(env, "left", envs=[2, 0, 2])
    for f, p in zip(full, pick):
        assert torch.equal(p, f[[2, 0, 2]])
    one = env.render("left", H, W, envs=torch.tensor([1], device="cuda:0"))
    assert torch.equal(one[0], full[2][1])
    with pytest.raises(dp.PianosimError, match="outside"):
        env.render("left", H, W, envs=[0, N])
    with pytest.raises(dp.PianosimError, match="outside"):
        env.render("left", H, W, envs=[-1])
    # through the C entry point: the bad index is counted and its image left as it was
    L = importlib.import_module("diffusion-piano_amd._lib").load()
    cam = dp.CAMERAS["left"].desc()
    sel = torch.tensor([1, 7, 0, -2], device="cuda:0", dtype=torch.int32)
    seg = torch.full((4, H, W), -77, device="cuda:0", dtype=torch.int32)
    rgb = torch.full((4, H, W, 3), 201, device="cuda:0", dtype=torch.uint8)
    nbad = torch.zeros(1, device="cuda:0", dtype=torch.int32)
    assert L.ps_render(env._h, C.byref(cam), W, H, sel.data_ptr(), 4, 2, rgb.data_ptr(), None, seg.data_ptr(),
                       nbad.data_ptr(), env.stream) == 0
    assert int(nbad.item()) == 2
    assert torch.equal(seg[0], full[0][1]) and torch.equal(seg[2], full[0][0])
    assert torch.equal(rgb[0], full[2][1]) and torch.equal(rgb[2], full[2][0])
    assert (seg[1] == -77).all() and (seg[3] == -77).all() and (rgb[1] == 201).all() and (rgb[3] == 201).all()


def test_camera_looking_up_sees_nothing(dp, ref):
    env, *_ = pair(dp, ref, "capsule")
    up = dp.Camera((0.1, 0.0, 1.5), (1, 0, 0, 0, -1, 0), fovy=60)  # z = x cross y = -world z: it looks along +z
    seg, depth, rgb = images(env, up)
    assert (seg == -1).all() and torch.isinf(depth).all() and (depth > 0).all()
    assert (rgb.reshape(-1, 3).cpu() == torch.tensor(BACKGROUND, dtype=torch.uint8)).all()
    down = dp.Camera((0.1, 0.0, 1.5), (1, 0, 0, 0, 1, 0), fovy=60)
    assert (env.render(down, H, W, segmentation=True) >= 0).all()


def test_refusals(dp, ref):
    env, *_ = pair(dp, ref, "capsule")
    E = dp.PianosimError
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(envs=[])):
        with pytest.raises(E):
            env.render("closeup", **{**dict(height=H, width=W), **kw})
    with pytest.raises(ValueError):
        env.render("closeup", H, W, depth=True, segmentation=True)
    with pytest.raises(ValueError):
        env.render("nowhere", H, W)
    # the library's own checks, past the Camera class: a raw ps_camera
    L = importlib.import_module("diffusion-piano_amd._lib").load()
    out = torch.zeros(N, H, W, 3, device="cuda:0", dtype=torch.uint8)

    def raw(x=(1, 0, 0), y=(0, 1, 0), fovy=45.0, rgb=True, n=N, w=W, h=H):
        cam = dp.rendering.CameraDesc((C.c_double * 3)(0, 0, 1), (C.c_double * 3)(*x), (C.c_double * 3)(*y), fovy)
        return L.ps_render(env._h, C.byref(cam), w, h, None, n, 0, out.data_ptr() if rgb else None, None, None, None,
                           env.stream)

    assert raw() == 0
    for kw, word in ((dict(fovy=0.0), "fovy"), (dict(fovy=180.0), "fovy"), (dict(fovy=-1.0), "fovy"),
                     (dict(fovy=float("nan")), "fovy"), (dict(x=(0, 0, 0)), "x axis"), (dict(y=(0, 0, 0)), "y axis"),
                     (dict(y=(2, 0, 0)), "y axis"), (dict(rgb=False), "NULL"), (dict(n=0), "positive"),
                     (dict(n=N - 1), "n_sel"), (dict(w=0), "positive"), (dict(h=0), "positive")):
        assert raw(**kw) < 0, kw
        assert word in L.ps_last_error().decode(), (kw, L.ps_last_error())
    cam = dp.CAMERAS["closeup"].desc()
    assert L.ps_render(env._h, C.byref(cam), W, H, None, N, 1 << 7, out.data_ptr(), None, None, None, env.stream) < 0
    torch.cuda.synchronize()


def test_one_hand_task_draws_one_hand(dp, ref):
    seq = song(dp, "twinkle")
    for side, gone in (("right", 1), ("left", 0)):
        task = dp.TaskConfig(hand_side=side)
        env = dp.BatchedPianoEnv(N, seq, task, device="cuda:0")
        md, st, tc = dp.compile_task(seq, task)
        env.reset()
        q, v = random_states(md, N, np.random.RandomState(SEED))
        q[:, 88 + 26 * gone:88 + 26 * (gone + 1)] = 0.0  # the detached hand's dofs are held at 0
        env.set_state(dict(qpos=q, qvel=np.zeros_like(v)))
        oracle = ref.OracleEnv(md, st, tc, N)
        oracle.reset()
        oracle.set_state({k: t.cpu().numpy() for k, t in env.get_state().items()})
        for camera in ("egocentric", "back"):
            gpu = images(env, camera)
            compare(gpu, reference(dp, oracle, md, st, tc, camera, key=("one", side, camera)), f"one-hand {side} {camera}")
            ids = np.unique(gpu[0].cpu().numpy())
            hand_of = np.where(ids < 40, ids // 20, (ids - 40) // 12)[(ids >= 0) & (ids < rr.SEG_KEY0)]
            assert len(hand_of) > 0 and (hand_of == 1 - gone).all(), ids
        env.close()


def test_randomized_hand_positions_match_the_oracle(dp, ref):
    seq = song(dp, "twinkle")
    task = dp.TaskConfig(randomize_hand_positions=True)
    env = dp.BatchedPianoEnv(N, seq, task, device="cuda:0", seed=11)
    md, st, tc = dp.compile_task(seq, task)
    oracle = ref.OracleEnv(md, st, tc, N, seed=11)
    env.reset()
    oracle.reset()
    dy = env.hand_offset()[0].cpu().numpy()
    assert np.abs(dy).max() > 1e-3 and len(np.unique(dy)) == N
    np.testing.assert_array_equal(dy.astype(np.float64), oracle.hand_offset()[0])
    for camera in ("topdown", "right"):
        gpu = images(env, camera)
        compare(gpu, reference(dp, oracle, md, st, tc, camera, key=("dy", camera)), f"randomized {camera}")
    # the shift is seen: the same env without it renders another image
    plain = dp.BatchedPianoEnv(N, seq, dp.TaskConfig(), device="cuda:0", seed=11)
    plain.reset()
    assert not torch.equal(plain.render("topdown", H, W, depth=True), gpu[1])
    plain.close()
    env.close()


def test_render_is_stream_ordered(dp, ref):
    """A render enqueued right after a step sees that step: the same image as after a sync."""
    env = dp.BatchedPianoEnv(N, song(dp, "twinkle"), dp.TaskConfig(), device="cuda:0")
    env.reset()
    before = env.render("closeup", H, W, depth=True).clone()
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    moved = False
    for _ in range(3):
        env.step(torch.rand(N, env.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        now = env.render("closeup", H, W, depth=True)
        torch.cuda.synchronize()
        again = env.render("closeup", H, W, depth=True)
        assert torch.equal(now, again)
        moved = moved or not torch.equal(now, before)
    assert moved
    env.close()


def same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_rendering_has_no_side_effects(dp, ref):
    """A twin that never renders stays bitwise equal through ten steps of the test-task song
    (T = 4: episode ends are crossed); and snapshots taken before and after the first render's
    lazy allocation both restore."""
    seq = song(dp, "test_task")
    envs = [dp.BatchedPianoEnv(N, seq, dp.TaskConfig(), device="cuda:0", seed=4) for _ in range(2)]
    q, v = random_states(envs[0].model_desc, N, np.random.RandomState(SEED))
    for e in envs:
        e.reset()
        e.set_state(dict(qpos=q, qvel=v))
    a, b = envs
    snap_before = a.snapshot()
    state_before = {k: t.clone() for k, t in a.get_state().items()}
    a.render("closeup", H, W)  # the first render: the planes, the scratch
    snap_after = a.snapshot()
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    lasts = 0
    for t in range(10):
        act = torch.rand(N, a.action_dim, device="cuda:0", generator=gen) * 2 - 1
        a.render(CAMERAS[t % 6], H, W, depth=t % 2 == 0)
        outs = [tuple(x.clone() for x in e.step(act)) for e in envs]
        a.render("topdown", 3, 17, envs=[1, 1, 0], segmentation=True)
        for x, y in zip(*outs):
            assert same(x, y)
        sa, sb = a.get_state(), b.get_state()
        assert all(same(sa[k], sb[k]) for k in sa) and same(a.solver_stats(), b.solver_stats())
        lasts += int((outs[0][3] == 2).sum())
    assert lasts >= N
    state_end = {k: t.clone() for k, t in a.get_state().items()}
    a.restore(snap_after)
    assert all(same(a.get_state()[k], state_before[k]) for k in state_before)
    a.restore(snap_before)
    assert all(same(a.get_state()[k], state_before[k]) for k in state_before)
    img = a.render("closeup", H, W, depth=True)
    b.set_state(state_before)
    assert torch.equal(img, b.render("closeup", H, W, depth=True))  # (b's first render)
    assert not all(same(state_end[k], state_before[k]) for k in state_before)
    for s in (snap_before, snap_after):
        s.close()
    for e in envs:
        e.close()
