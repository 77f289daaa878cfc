"""rendering.py without a GPU: the Camera's orthonormalisation and refusals, the named cameras,
write_png read back through zlib, and PixelWrapper's spec and observation logic on a stub env."""
import math
import struct
import zlib

import numpy as np
import pytest


def test_camera_is_orthonormalised(dp):
    cam = dp.Camera((1, 2, 3), (2, 0, 0, 1, 3, 0), fovy=30)
    np.testing.assert_allclose(cam.x, [1, 0, 0], atol=1e-15)
    np.testing.assert_allclose(cam.y, [0, 1, 0], atol=1e-15)  # the part of y along x is dropped
    np.testing.assert_allclose(cam.z, [0, 0, 1], atol=1e-15)
    assert cam.fovy == 30 and cam.pos.tolist() == [1, 2, 3]
    d = cam.desc()
    assert list(d.x) == [1, 0, 0] and list(d.y) == [0, 1, 0] and d.fovy_deg == 30 and list(d.pos) == [1, 2, 3]
    assert dp.Camera((0, 0, 0), (1, 0, 0, 0, 1, 0)).fovy == 45.0  # MuJoCo's default
    for name, c in dp.CAMERAS.items():  # the three-decimal xyaxes of the MJCF are not exactly orthonormal
        assert abs(c.x @ c.y) < 1e-15 and abs(np.linalg.norm(c.x) - 1) < 1e-15 and abs(np.linalg.norm(c.y) - 1) < 1e-15


@pytest.mark.parametrize("pos, axes, fovy", [
    ((0, 0, 0), (0, 0, 0, 0, 1, 0), 45),          # zero x
    ((0, 0, 0), (1, 0, 0, 0, 0, 0), 45),          # zero y
    ((0, 0, 0), (1, 0, 0, -3, 0, 0), 45),         # y parallel to x
    ((0, 0, 0), (1, 0, 0, 0, 1, 0), 0),           # fovy on the bounds and beyond
    ((0, 0, 0), (1, 0, 0, 0, 1, 0), 180),
    ((0, 0, 0), (1, 0, 0, 0, 1, 0), -10),
    ((0, 0, 0), (1, 0, 0, 0, 1, 0), float("nan")),
    ((0, float("inf"), 0), (1, 0, 0, 0, 1, 0), 45),
    ((0, 0), (1, 0, 0, 0, 1, 0), 45),             # shapes
    ((0, 0, 0), (1, 0, 0, 0, 1), 45),
])
def test_camera_refusals(dp, pos, axes, fovy):
    with pytest.raises(ValueError):
        dp.Camera(pos, axes, fovy)


def test_named_cameras(dp):
    assert list(dp.CAMERAS) == ["closeup", "left", "right", "back", "egocentric", "topdown"]
    top = dp.CAMERAS["topdown"]
    assert top.pos.tolist() == [0, 0, 1]
    np.testing.assert_allclose(top.x, [0, 1, 0], atol=0)   # image x runs along world +y
    np.testing.assert_allclose(top.z, [0, 0, 1], atol=0)   # it looks along -z: straight down
    assert top.fovy == pytest.approx(math.degrees(2 * math.atan2(0.5 * 0.6105, 1.0)), abs=1e-12)
    assert all(c.fovy == 45.0 for n, c in dp.CAMERAS.items() if n != "topdown")
    # every named camera sits above the floor and looks down at the piano
    for c in dp.CAMERAS.values():
        assert c.pos[2] > 0 and c.z[2] > 0
    r = dp.rendering
    assert r.camera_of("left") is dp.CAMERAS["left"] and r.camera_of(5) is top and r.camera_of(top) is top
    for bad in ("front", 6, -1):
        with pytest.raises(ValueError):
            r.camera_of(bad)
    for bad in (None, 1.5, True):
        with pytest.raises(TypeError):
            r.camera_of(bad)


def read_png(path):
    """(H, W, channels, pixels) of an 8-bit PNG whose rows all use filter 0; every CRC checked."""
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    i, chunks = 8, []
    while i < len(b):
        n, = struct.unpack(">I", b[i:i + 4])
        tag, data = b[i + 4:i + 8], b[i + 8:i + 8 + n]
        assert struct.unpack(">I", b[i + 8 + n:i + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        i += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, kind, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and kind in (0, 2)
    ch = 3 if kind == 2 else 1
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert (raw[:, 0] == 0).all()
    return h, w, ch, raw[:, 1:].reshape(h, w, ch)


def test_write_png_round_trip(dp, tmp_path):
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    dp.write_png(tmp_path / "a.png", img)
    h, w, ch, px = read_png(tmp_path / "a.png")
    assert (h, w, ch) == (5, 7, 3) and np.array_equal(px, img)
    grey = rng.randint(0, 256, (3, 1)).astype(np.uint8)
    dp.write_png(tmp_path / "g.png", grey)
    h, w, ch, px = read_png(tmp_path / "g.png")
    assert (h, w, ch) == (3, 1, 1) and np.array_equal(px[..., 0], grey)
    dp.write_png(tmp_path / "s.png", img[::2, ::-1])  # a non-contiguous view
    assert np.array_equal(read_png(tmp_path / "s.png")[3], img[::2, ::-1])
    for bad in (img.astype(np.float32), img[..., :2], img[0, 0], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            dp.write_png(tmp_path / "bad.png", bad)


class StubPhysics:
    def __init__(self):
        self.calls = []

    def render(self, height=240, width=320, camera_id="closeup", **kw):
        self.calls.append(dict(height=height, width=width, camera_id=camera_id, **kw))
        return np.full((height, width, 3), len(self.calls), np.uint8)


class StubEnv:
    """A dm_env-style single env: observation_spec(), reset() / step() -> TimeStep, physics.render."""

    def __init__(self, dp):
        self._dp, self.physics, self.extra = dp, StubPhysics(), "kept"

    def observation_spec(self):
        return {"goal": self._dp.Array((4,), np.float64, "goal")}

    def reset(self):
        return self._dp.TimeStep(self._dp.StepType.FIRST, None, None, {"goal": np.zeros(4)})

    def step(self, action):
        return self._dp.TimeStep(self._dp.StepType.MID, 1.5, 1.0, {"goal": np.ones(4) * action})


def test_pixel_wrapper_on_a_stub(dp):
    env = StubEnv(dp)
    w = dp.PixelWrapper(env, render_kwargs=dict(height=6, width=8, camera_id="left"))
    spec = w.observation_spec()
    assert list(spec) == ["goal", "pixels"]
    assert spec["pixels"].shape == (6, 8, 3) and spec["pixels"].dtype == np.uint8 and spec["pixels"].name == "pixels"
    assert spec["goal"] == env.observation_spec()["goal"] and "pixels" not in env.observation_spec()
    ts = w.reset()
    assert ts.first() and ts.reward is None and list(ts.observation) == ["goal", "pixels"]
    assert ts.observation["pixels"].shape == (6, 8, 3)
    ts2 = w.step(2.0)
    assert ts2.mid() and ts2.reward == 1.5 and ts2.discount == 1.0 and ts2.observation["goal"].tolist() == [2.0] * 4
    # one render for the spec, one per reset / step, each with the wrapper's kwargs
    assert ts.observation["pixels"][0, 0, 0] == 2 and ts2.observation["pixels"][0, 0, 0] == 3
    assert env.physics.calls == [dict(height=6, width=8, camera_id="left")] * 3
    assert w.extra == "kept"  # everything else is the wrapped env's
    # another key; the default kwargs; a clash with an existing key
    w = dp.PixelWrapper(env, observation_key="camera")
    assert w.observation_spec()["camera"].shape == (240, 320, 3) and "camera" in w.reset().observation
    with pytest.raises(ValueError):
        dp.PixelWrapper(env, observation_key="goal")
    with pytest.raises(TypeError):
        dp.PixelWrapper(object())
