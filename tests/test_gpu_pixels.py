"""PixelWrapper (rendering.py; robopianist/wrappers/pixels.py) over an Environment and over a
VectorizedPianoEnv: the spec's shape and dtype, `pixels` at reset and at every step, equal to the
env's own render called directly."""
import numpy as np
import pytest

from helpers import song

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KW = dict(height=20, width=36, camera_id="egocentric")


def test_pixel_wrapper_over_environment(dp):
    env = dp.Environment(song(dp, "twinkle"), dp.TaskConfig(), device="cuda:0")
    w = dp.PixelWrapper(env, render_kwargs=KW)
    spec = w.observation_spec()
    assert list(spec)[:-1] == list(env.observation_spec()) and list(spec)[-1] == "pixels"
    assert spec["pixels"].shape == (20, 36, 3) and spec["pixels"].dtype == np.uint8
    ts = w.reset()
    assert ts.first() and set(ts.observation) == set(spec)
    rng = np.random.RandomState(0)
    seen = [ts.observation["pixels"]]
    for _ in range(3):
        px = ts.observation["pixels"]
        assert isinstance(px, np.ndarray) and px.shape == (20, 36, 3) and px.dtype == np.uint8
        assert np.array_equal(px, env.physics.render(**KW))
        assert np.array_equal(px, env.core.render("egocentric", 20, 36)[0].cpu().numpy())
        ts = w.step(rng.uniform(-1, 1, env.core.action_dim))
        assert ts.mid() and "pixels" in ts.observation and ts.reward is not None
        seen.append(ts.observation["pixels"])
    assert any(not np.array_equal(seen[0], s) for s in seen[1:])  # the hands move
    # the reference's spelling: camera_id as an index, depth and segmentation as numpy [H, W]
    d = env.physics.render(12, 16, camera_id=5, depth=True)
    s = env.physics.render(12, 16, camera_id="topdown", segmentation=True)
    assert d.shape == (12, 16) and d.dtype == np.float32 and s.shape == (12, 16) and s.dtype == np.int32
    assert np.isfinite(d).all() and (s >= 0).all() and 0.5 < d.min() < d.max() <= 1.0 + 1e-6
    assert w.action_spec().shape == env.action_spec().shape
    env.core.close()


@pytest.mark.parametrize("as_numpy", [False, True])
def test_pixel_wrapper_over_vectorized(dp, as_numpy):
    n = 3
    vec = dp.VectorizedPianoEnv(n, song(dp, "twinkle"), return_numpy=as_numpy, device="cuda:0")
    w = dp.PixelWrapper(vec, render_kwargs=KW, observation_key="camera")
    spec = w.observation_spec()
    assert list(spec)[:-1] == list(vec.observation_spec) and spec["camera"].shape == (n, 20, 36, 3)
    assert spec["camera"].dtype == np.uint8
    obs = w.reset()
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for step in range(3):
        assert set(obs) == set(spec)
        px = obs["camera"]
        assert isinstance(px, np.ndarray if as_numpy else torch.Tensor) and tuple(px.shape) == (n, 20, 36, 3)
        direct = vec.core.render("egocentric", 20, 36)
        assert np.array_equal(px if as_numpy else px.cpu().numpy(), direct.cpu().numpy())
        obs, rew, dones = w.step(torch.rand(n, vec.core.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        assert len(rew) == n and len(dones) == n
    assert w.num_envs == n
    vec.core.close()
