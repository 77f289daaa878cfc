"""csrc/render_build.h - the host-only builder of the hull face planes the ray caster clips against
- through its stand-alone driver tools/render_build_check: no GPU, no HIP. Every vertex inside
every plane, every plane through at least three vertices, as many planes as qhull's merged facets,
and a hull over the per-hull cap refused by name."""
import importlib
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers

ROOT = Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tools" / "render_build_check"
MAXPLANE = 96  # psr::HULL_MAXPLANE


def run(tmp_path, hulls):
    """[(rc, message, planes [P, 4] or None)] of the driver on the hulls ([nv, 3] each)."""
    assert DRIVER.exists(), f"{DRIVER} is missing: run __graft_entry__.build()"
    src = tmp_path / "hulls.bin"
    with open(src, "wb") as f:
        for v in hulls:
            v = np.ascontiguousarray(v, np.float64)
            f.write(struct.pack("<i", len(v)) + v.tobytes())
    p = subprocess.run([str(DRIVER), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    out, i = [], 0
    for _ in hulls:
        rc, _, msg = lines[i].partition(" ")
        n = int(lines[i + 1])
        planes = np.array([[float(x) for x in lines[i + 2 + k].split()] for k in range(max(n, 0))]).reshape(-1, 4)
        out.append((int(rc), msg, planes if n >= 0 else None))
        i += 2 + max(n, 0)
    assert i == len(lines)
    return out


def merged_facets(v):
    """qhull's facets of the hull of v with coplanar ones counted once."""
    from scipy.spatial import ConvexHull
    return len(np.unique(np.round(ConvexHull(np.asarray(v, np.float64)).equations, 9), axis=0))


def check(v, planes):
    v = np.asarray(v, np.float64)
    s = v @ planes[:, :3].T - planes[:, 3]  # [nv, P]
    assert s.max() <= 1e-9, "a vertex outside a plane"
    np.testing.assert_allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, atol=1e-12)
    # distinct vertices on each plane
    for j in range(planes.shape[0]):
        on = np.unique(np.round(v[np.abs(s[:, j]) <= 1e-9], 12), axis=0)
        assert len(on) >= 3, f"plane {j} touches {len(on)} vertices"
    assert planes.shape[0] == merged_facets(v)


CUBE = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * [0.01, 0.02, 0.03]


def model_hulls(md):
    out = []
    for h in range(2):
        for i in range(12):
            if md.xgeom_type[h][i] == 2:
                v0, nv = md.xgeom_vert[h][i]
                out.append(np.array([[md.hull_vert[h][v0 + k][c] for c in range(3)] for k in range(nv)]))
    return out


def test_cube(tmp_path):
    (rc, msg, planes), = run(tmp_path, [CUBE])
    assert rc == 0 and planes.shape == (6, 4)
    check(CUBE, planes)
    assert sorted(np.round(planes[:, 3], 12).tolist()) == [0.01, 0.01, 0.02, 0.02, 0.03, 0.03]


def test_cube_with_duplicate_and_interior_vertices(tmp_path):
    rng = np.random.RandomState(1)
    v = np.concatenate([CUBE, CUBE[[0, 3, 3, 7]], rng.uniform(-0.5, 0.5, (9, 3)) * [0.01, 0.02, 0.03],
                        [[0.01, 0.0, 0.0], [0.0, 0.02, 0.011]]])  # the last two inside faces
    (rc, msg, planes), = run(tmp_path, [v[rng.permutation(len(v))]])
    assert rc == 0 and planes.shape == (6, 4)
    check(CUBE, planes)


def test_model_hulls(dp, tmp_path):
    """Every hull of helpers.box_hull_hand and of the default hull fingertips
    (TaskConfig(primitive_fingertip_collisions=False)), both hands."""
    model = importlib.import_module("diffusion-piano_amd.model")
    mds = [model.build_model(hand=helpers.box_hull_hand(dp)),
           dp.compile_task(helpers.song(dp, "twinkle"), dp.TaskConfig(primitive_fingertip_collisions=False))[0]]
    for md in mds:
        hulls = model_hulls(md)
        assert len(hulls) == 10
        for v, (rc, msg, planes) in zip(hulls, run(tmp_path, hulls)):
            assert rc == 0, msg
            assert 4 <= planes.shape[0] <= MAXPLANE
            check(v, planes)


def test_hull_over_the_cap_is_refused(tmp_path):
    """64 points in general position on a sphere: 2 V - 4 = 124 facets, over the cap of 96."""
    rng = np.random.RandomState(3)
    v = rng.normal(size=(64, 3))
    v = 0.01 * v / np.linalg.norm(v, axis=1, keepdims=True)
    assert merged_facets(v) == 124
    (rc, msg, planes), (rc2, _, planes2) = run(tmp_path, [v, CUBE])
    assert rc < 0 and "hull 0 of hand 0" in msg and "124" in msg and str(MAXPLANE) in msg
    assert planes.shape[0] == 124  # (the builder itself has no cap: the device table has)
    assert rc2 == 0 and planes2.shape[0] == 6


def test_flat_hull_is_refused(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.3, 0.2, 0]], float) * 0.01
    (rc, msg, planes), = run(tmp_path, [v])
    assert rc < 0 and planes is None and "hull 0 of hand 0" in msg
