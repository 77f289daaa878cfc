"""tests/render_ref.py, the fp64 restatement of the ray caster, pinned on hand-worked cases."""
import numpy as np
import pytest

import render_ref as rr

# a camera at the origin looking along world -z: image right = +x, image up = +y
CAM = dict(pos=(0, 0, 0), x=(1, 0, 0), y=(0, 1, 0))
I3 = np.eye(3)


def one(prims, fovy=45.0, H=1, W=1, floor=False, **cam):
    return rr.render(prims, rr.Cam(**{**CAM, **cam}, fovy=fovy), H, W, floor=floor)


def test_sphere_box_capsule_on_the_axis():
    sphere = dict(id=3, kind="capsule", p0=np.array([0, 0, -2.0]), p1=np.array([0, 0, -2.0]), r=0.5, color=rr.HAND)
    out = one([sphere])
    assert out["depth"][0, 0] == pytest.approx(1.5, abs=1e-14) and out["seg"][0, 0] == 3
    # the normal faces the camera: full light, 0.6 * (0.3 + 0.7) * 255 = 153
    assert out["rgb"][0, 0].tolist() == [153, 153, 153]
    box = dict(id=70, kind="box", c=np.array([0, 0, -3.0]), R=I3, hs=np.array([1, 1, 0.25]), color=rr.WHITE)
    out = one([box])
    assert out["depth"][0, 0] == pytest.approx(2.75, abs=1e-14) and out["seg"][0, 0] == 70
    assert out["rgb"][0, 0].tolist() == [230, 230, 230]  # floor(0.9 * 255 + 0.5)
    # a capsule across the axis: its cylinder; along the axis: its near cap
    cap = dict(id=0, kind="capsule", p0=np.array([-1, 0, -2.0]), p1=np.array([1, 0, -2.0]), r=0.25, color=rr.HAND)
    assert one([cap])["depth"][0, 0] == pytest.approx(1.75, abs=1e-14)
    cap = dict(id=0, kind="capsule", p0=np.array([0, 0, -2.0]), p1=np.array([0, 0, -4.0]), r=0.25, color=rr.HAND)
    assert one([cap])["depth"][0, 0] == pytest.approx(1.75, abs=1e-14)
    # the nearer of two wins, whatever the ids; behind the camera nothing is seen
    out = one([sphere, box])
    assert out["seg"][0, 0] == 3
    back = dict(id=1, kind="box", c=np.array([0, 0, 3.0]), R=I3, hs=np.array([1, 1, 0.25]), color=rr.WHITE)
    out = one([back])
    assert out["seg"][0, 0] == -1 and np.isinf(out["depth"][0, 0])
    assert out["rgb"][0, 0].tolist() == [13, 13, 26]  # the background, unshaded


def test_zero_length_capsule_is_a_sphere():
    c = np.array([0.1, -0.05, -1.0])
    cap = dict(id=5, kind="capsule", p0=c, p1=c.copy(), r=0.3, color=rr.HAND)
    cam = rr.Cam(**CAM, fovy=60)
    out = rr.render([cap], cam, 9, 11, floor=False)
    d = rr.rays(cam, 9, 11).reshape(-1, 3)
    # analytic: |t d - c| = r
    a, b, cc = (d * d).sum(1), d @ c, c @ c - 0.09
    disc = b * b - a * cc
    t = np.where(disc >= 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.inf).reshape(9, 11)
    assert np.array_equal(np.isfinite(t), out["seg"] == 5) and (out["seg"] == 5).sum() > 10
    np.testing.assert_allclose(out["depth"][out["seg"] == 5], t[out["seg"] == 5], rtol=0, atol=1e-12)


def test_box_seen_edge_on():
    """Rays parallel to a pair of faces: inside the slab they see the near face, on or outside it
    they see nothing; no NaN from 0 * inf."""
    for y, hit in ((0.0, True), (0.0999, True), (0.1001, False)):
        box = dict(id=64, kind="box", c=np.array([0, y, -2.0]), R=I3, hs=np.array([0.5, 0.1, 0.5]), color=rr.WHITE)
        out = one([box])
        assert (out["seg"][0, 0] == 64) == hit
        assert out["depth"][0, 0] == (pytest.approx(1.5, abs=1e-14) if hit else np.inf)
    # a box rotated 45 degrees about y shows its edge to the camera: depth = centre - half diagonal
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    box = dict(id=64, kind="box", c=np.array([1e-9, 0, -2.0]), R=R, hs=np.array([0.5, 0.5, 0.5]), color=rr.WHITE)
    assert one([box])["depth"][0, 0] == pytest.approx(2 - np.sqrt(0.5), abs=1e-8)


def test_pixel_centres():
    """1 x 1: the ray is the optical axis. 2 x 2: the centres sit at +-1/2 of the half extents,
    row 0 on top, column 0 on the left."""
    cam = rr.Cam(**CAM, fovy=90)
    np.testing.assert_allclose(rr.rays(cam, 1, 1)[0, 0], [0, 0, -1], atol=1e-15)
    d = rr.rays(cam, 2, 2)
    np.testing.assert_allclose(d[0, 0], [-0.5, 0.5, -1], atol=1e-15)
    np.testing.assert_allclose(d[0, 1], [0.5, 0.5, -1], atol=1e-15)
    np.testing.assert_allclose(d[1, 0], [-0.5, -0.5, -1], atol=1e-15)
    # a wide image keeps the vertical field of view: px scales with W / H
    d = rr.rays(cam, 2, 4)
    np.testing.assert_allclose(d[0, 0], [-1.5, 0.5, -1], atol=1e-15)
    np.testing.assert_allclose(d[1, 3], [1.5, -0.5, -1], atol=1e-15)
    # a small box in the upper left quadrant lands in pixel (0, 0) only
    box = dict(id=9, kind="box", c=np.array([-0.5, 0.5, -1.0]), R=I3, hs=np.array([0.05, 0.05, 0.05]), color=rr.WHITE)
    assert rr.render([box], cam, 2, 2, floor=False)["seg"].tolist() == [[9, -1], [-1, -1]]


def test_depth_is_axial():
    """A plane square to the optical axis has one depth all over the image, not the ray length."""
    wall = dict(id=1, kind="box", c=np.array([0, 0, -3.5]), R=I3, hs=np.array([50, 50, 0.5]), color=rr.WHITE)
    out = rr.render([wall], rr.Cam(**CAM, fovy=100), 5, 7, floor=False)
    np.testing.assert_allclose(out["depth"], 3.0, rtol=0, atol=1e-13)
    # the floor seen from straight above, by a camera 2 m up
    out = rr.render([], rr.Cam(pos=(0, 0, 2), x=(0, 1, 0), y=(-1, 0, 0), fovy=70), 4, 6)
    np.testing.assert_allclose(out["depth"], 2.0, rtol=0, atol=1e-13)
    assert (out["seg"] == rr.SEG_FLOOR).all()
    # shading falls off with the angle to the headlight: the corner is darker than the centre
    out = rr.render([], rr.Cam(pos=(0, 0, 2), x=(0, 1, 0), y=(-1, 0, 0), fovy=120), 5, 5)
    assert out["rgb"][2, 2].tolist() == [51, 77, 102] and out["rgb"][0, 0, 2] < out["rgb"][2, 2, 2]


def test_hull_equals_box():
    """A cube given as a hull renders as the box: depth, ids and the entering face's normal."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * [0.2, 0.1, 0.3]
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    c = np.array([0.05, -0.02, -1.5])
    cam = rr.Cam(**CAM, fovy=40)
    box = rr.render([dict(id=40, kind="box", c=c, R=R, hs=np.array([0.2, 0.1, 0.3]), color=rr.HAND)], cam, 12, 16, False)
    hull = rr.render([dict(id=40, kind="hull", c=c, R=R, hs=np.zeros(3), verts=v, color=rr.HAND)], cam, 12, 16, False)
    assert np.array_equal(box["seg"], hull["seg"]) and (box["seg"] == 40).sum() > 20
    m = box["seg"] == 40
    np.testing.assert_allclose(box["depth"][m], hull["depth"][m], rtol=0, atol=1e-12)
    assert np.array_equal(box["rgb"], hull["rgb"])


def test_unstable_marks_edges_only():
    box = dict(id=2, kind="box", c=np.array([0.013, 0.007, -1.0]), R=I3, hs=np.array([0.2, 0.2, 0.1]), color=rr.WHITE)
    cam = rr.Cam(**CAM, fovy=45)
    out = rr.render([box], cam, 24, 40, floor=False)
    bad = rr.unstable([box], cam, 24, 40, out["seg"], floor=False)
    assert bad.sum() == 0  # no centre within 1/128 pixel of this box's outline
    # a box whose left edge passes 1/256 pixel from a column of centres
    px = (2 * 10.5 / 40 - 1) * cam.th * 40 / 24 + (2 / 40) * cam.th * 40 / 24 / 256
    box = dict(id=2, kind="box", c=np.array([px * 0.9 + 0.2, 0.0, -1.0]), R=I3, hs=np.array([0.2, 0.2, 0.1]), color=rr.WHITE)
    out = rr.render([box], cam, 24, 40, floor=False)
    bad = rr.unstable([box], cam, 24, 40, out["seg"], floor=False)
    assert bad[:, 10].any() and not np.delete(bad, 10, axis=1).any()
