"""The one-loop MPR of csrc/collide_x.h (mpr_penetration_d: discovery, portal search and refinement as
one loop with a phase variable and one support search) against the fp64 checker, pair by pair, at
the placements where its control flow branches: hull-hull, hull-capsule, hull-box and hull-key
pairs, 64 of each kind at each of six placements - clearly apart, grazing (the gap within +-2e-6 m
of where the checker's contact appears), shallow (0.1 mm), deep (3 mm), coincident centres, and the
first support collinear with the centre line (MPR's exit before the loop).

The kernel runs through tools/libxcheck.so (xcheck_run_its: x_narrow_local per pair, and the trips
of each pair's MPR loop), ONE WAVE PER LAUNCH, the pairs of all kinds and placements shuffled
together, so the lanes of a wave are in different phases of the loop at the same trip - what the one
loop changed. Geom2 sits at the origin (the kernel's frame is geom2's centre: the shift is then
exact) and capsule end points on a 2^-26 m grid (their fp32 midpoint is exact), so kernel and
checker see the same fp64 colliders and differ only in the kernel's fp32 support selection (inside
the tie band both share) and its 1e-14 reciprocal square root.

The checker does not report its loop trips: _mpr_trips below restates its mpr_penetration
(oracle/pianosim_ref.c) in numpy fp64 with the trip counter of the kernel's `its`, and is itself held
to the checker's contact count on every pair, and to its depth where the restatement has one (the exit
before the loop), on the CPU, before it is used. It is a transcription, not the checker: a slip in
its loop structure that kept every contact count would pass that self-check, so the trip assertion
below is as good as this restatement and the kernel agreeing on all 1,536 pairs.

Held, for each of the launch forms - one pair per lane over all vertices, over the support-cell
masks and over the cell vertex tables; paired lanes over masks and over tables:
- the contact count equals the checker's on every pair, except that at the grazing placement at most
  2% of a kind's pairs may flip (the seed is one where the checker against its own 1e-9 m shift of
  geom1 stays inside that cap: test_grazing_seed_checker_self, CPU);
- where the counts agree: depth within 2e-6 m, normal within 1e-3, point within 1e-4 m, the
  per-contact tolerances of test_gpu_colliders.test_narrow_phase_matches_checker with its allowance
  of 1% of a kind's pairs for a portal that ends on a face edge of the Minkowski difference and takes
  the neighbouring face under rounding (no pair is skipped for depth here);
- the loop trips equal the checker's on every pair whose count agrees.
Measured on MI355X: no count flip, no contact outside the tolerances and no trip difference in any form.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

from helpers import capsule_points

KINDS = ("hull-hull", "hull-capsule", "hull-box", "hull-key")
PLACES = ("apart", "grazing", "shallow", "deep", "coincident", "collinear")
PER = 64
SEED = 20
EPS = 2.220446049250313e-16
KEY_HS = np.array([0.0117, 0.0235, 0.0113], np.float32)
GRID = 2.0 ** -26


def _f32(x):
    return np.asarray(x, np.float32)


def _rot(rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    t = rng.uniform(0, np.pi)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return _f32(np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K)


def _roll(axis, ang):
    """Rotation by ang about coordinate axis `axis`: that axis' row and column are exact."""
    c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R = np.zeros((3, 3), np.float32)
    R[axis, axis] = 1
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _z_to(axis):
    """Exact rotation (a cyclic permutation) taking local z to world coordinate axis `axis`."""
    P = np.zeros((3, 3), np.float32)
    for k in range(3):
        P[(axis + 1 + k) % 3, k] = 1  # local x, y, z -> world axis+1, axis+2, axis
    return P


class Col:
    """A collider with fp32-representable fields, as the kernel's packed form and the checker's."""

    def __init__(self, kind, c=(0, 0, 0), R=None, half=None, r=0.0, hs=(0, 0, 0), hull=None):
        self.kind = kind
        self.R = _f32(np.eye(3) if R is None else R)
        self.r, self.hs, self.hull = np.float32(r), _f32(hs), hull
        self.half = None if half is None else np.round(np.asarray(half, np.float64) / GRID) * GRID
        self.move(c)

    def move(self, c):
        """Centre at c (fp32; a capsule's end points on the grid about the gridded centre)."""
        if self.kind == "capsule":
            c = np.round(np.asarray(c, np.float64) / GRID) * GRID
            self.p0, self.p1 = _f32(c - self.half), _f32(c + self.half)
            assert np.all(self.p0 == c - self.half) and np.all(self.p1 == c + self.half)
        self.c = _f32(c).astype(np.float64)
        return self

    def centre(self):
        return (self.p0.astype(np.float64) + self.p1) * 0.5 if self.kind == "capsule" else self.c

    def pack(self):
        t = {"capsule": 0, "box": 1, "hull": 2}[self.kind]
        p0 = self.p0 if self.kind == "capsule" else np.zeros(3)
        p1 = self.p1 if self.kind == "capsule" else np.zeros(3)
        v0, nv = (self.hull[0], self.hull[1]) if self.kind == "hull" else (0, 0)
        return np.concatenate([[t], self.c, self.R.ravel(), p0, p1, [self.r], self.hs, [v0, nv]]).astype(np.float32)

    def ref(self, ref):
        if self.kind == "capsule":
            return ref.shape("capsule", p0=self.p0, p1=self.p1, r=self.r)
        if self.kind == "box":
            return ref.shape("box", c=self.c, R=self.R, hs=self.hs)
        return ref.shape("hull", c=self.c, R=self.R, verts=self.hull[2])


# ---- the checker's mpr_penetration (oracle/pianosim_ref.c) in numpy fp64, with the kernel's trip counter
def _nrmz(a):
    n = np.sqrt(a @ a)
    return a / n if n > 0.0 else a


def _support(s, d):
    if s.kind == "capsule":
        p0, p1 = s.p0.astype(np.float64), s.p1.astype(np.float64)
        ax = p1 - p0
        dn, da = np.sqrt(d @ d), ax @ d
        if abs(da) <= 1e-6 * np.sqrt(ax @ ax) * dn:
            da = 0.0
        base = p1 if da > 0.0 else (p0 if da < 0.0 else (p0 + p1) * 0.5)
        return base + d * (float(s.r) / dn) if dn > 0.0 else base
    R = s.R.astype(np.float64)
    dl = R.T @ d
    if s.kind == "box":
        mx = np.abs(dl).max()
        sg = np.where(np.abs(dl) <= 1e-6 * mx, 0.0, np.sign(dl))
        loc = sg * s.hs.astype(np.float64)
    else:
        v = s.hull[2]
        tie = 2e-6 * s.hull[3] * np.sqrt(dl @ dl)
        best, bd = 0, -np.inf
        for i, p in enumerate(v @ dl):
            if p > bd + tie:
                bd, best = p, i
        loc = v[best]
    return s.c + R @ loc


def _mpr_trips(A, B):
    """(contact found, depth, trips of the loop) as the checker's mpr_penetration on (A, B)."""
    zero = lambda x: abs(x) < EPS  # noqa: E731
    sup = lambda d: _support(A, d) - _support(B, -d)  # noqa: E731
    pdir = lambda P: _nrmz(np.cross(P[2] - P[1], P[3] - P[1]))  # noqa: E731

    def reach(P, v4, d):
        d4 = v4 @ d
        return min(d4 - P[1] @ d, d4 - P[2] @ d, d4 - P[3] @ d) <= 1e-6

    def expand(P, v4):
        x = np.cross(v4, P[0])
        if P[1] @ x > 0.0:
            P[1 if P[2] @ x > 0.0 else 3] = v4
        else:
            P[2 if P[3] @ x > 0.0 else 1] = v4

    P = [None] * 4
    P[0] = A.centre() - B.centre()
    if not P[0].any():
        P[0] = P[0] + np.array([10.0 * EPS, 0.0, 0.0])
    d = _nrmz(-P[0])
    P[1] = sup(d)
    dt = P[1] @ d
    if zero(dt) or dt < 0.0:
        return False, 0.0, 0
    d = np.cross(P[0], P[1])
    if zero(d @ d):
        return True, float(np.sqrt(P[1] @ P[1])), 0
    d = _nrmz(d)
    P[2] = sup(d)
    dt = P[2] @ d
    if zero(dt) or dt < 0.0:
        return False, 0.0, 0
    d = _nrmz(np.cross(P[1] - P[0], P[2] - P[0]))
    if d @ P[0] > 0.0:
        P[1], P[2], d = P[2], P[1], -d
    trips, it = 0, 0
    while True:
        trips += 1
        if it > 200:
            return False, 0.0, trips
        P[3] = sup(d)
        dt = P[3] @ d
        if zero(dt) or dt < 0.0:
            return False, 0.0, trips
        t = np.cross(P[1], P[3]) @ P[0]
        if t < 0.0 and not zero(t):
            P[2] = P[3]
        else:
            t = np.cross(P[3], P[2]) @ P[0]
            if t < 0.0 and not zero(t):
                P[1] = P[3]
            else:
                break
        d = _nrmz(np.cross(P[1] - P[0], P[2] - P[0]))
        it += 1
    it = 0
    while True:
        trips += 1
        if it > 200:
            return False, 0.0, trips
        d = pdir(P)
        dt = P[1] @ d
        if zero(dt) or dt > 0.0:
            break
        v4 = sup(d)
        d4 = v4 @ d
        if not (zero(d4) or d4 > 0.0) or reach(P, v4, d):
            return False, 0.0, trips
        expand(P, v4)
        it += 1
    it = 0
    while True:
        trips += 1
        d = pdir(P)
        v4 = sup(d)
        if reach(P, v4, d) or it > 50:
            return True, None, trips  # (the depth: the checker's own, compared through ref.narrow)
        expand(P, v4)
        it += 1


# ---- the pairs
def _hulls(dp):
    _, hull = dp.mjcf.convex_hull_collider(capsule_points(0.0085, 0.006))
    hull = hull.astype(np.float32).astype(np.float64)
    verts = np.zeros((len(hull), 4), np.float32)
    verts[:, :3] = hull
    # the pole of the capsule-shaped hull on its z axis: the support along +-z, alone
    # (x, y ~1e-18: a support difference along the axis to within 1e-20 m, collinear by MPR's |cross|^2 < 2.2e-16)
    on_axis = (np.abs(hull[:, 0]) < 1e-15) & (np.abs(hull[:, 1]) < 1e-15)
    assert np.any(on_axis & (hull[:, 2] > 0.014)) and np.any(on_axis & (hull[:, 2] < -0.014))
    return (0, len(hull), hull, float(np.sqrt((hull * hull).sum(axis=1)).max())), verts


def _geom1(kind, rng, tip, R=None, axis=None):
    """Geom1 of a pair of `kind` (geom2 is the tip hull), with rotation R, or its long axis on coordinate `axis`."""
    if kind == "hull-hull":
        return Col("hull", R=_z_to(axis) @ _roll(2, rng.uniform(0, 6.28)) if R is None else R, hull=tip)
    if kind == "hull-capsule":
        a = (_z_to(axis) if R is None else R)[:, 2].astype(np.float64)
        return Col("capsule", half=a * 0.01, r=0.008)
    if kind == "hull-box":
        hs = rng.uniform(0.005, 0.015, 3)
        return Col("box", R=_z_to(axis) @ _roll(2, rng.uniform(0, 6.28)) if R is None else R, hs=hs)
    # a key: its box turned about y by the key's travel; collinear: the centre line along y
    return Col("box", R=_roll(1, rng.uniform(0, 0.07)), hs=KEY_HS)


def _has(ref, A, B):
    return len(ref.narrow(A.ref(ref), B.ref(ref)))


def _depth(ref, A, B):
    w = ref.narrow(A.ref(ref), B.ref(ref))
    return -w[0][2] if w else -1.0


def _bisect(f, lo, hi, n=44):
    """t in [lo, hi] where f turns from true to false."""
    for _ in range(n):
        mid = 0.5 * (lo + hi)
        if f(mid):
            lo = mid
        else:
            hi = mid
    return lo


def make_pairs(dp, ref, seed=SEED):
    """[(kind, place, A, B, u, t)]: geom1 A at t u (a unit vector), geom2 B (the tip hull) at the origin."""
    rng = np.random.RandomState(seed)
    tip, verts = _hulls(dp)
    pairs = []
    for kind in KINDS:
        for place in PLACES:
            for _ in range(PER):
                if place == "collinear":
                    axis = 1 if kind == "hull-key" else rng.randint(3)
                    u = np.zeros(3)
                    u[axis] = rng.choice([-1.0, 1.0])
                    A = _geom1(kind, rng, tip, axis=axis)
                    B = Col("hull", R=_z_to(axis) @ _roll(2, rng.uniform(0, 6.28)), hull=tip)
                else:
                    u = rng.normal(size=3)
                    u /= np.linalg.norm(u)
                    A = _geom1(kind, rng, tip, R=_rot(rng))
                    B = Col("hull", R=_rot(rng), hull=tip)
                if place == "coincident":
                    pairs.append((kind, place, A.move(np.zeros(3)), B, u, 0.0))
                    continue
                touch = _bisect(lambda t: _has(ref, A.move(t * u), B), 0.0, 0.08)  # contact below, none above
                if place == "apart":
                    t = touch + rng.uniform(1e-3, 5e-3)
                elif place == "grazing":
                    t = touch + rng.uniform(-2e-6, 2e-6)
                elif place == "collinear":
                    t = touch + rng.uniform(-3e-3, 1e-3)
                else:
                    want = 1e-4 if place == "shallow" else 3e-3
                    t = _bisect(lambda t: _depth(ref, A.move(t * u), B) > want, 0.0, touch)
                pairs.append((kind, place, A.move(t * u), B, u, t))
    return pairs, verts


@pytest.fixture(scope="module")
def pairs(dp, ref):
    """The pairs, and per pair the checker's contacts and the trips of its MPR loop (computed once)."""
    ps, verts = make_pairs(dp, ref)
    want = [ref.narrow(A.ref(ref), B.ref(ref)) for _, _, A, B, _, _ in ps]
    trips = []
    for (kind, place, A, B, _, _), w in zip(ps, want):
        hit, depth, n = _mpr_trips(A, B)
        # the restatement is the checker's: the same contact count, and its depth where it has one
        assert hit == bool(w), (kind, place, hit, w)
        if depth is not None and hit:
            assert abs(depth + w[0][2]) < 1e-12, (kind, place, depth, w)
        trips.append(n)
    return ps, verts, want, np.array(trips)


def test_grazing_seed_checker_self(dp, ref, pairs):
    """The seed's grazing pairs: the checker against itself with geom1 moved by 1e-9 m along the centre
    line flips the contact count on at most 2% of a kind's pairs; every placement is what it says."""
    ps, _, want, trips = pairs
    flips = {k: 0 for k in KINDS}
    for (kind, place, A, B, u, t), w in zip(ps, want):
        if place == "grazing":
            c = A.centre() if A.kind == "capsule" else A.c
            if A.kind == "capsule":
                moved = ref.shape("capsule", p0=A.p0 + 1e-9 * u, p1=A.p1 + 1e-9 * u, r=A.r)
            else:
                moved = ref.shape(A.kind, c=c + 1e-9 * u, R=A.R, hs=A.hs, verts=A.hull[2] if A.hull else None)
            flips[kind] += len(ref.narrow(moved, B.ref(ref))) != len(w)
        elif place == "apart":
            assert not w
        elif place in ("shallow", "deep"):
            assert w and abs(-w[0][2] - (1e-4 if place == "shallow" else 3e-3)) < 2e-5, (kind, place, w)
        elif place == "coincident":
            assert w and not (A.centre() - B.centre()).any()
    assert all(v <= 0.02 * PER for v in flips.values()), flips
    # the placements reach the loop and the exits before it
    t = trips.reshape(len(KINDS), len(PLACES), PER)
    assert (t[:, PLACES.index("collinear")] == 0).all() and (t[:, PLACES.index("deep")] >= 3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [0, 1, 5, 3, 7], ids=["lane-scan", "lane-masks", "lane-tables", "paired-masks",
                                                         "paired-tables"])
def test_one_loop_mpr_matches_checker(dp, ref, pairs, cells):
    torch = pytest.importorskip("torch")
    ps, verts, want, trips = pairs
    lib = C.CDLL(os.environ.get("PS_XCHECK_LIB", str(Path(__file__).resolve().parents[1] / "tools" / "libxcheck.so")))
    lib.xcheck_run_its.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    n = len(ps)
    order = np.random.RandomState(SEED + 1).permutation(n)  # kinds and placements mixed in every wave
    dA = torch.from_numpy(np.stack([ps[i][2].pack() for i in order])).cuda()
    dB = torch.from_numpy(np.stack([ps[i][3].pack() for i in order])).cuda()
    dv = torch.from_numpy(verts).cuda()
    out = torch.zeros(n, 29, device="cuda:0")
    its = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    wave = 32 if cells & 2 else 64  # pairs of one wave
    for k in range(0, n, wave):
        m = min(wave, n - k)
        assert lib.xcheck_run_its(dv.data_ptr(), len(verts), dA[k:].data_ptr(), dB[k:].data_ptr(), out[k:].data_ptr(), m,
                                  cells, its[k:].data_ptr()) == 0
    o, got_trips = np.zeros((n, 29), np.float32), np.zeros(n, np.int64)
    o[order], got_trips[order] = out.cpu().numpy(), its.cpu().numpy()
    flips = {(k, p): 0 for k in KINDS for p in PLACES}
    bad = {k: [] for k in KINDS}
    wrong_trips = []
    for i, ((kind, place, A, B, _, _), w) in enumerate(zip(ps, want)):
        if int(o[i, 0]) != len(w):
            flips[kind, place] += 1
            continue
        if got_trips[i] != trips[i]:
            wrong_trips.append((kind, place, int(got_trips[i]), int(trips[i])))
        for j, (p, nrm, d) in enumerate(w):
            gp, gn, gd = o[i, 1 + 7 * j:4 + 7 * j], o[i, 4 + 7 * j:7 + 7 * j], o[i, 7 + 7 * j]
            if abs(gd - d) > 2e-6 or np.abs(gn - nrm).max() > 1e-3 or np.abs(gp - p).max() > 1e-4:
                bad[kind].append((place, d, float(gd), float(np.abs(gn - nrm).max()), float(np.abs(gp - p).max())))
    print(f"one-loop MPR, launch form {cells}: count flips {dict((k, v) for k, v in flips.items() if v)}, outside the "
          f"contact tolerances {dict((k, len(v)) for k, v in bad.items())}, trips differ on {len(wrong_trips)}")
    for (kind, place), v in flips.items():
        assert v <= (0.02 * PER if place == "grazing" else 0), (kind, place, v)
    for kind, v in bad.items():
        assert len(v) <= 0.01 * PER * len(PLACES), (kind, v[:10])
    assert not wrong_trips, wrong_trips[:10]
