"""The ray caster restated in fp64 numpy (test infrastructure): the checker of ps_render.

Same conventions as include/pianosim.h: pixel-centre rays d = px x + py y - z (not normalised, so
t is the depth along the optical axis), row 0 on top, only entering hits with t > 0, the lower id
on equal t, the floor z = 0 last, a miss = (+inf, -1, background), headlight shading
colour (ambient + diffuse max(0, -n . dhat)) rounded to u8. The scene comes from
``OracleEnv.shape`` (every collider's world shape in fp64) or is given by hand.

A primitive is a dict: ``id``, ``kind`` ("capsule": p0, p1, r; "box": c, R, hs; "hull": c, R, verts
in the geom frame) and ``color`` (an index into ``COLORS``).
"""
import numpy as np

AMBIENT, DIFFUSE = 0.3, 0.7
COLORS = np.array([(0.9, 0.9, 0.9), (0.1, 0.1, 0.1), (0.15, 0.15, 0.15), (0.2, 0.8, 0.2),
                   (0.8, 0.2, 0.8), (0.8, 0.2, 0.2), (0.2, 0.8, 0.8), (0.2, 0.2, 0.8), (0.8, 0.8, 0.2),
                   (0.6, 0.6, 0.6), (0.2, 0.3, 0.4), (0.05, 0.05, 0.1)])
WHITE, BLACK, BASE, ACTIVATION, FINGER0, HAND, FLOOR, BACKGROUND = 0, 1, 2, 3, 4, 9, 10, 11
SEG_KEY0, SEG_BASE, SEG_FLOOR = 64, 152, 153
KEY_THRESHOLD = 0.00872665  # the task's activation rule: within 0.5 degrees of the key's full travel
BLACK_KEYS = (1, 4, 6, 9, 11)  # key % 12, key 0 = A0


class Cam:
    """pos, image right x, image up y (orthonormalised, x first), fovy in degrees."""

    def __init__(self, pos, x, y, fovy=45.0):
        self.pos = np.asarray(pos, np.float64)
        x = np.asarray(x, np.float64)
        y = np.asarray(y, np.float64)
        self.x = x / np.linalg.norm(x)
        y = y - (self.x @ y) * self.x
        self.y = y / np.linalg.norm(y)
        self.z = np.cross(self.x, self.y)
        self.th = np.tan(np.radians(fovy) / 2)


def rays(cam, H, W, dc=0.0, dr=0.0):
    """d [H, W, 3] of the pixel centres shifted by (dc, dr) pixels (columns, rows)."""
    r = np.arange(H)[:, None] + 0.5 + dr
    c = np.arange(W)[None, :] + 0.5 + dc
    py = (1 - 2 * r / H) * cam.th
    px = (2 * c / W - 1) * cam.th * W / H
    return px[..., None] * cam.x + py[..., None] * cam.y - cam.z


def _sphere(o, d, c, r):
    oc = o - c
    dd = np.einsum("ij,ij->i", d, d)
    tm = -(d @ oc) / dd
    l = oc + d * tm[:, None]
    disc = r * r - np.einsum("ij,ij->i", l, l)
    ok = disc >= 0
    t = np.where(ok, tm - np.sqrt(np.where(ok, disc, 0) / dd), np.inf)
    n = (oc + d * np.where(np.isfinite(t), t, 0)[:, None]) / r
    return np.where(t > 0, t, np.inf), n


def _capsule(o, d, p0, p1, r):
    t, n = _sphere(o, d, p0, r)
    u = p1 - p0
    length = np.linalg.norm(u)
    if length < 1e-6:  # p0 == p1: a sphere
        return t, n
    t1, n1 = _sphere(o, d, p1, r)
    n = np.where((t1 < t)[:, None], n1, n)
    t = np.minimum(t, t1)
    u = u / length
    oc = o - p0
    du, ou = d @ u, oc @ u
    dp = d - du[:, None] * u
    op = oc - ou * u
    A = np.einsum("ij,ij->i", dp, dp)
    ok = A > 1e-12 * np.einsum("ij,ij->i", d, d)
    As = np.where(ok, A, 1.0)
    tm = -(dp @ op) / As
    l = op + dp * tm[:, None]
    disc = r * r - np.einsum("ij,ij->i", l, l)
    ok &= disc >= 0
    tc = tm - np.sqrt(np.where(ok, disc, 0) / As)
    s = ou + du * tc
    ok &= (tc > 0) & (s >= 0) & (s <= length)
    tc = np.where(ok, tc, np.inf)
    nc = (op + dp * np.where(ok, tc, 0)[:, None]) / r
    n = np.where((tc < t)[:, None], nc, n)
    return np.minimum(t, tc), n


def _box(o, d, c, R, hs):
    ol = R.T @ (o - c)
    dl = d @ R  # rows: R' d
    t0 = np.full(len(d), -np.inf)
    t1 = np.full(len(d), np.inf)
    axis = np.zeros(len(d), int)
    miss = np.zeros(len(d), bool)
    for k in range(3):
        par = dl[:, k] == 0
        miss |= par & (abs(ol[k]) > hs[k])
        inv = 1.0 / np.where(par, 1.0, dl[:, k])
        ta, tb = (-hs[k] - ol[k]) * inv, (hs[k] - ol[k]) * inv
        tn = np.where(par, -np.inf, np.minimum(ta, tb))
        tf = np.where(par, np.inf, np.maximum(ta, tb))
        up = tn > t0
        t0 = np.where(up, tn, t0)
        axis = np.where(up, k, axis)
        t1 = np.minimum(t1, tf)
    ok = ~miss & (t0 <= t1) & (t0 > 0)
    sg = np.where(dl[np.arange(len(d)), axis] > 0, -1.0, 1.0)
    n = sg[:, None] * R.T[axis]
    return np.where(ok, t0, np.inf), n


def hull_planes(verts):
    """(normals [P, 3], offsets [P]) of the hull's facets (inside: n . x <= off), from qhull."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(verts, np.float64)).equations
    return eq[:, :3], -eq[:, 3]


def _hull(o, d, c, R, planes):
    nrm, off = planes
    ol = R.T @ (o - c)
    dl = d @ R
    dn = dl @ nrm.T  # [M, P]
    dist = nrm @ ol - off  # [P]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -dist[None, :] / dn
    ent = np.where(dn < 0, t, -np.inf)
    ext = np.where(dn > 0, t, np.inf)
    miss = ((dn == 0) & (dist[None, :] > 0)).any(axis=1)
    face = ent.argmax(axis=1)
    t0, t1 = ent.max(axis=1), ext.min(axis=1)
    ok = ~miss & (t0 <= t1) & (t0 > 0)
    return np.where(ok, t0, np.inf), nrm[face] @ R.T


def trace(prims, o, d, floor=True):
    """The first hit of every ray d [M, 3] from o: (t [M], id [M], normal [M, 3], colour index [M])."""
    M = len(d)
    best = np.full(M, np.inf)
    ids = np.full(M, -1)
    col = np.full(M, BACKGROUND)
    nrm = np.zeros((M, 3))
    for p in sorted(prims, key=lambda p: p["id"]):
        if p["kind"] == "capsule":
            t, n = _capsule(o, d, p["p0"], p["p1"], p["r"])
        elif p["kind"] == "box":
            t, n = _box(o, d, p["c"], p["R"], p["hs"])
        else:
            if "planes" not in p:
                p["planes"] = hull_planes(p["verts"])
            t, n = _hull(o, d, p["c"], p["R"], p["planes"])
        up = t < best
        best = np.where(up, t, best)
        ids = np.where(up, p["id"], ids)
        col = np.where(up, p["color"], col)
        nrm = np.where(up[:, None], n, nrm)
    if floor and o[2] > 0:
        with np.errstate(divide="ignore"):
            t = np.where(d[:, 2] < 0, -o[2] / np.where(d[:, 2] < 0, d[:, 2], -1.0), np.inf)
        up = t < best
        best = np.where(up, t, best)
        ids = np.where(up, SEG_FLOOR, ids)
        col = np.where(up, FLOOR, col)
        nrm = np.where(up[:, None], np.array([0.0, 0.0, 1.0]), nrm)
    return best, ids, nrm, col


def shade(d, ids, nrm, col):
    dhat = d / np.linalg.norm(d, axis=1, keepdims=True)
    s = np.where(ids >= 0, AMBIENT + DIFFUSE * np.maximum(0.0, -np.einsum("ij,ij->i", nrm, dhat)), 1.0)
    return np.floor(np.clip(COLORS[col] * s[:, None], 0, 1) * 255 + 0.5).astype(np.uint8)


def render(prims, cam, H, W, floor=True):
    """dict(depth [H, W] f64, seg [H, W] int, rgb [H, W, 3] u8, rgb_f [H, W, 3] the unrounded levels)."""
    d = rays(cam, H, W).reshape(-1, 3)
    t, ids, nrm, col = trace(prims, cam.pos, d, floor)
    dhat = d / np.linalg.norm(d, axis=1, keepdims=True)
    s = np.where(ids >= 0, AMBIENT + DIFFUSE * np.maximum(0.0, -np.einsum("ij,ij->i", nrm, dhat)), 1.0)
    return dict(depth=t.reshape(H, W), seg=ids.reshape(H, W), rgb=shade(d, ids, nrm, col).reshape(H, W, 3),
                rgb_f=(np.clip(COLORS[col] * s[:, None], 0, 1) * 255).reshape(H, W, 3))


def unstable(prims, cam, H, W, seg, floor=True, shift=1.0 / 128):
    """Pixels whose id changes for one of the four rays shifted by +-shift pixels in x or y: an
    edge passes within rounding reach of the pixel centre. From the fp64 caster alone."""
    bad = np.zeros((H, W), bool)
    for dc, dr in ((shift, 0), (-shift, 0), (0, shift), (0, -shift)):
        _, ids, _, _ = trace(prims, cam.pos, rays(cam, H, W, dc, dr).reshape(-1, 3), floor)
        bad |= ids.reshape(H, W) != seg
    return bad


def object_colors(md, tc, song, qpos, t_idx, activation=False, colorize=False):
    """Colour index of every id 0 .. 152 of one env (ps_render's flags restated)."""
    col = np.full(153, HAND)
    for h in range(2):
        for g in range(20):
            for f in range(5):
                if colorize and md.geom_body[h][g] == md.site_body[h][f]:
                    col[h * 20 + g] = FINGER0 + f
        for i in range(12):
            for f in range(5):
                if colorize and md.xgeom_type[h][i] and md.xgeom_body[h][i] == md.site_body[h][f]:
                    col[40 + h * 12 + i] = FINGER0 + f
    goal = {}
    t = int(t_idx) - 1
    if colorize and 0 <= t < song.T:
        for i in range(min(int(song.count[t]), song.keys.shape[1])):
            f = int(song.fingers[t, i])
            if 0 <= f < 10 and (not tc.hand_side or (f < 5) == (tc.hand_side == 1)):
                goal[int(song.keys[t, i])] = f % 5
    for k in range(88):
        lo, hi = md.key_range[k]
        act = abs(min(max(qpos[k], lo), hi) - hi) <= KEY_THRESHOLD
        c = BLACK if k % 12 in BLACK_KEYS else WHITE
        if act:
            c = ACTIVATION if activation else c
        elif k in goal:
            c = FINGER0 + goal[k]
        col[SEG_KEY0 + k] = c
    col[SEG_BASE] = BASE
    return col


def oracle_scene(oracle, i, md, colors=None):
    """The drawn primitives of env i of an ``OracleEnv`` at its current state: the capsule and
    extra colliders in use, the 88 keys, the base."""
    colors = np.full(153, HAND) if colors is None else colors
    prims = []

    def add(pid, g):
        s, verts = oracle.shape(i, g)
        kind = ("capsule", "box", "hull")[int(s[0])]
        p = dict(id=pid, kind=kind, color=int(colors[pid]))
        if kind == "capsule":
            p.update(p0=s[13:16].copy(), p1=s[16:19].copy(), r=float(s[19]))
        else:
            p.update(c=s[1:4].copy(), R=s[4:13].reshape(3, 3).copy(), hs=s[20:23].copy(), verts=verts)
        prims.append(p)

    for h in range(2):
        for g in range(20):
            if md.geom_body[h][g] >= 0:
                add(h * 20 + g, h * 20 + g)
        for x in range(12):
            if md.xgeom_type[h][x]:
                add(40 + h * 12 + x, 40 + h * 12 + x)
    for k in range(88):
        add(SEG_KEY0 + k, -1 - k)
    add(SEG_BASE, -1000)
    return prims
