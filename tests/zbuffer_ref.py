"""The definition of include/adgs_zbuffer.h in numpy: int64 and float64, every sum written out in the stated order (no `@`, dot or einsum:
a BLAS may fuse).  A loop over the faces, vectorised over each face's box.  Also the references of count_faces and keep_faces, and an
independent float64 ray caster (Moeller-Trumbore at the unsnapped pixel centres) that the z-buffer is pinned against."""
import collections

import numpy as np

GUARD = 16384.0
SUB = 256
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

View = collections.namedtuple("View", "H W tan pose near max_depth cull")
View.__doc__ = "tan = (tanfovx, tanfovy); pose: 12 floats, R row-major then t, world to camera; cull: 0 none, 1 back faces"


def make_view(H, W, tan=(0.7, 0.55), pose=None, near=0.2, max_depth=np.inf, cull=0):
    pose = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0) if pose is None else pose
    return View(int(H), int(W), (float(tan[0]), float(tan[1])), tuple(float(x) for x in pose), float(near), float(max_depth), int(cull))


def pose_from(rotvec, t):
    """12 floats from a rotation vector (Rodrigues) and a translation."""
    r = np.asarray(rotvec, np.float64)
    th = np.sqrt((r * r).sum())
    K = np.zeros((3, 3))
    if th > 0:
        k = r / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)       # building a pose is not part of the definition
    return tuple(R.reshape(-1).tolist()) + tuple(float(x) for x in t)


def to_camera(view, p):
    """p [..., 3] float64 -> X_c, ((r0 x + r1 y) + r2 z) + t per row."""
    R, t = view.pose[:9], view.pose[9:]
    return np.stack([((R[3 * r] * p[..., 0] + R[3 * r + 1] * p[..., 1]) + R[3 * r + 2] * p[..., 2]) + t[r] for r in range(3)], -1)


Setup = collections.namedtuple("Setup", "status U V q A cam")     # status: 0 drawn, 1..5 the counter + 1 it lands in


def setup(vertices, faces, view):
    """Steps 1 to 7 for every face."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, nV = len(f), len(v)
    status = np.zeros(F, np.int64)
    bad = ((f < 0) | (f >= nV)).any(1)
    status[bad] = 1
    fi = np.where(bad[:, None], 0, f)
    p = v[fi] if nV else np.zeros((F, 3, 3))
    with np.errstate(all="ignore"):
        c = to_camera(view, p)                                   # [F, 3 corners, 3]
        near_ok = (np.isfinite(c).all(-1) & (c[..., 2] >= view.near)).all(1)
        status[(status == 0) & ~near_ok] = 2
        u = (c[..., 0] / c[..., 2]) / view.tan[0] * (view.W * 0.5) + (view.W - 1) * 0.5
        w = (c[..., 1] / c[..., 2]) / view.tan[1] * (view.H * 0.5) + (view.H - 1) * 0.5
        guard_ok = ((np.abs(u) <= GUARD) & (np.abs(w) <= GUARD)).all(1)      # NaN fails
        status[(status == 0) & ~guard_ok] = 3
        live = status == 0
        U = np.where(live[:, None], np.rint(SUB * np.where(live[:, None], u, 0.0)), 0).astype(np.int64)
        V = np.where(live[:, None], np.rint(SUB * np.where(live[:, None], w, 0.0)), 0).astype(np.int64)
        q = 1.0 / np.where(live[:, None], c[..., 2], 1.0)
    A = (U[:, 1] - U[:, 0]) * (V[:, 2] - V[:, 0]) - (V[:, 1] - V[:, 0]) * (U[:, 2] - U[:, 0])
    status[live & (A == 0)] = 4
    if view.cull:
        status[(status == 0) & (A > 0)] = 5
    return Setup(status, U, V, q, A, c)


def edges_at(s, k, X, Y):
    """E0, E1, E2 of face k at the lattice points (X, Y) (int64 arrays), and the (d.x, d.y) of the three edges."""
    sg = 1 if s.A[k] > 0 else -1
    E, D = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = sg * (s.U[k, b] - s.U[k, a]), sg * (s.V[k, b] - s.V[k, a])
        E.append(dx * (Y - s.V[k, a]) - dy * (X - s.U[k, a]))
        D.append((dx, dy))
    return E, D


def face_normals(vertices, faces, view, s):
    """The camera-space unit normal of every drawn face, turned towards the camera; float64 [F, 3] (0 for the others)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros((len(f), 3))
    R = view.pose[:9]
    for k in np.nonzero(s.status == 0)[0]:
        p0, p1, p2 = v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]
        a, b = p1 - p0, p2 - p0
        w = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        m = np.array([(R[3 * r] * w[0] + R[3 * r + 1] * w[1]) + R[3 * r + 2] * w[2] for r in range(3)])
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        if ln > 0 and np.isfinite(ln):
            c0 = s.cam[k, 0]
            sign = -1.0 if ((m[0] * c0[0] + m[1] * c0[1]) + m[2] * c0[2]) > 0 else 1.0
            out[k] = sign * m / ln
    return out


Render = collections.namedtuple("Render", "face depth cover counts normal setup")


def render(vertices, faces, view, normals=False):
    """face [H, W] int32, depth [H, W] float32, cover [H, W] int (the faces covering each centre, before max_depth), counts [5] int64,
    normal [3, H, W] float32 or None."""
    H, W = view.H, view.W
    s = setup(vertices, faces, view)
    counts = np.array([(s.status == k).sum() for k in range(1, 6)], np.int64)
    keys = np.full((H, W), NO_KEY, np.uint64)
    cover = np.zeros((H, W), np.int64)
    md = np.float32(view.max_depth)
    for k in np.nonzero(s.status == 0)[0]:
        x0, x1 = max(-((-s.U[k].min()) // SUB), 0), min(s.U[k].max() // SUB, W - 1)       # ceil, floor
        y0, y1 = max(-((-s.V[k].min()) // SUB), 0), min(s.V[k].max() // SUB, H - 1)
        if x1 < x0 or y1 < y0:
            continue
        Y, X = np.meshgrid(SUB * np.arange(y0, y1 + 1, dtype=np.int64), SUB * np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        E, D = edges_at(s, k, X, Y)
        inside = np.ones(X.shape, bool)
        for e, (dx, dy) in zip(E, D):
            inside &= (e > 0) | ((e == 0) & ((dy > 0) or (dy == 0 and dx > 0)))
        if not inside.any():
            continue
        assert ((E[0] + E[1] + E[2]) == abs(s.A[k])).all()
        cover[y0:y1 + 1, x0:x1 + 1] += inside
        S = (E[0].astype(np.float64) * s.q[k, 0] + E[1].astype(np.float64) * s.q[k, 1]) + E[2].astype(np.float64) * s.q[k, 2]
        with np.errstate(all="ignore"):
            depth = (np.float64(abs(s.A[k])) / np.where(inside, S, 1.0)).astype(np.float32)
        ok = inside & (depth <= md)
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(k)
        box = keys[y0:y1 + 1, x0:x1 + 1]
        box[ok] = np.minimum(box[ok], key[ok])
    won = keys != NO_KEY
    face = np.where(won, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(won, (keys >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
    nmap = None
    if normals:
        n = np.concatenate([face_normals(vertices, faces, view, s), np.zeros((1, 3))]).astype(np.float32)      # never empty
        nmap = np.where(won[None], np.moveaxis(n[np.maximum(face, 0)], -1, 0), np.float32(0)).astype(np.float32)
    return Render(face, depth, cover, counts, nmap, s)


def interpolate(r, faces, attributes, view, background=0.0):
    """[C, H, W] float32: (((E0 q0) a0 + (E1 q1) a1) + (E2 q2) a2) / S for the winners of r, background elsewhere."""
    a = np.asarray(attributes, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    H, W, C = view.H, view.W, a.shape[1]
    out = np.full((C, H, W), np.float32(background), np.float32)
    s = r.setup
    ys, xs = np.nonzero(r.face >= 0)
    if len(ys) == 0:
        return out
    k = r.face[ys, xs].astype(np.int64)
    sg = np.where(s.A[k] > 0, 1, -1)
    w = []
    for i, (ea, eb) in enumerate(((1, 2), (2, 0), (0, 1))):
        dx, dy = sg * (s.U[k, eb] - s.U[k, ea]), sg * (s.V[k, eb] - s.V[k, ea])
        E = dx * (SUB * ys - s.V[k, ea]) - dy * (SUB * xs - s.U[k, ea])
        w.append((E.astype(np.float64) * s.q[k, i])[:, None])
    S = (w[0] + w[1]) + w[2]
    a0, a1, a2 = a[f[k, 0]], a[f[k, 1]], a[f[k, 2]]
    out[:, ys, xs] = (((w[0] * a0 + w[1] * a1) + w[2] * a2) / S).astype(np.float32).T
    return out


def count_faces(face_maps, F):
    """views [F] int32, pixels [F] int64 over a list of face maps."""
    views, pixels = np.zeros(F, np.int32), np.zeros(F, np.int64)
    for m in face_maps:
        m = np.asarray(m).reshape(-1)
        n = np.bincount(m[(m >= 0) & (m < F)], minlength=F)
        pixels += n
        views += n > 0
    return views, pixels


def keep_faces(keep, vertices, faces, *attrs):
    """(vertices', faces', attrs'..., dropped): the faces with keep and indices in range, in order; the vertices they use, renumbered
    densely in their order; dropped = the kept faces lost to an index out of range."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(vertices)
    inr = ((f >= 0) & (f < V)).all(1)
    k = np.asarray(keep, bool) & inr
    used = np.zeros(V, bool)
    used[f[k].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out = [np.asarray(vertices)[used], new[f[k]].astype(np.int32).reshape(-1, 3)]
    out += [None if a is None else np.asarray(a)[used] for a in attrs]
    return tuple(out) + (int((np.asarray(keep, bool) & ~inr).sum()),)


def ray_cast(vertices, faces, view):
    """Independent of the snap: the ray through every pixel centre against every triangle (Moeller-Trumbore, float64, camera space).
    -> face [H, W] (nearest hit, -1 none), z [H, W] (its camera z, inf none), z2 [H, W] (the second-nearest hit's z, inf none)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    H, W = view.H, view.W
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(px - (W - 1) * 0.5) / (W * 0.5) * view.tan[0], (py - (H - 1) * 0.5) / (H * 0.5) * view.tan[1], np.ones_like(px)], -1)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    face = np.full((H, W), -1, np.int64)
    c = to_camera(view, v)
    for k in range(len(f)):
        p0, p1, p2 = c[f[k, 0]], c[f[k, 1]], c[f[k, 2]]
        e1, e2 = p1 - p0, p2 - p0
        h = np.cross(d, e2)
        a = (h * e1).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / a
            s = -p0                                              # the origin is the camera
            uu = inv * (h * s).sum(-1)
            qv = np.cross(s, e1)
            vv = inv * (d * qv).sum(-1)
            t = inv * (qv * e2).sum(-1)
        hit = (np.abs(a) > 1e-14) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 0)
        t = np.where(hit, t, np.inf)
        closer = t < best
        second = np.where(closer, best, np.minimum(second, t))
        face = np.where(closer, k, face)
        best = np.where(closer, t, best)
    return face, best, second


def edge_distance(vertices, faces, view, face_map):
    """[H, W]: the distance in pixels from each pixel centre to the nearest edge of the (unsnapped, projected) triangle face_map names
    there; inf where it names none."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    H, W = view.H, view.W
    c = to_camera(view, v)
    uv = np.stack([(c[:, 0] / c[:, 2]) / view.tan[0] * (W * 0.5) + (W - 1) * 0.5, (c[:, 1] / c[:, 2]) / view.tan[1] * (H * 0.5) + (H - 1) * 0.5], -1)
    out = np.full((H, W), np.inf)
    ys, xs = np.nonzero(face_map >= 0)
    P = np.stack([xs, ys], -1).astype(np.float64)
    tri = uv[f[face_map[ys, xs]]]                                # [n, 3, 2]
    dist = np.full(len(P), np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        A, B = tri[:, a], tri[:, b]
        ab = B - A
        tt = np.clip(((P - A) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
        dist = np.minimum(dist, np.sqrt((((A + tt[:, None] * ab) - P) ** 2).sum(-1)))
    out[ys, xs] = dist
    return out
