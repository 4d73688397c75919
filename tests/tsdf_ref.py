"""The float64 numpy reference of include/adgs_tsdf.h: TSDF integration of one rendered view and marching tetrahedra on a volume.

Integration evaluates the header's chain in float64 from the float32 inputs and stores float32 after every view.  It also returns the
near-gate flags of a view: the lattice points whose decision a different but equally valid evaluation order could flip -- `u + 0.5` or
`v + 0.5` within 1e-9 * size of an integer (the nearest pixel), z within 1e-9 of `near`, sdf within 1e-9 of -trunc, z_d within 1e-9 of
max_depth.  Tests compare outside them.

Extraction follows the header literally; the orientation of a triangle is DERIVED here (its right-hand normal must point from the
inside corners of its tet to the outside ones), which is what pins the kernel's constant table."""
import itertools

import numpy as np

SLOTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))          # the 7 edges a lattice point owns
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))                     # the axis orders of the 6 Kuhn tets
EVEN = (True, False, False, True, True, False)


def tet_corners(t):
    """The 4 corner offsets (x, y, z) of tet t of the unit cell: c, c + e_a, c + e_a + e_b, c + (1, 1, 1)."""
    a, b, _ = ORDERS[t]
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return ((0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1))


def tet_triangles(m):
    """The triangles of a tet with inside set m (bit q: tet vertex q inside) BEFORE orientation, as tuples of (tet vertex, tet vertex) edges."""
    ins = [q for q in range(4) if (m >> q) & 1]
    outs = [q for q in range(4) if not (m >> q) & 1]
    if len(ins) == 1:
        a = ins[0]
        return [((a, outs[0]), (a, outs[1]), (a, outs[2]))]
    if len(ins) == 3:
        d = outs[0]
        return [((d, ins[2]), (d, ins[1]), (d, ins[0]))]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = ((a, c), (a, d), (b, d), (b, c))
        return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return []


def reversed_sets(t):
    """The inside sets of tet t whose triangles must be reversed: decided geometrically, with the vertices at the edge midpoints (the
    orientation of a cut does not depend on where along its edges the vertices lie)."""
    P = np.array(tet_corners(t), dtype=np.float64)
    out = []
    for m in range(1, 15):
        ins = [q for q in range(4) if (m >> q) & 1]
        outs = [q for q in range(4) if not (m >> q) & 1]
        want = P[outs].mean(0) - P[ins].mean(0)
        signs = []
        for tri in tet_triangles(m):
            p = [0.5 * (P[a] + P[b]) for a, b in tri]
            signs.append(float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), want)))
        assert all(s != 0 for s in signs) and len({s > 0 for s in signs}) == 1, (t, m, signs)
        if signs[0] < 0:
            out.append(m)
    return out


def f32(x):
    return np.float64(np.float32(x))


class Volume:
    """tsdf, wsum [nz, ny, nx] and color [3, nz, ny, nx] (or None) as float32 numpy arrays; origin and voxel_size are rounded to float32
    as the ABI carries them."""

    def __init__(self, origin, voxel_size, dims, color=True):
        self.origin = np.array([f32(o) for o in origin])
        self.voxel_size = f32(voxel_size)
        self.dims = tuple(int(d) for d in dims)                 # (nx, ny, nz)
        nx, ny, nz = self.dims
        self.tsdf = np.ones((nz, ny, nx), np.float32)
        self.wsum = np.zeros((nz, ny, nx), np.float32)
        self.color = np.zeros((3, nz, ny, nx), np.float32) if color else None

    def copy(self):
        v = Volume(self.origin, self.voxel_size, self.dims, self.color is not None)
        v.tsdf, v.wsum = self.tsdf.copy(), self.wsum.copy()
        v.color = None if self.color is None else self.color.copy()
        return v

    def points(self):
        """X [nz, ny, nx, 3] float64."""
        nx, ny, nz = self.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return self.origin + self.voxel_size * np.stack([i, j, k], -1).astype(np.float64)


def integrate(vol, depth, opacity, tan, pose, image=None, weight=None, inv_depth=True, min_opacity=0.5, near=0.2, max_depth=np.inf, trunc=None,
              max_weight=64.0):
    """One view into `vol` (in place).  depth, opacity [H, W], image [3, H, W], weight [H, W]: float32 arrays; pose [3, 4] float64 (R | t),
    world to camera.  -> (updated [nz, ny, nx] bool, flagged [nz, ny, nx] bool)."""
    D, O = np.asarray(depth, np.float32), np.asarray(opacity, np.float32)
    H, W = D.shape
    pose = np.asarray(pose, np.float64)
    R, t = pose[:, :3], pose[:, 3]
    tx, ty = f32(tan[0]), f32(tan[1])
    near, max_depth, max_weight, mo = f32(near), f32(max_depth), f32(max_weight), f32(min_opacity)
    trunc = f32(4 * vol.voxel_size if trunc is None else trunc)
    Xc = vol.points() @ R.T + t
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    front = z > near
    flagged = np.abs(z - near) <= 1e-9
    zs = np.where(front, z, 1.0)
    u = (x / zs) / tx * W / 2 + (W - 1) / 2
    v = (y / zs) / ty * H / 2 + (H - 1) / 2
    uf, vf = np.floor(u + 0.5), np.floor(v + 0.5)
    tie = (np.abs(u + 0.5 - np.round(u + 0.5)) <= 1e-9 * W) | (np.abs(v + 0.5 - np.round(v + 0.5)) <= 1e-9 * H)
    flagged |= front & tie
    inside = front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    xi, yi = np.where(inside, uf, 0).astype(np.int64), np.where(inside, vf, 0).astype(np.int64)
    Op, Dp = O[yi, xi], D[yi, xi]
    wp = np.ones_like(Op) if weight is None else np.asarray(weight, np.float32)[yi, xi]
    good = inside & (Op >= np.float32(mo)) & (Dp > 0) & (wp > 0)
    Od, Dd = Op.astype(np.float64), np.where(good, Dp, 1).astype(np.float64)
    zd = Od / Dd if inv_depth else Dd / np.where(good, Od, 1.0)
    flagged |= good & (np.abs(zd - max_depth) <= 1e-9)
    good &= zd <= max_depth
    sdf = zd - z
    flagged |= good & (np.abs(sdf + trunc) <= 1e-9)
    upd = good & (sdf >= -trunc)
    d = np.minimum(1.0, sdf / trunc)
    w = wp.astype(np.float64)
    W0 = vol.wsum.astype(np.float64)
    Wn = np.where(upd, W0 + w, 1.0)
    vol.tsdf = np.where(upd, (vol.tsdf.astype(np.float64) * W0 + d * w) / Wn, vol.tsdf).astype(np.float32)
    if vol.color is not None:
        assert image is not None
        Ip = np.asarray(image, np.float32)[:, yi, xi].astype(np.float64)
        vol.color = np.where(upd[None], (vol.color.astype(np.float64) * W0 + Ip * w) / Wn, vol.color).astype(np.float32)
    vol.wsum = np.where(upd, np.minimum(W0 + w, max_weight), vol.wsum).astype(np.float32)
    return upd, flagged


def extract(vol, min_weight=1.0):
    """-> (vertices [V, 3] float64, faces [F, 3] int32, colors [V, 3] float64 or None) of the header's marching tetrahedra, in its order."""
    nx, ny, nz = vol.dims
    n = nx * ny * nz
    T = vol.tsdf.astype(np.float64)
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int32), None if vol.color is None else np.zeros((0, 3)))
    if min(nx, ny, nz) < 2:
        return empty
    inside = vol.tsdf < 0
    ok = vol.wsum >= np.float32(min_weight)
    cell = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        cell &= ok[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    # exists[k, j, i, s]: the vertex on the edge from (i, j, k) along slot s
    exists = np.zeros((nz, ny, nx, 7), bool)
    for s, (ox, oy, oz) in enumerate(SLOTS):
        used = np.zeros((nz, ny, nx), bool)                     # some valid cell contains the edge
        for bz, by, bx in itertools.product((0, 1), repeat=3):  # the edge starts at corner b of the cell and must end inside it
            if bx + ox <= 1 and by + oy <= 1 and bz + oz <= 1:
                used[bz:bz + nz - 1, by:by + ny - 1, bx:bx + nx - 1] |= cell
        cut = np.zeros((nz, ny, nx), bool)
        cut[:nz - oz, :ny - oy, :nx - ox] = inside[:nz - oz, :ny - oy, :nx - ox] != inside[oz:, oy:, ox:]
        exists[..., s] = used & cut
    flat = exists.reshape(-1)
    ids = (np.cumsum(flat) - 1).reshape(n, 7)
    ids = np.where(exists.reshape(n, 7), ids, -1)
    owner, slot = np.nonzero(exists.reshape(n, 7))
    off = np.array(SLOTS)[slot]                                 # (ox, oy, oz)
    pi, pj, pk = owner % nx, (owner // nx) % ny, owner // (nx * ny)
    q = owner + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    Tf = T.reshape(-1)
    tt = Tf[owner] / (Tf[owner] - Tf[q])
    P = np.stack([pi, pj, pk], -1).astype(np.float64)
    vertices = vol.origin + vol.voxel_size * (P + tt[:, None] * off)
    colors = None
    if vol.color is not None:
        C = vol.color.reshape(3, -1).astype(np.float64)
        colors = (C[:, owner] + tt * (C[:, q] - C[:, owner])).T.copy()
    # faces
    ck, cj, ci = np.nonzero(cell)
    cidx = (ck * ny + cj) * nx + ci                              # ascending
    insf = inside.reshape(-1)
    slot_of = {o: s for s, o in enumerate(SLOTS)}
    keys, tris = [], []
    for t in range(6):
        corners = tet_corners(t)
        lin = [cidx + c[0] + c[1] * nx + c[2] * nx * ny for c in corners]
        m = sum(insf[lin[qv]].astype(np.int64) << qv for qv in range(4))
        rev = set(reversed_sets(t))
        for mv in range(1, 15):
            sel = np.nonzero(m == mv)[0]
            if not sel.size:
                continue
            for r, tri in enumerate(tet_triangles(mv)):
                cols = []
                for a, b in tri:
                    lo, hi = min(a, b), max(a, b)
                    s = slot_of[tuple(h - l for h, l in zip(corners[hi], corners[lo]))]
                    vid = ids[lin[lo][sel], s]
                    assert (vid >= 0).all()
                    cols.append(vid)
                if mv in rev:
                    cols = cols[::-1]
                tris.append(np.stack(cols, -1))
                keys.append((cidx[sel] * 6 + t) * 2 + r)
    if not tris:
        return vertices, np.zeros((0, 3), np.int32), colors
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.argsort(keys, kind="stable")
    return vertices, tris[order].astype(np.int32), colors


# ---- mesh properties the tests assert ----

def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_stats(faces):
    """(directed edges used more than once, directed edges whose opposite is missing, undirected edges)."""
    e = directed_edges(faces)
    big = int(e.max()) + 1 if e.size else 1
    code = e[:, 0] * big + e[:, 1]
    uniq, cnt = np.unique(code, return_counts=True)
    opp = e[:, 1] * big + e[:, 0]
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * big + np.maximum(e[:, 0], e[:, 1]))
    return int((cnt > 1).sum()), int((~np.isin(opp, uniq)).sum()), int(und.size)


def signed_volume(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def face_normals(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
