"""The float64 numpy reference of include/adgs_sparse_tsdf.h: the allocation rule of a view, integration over a set of blocks (through
tests/tsdf_ref.integrate on the blocks' points) and marching tetrahedra on the unbounded lattice in the sparse order.  The tables and the
triangle rules are those of tests/tsdf_ref.py.

Allocation also returns the FLAGGED samples: those whose decision an equally valid evaluation order could flip -- a face of the sample's
cube within 1e-9 block of a block boundary, z_m within 1e-9 of `near`, z_d within 1e-9 of max_depth.  Tests compare key sets outside the
blocks that only flagged samples reach."""
import collections
import itertools
import math

import numpy as np

from tests import tsdf_ref as ref

B = 8
LIMIT = 1 << 20


def block_key(b):
    """The key of block coordinates [..., 3] (bx, by, bz) as int64."""
    b = np.asarray(b, np.int64) + LIMIT
    return (b[..., 2] << 42) | (b[..., 1] << 21) | b[..., 0]


Allocation = collections.namedtuple("Allocation", "sure flagged maybe skipped")


def steps_of(trunc, voxel_size):
    """n = ceil(trunc / voxel_size) from the float32 fields, in double."""
    return int(math.ceil(ref.f32(trunc) / ref.f32(voxel_size)))


def allocation(depth, opacity, tan, pose, origin, voxel_size, trunc, margin=2.0, weight=None, inv_depth=True, min_opacity=0.5, near=0.2,
               max_depth=np.inf):
    """The blocks one view marks -> Allocation(sure, flagged, maybe, skipped): `sure` the set of (bx, by, bz) marked by samples that are not
    flagged, `flagged` what the flagged samples mark by this evaluation's own decision, `maybe` every block a flagged sample could mark
    under either decision (a superset of `flagged`), `skipped` the number of samples with a block coordinate outside the range."""
    D, O = np.asarray(depth, np.float32), np.asarray(opacity, np.float32)
    H, W = D.shape
    pose = np.asarray(pose, np.float64)
    R, t = pose[:, :3], pose[:, 3]
    o = np.array([ref.f32(v) for v in origin])
    vs, tr, rho = ref.f32(voxel_size), ref.f32(trunc), ref.f32(margin)
    near, max_depth, mo = ref.f32(near), ref.f32(max_depth), np.float32(min_opacity)
    kx, ky = W / (2.0 * ref.f32(tan[0])), H / (2.0 * ref.f32(tan[1]))
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    w = np.ones_like(O) if weight is None else np.asarray(weight, np.float32)
    good = (O >= mo) & (D > 0) & (w > 0)
    Od, Dd = O.astype(np.float64), np.where(good, D, 1).astype(np.float64)
    zd = Od / Dd if inv_depth else Dd / np.where(good, Od, 1.0)
    tie = good & (np.abs(zd - max_depth) <= 1e-9)
    good &= zd <= max_depth
    yi, xi = np.nonzero(good)
    zd, tie = zd[yi, xi], tie[yi, xi]
    rx, ry = (xi - cx) / kx, (yi - cy) / ky
    n = steps_of(trunc, voxel_size)
    sure, flagged, maybe, skipped = set(), set(), set(), 0
    for m in range(n + 1):
        zm = zd - tr + m * (2.0 * tr / n)
        live = zm > near
        flag = tie | (np.abs(zm - near) <= 1e-9)
        Xc = np.stack([rx * zm, ry * zm, zm], -1)
        g = ((Xc - t) @ R - o) / vs                              # R^T (X_c - t) as row vectors
        lo_f, hi_f = (g - rho) / B, (g + rho) / B
        flag |= (np.abs(lo_f - np.round(lo_f)) <= 1e-9).any(-1) | (np.abs(hi_f - np.round(hi_f)) <= 1e-9).any(-1)
        lo, hi = np.floor(lo_f), np.floor(hi_f)
        inside = np.isfinite(g).all(-1) & (lo >= -LIMIT).all(-1) & (hi < LIMIT).all(-1)
        skipped += int((live & ~inside & ~flag).sum())
        finite = np.isfinite(g).all(-1)
        for sel, out, grow in ((live & inside & ~flag, sure, 0), (live & inside & flag, flagged, 0),
                               ((live | (np.abs(zm - near) <= 1e-9)) & flag & finite, maybe, 1)):
            l, h = lo[sel].astype(np.int64) - grow, hi[sel].astype(np.int64) + grow
            for c in itertools.product(*([range(2 + 2 * grow)] * 3)):
                b = np.minimum(l + np.array(c), h)
                out.update(map(tuple, np.unique(b, axis=0)))
    maybe = {b for b in maybe if all(-LIMIT <= v < LIMIT for v in b)}
    return Allocation(sure, flagged, maybe, skipped)


class BlockVolume(ref.Volume):
    """The points of a list of blocks as a tests/tsdf_ref.Volume: block r occupies the z-slabs 8 r .. 8 r + 7 of arrays [8 NB, 8, 8], and
    its points are origin + voxel_size (8 b + l), formed from the GLOBAL index as the header says."""

    def __init__(self, origin, voxel_size, blocks, color=True):
        self.blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
        super().__init__(origin, voxel_size, (B, B, B * len(self.blocks)), color)

    def copy(self):
        v = BlockVolume(self.origin, self.voxel_size, self.blocks, self.color is not None)
        v.tsdf, v.wsum = self.tsdf.copy(), self.wsum.copy()
        v.color = None if self.color is None else self.color.copy()
        return v

    def points(self):
        l = np.stack(np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij")[::-1], -1)     # [lz, ly, lx, (x, y, z)]
        idx = (B * self.blocks[:, None, None, None, :] + l[None]).reshape(-1, B, B, 3)
        return self.origin + self.voxel_size * idx.astype(np.float64)

    def pool(self):
        """(tsdf [NB, 8, 8, 8], wsum [NB, 8, 8, 8], color [NB, 3, 8, 8, 8] or None) in the order of `blocks`."""
        nb = len(self.blocks)
        c = None if self.color is None else self.color.reshape(3, nb, B, B, B).transpose(1, 0, 2, 3, 4)
        return self.tsdf.reshape(nb, B, B, B), self.wsum.reshape(nb, B, B, B), c


def from_dense(vol, offset=(0, 0, 0)):
    """The blocks that cover the dense tests/tsdf_ref.Volume `vol` when its lattice point (0, 0, 0) is the sparse lattice's 8 offset, as a
    BlockVolume with the dense values and 1 / 0 / 0 in the padding; its origin is vol.origin - 8 voxel_size offset."""
    nx, ny, nz = vol.dims
    nb = [-(-d // B) for d in (nx, ny, nz)]
    pad = lambda a, fill: np.pad(a, [(0, 0)] * (a.ndim - 3) + [(0, B * nb[2] - nz), (0, B * nb[1] - ny), (0, B * nb[0] - nx)], constant_values=fill)
    blocks = np.array([(x, y, z) for z in range(nb[2]) for y in range(nb[1]) for x in range(nb[0])], np.int64).reshape(-1, 3)
    out = BlockVolume(vol.origin - B * vol.voxel_size * np.array(offset), vol.voxel_size, blocks + np.array(offset), vol.color is not None)
    split = lambda a: a.reshape(nb[2], B, nb[1], B, nb[0], B).transpose(0, 2, 4, 1, 3, 5).reshape(-1, B, B)
    out.tsdf, out.wsum = split(pad(vol.tsdf, 1.0)), split(pad(vol.wsum, 0.0))
    if vol.color is not None:
        out.color = np.stack([split(pad(vol.color[c], 0.0)) for c in range(3)])
    return out


def extract(vol, min_weight=1.0):
    """Marching tetrahedra on the unbounded lattice of a BlockVolume, a point in no block counting as tsdf 1 / wsum 0 -> (vertices [V, 3]
    float64, faces [F, 3] int32, colors or None) in the sparse order: vertices by (block key of the owner, local index, slot), faces by
    (block key of the cell's lowest corner, local index, tet, triangle)."""
    assert min_weight > 0
    nb = len(vol.blocks)
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int32), None if vol.color is None else np.zeros((0, 3)))
    if nb == 0:
        return empty
    keys = block_key(vol.blocks)
    order = np.argsort(keys)
    skeys = keys[order]
    assert (np.diff(skeys) > 0).all()
    T, Wt, C = vol.pool()
    T, Wt = T[order].reshape(-1), Wt[order].reshape(-1)
    C = None if C is None else C[order].transpose(1, 0, 2, 3, 4).reshape(3, -1)
    # the points in the sparse order: rank of the block, then (lz 8 + ly) 8 + lx
    lz, ly, lx = np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij")
    local = np.stack([lx, ly, lz], -1).reshape(-1, 3)
    P = (B * vol.blocks[order][:, None, :] + local[None]).reshape(-1, 3)           # global indices [NB 512, 3]

    def index_of(Q):
        """The position in the sparse order of the global lattice points Q [..., 3], -1 where the block is not allocated."""
        Q = np.asarray(Q, np.int64)
        b = Q >> 3
        ok = ((b >= -LIMIT) & (b < LIMIT)).all(-1)
        k = block_key(np.where(ok[..., None], b, 0))
        r = np.minimum(np.searchsorted(skeys, k), nb - 1)
        ok &= skeys[r] == k
        l = Q & 7
        return np.where(ok, r * 512 + (l[..., 2] * B + l[..., 1]) * B + l[..., 0], -1)

    def values(Q):
        i = index_of(Q)
        return np.where(i >= 0, T[i], np.float32(1.0)), np.where(i >= 0, Wt[i], np.float32(0.0)), i

    inside = T < 0
    # valid[q]: the cell whose lowest corner is P + q - 1, q in {0, 1}^3 (the 8 cells around P), has 8 observed corners
    okc = {d: values(P + np.array(d))[1] >= np.float32(min_weight) for d in itertools.product((-1, 0, 1), repeat=3)}
    valid = {}
    for q in itertools.product((0, 1), repeat=3):
        v = np.ones(len(P), bool)
        for e in itertools.product((0, 1), repeat=3):
            v &= okc[tuple(q[a] - 1 + e[a] for a in range(3))]
        valid[q] = v
    exists = np.zeros((len(P), 7), bool)
    ends = []
    for s, off in enumerate(ref.SLOTS):
        Tq, _, iq = values(P + np.array(off))
        ends.append(iq)
        used = np.zeros(len(P), bool)
        for q in itertools.product((0, 1), repeat=3):         # the cell starts at P on the axes the edge spans, at P - 1 or P on the others
            if all(q[a] == 1 for a in range(3) if off[a]):
                used |= valid[q]
        exists[:, s] = used & (inside != (Tq < 0))
    ids = np.where(exists, (np.cumsum(exists.reshape(-1)) - 1).reshape(-1, 7), -1)
    owner, slot = np.nonzero(exists)
    off = np.array(ref.SLOTS)[slot]
    q = np.array(ends)[slot, owner]
    assert (q >= 0).all()
    Td = T.astype(np.float64)
    tt = Td[owner] / (Td[owner] - Td[q])
    vertices = vol.origin + vol.voxel_size * (P[owner].astype(np.float64) + tt[:, None] * off)
    colors = None
    if C is not None:
        Cd = C.astype(np.float64)
        colors = (Cd[:, owner] + tt * (Cd[:, q] - Cd[:, owner])).T.copy()
    # faces: the cells whose lowest corner is a point of the order
    cells = np.nonzero(valid[(1, 1, 1)])[0]
    slot_of = {o: s for s, o in enumerate(ref.SLOTS)}
    fkeys, tris = [], []
    for t in range(6):
        corners = ref.tet_corners(t)
        at = [index_of(P[cells] + np.array(c)) for c in corners]
        m = sum(inside[a].astype(np.int64) << qv for qv, a in enumerate(at))
        rev = set(ref.reversed_sets(t))
        for mv in range(1, 15):
            sel = np.nonzero(m == mv)[0]
            if not sel.size:
                continue
            for r, tri in enumerate(ref.tet_triangles(mv)):
                cols = []
                for a, b in tri:
                    lo, hi = min(a, b), max(a, b)
                    s = slot_of[tuple(h - l for h, l in zip(corners[hi], corners[lo]))]
                    vid = ids[at[lo][sel], s]
                    assert (vid >= 0).all()
                    cols.append(vid)
                if mv in rev:
                    cols = cols[::-1]
                tris.append(np.stack(cols, -1))
                fkeys.append((cells[sel] * 6 + t) * 2 + r)
    if not tris:
        return vertices, np.zeros((0, 3), np.int32), colors
    fkeys, tris = np.concatenate(fkeys), np.concatenate(tris)
    return vertices, tris[np.argsort(fkeys, kind="stable")].astype(np.int32), colors


def match_meshes(a, b, quantum=0.0):
    """Whether two meshes (vertices, faces, colors) are equal up to the order of vertices and faces: the vertex rows (with the colours) must
    be equal as a multiset -- and distinct, so that the permutation is unique --, the faces equal after mapping through it and sorting.
    quantum > 0: positions are compared as multiples of it (two float64 evaluations of one position from differently placed origins differ
    by rounding; a quantum of 2^-24 voxel is far above that and far below the distance of two vertices)."""
    Va, Fa, Ca = a
    Vb, Fb, Cb = b
    if len(Va) != len(Vb) or len(Fa) != len(Fb) or (Ca is None) != (Cb is None):
        return False
    if len(Va) == 0:
        return len(Fa) == 0
    ra, rb = np.asarray(Va, np.float64), np.asarray(Vb, np.float64)
    if quantum > 0:
        ra, rb = np.round(ra / quantum), np.round(rb / quantum)
    oa, ob = np.lexsort(ra.T[::-1]), np.lexsort(rb.T[::-1])
    if not np.array_equal(ra[oa], rb[ob]) or (np.diff(ra[oa], axis=0) == 0).all(1).any():
        return False
    if Ca is not None and not np.array_equal(np.asarray(Ca, np.float64)[oa], np.asarray(Cb, np.float64)[ob]):
        return False
    to_b = np.empty(len(ra), np.int64)
    to_b[oa] = ob                                               # vertex i of a is vertex to_b[i] of b
    fa, fb = to_b[np.asarray(Fa, np.int64)], np.asarray(Fb, np.int64)
    return np.array_equal(fa[np.lexsort(fa.T[::-1])], fb[np.lexsort(fb.T[::-1])])
