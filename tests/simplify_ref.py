"""The numpy float64 oracle of include/adgs_simplify.h: vertex clustering on a lattice, the face rules, the output numbering and the two
placements, with the summation orders of the definition (np.add.at adds in index order, one element at a time).  Nothing here shares code
with the device: clusters come from np.unique over the integer cells, duplicates from np.unique over the rotated triples."""
import types

import numpy as np

AXIS_LIMIT = 2.0 ** 20


def lattice(cell_size, origin):
    """The float32 values the device is given, as doubles."""
    return float(np.float32(cell_size)), np.asarray(origin, np.float32).astype(np.float64)


def cells_of(vertices, cell, origin):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((vertices.astype(np.float64) - origin) / cell)


def rotated(triples):
    """Every row rotated so that its smallest entry is first (the cyclic order, hence the orientation, kept)."""
    t = np.asarray(triples).reshape(-1, 3)
    k = np.argmin(t, axis=1)
    return np.take_along_axis(t, (k[:, None] + np.arange(3)[None, :]) % 3, axis=1)


def first_of_each(triples):
    """Indices (ascending) of the rows that are the first with their value."""
    if len(triples) == 0:
        return np.zeros(0, np.int64)
    _, first = np.unique(triples, axis=0, return_index=True)
    return np.sort(first)


def cluster(vertices, faces, cell_size, origin=(0.0, 0.0, 0.0)):
    """Steps 1-4 -> namespace(vertex_cluster, root, num_vertices, members, member_starts, faces, face_source, counts, cell, origin)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(v)
    cell, org = lattice(cell_size, origin)
    bad = ((f < 0) | (f >= V)).any(axis=1)
    if bad.any():
        raise ValueError("%d faces index outside the %d vertices" % (int(bad.sum()), V))
    finite = np.isfinite(v).all(axis=1)
    c = cells_of(v, cell, org)
    unkeyed = finite & (np.abs(c) >= AXIS_LIMIT).any(axis=1)
    if unkeyed.any():
        raise ValueError("%d vertices lie 2^20 cells or more from the origin: enlarge cell_size or move origin" % int(unkeyed.sum()))
    kc = np.full(V, -1, np.int64)                               # the cluster of a vertex, clusters in any order
    ids = np.flatnonzero(finite)
    K = 0
    if len(ids):
        _, inv = np.unique(c[ids].astype(np.int64), axis=0, return_inverse=True)
        kc[ids] = inv.reshape(-1)
        K = int(kc.max()) + 1
    kroot = np.full(K, V, np.int64)
    np.minimum.at(kroot, kc[ids], ids)
    fc = kc[f.astype(np.int64)]                                 # [F, 3]
    dropped = (fc < 0).any(axis=1)
    degenerate = ~dropped & ((fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2]))
    rest = np.flatnonzero(~dropped & ~degenerate)
    # compare by the ROOTS of the clusters: equal clusters have equal roots, and the result cannot depend on how np.unique numbered them
    keep = rest[first_of_each(rotated(kroot[fc[rest]]))]
    used = np.zeros(K, bool)
    used[fc[keep].reshape(-1)] = True
    out_roots = np.sort(kroot[used])                            # output vertices by ascending root
    out_of_cluster = np.full(K + 1, -1, np.int64)               # [-1] serves kc = -1
    out_of_cluster[np.flatnonzero(used)] = np.searchsorted(out_roots, kroot[used])
    vc = out_of_cluster[kc]
    V2 = len(out_roots)
    inside = np.flatnonzero(vc >= 0)                            # ascending vertex id
    members = inside[np.argsort(vc[inside], kind="stable")]
    num = np.bincount(vc[inside], minlength=V2)
    starts = np.concatenate([[0], np.cumsum(num)])
    counts = {"nonfinite_vertices": int((~finite).sum()), "dropped_faces": int(dropped.sum()), "degenerate_faces": int(degenerate.sum()),
              "duplicate_faces": int(len(rest) - len(keep))}
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return types.SimpleNamespace(vertex_cluster=i32(vc), root=i32(out_roots), num_vertices=i32(num), members=i32(members), member_starts=i32(starts),
                                 faces=i32(vc[f[keep].astype(np.int64)]).reshape(-1, 3), face_source=i32(keep), counts=counts, cell=cell, origin=org)


def quadrics(cl, vertices, faces):
    """cbar [V2, 3] and the sums A [V2, 3, 3], g [V2, 3], t [V2] of the definition, in its order."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    V2 = len(cl.root)
    vc = cl.vertex_cluster.astype(np.int64)
    inside = np.flatnonzero(vc >= 0)
    S = np.zeros((V2, 3))
    np.add.at(S, vc[inside], v[inside])
    n = cl.num_vertices.astype(np.float64)[:, None]
    cbar = S / n
    A, g, t = np.zeros((V2, 3, 3)), np.zeros((V2, 3)), np.zeros(V2)
    if len(f) and V2:
        p = v[f]                                                # [F, 3, 3]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            kx, ky, kz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
            L = np.sqrt(kx * kx + ky * ky + kz * kz)
            ok = np.isfinite(p).all(axis=(1, 2)) & (L > 0.0)
            nrm = np.stack([kx / L, ky / L, kz / L], 1)
        w = L / 2.0
        corner_cluster = vc[f].reshape(-1)                      # corner id 3 f + k, ascending
        face_of = np.repeat(np.arange(len(f)), 3)
        sel = np.flatnonzero(ok[face_of] & (corner_cluster >= 0))
        cc, ff = corner_cluster[sel], face_of[sel]
        d = p.reshape(-1, 3)[sel] - cbar[cc]
        nn, ww = nrm[ff], w[ff]
        e = nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1] + nn[:, 2] * d[:, 2]
        for i in range(3):
            for j in range(3):
                np.add.at(A[:, i, j], cc, ww * nn[:, i] * nn[:, j])
            np.add.at(g[:, i], cc, ww * e * nn[:, i])
        np.add.at(t, cc, ww)
    return cbar, A, g, t


def cell_box(cl, vertices):
    """lo, hi [V2, 3] of the cell of every output vertex."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    c = cells_of(v[cl.root], cl.cell, cl.origin)
    return cl.origin + c * cl.cell, cl.origin + (c + 1.0) * cl.cell


def solve(cl, vertices, faces, regularization=1e-3):
    """(cbar, delta before the clamp, delta, clamp bounds) of the quadric placement."""
    cbar, A, g, t = quadrics(cl, vertices, faces)
    delta = np.zeros_like(cbar)
    on = t > 0.0
    if on.any():
        M = A[on] + (regularization * t[on])[:, None, None] * np.eye(3)[None]
        delta[on] = np.linalg.solve(M, g[on][:, :, None])[:, :, 0]
    lo, hi = cell_box(cl, vertices)
    dmin, dmax = np.minimum(lo - cbar, 0.0), np.maximum(hi - cbar, 0.0)
    return cbar, delta, np.minimum(np.maximum(delta, dmin), dmax), (dmin, dmax)


def place(cl, vertices, faces, colors=None, placement="quadric", regularization=1e-3):
    """Step 5 -> (vertices2 float32, colors2 float32 or None)."""
    if placement not in ("quadric", "average"):
        raise ValueError(placement)
    if placement == "quadric":
        cbar, _, delta, _ = solve(cl, vertices, faces, regularization)
    else:
        cbar = quadrics(cl, vertices, np.zeros((0, 3), np.int32))[0]
        delta = np.zeros_like(cbar)
    out = (cbar + delta).astype(np.float32)
    col = None
    if colors is not None:
        c = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
        vc = cl.vertex_cluster.astype(np.int64)
        inside = np.flatnonzero(vc >= 0)
        S = np.zeros((len(cl.root), 3))
        np.add.at(S, vc[inside], c[inside])
        col = (S / cl.num_vertices.astype(np.float64)[:, None]).astype(np.float32)
    return out, col


def simplify(vertices, faces, colors=None, cell_size=1.0, origin=(0.0, 0.0, 0.0), placement="quadric", regularization=1e-3):
    cl = cluster(vertices, faces, cell_size, origin)
    out, col = place(cl, vertices, faces, colors, placement, regularization)
    return out, cl.faces, col
