"""The integer / float64 numpy reference of include/adgs_mesh.h: connected components by a sequential union-find (no scipy), the
component table, the 2DGS selection rule, keep, areas and area-weighted vertex normals.

Faces with an index outside [0, V) are left out of everything (`valid_faces`), as the kernels skip them.  normals() also returns S_v and
the per-vertex flag |sum| < 2^-20 S_v: the vertices whose direction is a cancellation, which the GPU test leaves out of its comparison."""
import collections

import numpy as np

Components = collections.namedtuple("Components", "vertex_component root num_faces num_vertices area")


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def components(faces, V, vertices=None):
    """-> Components (int32 arrays; area float64 or None), numbered by ascending smallest vertex index."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f[ok].tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    rootof = np.array([find(v) for v in range(V)], np.int64).reshape(V)
    root = np.nonzero(rootof == np.arange(V))[0]
    number = np.full(V, -1, np.int64)
    number[root] = np.arange(root.size)
    vc = number[rootof]
    C = root.size
    nv = np.bincount(vc, minlength=C)
    fc = vc[f[ok, 0]]
    nf = np.bincount(fc, minlength=C)
    area = None
    if vertices is not None:
        area = np.bincount(fc, weights=face_areas(vertices, f[ok]), minlength=C).astype(np.float64)
    return Components(vc.astype(np.int32), root.astype(np.int32), nf.astype(np.int32), nv.astype(np.int32), area)


def face_cross(vertices, faces):
    p = np.asarray(vertices, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p


def face_areas(vertices, faces):
    return 0.5 * np.linalg.norm(face_cross(vertices, faces)[0], axis=1)


def edge_products(vertices, faces):
    """|p1 - p0| |p2 - p0| per face."""
    p = face_cross(vertices, faces)[1]
    return np.linalg.norm(p[:, 1] - p[:, 0], axis=1) * np.linalg.norm(p[:, 2] - p[:, 0], axis=1)


def area_bounds(comps, vertices, faces):
    """S_c: the sum over the component's faces of 0.5 |p1 - p0| |p2 - p0|."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, len(comps.vertex_component))]
    return np.bincount(comps.vertex_component[f[:, 0]], weights=0.5 * edge_products(vertices, f), minlength=len(comps.root))


def select(num_faces, largest=50, min_faces=50, area=None, min_area=None):
    """2DGS post_process_mesh: keep num_faces >= max(min_faces, the largest-th largest count; the smallest with fewer components)."""
    n = np.asarray(num_faces, np.int64)
    if n.size == 0:
        return np.zeros(0, bool)
    kth = np.sort(n)[::-1][min(largest, n.size) - 1]
    keep = n >= max(int(kth), min_faces)
    if min_area is not None:
        keep &= np.asarray(area) >= min_area
    return keep


def keep(comps, keep_mask, vertices, faces, colors=None, normals=None):
    """-> (vertices, faces int32, colors, normals): gathers, order preserved."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(comps.vertex_component)
    kv = np.asarray(keep_mask, bool)[comps.vertex_component] if V else np.zeros(0, bool)
    ok = valid_faces(f, V)
    kf = ok.copy()
    kf[ok] = kv[f[ok, 0]]
    new = np.cumsum(kv) - 1
    g = lambda a: None if a is None else np.asarray(a)[kv]
    return g(vertices), new[f[kf]].astype(np.int32).reshape(-1, 3), g(colors), g(normals)


def remove_small_components(vertices, faces, colors=None, largest=50, min_faces=50, min_area=None):
    comps = components(faces, len(vertices), vertices if min_area is not None else None)
    return keep(comps, select(comps.num_faces, largest, min_faces, comps.area, min_area), vertices, faces, colors)[:3]


def normals(vertices, faces):
    """-> (normals [V, 3] float64, S [V], flagged [V] bool: 0 < |sum| < 2^-20 S_v)."""
    V = len(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    n, _ = face_cross(vertices, f)
    e = edge_products(vertices, f)
    total, S = np.zeros((V, 3)), np.zeros(V)
    for c in range(3):                                          # a face counts once per corner that is v
        np.add.at(total, f[:, c], n)
        np.add.at(S, f[:, c], e)
    length = np.linalg.norm(total, axis=1)
    zero = (S == 0) | (length <= 2.0 ** -40 * S)
    out = np.where(zero[:, None], 0.0, total / np.where(zero, 1.0, length)[:, None])
    return out, S, ~zero & (length < 2.0 ** -20 * S)


def bfs_components(faces, V):
    """An independent labelling: breadth-first search over vertex adjacency -> the smallest vertex of every vertex's component."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    adj = [[] for _ in range(V)]
    for a, b, c in f.tolist():
        adj[a] += (b, c); adj[b] += (a, c); adj[c] += (a, b)
    label = np.full(V, -1, np.int64)
    for s in range(V):
        if label[s] >= 0:
            continue
        label[s] = s
        queue = collections.deque([s])
        while queue:
            x = queue.popleft()
            for y in adj[x]:
                if label[y] < 0:
                    label[y] = s
                    queue.append(y)
    return label
