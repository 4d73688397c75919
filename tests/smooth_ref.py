"""NumPy reference of include/adgs_smooth.h: the one-ring adjacency of a triangle mesh and Laplacian / Taubin smoothing over it with uniform
weights, evaluated in float64 exactly as the header defines it -- the row of a vertex summed in ascending neighbour order from 0.0, one
division, one subtraction, one multiplication and one addition per component, the previous step's state read by every vertex, one rounding
to float32 at the end -- so that the device's output can be compared with it AS BITS.  Pinned by tests/test_smooth_ref.py."""
import numpy as np

COUNT_NAMES = ("edges", "boundary_edges", "nonmanifold_edges", "degenerate_faces", "isolated_vertices", "bad_faces")


class Adjacency:
    """starts [V + 1] int32, neighbors [2 E] int32, boundary [V] bool, counts; incidence [E] of the edges (lo, hi) [E, 2] in ascending
    (lo, hi) order."""

    def __init__(self, starts, neighbors, boundary, counts, edges, incidence):
        self.starts, self.neighbors, self.boundary, self.counts, self.edges, self.incidence = starts, neighbors, boundary, counts, edges, incidence

    def degree(self):
        return self.starts[1:] - self.starts[:-1]


def adjacency(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    g = f[ok]
    a, b = g.reshape(-1), g[:, [1, 2, 0]].reshape(-1)           # slot k of a face: (i_k, i_k+1)
    same = a == b
    W = max(V, 1)
    key, inc = np.unique((np.minimum(a, b) * W + np.maximum(a, b))[~same], return_counts=True)     # undirected keys, their incidence
    lo, hi = key // W, key % W
    directed = np.unique(np.concatenate([lo * W + hi, hi * W + lo]))
    src, nb = directed // W, directed % W
    starts = np.searchsorted(src, np.arange(V + 1)).astype(np.int32)
    boundary = np.zeros(V, bool)
    boundary[lo[inc == 1]] = True
    boundary[hi[inc == 1]] = True
    counts = dict(edges=len(key), boundary_edges=int((inc == 1).sum()), nonmanifold_edges=int((inc > 2).sum()),
                  degenerate_faces=int(same.reshape(-1, 3).any(1).sum()), isolated_vertices=int((np.diff(starts) == 0).sum()), bad_faces=int((~ok).sum()))
    return Adjacency(starts, nb.astype(np.int32), boundary, counts, np.stack([lo, hi], 1), inc)


def step(x, adj, s, fixed):
    """One step on the float64 state x [V, 3] -> a new array.  The k-th neighbour of every row that has one is added in pass k, so every
    row is summed in ascending neighbour order."""
    d = adj.degree().astype(np.int64)
    order = np.argsort(-d, kind="stable")                       # the rows with more than k entries are a prefix of it
    longer = np.searchsorted(-d[order], -np.arange(int(d.max()) if len(d) else 0), side="left")
    first = adj.starts[:-1].astype(np.int64)
    S = np.zeros_like(x)
    for k, m in enumerate(longer):
        rows = order[:m]
        S[rows] = S[rows] + x[adj.neighbors[first[rows] + k]]
    move = (d > 0) & ~fixed
    out = x.copy()
    n = d[move].astype(np.float64)[:, None]
    out[move] = x[move] + s * (S[move] / n - x[move])
    return out


def factors(iterations, method, lam, mu):
    return [lam] * iterations if method == "laplacian" else [lam, mu] * iterations


def smooth(vertices, faces, iterations=10, method="taubin", lam=0.5, mu=-0.53, boundary="fixed", fixed=None, adj=None):
    """-> vertices' [V, 3] float32."""
    assert method in ("taubin", "laplacian") and boundary in ("fixed", "free")
    vertices = np.asarray(vertices, np.float32)
    V = len(vertices)
    adj = adjacency(faces, V) if adj is None else adj
    keep = adj.boundary.copy() if boundary == "fixed" else np.zeros(V, bool)
    if fixed is not None:
        keep |= np.asarray(fixed, bool)
    x = vertices.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in factors(iterations, method, float(lam), float(mu)):
            x = step(x, adj, s, keep)
        return x.astype(np.float32)


def umbrella_residual(vertices, adj):
    """RMS over the vertices with neighbours of |mean(neighbours) - x|."""
    x = np.asarray(vertices, np.float64)
    d = adj.degree()
    S = np.zeros_like(x)
    np.add.at(S, np.repeat(np.arange(len(x)), d), x[adj.neighbors])
    has = d > 0
    r = S[has] / d[has][:, None] - x[has]
    return float(np.sqrt((r * r).sum(1).mean()))
