"""Mesh smoothing on the device (include/adgs_smooth.h): the one-ring adjacency of a triangle mesh in CSR form, and Laplacian / Taubin
smoothing over it with uniform (umbrella) weights, what Open3D's filter_smooth_laplacian / filter_smooth_taubin do on the host.

    vertices, faces, colors = adgs.mesh.remove_small_components(vertices, faces, colors)
    vertices = adgs.smooth.smooth_mesh(vertices, faces, iterations=10)              # Taubin, boundary vertices fixed
    vertices, faces, colors = adgs.simplify.simplify_mesh(vertices, faces, colors, cell_size=2 * voxel_size)
    normals = adgs.mesh.vertex_normals(vertices, faces)

Smoothing comes before the normals and the simplification: both read the faces' planes, and on a mesh fused from noisy depth those are
terraces.  Taubin smoothing (a step with lam, then a step with mu < -lam) does not shrink the mesh; Laplacian smoothing does.

    adj = adgs.smooth.mesh_adjacency(faces, V)
    adj.counts      # edges, boundary_edges, nonmanifold_edges, degenerate_faces, isolated_vertices, bad_faces
    closed_and_manifold = adj.counts["boundary_edges"] == 0 and adj.counts["nonmanifold_edges"] == 0

Faces, vertex order and colours are untouched, so a canonical mesh stays canonical.  The adjacency is reproducible to the integer and the
smoothed vertices to the bit: float64 state, the row of a vertex summed in ascending neighbour order, no atomics.  NOTHING HERE IS
DIFFERENTIABLE: everything runs under no_grad on detached inputs.  There is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _ptr
from .mesh import _bad_faces, _check_faces, _check_rows, _count, _need_device

METHODS = ("taubin", "laplacian")
BOUNDARIES = ("fixed", "free")
COUNT_NAMES = ("edges", "boundary_edges", "nonmanifold_edges", "degenerate_faces", "isolated_vertices")
MAX_ITERATIONS = 10000


class Adjacency:
    """The one-ring adjacency of a mesh, on the device: neighbors [2 E] int32 with starts [V + 1] int32, the CSR of the set of vertices
    that share an edge with each vertex, ascending; boundary [V] bool, the ends of the edges with exactly one (face, edge) contribution.
    counts: host ints edges, boundary_edges (incidence 1), nonmanifold_edges (incidence > 2), degenerate_faces (a repeated index),
    isolated_vertices (empty rows) and bad_faces.  len() = E."""

    def __init__(self, starts, neighbors, boundary, counts):
        self.starts, self.neighbors, self.boundary, self.counts = starts, neighbors, boundary, counts

    def __len__(self):
        return int(self.neighbors.shape[0]) // 2

    def degree(self):
        """The row lengths [V] int32."""
        return self.starts[1:] - self.starts[:-1]


def _adjacency(f, V, who):
    F, dev = int(f.shape[0]), f.device
    if 6 * F >= 2 ** 31:
        raise ValueError("%s: 6 F must be below 2^31" % who)
    boundary = torch.empty(V, dtype=torch.bool, device=dev)
    counts = (ctypes.c_longlong * 7)(*([0] * 7))
    temp = None
    if V or F:
        temp = torch.empty(int(_lib.lib().adgs_smooth_adjacency_temp_bytes(V, F)), dtype=torch.uint8, device=dev) if F else None
        with _lib.on_device(dev):
            code = _lib.lib().adgs_smooth_adjacency_count(V, F, _ptr(f), _ptr(temp), _ptr(boundary), counts, _lib.stream_ptr(dev))
        if code < 0 and counts[1] > 0:
            raise _bad_faces(who, counts, V)
        _lib.check(code, "adgs_smooth_adjacency_count")
    N = int(counts[0])
    starts = torch.empty(V + 1, dtype=torch.int32, device=dev) if V else torch.zeros(1, dtype=torch.int32, device=dev)
    neighbors = torch.empty(N, dtype=torch.int32, device=dev)
    if V:
        _lib.call("adgs_smooth_adjacency_emit", dev, V, F, _ptr(temp), counts, starts.data_ptr(), _ptr(neighbors))
    host = dict(zip(COUNT_NAMES, (int(counts[k]) for k in range(2, 7))), bad_faces=int(counts[1]))
    return Adjacency(starts, neighbors, boundary, host)


@torch.no_grad()
def mesh_adjacency(faces, num_vertices):
    """The adjacency of the mesh (faces [F, 3] int32 over num_vertices vertices) -> Adjacency.  Synchronises exactly once: the sizes and
    the counts come back together.  A face with an index outside [0, V) is never dereferenced and raises ValueError naming how many
    there are."""
    who = "mesh_adjacency"
    f = _check_faces(faces, who)
    V = _count(num_vertices, "num_vertices", who)
    _need_device(f, who)
    return _adjacency(f, V, who)


def _factor(x, name, lo, hi, who):
    """A finite number in (lo, hi] for lam, in [lo, hi) for mu."""
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise TypeError("%s: %s must be a number, got %r" % (who, name, x))
    x = float(x)
    inside = (lo < x <= hi) if name == "lam" else (lo <= x < hi)
    if not (math.isfinite(x) and inside):
        raise ValueError("%s: %s must be a finite number in %s, got %r" % (who, name, "(0, 1]" if name == "lam" else "[-1.5, 0)", x))
    return x


@torch.no_grad()
def smooth_mesh(vertices, faces, iterations=10, method="taubin", lam=0.5, mu=-0.53, boundary="fixed", fixed=None, adjacency=None, check=True):
    """The vertices [V, 3] float32 after `iterations` of smoothing with uniform weights: method "laplacian" is `iterations` steps
    x' = x + lam (mean of the neighbours - x); "taubin" `iterations` times a step with lam, then a step with mu (the defaults are
    Open3D's).  boundary "fixed" keeps the ends of boundary edges where they are -- a fused mesh ends where observation ends, and a free
    boundary shrinks inward --, "free" fixes nothing; fixed ([V] bool): more vertices to keep, OR-ed onto either.  A vertex without
    neighbours keeps its value, and iterations=0 returns the input's bits.  adjacency: the Adjacency of mesh_adjacency(faces, V), to
    build it once for several calls; then nothing is read back but `check`.  check=True validates isfinite(vertices).all() with one
    torch reduction (ValueError); with check=False non-finite coordinates spread as IEEE arithmetic dictates."""
    who = "smooth_mesh"
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    V, dev = int(v.shape[0]), f.device
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise TypeError("%s: iterations must be an integer, got %r" % (who, iterations))
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError("%s: iterations must lie in [0, %d], got %r" % (who, MAX_ITERATIONS, iterations))
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError("%s: method must be 'taubin' or 'laplacian', got %r" % (who, method))
    if not isinstance(boundary, str) or boundary not in BOUNDARIES:
        raise ValueError("%s: boundary must be 'fixed' or 'free', got %r" % (who, boundary))
    lam, mu = _factor(lam, "lam", 0.0, 1.0, who), _factor(mu, "mu", -1.5, 0.0, who)
    if fixed is not None:
        if not torch.is_tensor(fixed) or fixed.dtype != torch.bool or tuple(fixed.shape) != (V,):
            raise ValueError("%s: fixed must be a bool [V] = [%d] tensor" % (who, V))
        if fixed.device != dev:
            raise RuntimeError("%s: fixed is on %s, faces on %s" % (who, fixed.device, dev))
    if adjacency is not None:
        if not isinstance(adjacency, Adjacency):
            raise TypeError("%s: adjacency must be the Adjacency of mesh_adjacency, got %s" % (who, type(adjacency).__name__))
        if int(adjacency.starts.shape[0]) != V + 1 or int(adjacency.boundary.shape[0]) != V:
            raise ValueError("%s: the adjacency is of %d vertices, vertices has %d" % (who, int(adjacency.starts.shape[0]) - 1, V))
        if adjacency.starts.device != dev:
            raise RuntimeError("%s: the adjacency is on %s, faces on %s" % (who, adjacency.starts.device, dev))
    if V >= 2 ** 31:
        raise ValueError("%s: V must be below 2^31" % who)
    _need_device(f, who)
    if check and V and not bool(torch.isfinite(v).all()):
        raise ValueError("%s: vertices must be finite (check=False lets non-finite coordinates spread)" % who)
    adj = _adjacency(f, V, who) if adjacency is None else adjacency
    keep = adj.boundary if boundary == "fixed" else None
    if fixed is not None:
        keep = fixed.detach() if keep is None else keep | fixed.detach()
    k8 = None if keep is None else keep.contiguous().view(torch.uint8)
    steps = iterations if method == "laplacian" else 2 * iterations
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if V:
        N = int(adj.neighbors.shape[0])
        temp = torch.empty(int(_lib.lib().adgs_smooth_steps_temp_bytes(V, N)), dtype=torch.uint8, device=dev) if steps else None
        _lib.call("adgs_smooth_steps", dev, V, N, v.data_ptr(), adj.starts.data_ptr(), _ptr(adj.neighbors), _ptr(k8), steps, lam,
                  lam if method == "laplacian" else mu, _ptr(temp), out.data_ptr())
    return out
