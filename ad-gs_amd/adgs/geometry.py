"""Geometry evaluation on the device (include/adgs_geometry.h): how good is the mesh that adgs.tsdf / adgs.mesh produced?  What 2DGS, GOF
and PGSR report with KD-trees on the host: sample the reconstructed surface, take nearest-neighbour distances to a ground-truth point set
(for a driving scene the aggregated LiDAR sweep) and back, and report accuracy / completeness / Chamfer distance (the DTU protocol) and
precision / recall / F-score at distance thresholds (the Tanks-and-Temples protocol).

    m = adgs.geometry.evaluate_mesh(vertices, faces, lidar_points, thresholds=(0.05, 0.1), max_dist=0.5)
    m["chamfer"], m["fscore"]                                   # Python floats

    grid = adgs.geometry.PointGrid(lidar_points, cell_size=0.5)
    dist2, idx = grid.nearest(samples, max_dist=0.5)            # public results: colour a mesh by its error with them

PointGrid is an exact bounded nearest-neighbour search over a uniform grid with a compact table of the occupied cells: bit-equal to a
brute force in float32 with the stated operation order, ties to the lowest index, equal from run to run.  sample_surface is area-weighted
and counter-based (splitmix64): sample k depends on (seed, k) alone.

NOTHING HERE IS DIFFERENTIABLE: everything runs under no_grad on detached inputs.  There is no CPU fallback.

OUT OF SCOPE: exact point-to-triangle distances (the surface is sampled); cropping volumes and observation masks (index the tensors with
torch first: mesh and ground truth must cover the same region); normal-consistency metrics; adgs.knn.knn_points and simple_knn's distCUDA2
are untouched and share nothing with this module.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _ptr
from .mesh import _check_faces, _check_rows, _count

MAX_THRESHOLDS = 4
MAX_RADIUS = 8


def _check_points(t, name, who):
    """A float32 [n, 3] tensor with n < 2^31, wherever it lives."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s: %s must be [n, 3], got %s" % (who, name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    if t.shape[0] >= 2 ** 31:
        raise ValueError("%s: %s must have fewer than 2^31 rows" % (who, name))
    return t.detach().contiguous()


def _positive(v, name, who):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s: %s must be a number, got %r" % (who, name, v))
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise ValueError("%s: %s must be finite and positive, got %r" % (who, name, v))
    return v


def _f32(v):
    """The float32 the C ABI receives, as a Python float."""
    return ctypes.c_float(v).value


def _need_device(t, who):
    """Last of the checks, as in adgs.mesh: types, shapes and dtypes are refused wherever the tensors live."""
    if not t.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)


def _same_device(t, name, device, who):
    if t.device != device:
        raise RuntimeError("%s: %s is on %s, expected %s" % (who, name, t.device, device))


def search_radius(max_dist, cell_size):
    """R of include/adgs_geometry.h: ceil(max_dist (1 + 2^-20) / cell_size) cells, from the float32 values the kernels receive."""
    return math.ceil(_f32(max_dist) * (1.0 + 2.0 ** -20) / _f32(cell_size))


class PointGrid:
    """A uniform grid over points [M, 3] float32 (on the device) for exact bounded nearest-neighbour queries.  Building it sorts the points
    by cell, gathers them into 16-byte records and keeps a compact table of the occupied cells (memory is O(M), whatever the extent);
    it synchronises ONCE, to read the bounding box of the finite points back.  Points with a non-finite coordinate are never found.
    Refused (ValueError): a cell_size that gives an axis more than 2^21 cells."""

    @torch.no_grad()
    def __init__(self, points, cell_size):
        who = "PointGrid"
        p = _check_points(points, "points", who)
        self.cell_size = _f32(_positive(cell_size, "cell_size", who))
        if not self.cell_size > 0:
            raise ValueError("%s: cell_size %r is zero as a float32" % (who, cell_size))
        _need_device(p, who)
        M, dev = int(p.shape[0]), p.device
        self.device, self.num_points, self.num_finite = dev, M, 0
        self._origin, self._dims = (ctypes.c_float * 3)(), (ctypes.c_int * 3)()
        self.records = torch.empty((M, 4), dtype=torch.float32, device=dev)
        self.cell_keys = torch.empty(M, dtype=torch.int64, device=dev)
        self.cell_starts = torch.empty(M + 1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)
        if M == 0:
            return
        lib = _lib.lib()
        temp = torch.empty(int(lib.adgs_geometry_grid_temp_bytes(M)), dtype=torch.uint8, device=dev)
        finite = ctypes.c_longlong(0)
        with _lib.on_device(dev):
            code = lib.adgs_geometry_grid_plan(M, p.data_ptr(), self.cell_size, temp.data_ptr(), self._origin, self._dims, ctypes.byref(finite),
                                               _lib.stream_ptr(dev))
        if code == -2:
            raise ValueError("%s: %s" % (who, _lib.last_error()))
        _lib.check(code, "adgs_geometry_grid_plan")
        self.num_finite = int(finite.value)
        if self.num_finite:
            _lib.call("adgs_geometry_grid_build", dev, M, p.data_ptr(), self.cell_size, self._origin, self._dims, temp.data_ptr(), self.records.data_ptr(),
                      self.cell_keys.data_ptr(), self.cell_starts.data_ptr(), self.counts.data_ptr())

    @property
    def origin(self):
        return tuple(float(v) for v in self._origin)

    @property
    def dims(self):
        """(nx, ny, nz); (0, 0, 0) without a finite point."""
        return tuple(int(v) for v in self._dims)

    @torch.no_grad()
    def nearest(self, queries, max_dist):
        """For every query [N, 3] float32 the nearest point within max_dist (inclusive) -> (dist2 [N] float32, idx [N] int32): the squared
        distance (dx dx + dy dy) + dz dz in float32 and the point's index, ties to the lowest index; +inf and -1 without one, and for a
        query with a non-finite coordinate.  No read-back, no synchronisation.  Refused (ValueError): max_dist beyond 8 cells."""
        who = "PointGrid.nearest"
        q = _check_points(queries, "queries", who)
        md = _f32(_positive(max_dist, "max_dist", who))
        if not md > 0:
            raise ValueError("%s: max_dist %r is zero as a float32" % (who, max_dist))
        R = search_radius(md, self.cell_size)
        if R > MAX_RADIUS:
            raise ValueError("%s: max_dist %g spans %d cells of %g, at most %d are searched: enlarge cell_size" % (who, md, R, self.cell_size, MAX_RADIUS))
        _need_device(q, who)
        _same_device(q, "queries", self.device, who)
        N = int(q.shape[0])
        dist2 = torch.empty(N, dtype=torch.float32, device=self.device)
        idx = torch.empty(N, dtype=torch.int32, device=self.device)
        if N:
            temp = None
            if self.num_finite:
                temp = torch.empty(int(_lib.lib().adgs_geometry_nearest_temp_bytes(N)), dtype=torch.uint8, device=self.device)
            _lib.call("adgs_geometry_nearest", self.device, self.num_points, N, q.data_ptr(), md, self.cell_size, self._origin, self._dims,
                      self.records.data_ptr(), self.cell_keys.data_ptr(), self.cell_starts.data_ptr(), self.counts.data_ptr(), _ptr(temp),
                      dist2.data_ptr(), idx.data_ptr())
        return dist2, idx


def _check_mesh(vertices, faces, who):
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
        raise ValueError("%s: V and F must be below 2^31" % who)
    return v, f


@torch.no_grad()
def face_areas(vertices, faces):
    """0.5 |(p1 - p0) x (p2 - p0)| per face in double from the float32 positions -> [F] float64.  A face with an index outside [0, V) is
    never dereferenced and has area 0.  No read-back."""
    who = "face_areas"
    v, f = _check_mesh(vertices, faces, who)
    _need_device(f, who)
    V, F = int(v.shape[0]), int(f.shape[0])
    out = torch.empty(F, dtype=torch.float64, device=f.device)
    if F:
        _lib.call("adgs_geometry_face_areas", f.device, V, F, _ptr(v), f.data_ptr(), out.data_ptr())
    return out


@torch.no_grad()
def sample_from_cdf(vertices, faces, cdf, n, seed=0):
    """n points on the mesh, the face of each drawn from cdf [F] float64 (the inclusive running sum of the face weights) and the point
    uniform in the face -> (points [n, 3] float32, face [n] int32).  Sample k is a function of (seed, k) alone (three splitmix64 words;
    include/adgs_geometry.h).  A face that adds nothing to the cdf is never chosen.  Reads cdf[-1] back (one synchronisation) so that an
    empty or non-finite total is refused (ValueError) before anything is launched."""
    who = "sample_from_cdf"
    v, f = _check_mesh(vertices, faces, who)
    V, F = int(v.shape[0]), int(f.shape[0])
    if not torch.is_tensor(cdf):
        raise TypeError("%s: cdf must be a tensor, got %s" % (who, type(cdf).__name__))
    if cdf.dtype != torch.float64:
        raise TypeError("%s: cdf must be float64, got %s" % (who, cdf.dtype))
    if tuple(cdf.shape) != (F,):
        raise ValueError("%s: cdf must be [F] = [%d], got %s" % (who, F, tuple(cdf.shape)))
    n = _count(n, "n", who)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise TypeError("%s: seed must be an integer in [0, 2^64), got %r" % (who, seed))
    if n > 0 and F == 0:
        raise ValueError("%s: no face to sample from" % who)
    _same_device(cdf, "cdf", f.device, who)
    _need_device(f, who)
    dev = f.device
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        c = cdf.detach().contiguous()
        total = float(c[-1])
        if not (math.isfinite(total) and total > 0):
            raise ValueError("%s: the total area is %r: nothing to sample from" % (who, total))
        _lib.call("adgs_geometry_sample", dev, V, F, n, _ptr(v), f.data_ptr(), c.data_ptr(), total, seed, points.data_ptr(), face.data_ptr())
    return points, face


@torch.no_grad()
def sample_surface(vertices, faces, n, seed=0):
    """n points uniform over the surface of the mesh (area-weighted faces) -> (points [n, 3] float32, face [n] int32): face_areas, a
    float64 torch.cumsum, sample_from_cdf.  Zero-area faces and faces with an index outside the vertices are never sampled."""
    who = "sample_surface"
    v, f = _check_mesh(vertices, faces, who)
    n = _count(n, "n", who)
    if n > 0 and f.shape[0] == 0:
        raise ValueError("%s: no face to sample from" % who)
    return sample_from_cdf(v, f, torch.cumsum(face_areas(v, f), 0), n, seed)


def _check_thresholds(thresholds, max_dist, who):
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    try:
        taus = [_positive(t, "a threshold", who) for t in thresholds]
    except TypeError as e:
        raise TypeError("%s: thresholds must be a sequence of at most %d numbers (%s)" % (who, MAX_THRESHOLDS, e))
    if len(taus) > MAX_THRESHOLDS:
        raise ValueError("%s: at most %d thresholds, got %d" % (who, MAX_THRESHOLDS, len(taus)))
    for t in taus:                                              # against max_dist as given, before its rounding to float32
        if t > max_dist:
            raise ValueError("%s: threshold %g exceeds max_dist %g: distances are only known up to max_dist" % (who, t, max_dist))
    return taus


@torch.no_grad()
def distance_stats(dist2, thresholds, max_dist):
    """The sums of one direction over dist2 [N] float32 (PointGrid.nearest's) -> [8] float64 on the device, no read-back:
    [0] the sum of min(sqrt(d2), max_dist), max_dist for an element without a neighbour; [1] N; [2] the number without a neighbour;
    [3 + k] the number with d2 < thresholds[k]^2 (strict, in double).  Reproducible to the bit from run to run.  Thresholds are checked
    against max_dist AS GIVEN (each <= max_dist); max_dist is then rounded to float32, the value nearest() searched with.  Where that
    rounding goes down (0.16 -> 0.15999999642) a threshold equal to max_dist lies above the searched radius: a pair with d in
    (float32(max_dist), threshold) was not found and is not counted."""
    who = "distance_stats"
    if not torch.is_tensor(dist2):
        raise TypeError("%s: dist2 must be a tensor, got %s" % (who, type(dist2).__name__))
    if dist2.dim() != 1:
        raise ValueError("%s: dist2 must be [N], got %s" % (who, tuple(dist2.shape)))
    if dist2.dtype != torch.float32:
        raise TypeError("%s: dist2 must be float32, got %s" % (who, dist2.dtype))
    if dist2.shape[0] >= 2 ** 31:
        raise ValueError("%s: N must be below 2^31" % who)
    given = _positive(max_dist, "max_dist", who)
    md, taus = _f32(given), _check_thresholds(thresholds, given, who)
    _need_device(dist2, who)
    return _stats(dist2, taus, md)


def _stats(dist2, taus, md):
    """distance_stats behind its checks: taus already validated (against max_dist as given), md already a float32 value."""
    d, dev = dist2.detach().contiguous(), dist2.device
    out = torch.empty(8, dtype=torch.float64, device=dev)
    temp = torch.empty(int(_lib.lib().adgs_geometry_stats_temp_bytes(d.shape[0])), dtype=torch.uint8, device=dev)
    _lib.call("adgs_geometry_distance_stats", dev, int(d.shape[0]), _ptr(d) if d.shape[0] else None, len(taus), (ctypes.c_double * max(len(taus), 1))(*taus),
              md, temp.data_ptr(), out.data_ptr())
    return out


def metrics_from_stats(pred_stats, gt_stats, thresholds, max_dist):
    """The metric dict from the two [8] rows of distance_stats (host values)."""
    p, g = [float(x) for x in pred_stats], [float(x) for x in gt_stats]
    acc, comp = p[0] / p[1], g[0] / g[1]
    res = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "max_dist": float(max_dist), "num_pred": int(p[1]), "num_gt": int(g[1]),
           "pred_without_neighbour": int(p[2]), "gt_without_neighbour": int(g[2]), "thresholds": [float(t) for t in thresholds],
           "precision": [], "recall": [], "fscore": [], "pred_below": [], "gt_below": []}
    for k in range(len(thresholds)):
        P, R = p[3 + k] / p[1], g[3 + k] / g[1]
        res["precision"].append(P)
        res["recall"].append(R)
        res["fscore"].append(2 * P * R / (P + R) if P + R > 0 else 0.0)
        res["pred_below"].append(int(p[3 + k]))
        res["gt_below"].append(int(g[3 + k]))
    return res


@torch.no_grad()
def evaluate_points(pred_points, gt_points, thresholds, max_dist, cell_size=None):
    """Both directions between two point sets [n, 3] float32 on the device -> dict of Python values:
      accuracy      the mean over pred of min(d, max_dist), d the distance to the nearest gt point (max_dist without one within max_dist)
      completeness  the same over gt, towards pred;   chamfer = (accuracy + completeness) / 2
      precision[k]  the share of pred points with d < thresholds[k] (strict);  recall[k] the same over gt;  fscore[k] = 2PR / (P + R), 0 at P + R = 0
      num_pred, num_gt, pred_without_neighbour, gt_without_neighbour, pred_below[k], gt_below[k]: the counts
    Up to 4 thresholds, each <= max_dist as given; the search runs at float32(max_dist) (see distance_stats for a threshold equal to a
    max_dist that rounds down).  cell_size None: 1.001 max_dist (27 cells searched).  Two grids, two queries; the two PointGrids
    synchronise once each, and the results come back in ONE read-back.  An empty set on either side is a ValueError."""
    who = "evaluate_points"
    p, g = _check_points(pred_points, "pred_points", who), _check_points(gt_points, "gt_points", who)
    given = _positive(max_dist, "max_dist", who)
    md, taus = _f32(given), _check_thresholds(thresholds, given, who)
    cell = 1.001 * md if cell_size is None else _positive(cell_size, "cell_size", who)
    if p.shape[0] == 0 or g.shape[0] == 0:
        raise ValueError("%s: an empty point set (pred %d, gt %d points)" % (who, p.shape[0], g.shape[0]))
    _need_device(p, who)
    _same_device(g, "gt_points", p.device, who)
    to_gt, _ = PointGrid(g, cell).nearest(p, md)
    to_pred, _ = PointGrid(p, cell).nearest(g, md)
    both = torch.stack([_stats(to_gt, taus, md), _stats(to_pred, taus, md)]).cpu()     # the one read-back
    return metrics_from_stats(both[0], both[1], taus, md)


@torch.no_grad()
def evaluate_mesh(vertices, faces, gt_points, thresholds, max_dist, samples=1_000_000, seed=0):
    """sample_surface(vertices, faces, samples, seed), then evaluate_points(the samples, gt_points, ...) with its default cell size -> its dict, plus
    "samples": the [samples, 3] points on the device (for another cell size call the two steps)."""
    who = "evaluate_mesh"
    v, f = _check_mesh(vertices, faces, who)
    g = _check_points(gt_points, "gt_points", who)
    n = _count(samples, "samples", who)
    if n == 0 or g.shape[0] == 0:
        raise ValueError("%s: an empty point set (%d samples, gt %d points)" % (who, n, g.shape[0]))
    md = _positive(max_dist, "max_dist", who)
    _check_thresholds(thresholds, md, who)
    points, _ = sample_surface(v, f, n, seed)
    res = evaluate_points(points, g, thresholds, md)
    res["samples"] = points
    return res
