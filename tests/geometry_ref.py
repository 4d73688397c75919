"""The definitions of include/adgs_geometry.h restated in numpy, one rounding per operation, for the CPU and GPU tests of adgs.geometry.

nearest        brute force in float32 with the stated operation order, chunked over the queries
splitmix_units the three random words of every sample;  sample_from_cdf: the cdf search, the fold and the point, in float64
face_areas     0.5 |(p1 - p0) x (p2 - p0)| in float64, 0 for a face with an index outside the vertices
distance_stats / evaluate_points: the sums and the metrics
"""
import math

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MIX1 = np.uint64(0xBF58476D1CE4E5B9)
MIX2 = np.uint64(0x94D049BB133111EB)


def f32(v):
    return float(np.float32(v))


def search_radius(max_dist, cell_size):
    return math.ceil(f32(max_dist) * (1.0 + 2.0 ** -20) / f32(cell_size))


def nearest(queries, targets, max_dist, chunk=256):
    """-> (dist2 [N] float32, idx [N] int32): d2 = (dx dx + dy dy) + dz dz in float32; a neighbour has (double)d2 <= (double)max_dist^2
    (max_dist as float32); the smallest d2 wins, ties to the lowest index (np.argmin returns the first minimum); +inf / -1 without one."""
    q, t = np.ascontiguousarray(queries, np.float32), np.ascontiguousarray(targets, np.float32)
    N, M = len(q), len(t)
    dist2, idx = np.full(N, np.inf, np.float32), np.full(N, -1, np.int32)
    if N == 0 or M == 0:
        return dist2, idx
    limit = np.float64(np.float32(max_dist)) * np.float64(np.float32(max_dist))
    usable = np.isfinite(t).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, N, chunk):
            qc = q[a:a + chunk]
            dx, dy, dz = (qc[:, None, k] - t[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            ok = usable[None, :] & (d2.astype(np.float64) <= limit) & np.isfinite(qc).all(1)[:, None]
            d2 = np.where(ok, d2, np.float32(np.inf))
            j = np.argmin(d2, axis=1)
            best = d2[np.arange(len(qc)), j]
            found = np.isfinite(best)
            dist2[a:a + chunk] = best
            idx[a:a + chunk] = np.where(found, j, -1)
    return dist2, idx


def splitmix_units(seed, n):
    """u [n, 3] float64: u_j of sample k from z = seed + GOLDEN (3 k + j + 1) through the splitmix64 finaliser."""
    with np.errstate(over="ignore"):
        counter = (np.uint64(3) * np.arange(n, dtype=np.uint64)[:, None] + np.arange(1, 4, dtype=np.uint64)[None, :])
        z = np.uint64(seed) + GOLDEN * counter
        z = (z ^ (z >> np.uint64(30))) * MIX1
        z = (z ^ (z >> np.uint64(27))) * MIX2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def valid_faces(vertices, faces):
    f = np.asarray(faces).reshape(-1, 3)
    return ((f >= 0) & (f < len(vertices))).all(1)


def face_areas(vertices, faces):
    v, f = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(faces).reshape(-1, 3)
    ok = valid_faces(vertices, f)
    area = np.zeros(len(f), np.float64)
    p = v[f[ok]]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area[ok] = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    return area


def sample_from_cdf(vertices, faces, cdf, n, seed):
    """-> (points [n, 3] float32, face [n] int32, points in float64 before the one rounding)."""
    v, f = np.asarray(vertices, np.float32).astype(np.float64), np.asarray(faces).reshape(-1, 3)
    cdf = np.asarray(cdf, np.float64)
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros((0, 3))
    total = cdf[-1]
    assert len(f) > 0 and np.isfinite(total) and total > 0
    u = splitmix_units(seed, n)
    t = np.minimum(u[:, 0] * total, np.nextafter(total, 0.0))
    face = np.searchsorted(cdf, t, side="right")               # the first f with cdf[f] > t
    assert (face < len(f)).all()
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    fold = u1 + u2 > 1.0
    u1[fold], u2[fold] = 1.0 - u1[fold], 1.0 - u2[fold]
    assert valid_faces(vertices, f[face]).all(), "the cdf steps at a face with an index outside the vertices"
    p = v[f[face]]
    exact = (p[:, 0] + u1[:, None] * (p[:, 1] - p[:, 0])) + u2[:, None] * (p[:, 2] - p[:, 0])
    return exact.astype(np.float32), face.astype(np.int32), exact


def sample_surface(vertices, faces, n, seed):
    return sample_from_cdf(vertices, faces, np.cumsum(face_areas(vertices, faces)), n, seed)


def barycentric(vertices, faces, points, face):
    """(b0, b1, b2) of every point in its face and its distance from the face's plane, in float64; the faces must have area."""
    v = np.asarray(vertices, np.float64)
    p = v[np.asarray(faces)[face]]
    a, b, c = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], np.asarray(points, np.float64) - p[:, 0]
    n = np.cross(a, b)
    nn = (n * n).sum(1)
    b1 = (np.cross(c, b) * n).sum(1) / nn
    b2 = (np.cross(a, c) * n).sum(1) / nn
    return np.stack([1.0 - b1 - b2, b1, b2], 1), np.abs((c * n).sum(1)) / np.sqrt(nn)


def count_bound(n, p):
    """How far a face's sample count may be from n p: six binomial standard deviations and one."""
    return 6.0 * np.sqrt(n * p * (1.0 - p)) + 1.0


def distance_stats(dist2, thresholds, max_dist):
    """[8] float64 as adgs_geometry_distance_stats writes them (max_dist as float32)."""
    d2 = np.asarray(dist2, np.float32).astype(np.float64)
    md = np.float64(np.float32(max_dist))
    none = ~(d2 < np.inf)
    with np.errstate(invalid="ignore"):
        d = np.where(none, md, np.minimum(np.sqrt(d2), md))
    out = np.zeros(8)
    out[0], out[1], out[2] = math.fsum(d), len(d2), none.sum()
    for k, tau in enumerate(thresholds):
        out[3 + k] = (d2 < np.float64(tau) * np.float64(tau)).sum()
    return out


def metrics(pred_stats, gt_stats, thresholds):
    p, g = pred_stats, gt_stats
    acc, comp = p[0] / p[1], g[0] / g[1]
    res = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "num_pred": int(p[1]), "num_gt": int(g[1]),
           "pred_without_neighbour": int(p[2]), "gt_without_neighbour": int(g[2]), "precision": [], "recall": [], "fscore": [], "pred_below": [],
           "gt_below": []}
    for k in range(len(thresholds)):
        P, R = p[3 + k] / p[1], g[3 + k] / g[1]
        res["precision"].append(P)
        res["recall"].append(R)
        res["fscore"].append(2 * P * R / (P + R) if P + R > 0 else 0.0)
        res["pred_below"].append(int(p[3 + k]))
        res["gt_below"].append(int(g[3 + k]))
    return res


def evaluate_points(pred, gt, thresholds, max_dist):
    """-> (metrics, dist2 pred -> gt, dist2 gt -> pred)."""
    to_gt, _ = nearest(pred, gt, max_dist)
    to_pred, _ = nearest(gt, pred, max_dist)
    return metrics(distance_stats(to_gt, thresholds, max_dist), distance_stats(to_pred, thresholds, max_dist), thresholds), to_gt, to_pred
