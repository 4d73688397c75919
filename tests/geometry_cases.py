"""The inputs adgs.geometry (include/adgs_geometry.h) is tested on, shared by the CPU and GPU tests: small, and shaped like what the kernels
can go wrong on.  Everything is built once (lru_cache) and nobody writes into what these return.

Nearest neighbour: nn(name) -> (targets [M, 3], queries [N, 3], cell_size, max_dist); nn_reference(name) -> tests/geometry_ref.nearest on it.
  single, no_targets, no_queries          M = 1, M = 0, N = 0
  one_cell                                 300 targets in one cell: more than a wave and more than a 256-record tile
  odd                                      N = 257, M = 1000: no multiples of 64 or 256
  duplicates                               every target three times, shuffled: ties inside a cell
  tie_across_cells                         two targets equidistant from the query in different cells, index order opposite to key order
  lattice_r2, lattice_r1, lattice_r3       a lattice at spacing cell_size with queries exactly max_dist outside its faces along an axis, on
                                           both sides: cell_size = max_dist (R = 2), 1.001 max_dist (R = 1), max_dist / 2.5 (R = 3)
  outside                                  queries outside the box: within max_dist of a boundary target, and far away
  plane                                    all targets in a plane: nz = 1
  far_coordinates                          coordinates around -10^4 with cell_size 0.05
  nonfinite                                NaN / +inf / -inf in three targets and three queries
  clustered0, clustered1, clustered2       M = 20 000, N = 5 000 around common cluster centres
Sampling: sampling_mesh(name) -> (vertices, faces), from here and from tests/mesh_cases.py.
Metrics: hand-computed sets in metric_sets().
"""
import functools

import numpy as np

from tests import geometry_ref as ref
from tests import mesh_cases

NN_NAMES = ("single", "no_targets", "no_queries", "one_cell", "odd", "duplicates", "tie_across_cells", "lattice_r2", "lattice_r1", "lattice_r3",
            "outside", "plane", "far_coordinates", "nonfinite", "clustered0", "clustered1", "clustered2")
CLUSTERED = ("clustered0", "clustered1", "clustered2")
EXPECTED_RADIUS = {"lattice_r2": 2, "lattice_r1": 1, "lattice_r3": 3}


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def lattice(cell_size, max_dist, n=5):
    """n^3 targets at spacing cell_size from 0; queries exactly max_dist (as far as float32 allows; exactly, on the low side) outside each
    of the six faces, opposite every boundary target, plus the lattice's own points moved by max_dist / 2."""
    cs, md = np.float32(cell_size), np.float32(max_dist)
    k = np.arange(n, dtype=np.float32) * cs
    t = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    q = []
    for axis in range(3):
        for side, value in ((0, k[0]), (1, k[-1])):
            face = t[t[:, axis] == value].copy()
            face[:, axis] = face[:, axis] - md if side == 0 else face[:, axis] + md
            q.append(face)
    q.append(t + md / np.float32(2))
    return f32(t), f32(np.concatenate(q)), float(cs), float(md)


def clustered(seed, M=20000, N=5000):
    rng = np.random.default_rng(100 + seed)
    centres = rng.uniform(0, 10, (20, 3))
    sigma = rng.uniform(0.1, 0.5, 20)
    ct, cq = rng.integers(0, 20, M), rng.integers(0, 20, N)
    t = centres[ct] + sigma[ct, None] * rng.standard_normal((M, 3))
    q = centres[cq] + 1.5 * sigma[cq, None] * rng.standard_normal((N, 3))
    return f32(t), f32(q), 0.3 * 1.001, 0.3


@functools.lru_cache(maxsize=None)
def nn(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "single":
        return f32([[0.25, -1.5, 3.0]]), f32([[0.25, -1.5, 3.0], [0.3, -1.5, 3.0], [0.25, -1.0, 3.0], [0.25, -1.5, 3.50001], [9, 9, 9]]), 0.5, 0.5
    if name == "no_targets":
        return np.zeros((0, 3), np.float32), f32(rng.uniform(-1, 1, (70, 3))), 0.5, 0.5
    if name == "no_queries":
        return f32(rng.uniform(-1, 1, (70, 3))), np.zeros((0, 3), np.float32), 0.5, 0.5
    if name == "one_cell":
        t = rng.uniform(0.0, 0.9, (300, 3))
        t[0] = 0.0                                              # the origin of the grid
        return f32(t), f32(rng.uniform(-0.5, 1.5, (200, 3))), 1.0, 0.75
    if name == "odd":
        return f32(rng.uniform(0, 4, (1000, 3))), f32(rng.uniform(-0.3, 4.3, (257, 3))), 0.5, 0.5
    if name == "duplicates":
        base = f32(rng.uniform(0, 2, (150, 3)))
        t = np.repeat(base, 3, axis=0)[rng.permutation(450)]
        return f32(t), f32(np.concatenate([base[:100], rng.uniform(0, 2, (100, 3))])), 0.4, 0.4
    if name == "tie_across_cells":
        # origin x = 0.5, cell 1: index 1 lies in cell x = 0, index 0 in cell x = 1, so index 0 has the LARGER key and is met second;
        # both are exactly 0.5 from the first query, and the rule gives it index 0.  The same along y and z with indices 2 .. 5.
        t = [[1.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 3.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 3.5], [0.5, 0.5, 2.5], [3.5, 3.5, 3.5]]
        q = [[1.0, 0.5, 0.5], [0.5, 3.0, 0.5], [0.5, 0.5, 3.0]]
        return f32(t), f32(q), 1.0, 1.0
    if name == "lattice_r2":
        return lattice(0.25, 0.25)
    if name == "lattice_r1":
        return lattice(np.float32(1.001) * np.float32(0.25), 0.25)
    if name == "lattice_r3":
        return lattice(np.float32(0.25) / np.float32(2.5), 0.25, n=9)
    if name == "outside":
        t = f32(rng.uniform(0, 1, (400, 3)))
        near = t[:60] + f32(rng.uniform(-0.2, 0.2, (60, 3)))
        shell = f32(rng.uniform(-0.25, 1.25, (200, 3)))
        far = f32([[100, 0.5, 0.5], [-100, 0.5, 0.5], [0.5, 1e6, 0.5], [0.5, 0.5, -1e6], [1e30, 1e30, 1e30], [-3e38, 0, 0], [0.5, 0.5, 1.3], [1.26, 0.5, 0.5]])
        return t, f32(np.concatenate([near, shell, far])), 0.25, 0.25
    if name == "plane":
        t = rng.uniform(0, 3, (500, 3))
        t[:, 2] = 0.5
        q = rng.uniform(0, 3, (300, 3))
        q[:, 2] = rng.uniform(0.2, 0.8, 300)
        return f32(t), f32(q), 0.3, 0.3
    if name == "far_coordinates":
        return f32(-1e4 + rng.uniform(0, 1, (2000, 3))), f32(-1e4 + rng.uniform(-0.05, 1.05, (700, 3))), 0.05, 0.05
    if name == "nonfinite":
        t, q = f32(rng.uniform(0, 2, (300, 3))), f32(rng.uniform(0, 2, (130, 3)))
        t[7, 0], t[100, 1], t[299, 2] = np.nan, np.inf, -np.inf
        q[0, 2], q[64, 0], q[129, 1] = np.nan, -np.inf, np.inf
        return t, q, 0.4, 0.4
    if name in CLUSTERED:
        return clustered(int(name[-1]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def nn_reference(name):
    t, q, _, md = nn(name)
    return ref.nearest(q, t, md)


# ---- sampling ----

SAMPLING = {"triangle": 777, "two_1_1000": 4096, "zero_area": 3000, "out_of_range": 2000, "tsdf": 10000, "one_sample": 1, "no_sample": 0}


@functools.lru_cache(maxsize=None)
def sampling_mesh(name):
    if name in ("triangle", "one_sample", "no_sample"):
        return f32([[0.5, 0.25, 1.0], [2.5, 0.5, 1.5], [1.0, 3.0, -0.5]]), np.array([[0, 1, 2]], np.int32)
    if name == "two_1_1000":
        v = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [10 + np.sqrt(1000.0), 0, 1], [10, np.sqrt(1000.0), 2]])
        return v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    if name == "zero_area":                                     # zero-area faces in the middle (repeated index, collinear) and at the end
        v = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 1], [3, 0, 1], [3, 1, 2], [4, 0, 0], [5, 0, 0], [6, 0, 0]])
        return v, np.array([[0, 1, 2], [1, 1, 3], [6, 7, 8], [3, 4, 5], [2, 3, 4], [4, 4, 4], [6, 8, 7]], np.int32)
    if name == "out_of_range":
        return mesh_cases.mesh(mesh_cases.BAD)
    if name == "tsdf":
        return mesh_cases.mesh("tsdf")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sampling_reference(name, seed=3):
    """(cdf, points float32, face, points float64) of the reference with SAMPLING[name] samples."""
    v, f = sampling_mesh(name)
    cdf = np.cumsum(ref.face_areas(v, f))
    return (cdf,) + ref.sample_from_cdf(v, f, cdf, SAMPLING[name], seed)


COUNT_N, COUNT_SEED = 65536, 11


@functools.lru_cache(maxsize=None)
def count_mesh():
    """8 disjoint right triangles whose areas spread over 1 : 1000 (legs scaled by 1000^(k / 14))."""
    v, f = [], []
    for k in range(8):
        s = 1000.0 ** (k / 14.0)
        v += [[10.0 * k, 0, 0.1 * k], [10.0 * k + s, 0, 0.1 * k], [10.0 * k, s, 0.2 * k]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return f32(v), np.array(f, np.int32)


def count_condition(vertices, faces, face, n):
    """The per-face counts of `face` [n] against n p, p the face's share of the area: (counts, expected, bound)."""
    area = ref.face_areas(vertices, faces)
    p = area / area.sum()
    return np.bincount(face, minlength=len(faces)), n * p, ref.count_bound(n, p)


# ---- metrics ----

@functools.lru_cache(maxsize=None)
def metric_sets():
    """name -> (pred, gt, thresholds, max_dist, expected or None): exactly representable coordinates, shifts along x."""
    k = np.arange(4, dtype=np.float32)
    base = f32(np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3))          # 64 points at spacing 1
    shift = lambda s: f32(base + np.float32([s, 0, 0]))                                    # the nearest point is then s away, for s < 0.5
    return {
        "identical": (base, base, (0.25,), 0.5, {"accuracy": 0.0, "completeness": 0.0, "chamfer": 0.0, "precision": [1.0], "recall": [1.0], "fscore": [1.0]}),
        "shift_below": (shift(0.125), base, (0.25,), 0.5, {"accuracy": 0.125, "completeness": 0.125, "chamfer": 0.125, "precision": [1.0], "recall": [1.0],
                                                          "fscore": [1.0]}),
        "shift_at": (shift(0.25), base, (0.25, 0.375), 0.5, {"accuracy": 0.25, "completeness": 0.25, "chamfer": 0.25, "precision": [0.0, 1.0],
                                                            "recall": [0.0, 1.0], "fscore": [0.0, 1.0]}),
        "shift_above": (shift(0.375), base, (0.25,), 0.5, {"accuracy": 0.375, "completeness": 0.375, "chamfer": 0.375, "precision": [0.0], "recall": [0.0],
                                                          "fscore": [0.0]}),
        # half a spacing along every axis: sqrt(0.75) from the nearest point, beyond max_dist -- every point contributes max_dist
        "apart": (f32(base + np.float32(0.5)), base, (0.25, 0.5), 0.5, {"accuracy": 0.5, "completeness": 0.5, "chamfer": 0.5, "precision": [0.0, 0.0],
                                                                       "recall": [0.0, 0.0], "fscore": [0.0, 0.0], "pred_without_neighbour": 64,
                                                                       "gt_without_neighbour": 64}),
        "clustered": clustered(0, 3000, 2000)[:2] + ((0.05, 0.1, 0.2, 0.3), 0.3, None),
        # a threshold EQUAL to a max_dist that rounds down to float32 (0.16 -> 0.15999999642): accepted; the search runs at the float32 value
        "tau_at_max_dist": clustered(1, 3000, 2000)[:2] + ((0.08, 0.16), 0.16, None),
    }
