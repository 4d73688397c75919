"""The meshes the mesh clean-up (include/adgs_mesh.h) is tested on, shared by the CPU and GPU tests; small, and shaped like what the kernels
can go wrong on.  A case is (vertices [V, 3] float32, faces [F, 3] int32); mesh(name) builds it once, reference(name) computes
tests/mesh_ref.py on it once.  Nobody writes into what these return.

 1 empty            V = F = 0
 2 points           V = 7, F = 0: seven components without a face
 3 triangle         one triangle
 4 bowtie           two triangles sharing ONE vertex: one component (vertex connectivity; edge connectivity would say two)
 5 strip*           a strip of 5 000 triangles with ascending, reversed and randomly permuted vertex indices: deep trees, long find paths,
                    many failed CAS
 6 fan              4 096 faces around one hub: every link contends for one root, and the hub's row of corners is 4 096 long
 7 scattered        3 000 disjoint triangles with 1 000 unused vertices interleaved: C = 4 000 crosses the scan's tile (2 048), and nearly
                    every wave holds several components
 8 tsdf, tsdf_perm  marching tetrahedra (tests/tsdf_ref.py) on a 40 x 36 x 32 host-made volume with two spheres and a dozen blobs of one to
                    three lattice points; as extracted, and with vertex indices and face order under a seeded permutation
 9 repeated         faces (a, a, b), and a vertex all of whose faces are such: its normal is exactly (0, 0, 0)
10 out_of_range     a face with index -1 and one with index V among valid ones
"""
import functools

import numpy as np

from tests import mesh_ref as ref
from tests import tsdf_ref

TSDF_DIMS = (40, 36, 32)
SPHERES = (((11.2, 12.1, 13.3), 7.3), ((27.4, 22.3, 17.2), 5.1))          # (centre, radius) in lattice units; voxel_size 1
BLOBS = (((3, 3, 3),), ((36, 4, 5),), ((5, 30, 4),), ((30, 5, 27),), ((4, 31, 27),), ((35, 31, 4),),
         ((20, 3, 3), (21, 3, 3)), ((3, 18, 27), (3, 19, 27)), ((36, 15, 28), (36, 15, 29)), ((22, 32, 27), (23, 32, 27)),
         ((25, 4, 26), (26, 4, 26), (27, 4, 26)), ((12, 31, 5), (12, 32, 5), (13, 32, 5)))
NAMES = ("empty", "points", "triangle", "bowtie", "strip", "strip_reversed", "strip_permuted", "fan", "scattered", "tsdf", "tsdf_perm", "repeated")
NO_FLAG = ("strip", "strip_reversed", "strip_permuted", "fan", "scattered", "tsdf", "tsdf_perm")       # cases 5 to 8
BAD = "out_of_range"


def permuted(vertices, faces, perm, face_order=None):
    """Vertex v becomes perm[v]; faces reordered by face_order."""
    v = np.empty_like(vertices)
    v[perm] = vertices
    f = perm[faces].astype(np.int32)
    return v, (f if face_order is None else f[face_order])


def strip(n=5000):
    i = np.arange(n + 2)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.1 * np.sin(0.37 * i)], 1).astype(np.float32)
    t = np.arange(n)
    f = np.where((t % 2 == 0)[:, None], np.stack([t, t + 1, t + 2], 1), np.stack([t + 1, t, t + 2], 1)).astype(np.int32)
    if ref.face_cross(v, f)[0][0, 2] < 0:
        f = f[:, [1, 0, 2]]
    return v, f


def fan(n=4096, hub=2048):
    a = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * np.cos(5 * a)], 1)
    v = np.insert(rim, hub, (0.0, 0.0, 1.0), axis=0).astype(np.float32)
    r = lambda k: np.where(k < hub, k, k + 1)                   # rim point k's vertex index
    k = np.arange(n)
    return v, np.stack([np.full(n, hub), r(k), r((k + 1) % n)], 1).astype(np.int32)


def scattered(groups=1000, seed=5):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (10 * groups, 3)).astype(np.float32)
    base = 10 * np.arange(groups)[:, None]
    slot = rng.integers(0, 10, groups)[:, None]                 # the unused vertex of the group
    used = np.stack([np.delete(np.arange(10), s) for s in slot[:, 0]]) + base
    return v, used.reshape(-1, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tsdf_volume():
    """tsdf = the distance to the nearer sphere / trunc, clipped; wsum = 1 everywhere; the blobs: lattice points set to -0.5 in free space."""
    vol = tsdf_ref.Volume((0.0, 0.0, 0.0), 1.0, TSDF_DIMS, color=True)
    X = vol.points()
    d = np.minimum.reduce([np.linalg.norm(X - np.array(c), axis=-1) - r for c, r in SPHERES])
    vol.tsdf = np.clip(d / 3.0, -1.0, 1.0).astype(np.float32)
    for blob in BLOBS:
        for i, j, k in blob:
            assert vol.tsdf[k, j, i] == 1.0
            vol.tsdf[k, j, i] = -0.5
    vol.wsum[:] = 1.0
    vol.color = (0.5 + 0.5 * np.sin(np.moveaxis(X, -1, 0) * 0.3)).astype(np.float32)
    return vol


@functools.lru_cache(maxsize=None)
def tsdf_mesh():
    """(vertices float32, faces, colors float32) as the device returns them: float32 roundings of the reference's."""
    v, f, c = tsdf_ref.extract(tsdf_volume(), 1.0)
    return v.astype(np.float32), f, c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    z3 = np.zeros((0, 3), np.float32)
    if name == "empty":
        return z3, np.zeros((0, 3), np.int32)
    if name == "points":
        return np.arange(21, dtype=np.float32).reshape(7, 3), np.zeros((0, 3), np.int32)
    if name == "triangle":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    if name == "bowtie":
        return (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0.5], [0, -1, 0.5]], np.float32), np.array([[0, 1, 2], [0, 3, 4]], np.int32))
    if name == "strip":
        return strip()
    if name == "strip_reversed":
        v, f = strip()
        return permuted(v, f, np.arange(len(v))[::-1].copy())
    if name == "strip_permuted":
        v, f = strip()
        return permuted(v, f, np.random.default_rng(11).permutation(len(v)))
    if name == "fan":
        return fan()
    if name == "scattered":
        return scattered()
    if name == "tsdf":
        return tsdf_mesh()[:2]
    if name == "tsdf_perm":
        v, f = tsdf_mesh()[:2]
        rng = np.random.default_rng(23)
        return permuted(v, f, rng.permutation(len(v)), rng.permutation(len(f)))
    if name == "repeated":
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 1], [3, 0, 1], [3, 1, 2], [5, 5, 5]], np.float32)
        return v, np.array([[0, 1, 2], [1, 1, 3], [3, 1, 3], [4, 4, 4], [5, 4, 5], [2, 1, 0], [0, 2, 4]], np.int32)
    if name == BAD:
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 1], [2, 1, 1], [3, 0, 0]], np.float32)
        return v, np.array([[0, 1, 2], [1, -1, 2], [1, 3, 2], [4, 5, 7], [4, 5, 6]], np.int32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Components with areas, (normals, S, flagged)) of tests/mesh_ref.py."""
    v, f = mesh(name)
    return ref.components(f, len(v), v), ref.normals(v, f)


def sphere_vertices(vertices):
    """Per sphere: the mask of the vertices within one voxel of its surface."""
    return [np.abs(np.linalg.norm(vertices.astype(np.float64) - np.array(c), axis=1) - r) < 1.0 for c, r in SPHERES]
