"""The meshes the adjacency and the smoothing (include/adgs_smooth.h) are tested on, shared by the CPU and GPU tests: every case of
tests/mesh_cases.py -- `tsdf` is closed and manifold, `fan` has a row of 4 096, `repeated` has boundary and non-manifold edges, `strip` and
`scattered` are all boundary -- and three with interior AND boundary vertices together:

 patch       an open lattice patch of 33 x 17 cells, each split into two triangles along alternating diagonals, over a bumpy height field:
             V = 34 x 18 = 612 and 6 F = 6 x 1 122 = 6 732 are no multiples of 256 (the workgroup), and V spans more than one workgroup
 patch_perm  the same patch with its faces under a seeded permutation: the adjacency and the smoothed bits may not change
 patch_dup   the patch with four faces appended again (one of them twice, so edges of incidence 3 and 4), one degenerate face (a, a, b) between
             two vertices that share no other edge, and one isolated vertex appended

A case is (vertices [V, 3] float32, faces [F, 3] int32); adjacency(name) and smoothed(name, ...) compute tests/smooth_ref.py on it once.
Nobody writes into what these return."""
import functools

import numpy as np

from tests import mesh_cases
from tests import smooth_ref as ref

PATCH_CELLS = (33, 17)
PATCHES = ("patch", "patch_perm", "patch_dup")
NAMES = mesh_cases.NAMES + PATCHES
SMOOTHED = ("tsdf", "tsdf_perm", "fan", "bowtie", "repeated") + PATCHES        # the cases whose smoothed bits are compared
DEGENERATE = (40, 40, 300)                                      # patch_dup's (a, a, b)
DUPLICATED = (5, 100, 100, 700)


def patch():
    nx, ny = PATCH_CELLS
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    rng = np.random.default_rng(31)
    z = 0.5 * np.sin(0.7 * i) * np.cos(0.9 * j) + 0.08 * rng.standard_normal(i.shape)
    v = np.stack([i + 0.2 * np.sin(1.3 * j), j + 0.2 * np.cos(1.1 * i), z], -1).reshape(-1, 3).astype(np.float32)
    ci, cj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    p00, p10, p01, p11 = (((ci + a) * (ny + 1) + cj + b).reshape(-1) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1)))
    even = ((ci + cj) % 2 == 0).reshape(-1)[:, None]
    t0 = np.where(even, np.stack([p00, p10, p11], 1), np.stack([p00, p10, p01], 1))
    t1 = np.where(even, np.stack([p00, p11, p01], 1), np.stack([p10, p11, p01], 1))
    return v, np.stack([t0, t1], 1).reshape(-1, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "patch":
        return patch()
    if name == "patch_perm":
        v, f = patch()
        return v, f[np.random.default_rng(37).permutation(len(f))]
    if name == "patch_dup":
        v, f = patch()
        v = np.concatenate([v, np.array([[40.0, 20.0, 3.0]], np.float32)])
        return v, np.concatenate([f, f[list(DUPLICATED)], np.array([DEGENERATE], np.int32)]).astype(np.int32)
    return mesh_cases.mesh(name)


@functools.lru_cache(maxsize=None)
def adjacency(name):
    v, f = mesh(name)
    return ref.adjacency(f, len(v))


def user_mask(name):
    """A seeded fixed [V] bool mask with about a fifth of the vertices set."""
    return np.random.default_rng(41).random(len(mesh(name)[0])) < 0.2


@functools.lru_cache(maxsize=None)
def smoothed(name, iterations=10, method="taubin", lam=0.5, mu=-0.53, boundary="fixed", masked=False):
    v, f = mesh(name)
    return ref.smooth(v, f, iterations, method, lam, mu, boundary, user_mask(name) if masked else None, adj=adjacency(name))
