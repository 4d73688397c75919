"""The meshes the simplification (include/adgs_simplify.h) is tested on, shared by the CPU and GPU tests.  A case is a dict: vertices
[V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 or None, cell_size, origin.  case(name) builds it once, reference(name) runs
tests/simplify_ref.py on it once (clustering and both placements).  Nobody writes into what these return.

 empty, points, one_cell, three_cells   the tiny ones: no mesh; vertices without faces; a triangle inside one cell; a triangle across three
 identity       a jittered planar grid of 160 x 128 vertices (spacing 1, in-plane jitter +-0.3), cell 0.25: neighbours differ by at least 0.4
                along an axis, so every vertex has a cell of its own.  20 480 vertices: 10 scan tiles (2 048), 5 sort blocks (4 096)
 grid_coarse    the same grid with z jitter, shifted so that coordinates of both signs occur, cell 2.5, origin (0.3, -0.2, 0.1)
 tsdf_2.0, tsdf_3.7   mesh_cases.tsdf_mesh() with its colours
 crease         a regular 17 x 11 grid folded by 90 degrees along its middle column, cell 3 with the fold at the centre of a cell
 duplicates     hand-built: the same triple twice, rotated, with the opposite orientation, through another member of a cluster; degenerates
 long_run       5 000 vertices in one cell, each in a face with the same two far vertices, and a triangle across three other cells
 nonfinite      a small grid with NaN, +inf and -inf vertices
 weld           the identity grid cut in two halves that both own the seam column, concatenated; cell 2^-10
"""
import functools

import numpy as np

from tests import mesh_cases
from tests import simplify_ref as ref

GRID = (160, 128)
TINY = ("empty", "points", "one_cell", "three_cells")
NAMES = TINY + ("identity", "grid_coarse", "tsdf_2.0", "tsdf_3.7", "crease", "duplicates", "long_run", "nonfinite", "weld")
CREASE = (17, 11)
SEAM = 80                                                       # the column both halves of `weld` own


def grid_faces(nx, ny):
    """Two triangles per quad of an nx x ny grid, vertex (i, j) at j * nx + i."""
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="xy")
    a = (j * nx + i).reshape(-1)
    return np.stack([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)], 1).reshape(-1, 3).astype(np.int32)


def grid(nx, ny, jitter=0.3, zjitter=0.0, shift=(0.0, 0.0, 0.0), seed=1):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    p = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float64)
    p[:, :2] += rng.uniform(-jitter, jitter, (len(p), 2))
    p[:, 2] += rng.uniform(-zjitter, zjitter, len(p)) if zjitter else 0.0
    return (p + np.asarray(shift)).astype(np.float32), grid_faces(nx, ny)


def colors_for(v, seed=2):
    return np.random.default_rng(seed).random((len(v), 3)).astype(np.float32)


def crease():
    nx, ny = CREASE
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    u = (i - nx // 2).reshape(-1).astype(np.float64)
    p = np.stack([np.minimum(u, 0.0), j.reshape(-1).astype(np.float64), np.maximum(u, 0.0)], 1)     # z = 0 up to the fold, x = 0 behind it
    return p.astype(np.float32), grid_faces(nx, ny)


def weld_halves():
    v, _ = grid(*GRID)
    nx, ny = GRID
    cols = [np.arange(0, SEAM + 1), np.arange(SEAM, nx)]
    vs, fs, base = [], [], 0
    for c in cols:
        idx = (np.arange(ny)[:, None] * nx + c[None, :]).reshape(-1)
        vs.append(v[idx])
        fs.append(grid_faces(len(c), ny) + base)
        base += len(idx)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def _case(v, f, cell_size, origin=(0.0, 0.0, 0.0), colors=True):
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    return {"vertices": v, "faces": np.ascontiguousarray(f, np.int32).reshape(-1, 3), "colors": colors_for(v) if colors is True else colors,
            "cell_size": cell_size, "origin": origin}


@functools.lru_cache(maxsize=None)
def case(name):
    nof = np.zeros((0, 3), np.int32)
    if name == "empty":
        return _case(np.zeros((0, 3)), nof, 1.0)
    if name == "points":
        return _case(np.arange(21).reshape(7, 3), nof, 1.0)
    if name == "one_cell":
        return _case([[0.1, 0.1, 0.1], [0.8, 0.2, 0.1], [0.2, 0.9, 0.3]], [[0, 1, 2]], 1.0)
    if name == "three_cells":
        return _case([[0.1, 0.1, 0.1], [1.8, 0.2, 0.1], [0.2, 1.9, 0.3]], [[0, 1, 2]], 1.0)
    if name == "identity":
        return _case(*grid(*GRID), 0.25)
    if name == "grid_coarse":
        return _case(*grid(*GRID, zjitter=0.4, shift=(-71.3, -40.6, -0.05)), 2.5, (0.3, -0.2, 0.1))
    if name.startswith("tsdf_"):
        v, f, c = mesh_cases.tsdf_mesh()
        return _case(v, f, float(name[5:]), colors=c)
    if name == "crease":
        return _case(*crease(), 3.0, (-1.5, -1.5, -1.5))
    if name == "duplicates":
        # vertices 0 and 6 share a cell; 1 .. 5 have their own
        v = [[0.2, 0.2, 0.2], [3.5, 0.1, 0.3], [0.4, 3.6, 0.2], [3.3, 3.4, 1.2], [6.5, 0.5, 0.5], [6.4, 3.5, 0.6], [0.7, 0.6, 0.5]]
        f = [[0, 1, 2], [0, 1, 2], [1, 2, 0], [0, 2, 1], [0, 6, 3], [3, 4, 5], [6, 1, 2], [2, 1, 6], [5, 3, 4], [3, 3, 4], [1, 3, 2], [4, 3, 5]]
        return _case(v, f, 1.0)
    if name == "long_run":
        rng = np.random.default_rng(4)
        n = 5000
        big = rng.uniform(0.05, 0.95, (n, 3))
        far = [[4.5, 0.5, 0.3], [0.5, 4.5, 0.7], [8.2, 8.3, 8.4], [9.5, 8.1, 8.2], [8.4, 9.6, 8.8]]
        f = np.concatenate([np.stack([np.arange(n), np.full(n, n), np.full(n, n + 1)], 1), [[n + 2, n + 3, n + 4]]])
        return _case(np.concatenate([big, far]), f, 1.0)
    if name == "nonfinite":
        v, f = grid(14, 11, zjitter=0.3)
        v = v.copy()
        v[17, 1], v[40, 0], v[41, 2], v[100] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 0.0)
        return _case(v, f, 2.0, (0.1, 0.1, 0.1))
    if name == "weld":
        return _case(*weld_halves(), 2.0 ** -10)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(clustering, {placement: (vertices2, colors2)}) of tests/simplify_ref.py."""
    c = case(name)
    cl = ref.cluster(c["vertices"], c["faces"], c["cell_size"], c["origin"])
    return cl, {p: ref.place(cl, c["vertices"], c["faces"], c["colors"], p) for p in ("quadric", "average")}


def sphere_distance(vertices, roots_mask):
    """The mean distance of the vertices under the mask from the surface of the nearer sphere of mesh_cases.SPHERES."""
    p = np.asarray(vertices, np.float64)[roots_mask]
    d = np.min([np.abs(np.linalg.norm(p - np.array(c), axis=1) - r) for c, r in mesh_cases.SPHERES], axis=0)
    return float(d.mean())


def sphere_roots(name):
    """The output vertices of a tsdf case whose root lies within one voxel of a sphere (not on one of the blobs)."""
    cl, _ = reference(name)
    m = np.logical_or.reduce(mesh_cases.sphere_vertices(case(name)["vertices"]))
    return m[cl.root]


def crease_straddlers():
    """The output vertices of `crease` with members on both sides of the fold."""
    c = case("crease")
    cl, _ = reference("crease")
    v = c["vertices"]
    flat, up = np.zeros(len(cl.root), bool), np.zeros(len(cl.root), bool)
    inside = cl.vertex_cluster >= 0
    np.logical_or.at(flat, cl.vertex_cluster[inside], v[inside, 0] < 0)
    np.logical_or.at(up, cl.vertex_cluster[inside], v[inside, 2] > 0)
    return flat & up
