"""Inputs of tests/test_gpu_tsdf_sparse.py and tests/test_tsdf_sparse_ref.py: block sets with host-made float32 values, which both sides see
bit for bit, and the views of tests/tsdf_cases.py.

MARGIN = 2 voxels is the volume's default.  It is enough for the end-to-end sphere (tests/test_tsdf_sparse_ref.py checks that the reference
sparse mesh from the six views' allocation equals the reference dense mesh): the rays are 0.33 voxel apart at the sphere and the samples
along a ray 2 voxels, so every cell with a sign change has all corners within 2 voxels of some sample.

Extraction shapes, the smallest at which the kernel can go wrong: one block; two blocks adjacent along x, y, z with a slanted plane through
their shared boundary, and the eight blocks around a lattice corner for the +x+y+z diagonal (two blocks that touch in a corner alone share
no valid cell), so that vertex ids cross blocks in every owner direction; the same with one block missing (a boundary; nothing of the
missing block is read); a pool in reverse key order; negative coordinates with exactly representable positions;
blocks at -2^20 and 2^20 - 1 on each axis; tables of 1, 2 and 65 blocks; the volumes of tests/tsdf_cases.py embedded at a block offset."""
import functools

import numpy as np

from tests import tsdf_cases as cases
from tests import tsdf_ref as ref
from tests import tsdf_sparse_ref as sref

MARGIN = 2.0
OFFSET = (3, -5, 2)                                             # where the dense volumes of tsdf_cases are embedded, in blocks
LIMIT = sref.LIMIT
EMBEDDED = ("sphere", "half_unseen", "min_weight", "fused_base")
# the blocks that cover the 41 x 17 x 38 lattice of the integration cases, plus one wholly behind the fourth camera (z in [0.4, 1.8] while that camera
# stands at z = 3.1 looking down +z) and one 64 m below everything, outside every frustum
LATTICE_BLOCKS = tuple((x, y, z) for z in range(5) for y in range(3) for x in range(6))
BEHIND_FOURTH, FAR_OUTSIDE = (2, 0, -1), (0, 40, 0)


def plane_blocks(blocks, normal, point, voxel=0.25, origin=(0.3, -1.7, 2.1), color=False, seed=6):
    """A BlockVolume over `blocks` with tsdf = clip(normal . (global index - point), -1, 1) in float32, every weight 1."""
    v = sref.BlockVolume(origin, voxel, blocks, color=color)
    l = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")[::-1], -1)
    idx = (8 * v.blocks[:, None, None, None, :] + l[None]).reshape(-1, 8, 8, 3).astype(np.float64)
    v.tsdf = np.clip((idx - np.array(point, np.float64)) @ np.array(normal, np.float64), -1.0, 1.0).astype(np.float32)
    v.wsum[:] = 1.0
    if color:
        v.color = np.random.default_rng(seed).random(v.color.shape, dtype=np.float32)
    return v


NORMAL = (0.31, 0.37, 0.41)                                      # slanted against every axis: each owner direction carries vertices
BASE_BLOCK = np.array((2, -3, 1))


def pair(direction, missing=False, color=False):
    """Two blocks adjacent along `direction` with the plane through the middle of their shared boundary (or the first block alone)."""
    d = np.array(direction)
    blocks = [BASE_BLOCK] if missing else [BASE_BLOCK, BASE_BLOCK + d]
    through = 8.0 * BASE_BLOCK + np.where(d > 0, 7.5, 3.5)
    return plane_blocks(blocks, NORMAL, through, color=color)


@functools.lru_cache(maxsize=None)
def extraction_volume(name):
    """-> (BlockVolume, min_weight, rounds): rounds is the list of block lists to hand to allocate_blocks, in this order."""
    one = lambda v: (v, 1.0, [v.blocks])
    if name == "single":
        return one(plane_blocks([(0, 0, 0)], NORMAL, (3.5, 3.5, 3.5), color=True))
    if name.startswith("pair_") or name.startswith("missing_"):
        d = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}[name.split("_")[1]]
        return one(pair(d, missing=name.startswith("missing_"), color=name == "pair_z"))
    if name in ("corner", "corner_missing"):                    # the 2 x 2 x 2 blocks around a lattice corner with the plane through it: the cell that
        # spans all eight is cut, and its vertex on the +x+y+z edge belongs to the first block and ends in the last -- which `corner_missing` lacks
        blocks = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]) + BASE_BLOCK
        return one(plane_blocks(blocks[:8 if name == "corner" else 7], NORMAL, 8.0 * BASE_BLOCK + 7.5, color=True))
    if name == "reverse_pool":                                  # 2 x 2 x 2 blocks, the four with the higher keys allocated first
        blocks = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]) + BASE_BLOCK
        v = plane_blocks(blocks, NORMAL, 8.0 * BASE_BLOCK + 7.5, color=True)
        return v, 1.0, [blocks[4:][::-1], blocks[:4][::-1]]
    if name == "negative":                                      # every position is a dyadic number: both sides are exact
        blocks = np.array([(x, y, z) for z in (-2, -1) for y in (-1, 0) for x in (-3, -2)])
        return one(plane_blocks(blocks, (0.25, 0.5, 0.375), (-12.5, -0.5, -8.5), voxel=0.0625, origin=(4.0, -2.0, 1.0), color=True))
    if name == "extreme":                                       # the ends of the coordinate range on each axis, and a pair across a corner of it
        ends = [tuple(e if a == b else 0 for b in range(3)) for a in range(3) for e in (-LIMIT, LIMIT - 1)]
        ends += [(-LIMIT, -LIMIT, -LIMIT), (-LIMIT + 1, -LIMIT, -LIMIT), (LIMIT - 1, LIMIT - 1, LIMIT - 1), (LIMIT - 2, LIMIT - 1, LIMIT - 1)]
        v = sref.BlockVolume((0.0, 0.0, 0.0), 0.0625, ends, color=False)
        l = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")[::-1], -1).astype(np.float64)
        # the plane through each block's own middle (and so through the shared face of the two pairs, which are adjacent along x)
        v.tsdf = np.tile(np.clip((l - 3.5) @ np.array((0.05, 0.37, 0.41)), -1.0, 1.0).astype(np.float32), (len(ends), 1, 1))
        v.wsum[:] = 1.0
        return one(v)
    if name.startswith("table_"):
        n = int(name.split("_")[1])
        blocks = [(x - 30, 1, -1) for x in range(n)]
        return one(plane_blocks(blocks, (0.005, 0.37, 0.41), (-236.5, 11.5, -4.5)))     # from the first block's middle, through all 65
    if name == "all_positive":
        v = plane_blocks([(0, 0, 0), (1, 0, 0)], NORMAL, (7.5, 3.5, 3.5))
        v.tsdf = np.abs(v.tsdf) + np.float32(0.01)
        return one(v)
    if name.startswith("embedded_"):
        vol, mw = cases.extraction_volume(name[len("embedded_"):])
        v = sref.from_dense(vol, OFFSET)
        return v, mw, [v.blocks]
    raise KeyError(name)


EXTRACTION = ("single", "pair_x", "pair_y", "pair_z", "corner", "missing_x", "missing_y", "missing_z", "corner_missing", "reverse_pool", "negative", "extreme",
              "table_1", "table_2", "table_65", "embedded_sphere", "embedded_sphere_color", "embedded_min_weight", "all_positive")


@functools.lru_cache(maxsize=None)
def extraction_reference(name):
    vol, mw, _ = extraction_volume(name)
    return sref.extract(vol, mw)


def lattice_units(vertices, vol, offset=(0, 0, 0)):
    """Positions as lattice coordinates of the volume `vol`, less 8 offset."""
    return (np.asarray(vertices, np.float64) - vol.origin) / vol.voxel_size - 8.0 * np.array(offset)


# ---- allocation and fusion ----

@functools.lru_cache(maxsize=None)
def allocations(name, margin=MARGIN):
    """The reference allocation of each of the four views of an integration case of tests/tsdf_cases.py."""
    kw = cases.integrate_kwargs(name)
    return tuple(sref.allocation(v.D, v.O, cases.TAN, v.pose, cases.ORIGIN, cases.VOXEL, cases.TRUNC, margin, v.weight, **kw) for v in cases.views(name))


def fuse_blocks(name, vol):
    """Applies the case's views to the BlockVolume `vol` in sequence -> [(volume after the view, updated, flagged)]."""
    c = cases.BY_NAME[name]
    steps = []
    for v in cases.views(name):
        upd, flagged = ref.integrate(vol, v.D, v.O, cases.TAN, v.pose, image=v.image, weight=v.weight, trunc=cases.TRUNC, max_weight=c.max_weight,
                                     **cases.integrate_kwargs(name))
        steps.append((vol.copy(), upd, flagged))
    return steps


@functools.lru_cache(maxsize=None)
def sphere_allocations(margin=MARGIN):
    return tuple(sref.allocation(v.D, v.O, cases.E2E_TAN, v.pose, (0.0, 0.0, 0.0), 1.0, cases.E2E_TRUNC, margin) for v in cases.sphere_views())


@functools.lru_cache(maxsize=None)
def sphere_pipeline(margin=MARGIN):
    """The reference pipeline end to end: allocate for the six views, integrate them all, extract -> (BlockVolume, mesh)."""
    blocks = set()
    for a in sphere_allocations(margin):
        blocks |= a.sure | a.flagged
    vol = sref.BlockVolume((0.0, 0.0, 0.0), 1.0, sorted(blocks), color=False)
    for v in cases.sphere_views():
        ref.integrate(vol, v.D, v.O, cases.E2E_TAN, v.pose, trunc=cases.E2E_TRUNC, max_weight=64.0, inv_depth=True, min_opacity=0.5, near=0.2)
    return vol, sref.extract(vol, 1.0)
