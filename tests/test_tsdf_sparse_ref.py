"""The float64 reference of the block-sparse TSDF volume (tests/tsdf_sparse_ref.py) and the cases of tests/tsdf_sparse_cases.py, on the CPU.

The sparse reference extraction of a block set equals tests/tsdf_ref.extract on the scattered dense volume: the vertices as a multiset of
rows (compared in lattice units, where the two differently placed origins drop out), the faces after mapping through that vertex
permutation and sorting.

The conditions of the GPU cases -- conditions, not measurements:
  per view, the blocks reachable only through flagged samples are at most 1 % of the marked blocks;
  for the end-to-end sphere, with allocation from its six views at the case's margin, the reference sparse mesh equals the reference dense
  mesh;
  no reference tsdf of that pipeline is within 1e-5 of zero."""
import os
import re

import numpy as np
import pytest

from tests import tsdf_cases as cases
from tests import tsdf_ref as ref
from tests import tsdf_sparse_cases as scases
from tests import tsdf_sparse_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", scases.EMBEDDED)
def test_sparse_extraction_equals_dense_extraction_of_the_scattered_volume(name):
    vol, mw = cases.extraction_volume(name)
    bv = sref.from_dense(vol, scases.OFFSET)
    assert (bv.blocks.min(0) == scases.OFFSET).all() and any(scases.OFFSET)
    V, F, C = sref.extract(bv, mw)
    Vd, Fd, Cd = cases.extraction_reference(name)
    assert len(F) == len(Fd) > 400 and len(V) == len(Vd)
    assert sref.match_meshes((scases.lattice_units(V, bv, scases.OFFSET), F, C), (scases.lattice_units(Vd, vol), Fd, Cd), quantum=2.0 ** -24), name
    # a permutation, not the identity: the sparse order goes block by block
    assert not np.array_equal(F, Fd)
    # and the test can fail: one face turned round is no longer the same mesh
    turned = F.copy()
    turned[0] = turned[0][::-1]
    assert not sref.match_meshes((scases.lattice_units(V, bv, scases.OFFSET), turned, C), (scases.lattice_units(Vd, vol), Fd, Cd), quantum=2.0 ** -24)


def test_sparse_order_is_block_key_then_local_index():
    """Vertices ascend by (block key of the owner, local index, slot), faces by (block key of the lowest corner, local index, tet)."""
    vol, mw, _ = scases.extraction_volume("reverse_pool")
    V, F, _ = sref.extract(vol, mw)
    p = np.floor(scases.lattice_units(V, vol) + 1e-9).astype(np.int64)          # the owner: the lower end of the vertex's edge (t < 1)
    key = sref.block_key(p >> 3)
    local = ((p[:, 2] & 7) * 8 + (p[:, 1] & 7)) * 8 + (p[:, 0] & 7)
    order = key.astype(np.float64) * 512 + local
    assert (np.diff(order) >= 0).all() and len(np.unique(key)) > 4
    # every face's first-listed cell order: the lowest corner of a face's cell is the componentwise floor of its vertices' minimum
    c = np.floor(scases.lattice_units(V, vol)[F].min(1) + 1e-9).astype(np.int64)
    ckey = sref.block_key(c >> 3).astype(np.float64) * 512 + ((c[:, 2] & 7) * 8 + (c[:, 1] & 7)) * 8 + (c[:, 0] & 7)
    assert (np.diff(ckey) >= 0).all()


@pytest.mark.parametrize("name", scases.EXTRACTION)
def test_extraction_cases_are_what_they_claim(name):
    vol, mw, rounds = scases.extraction_volume(name)
    V, F, C = scases.extraction_reference(name)
    assert sorted(map(tuple, np.concatenate(rounds))) == sorted(map(tuple, vol.blocks))
    if name == "all_positive":
        assert V.shape == (0, 3) and F.shape == (0, 3)
        return
    assert len(F) and np.unique(F).size == len(V) and ref.edge_stats(F)[0] == 0
    if name.startswith("pair_"):
        # vertices owned on both sides, and faces that use vertices of both blocks
        side = (np.floor(scases.lattice_units(V, vol) + 1e-9).astype(np.int64) >> 3 != scases.BASE_BLOCK).any(1)
        assert side.any() and not side.all() and (side[F].any(1) & ~side[F].all(1)).any()
        alone = scases.extraction_reference(name.replace("pair_", "missing_"))
        assert 0 < len(alone[1]) < len(F)                       # the missing block leaves a boundary
    if name == "corner":
        # the cell across the corner is cut, and a vertex on its main diagonal is owned by the first block; without the last block it is gone
        p = np.floor(scases.lattice_units(V, vol) + 1e-9).astype(np.int64)
        frac = scases.lattice_units(V, vol) - p
        top = 8 * scases.BASE_BLOCK + 7
        assert ((p == top).all(1) & (frac > 0).all(1)).sum() == 1
        assert 0 < len(scases.extraction_reference("corner_missing")[1]) < len(F)
    if name == "reverse_pool":
        keys = [sref.block_key(r) for r in rounds]
        assert keys[0].min() > keys[1].max()
    if name == "extreme":
        assert np.abs(vol.blocks).max() == scases.LIMIT and vol.blocks.max() == scases.LIMIT - 1


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_allocation_cases_meet_the_condition(name):
    marked = set()
    for view, a in enumerate(scases.allocations(name)):
        only_flagged = a.flagged - a.sure
        print("%s view %d: %d blocks marked, %d only through flagged samples, %d more possible, %d skipped samples"
              % (name, view, len(a.sure | a.flagged), len(only_flagged), len(a.maybe - a.sure - a.flagged), a.skipped))
        assert len(a.sure) >= 15 and a.skipped == 0
        assert len(only_flagged) <= 0.01 * len(a.sure | a.flagged), (name, view)
        assert a.flagged <= a.maybe
        marked |= a.sure
    lattice = set(scases.LATTICE_BLOCKS)
    assert len(marked & lattice) >= 30 and len(marked - lattice) >= 10          # the views reach beyond the dense lattice of tsdf_cases


def test_allocation_rule_on_a_single_ray():
    """One pixel looking down +z from the origin at a wall 10 m away, 0.5 m voxels, trunc 1: samples at z = 9, 10, 11; margin 2 voxels."""
    D, O = np.full((1, 1), 0.1, np.float32), np.ones((1, 1), np.float32)
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    a = sref.allocation(D, O, (0.5, 0.5), pose, (0.25, 0.25, 0.25), 0.5, 1.0, margin=2.0)
    # g = (-0.5, -0.5, z / 0.5 - 0.5): x and y span blocks -1 and 0, z the blocks of 17.5 +- 2, 19.5 +- 2, 21.5 +- 2 -> 1, 2 and 2, 2 and 2
    assert not a.flagged and a.skipped == 0
    assert a.sure == {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (1, 2)}
    # n comes from the float32 fields: 0.6f / 0.2f = 3.00000007 in double, so the integration cases have n = 4
    assert sref.steps_of(1.0, 0.5) == 2 and sref.steps_of(0.6, 0.2) == 4 and sref.steps_of(3.0, 1.0) == 3
    # a block coordinate beyond the range is skipped and counted, never wrapped
    far = sref.allocation(D, O, (0.5, 0.5), pose, (0.25, 0.25, -0.5 * 8 * (scases.LIMIT + 4)), 0.5, 1.0, margin=2.0)
    assert not far.sure and far.skipped == 3
    # margin 0 marks the sample's own block only
    assert sref.allocation(D, O, (0.5, 0.5), pose, (0.25, 0.25, 0.25), 0.5, 1.0, margin=0.0).sure == {(-1, -1, 2)}
    assert int(sref.block_key((-scases.LIMIT, 0, 1))) == ((scases.LIMIT + 1) << 42) | (scases.LIMIT << 21)


def test_end_to_end_sphere_is_decided():
    for a in scases.sphere_allocations():
        assert not (a.flagged - a.sure) and a.skipped == 0
    vol, mesh = scases.sphere_pipeline()
    dense, flags = cases.sphere_fused()
    assert not flags.any()
    assert np.abs(vol.tsdf).min() >= 1e-5
    want = ref.extract(dense, 1.0)
    assert len(want[1]) > 500
    assert sref.match_meshes(mesh, want)                         # unit voxels at the origin: the positions are equal as float64
    # The six views leave holes (5 % of their pixels are below min_opacity), in the dense reference too, so "closed" can only mean: closed
    # wherever the dense mesh is.  Every directed edge occurs once, the open edges are the dense mesh's, and the signed volume is positive.
    twice, unmatched, _ = ref.edge_stats(mesh[1])
    print("end-to-end sphere: V %d, F %d, %d open edges; signed volume %.1f" % (len(mesh[0]), len(mesh[1]), unmatched, ref.signed_volume(mesh[0], mesh[1])))
    assert twice == 0 and unmatched == ref.edge_stats(want[1])[1] and ref.signed_volume(mesh[0], mesh[1]) > 0


def test_block_integration_is_the_dense_integration_on_shared_points():
    """tests/tsdf_ref.integrate over the blocks' points gives, on the dense lattice, the dense reference's bits."""
    vol = sref.BlockVolume(cases.ORIGIN, cases.VOXEL, scases.LATTICE_BLOCKS, color=True)
    nz, ny, nx = cases.DIMS[::-1]
    for (dense, upd, _), (sparse, supd, _) in zip(cases.reference(cases.BASE), scases.fuse_blocks(cases.BASE, vol)):
        t = sparse.pool()[0].reshape(5, 3, 6, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(40, 24, 48)[:nz, :ny, :nx]
        u = supd.reshape(5, 3, 6, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(40, 24, 48)[:nz, :ny, :nx]
        assert np.array_equal(u, upd) and np.array_equal(t.view(np.uint32), dense.tsdf.view(np.uint32))


def test_the_kernels_share_the_dense_chain():
    """The per-point chain, classify and the triangle rule exist once, in the shared header; both .hip files include it and are built alike."""
    src = lambda f: open(os.path.join(ROOT, "ad-gs_amd", "csrc", f)).read()
    shared = src("tsdf_shared.h")
    for fn in ("tsdf_update_point", "classify", "cell_faces", "cell_emit_faces"):
        assert len(re.findall(r"__device__[^;{]*\b%s\s*\(" % fn, shared)) == 1, fn
        for f in ("tsdf.hip", "tsdf_sparse.hip"):
            assert '#include "tsdf_shared.h"' in src(f) and re.search(r"\b%s\s*\(" % fn, src(f)) and not re.search(r"__device__[^;{]*\b%s\s*\(" % fn, src(f)), (f, fn)
    make = src("Makefile")
    assert "$(OUT)/tsdf_sparse.o" in make and not re.search(r"^\$\(OUT\)/tsdf(_sparse)?\.o:", make, re.M)      # both through the generic rule
