"""The block-sparse TSDF volume on the GPU (adgs.tsdf_sparse over include/adgs_sparse_tsdf.h, csrc/tsdf_sparse.hip) against
tests/tsdf_sparse_ref.py (float64 numpy), on the cases of tests/tsdf_cases.py (36 x 48 views, 0.2 m voxels) and tests/tsdf_sparse_cases.py.

Allocation: after every view the key set equals the reference's, outside the blocks that only flagged samples reach; pool order is
rounds, then ascending key.  Integration: NO tolerance -- the dense TSDFVolume of the same origin holds the same bits on the dense lattice
after every view (one device function, one set of flags); a skipped point keeps its bits.  Extraction from host-made float32 volumes:
`faces` EQUAL as integers, vertices and colours by the tolerance rule of tests/test_gpu_tsdf.py::check_mesh."""
import numpy as np
import pytest
import torch

from tests import tsdf_cases as cases
from tests import tsdf_ref as ref
from tests import tsdf_sparse_cases as scases
from tests import tsdf_sparse_ref as sref
from tests.multiview_cases import TAN

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_volume(name="base", capacity=4096, margin=scases.MARGIN, origin=cases.ORIGIN):
    from adgs import tsdf_sparse
    c = cases.BY_NAME[name]
    return tsdf_sparse.SparseTSDFVolume(cases.VOXEL, origin=origin, trunc=cases.TRUNC, max_weight=c.max_weight, color=c.image, capacity=capacity, margin=margin)


def view_args(view, name, image=True):
    kw = dict(weight=up(view.weight), **cases.integrate_kwargs(name))
    if image:
        kw["image"] = up(view.image)
    return (up(view.D), up(view.O), (TAN, torch.from_numpy(view.pose))), kw


def coords_of(blocks):
    return torch.tensor(np.ascontiguousarray(np.asarray(blocks).reshape(-1, 3)), dtype=torch.int32, device="cuda")


def check_table(v, rounds):
    """block_coords is the pool order (rounds, each in ascending key order); the table is the keys in ascending order with their rows."""
    from adgs import tsdf_sparse
    bc = v.block_coords.cpu().numpy()
    assert bc.shape == (v.num_blocks, 3) and sum(rounds) == v.num_blocks
    keys = sref.block_key(bc)
    at = 0
    for n in rounds:
        assert (np.diff(keys[at:at + n]) > 0).all()
        at += n
    assert len(np.unique(keys)) == len(keys)
    tk, ts = v.keys.cpu().numpy(), v.slots.cpu().numpy()
    assert (np.diff(tk) > 0).all() and sorted(ts) == list(range(v.num_blocks)) and np.array_equal(keys[ts], tk)
    assert torch.equal(tsdf_sparse.block_keys(v.block_coords), v.keys[torch.argsort(v.slots)])
    return set(map(tuple, bc))


@pytest.mark.parametrize("name", ["base", "lin", "noweight", "maxdepth"])
def test_allocation_matches_the_reference(name):
    v = new_volume(name, capacity=16)
    sure, maybe, rounds = set(), set(), []
    for view, a in zip(cases.views(name), scases.allocations(name)):
        args, kw = view_args(view, name, image=False)
        before = v.num_blocks
        new = v.allocate(*args, **kw)
        assert new == v.num_blocks - before and v.capacity >= v.num_blocks
        rounds.append(new)
        sure |= a.sure
        maybe |= a.maybe | a.flagged
        got = check_table(v, rounds)
        print("%s: %d new blocks, %d in all; reference %d sure, %d possible" % (name, new, len(got), len(sure), len(maybe - sure)))
        assert sure <= got and got <= sure | maybe, (name, sorted(sure - got), sorted(got - sure - maybe))
        assert v.allocate(*args, **kw) == 0 and v.num_blocks == before + new      # the same view again adds nothing
    assert v.skipped_samples == 0 and bool((v.tsdf == 1).all()) and not bool(v.wsum.any())
    assert v.memory_bytes >= v.num_blocks * 512 * 4 * 2


def test_allocate_blocks_with_duplicates_and_existing_blocks():
    v = new_volume("noimage", capacity=2)
    first = [(3, 0, 0), (-1, 2, 5), (3, 0, 0), (0, 0, -7), (-1, 2, 5)]
    assert v.allocate_blocks(coords_of(first)) == 3 and v.capacity >= 3
    assert check_table(v, [3]) == set(first)
    assert v.block_coords.tolist() == [[0, 0, -7], [3, 0, 0], [-1, 2, 5]]      # ascending key: z-major
    second = [(5, 5, 5), (3, 0, 0), (-4, 0, -7), (5, 5, 5), (0, 0, -7)]
    assert v.allocate_blocks(coords_of(second)) == 2
    assert check_table(v, [3, 2]) == set(first) | set(second)
    assert v.block_coords.tolist()[3:] == [[-4, 0, -7], [5, 5, 5]]
    assert v.allocate_blocks(coords_of(first + second)) == 0 and v.num_blocks == 5
    assert v.allocate_blocks(torch.zeros((0, 3), dtype=torch.int32, device="cuda")) == 0
    # a coordinate outside the range is counted and skipped, never wrapped
    L = scases.LIMIT
    assert v.allocate_blocks(coords_of([(L, 0, 0), (0, -L - 1, 0), (L - 1, -L, 0)])) == 1 and v.skipped_samples == 2
    assert v.block_coords.tolist()[5] == [L - 1, -L, 0]
    v.reset()
    assert v.num_blocks == 0 and v.skipped_samples == 0 and v.extract_mesh()[1].shape == (0, 3)


def dense_crop(d):
    nz, ny, nx = cases.DIMS[::-1]
    return (d.tsdf[:nz, :ny, :nx].cpu().numpy(), d.wsum[:nz, :ny, :nx].cpu().numpy(), None if d.color is None else d.color[:, :nz, :ny, :nx].cpu().numpy())


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_dense_equivalence_as_bits(name):
    """Every block that covers the dense 41 x 17 x 38 lattice is preallocated; the same four views go into it and into a dense TSDFVolume with
    the same origin.  tsdf, wsum and colour are equal as bits on the dense lattice after every view."""
    from adgs import tsdf
    c = cases.BY_NAME[name]
    v = new_volume(name, capacity=128)
    assert v.allocate_blocks(coords_of(scases.LATTICE_BLOCKS)) == 90
    d = tsdf.TSDFVolume(cases.ORIGIN, cases.VOXEL, cases.DIMS, trunc=cases.TRUNC, max_weight=c.max_weight, color=c.image)
    for view in cases.views(name):
        args, kw = view_args(view, name)
        v.integrate(*args, allocate=False, **kw)
        d.integrate(*args, **kw)
        assert v.num_blocks == 90
        got, want = dense_crop(v.to_dense((0, 0, 0), (6, 3, 5))), (d.tsdf.cpu().numpy(), d.wsum.cpu().numpy(), None if d.color is None else d.color.cpu().numpy())
        assert want[1].max() > 0
        for g, w in zip(got, want):
            assert (g is None) == (w is None) and (g is None or np.array_equal(bits(g), bits(w))), name


@pytest.mark.parametrize("name", ["base", "maxdepth"])
def test_a_skipped_point_is_not_written(name):
    """A poisoned pool (0.123 / 7 / 0.5) keeps its bits wherever the reference does not update (and does not flag) -- among the blocks one
    wholly behind the fourth camera and one outside every frustum, which the block test drops as a whole."""
    blocks = list(scases.LATTICE_BLOCKS) + [scases.BEHIND_FOURTH, scases.FAR_OUTSIDE]
    v = new_volume(name)
    assert v.allocate_blocks(coords_of(blocks)) == len(blocks)
    v.tsdf.fill_(0.123)
    v.wsum.fill_(7.0)
    if v.color is not None:
        v.color.fill_(0.5)
    order = [tuple(b) for b in v.block_coords.tolist()]
    start = sref.BlockVolume(cases.ORIGIN, cases.VOXEL, order, color=v.color is not None)
    start.tsdf[:], start.wsum[:] = 0.123, 7.0
    if start.color is not None:
        start.color[:] = 0.5
    snap = lambda: (v.tsdf.cpu().numpy().reshape(-1, 8, 8), v.wsum.cpu().numpy().reshape(-1, 8, 8),
                    None if v.color is None else v.color.cpu().numpy().transpose(1, 0, 2, 3, 4).reshape(3, -1, 8, 8))
    prev, excluded = snap(), np.zeros(start.tsdf.shape, bool)
    never = np.ones(start.tsdf.shape, bool)
    behind, far = order.index(scases.BEHIND_FOURTH), order.index(scases.FAR_OUTSIDE)
    for n, (view, (rv, upd, flagged)) in enumerate(zip(cases.views(name), scases.fuse_blocks(name, start))):
        args, kw = view_args(view, name)
        v.integrate(*args, allocate=False, **kw)
        now = snap()
        excluded |= flagged
        never &= ~upd & ~flagged
        keep = ~upd & ~excluded
        for a, b in zip(now, prev):
            assert a is None or np.array_equal(bits(a)[..., keep], bits(b)[..., keep]), (name, n)
        hit = upd & ~excluded
        assert hit.any() and np.abs(now[0].astype(np.float64) - rv.tsdf)[hit].max() <= 2.0 ** -22
        assert not upd[8 * far:8 * far + 8].any() and (n < 3 or not upd[8 * behind:8 * behind + 8].any())
        prev = now
    t, w, c = snap()
    assert never.mean() > 0.2 and never[8 * far:8 * far + 8].all()
    assert (bits(t)[never] == bits(np.float32(0.123).reshape(1))[0]).all() and (w[never] == 7.0).all() and (c is None or (c[:, never] == 0.5).all())


def test_growth_keeps_every_bit():
    """capacity = 1 and blocks allocated view by view, against a run with ample capacity."""
    name = "base"
    small, ample = new_volume(name, capacity=1), new_volume(name, capacity=4096)
    grew = 0
    for view in cases.views(name):
        args, kw = view_args(view, name)
        for v in (small, ample):
            cap = v.capacity
            v.integrate(*args, allocate=True, **kw)
            grew += v is small and v.capacity > cap
        assert small.num_blocks == ample.num_blocks and small.capacity < 4096 == ample.capacity
        assert torch.equal(small.block_coords, ample.block_coords) and torch.equal(small.keys, ample.keys) and torch.equal(small.slots, ample.slots)
        for a, b in ((small.tsdf, ample.tsdf), (small.wsum, ample.wsum), (small.color, ample.color)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert grew >= 2 and small.num_blocks > 100 and bool((small.wsum > 0).any())
    cap = small.capacity
    small.reserve(cap + 7)
    assert small.capacity == cap + 7 and torch.equal(small.tsdf.view(torch.int32), ample.tsdf.view(torch.int32))
    assert bool((small._pool[0][small.num_blocks:] == 1).all()) and not bool(small._pool[1][small.num_blocks:].any())


def device_volume(bv, rounds, min_capacity=1):
    """A SparseTSDFVolume holding the bits of the reference BlockVolume `bv`, its blocks allocated in the given rounds."""
    from adgs import tsdf_sparse
    v = tsdf_sparse.SparseTSDFVolume(bv.voxel_size, origin=tuple(bv.origin), color=bv.color is not None, capacity=min_capacity)
    for r in rounds:
        assert v.allocate_blocks(coords_of(r)) == len(r)
    where = {tuple(b): i for i, b in enumerate(bv.blocks.tolist())}
    rows = [where[tuple(b)] for b in v.block_coords.tolist()]
    T, W, C = bv.pool()
    v.tsdf.copy_(up(T[rows]))
    v.wsum.copy_(up(W[rows]))
    if C is not None:
        v.color.copy_(up(C[rows]))
    return v


def check_mesh(got, want, bv, what):
    """tests/test_gpu_tsdf.py::check_mesh for a block set: faces equal, vertices and colours within 2^-21 max(|coordinate| over the blocks,
    voxel_size)."""
    verts, faces, colors = got
    V, F, C = want
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    assert tuple(verts.shape) == V.shape and tuple(faces.shape) == F.shape, (what, verts.shape, faces.shape, V.shape, F.shape)
    assert (colors is None) == (C is None)
    assert np.array_equal(faces.cpu().numpy(), F), what
    lo, hi = 8 * bv.blocks.min(0), 8 * bv.blocks.max(0) + 7
    corner = np.abs(np.stack([bv.origin + bv.voxel_size * lo, bv.origin + bv.voxel_size * hi])).max()
    tol = 2.0 ** -21 * max(corner, bv.voxel_size)
    e_v = np.abs(verts.cpu().numpy().astype(np.float64) - V).max() if len(V) else 0.0
    e_c = np.abs(colors.cpu().numpy().astype(np.float64) - C).max() if C is not None and len(V) else 0.0
    print("%s: V %d, F %d; max error vertices %.2e, colours %.2e (tolerance %.2e)" % (what, len(V), len(F), e_v, e_c, tol))
    assert e_v <= tol and e_c <= tol, what


@pytest.mark.parametrize("name", scases.EXTRACTION)
def test_extraction_matches_the_sparse_reference(name):
    bv, min_weight, rounds = scases.extraction_volume(name)
    v = device_volume(bv, rounds)
    if name == "reverse_pool":                                  # the pool order is the reverse of the key order, half by half
        assert v.slots.tolist() == [4, 5, 6, 7, 0, 1, 2, 3]
    before = [t.clone() for t in (v.tsdf, v.wsum, v.keys, v.slots, v.block_coords)] + ([] if v.color is None else [v.color.clone()])
    got = v.extract_mesh(min_weight=min_weight)
    check_mesh(got, scases.extraction_reference(name), bv, name)
    if name == "all_positive":
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    if name == "negative":                                      # a dyadic lattice: both sides form the same doubles, and the device rounds them once
        assert np.array_equal(got[0].cpu().numpy(), scases.extraction_reference(name)[0].astype(np.float32))
    after = [v.tsdf, v.wsum, v.keys, v.slots, v.block_coords] + ([] if v.color is None else [v.color])
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(after, before))                   # extraction reads the volume only
    again = v.extract_mesh(min_weight=min_weight)                # and is deterministic to the bit
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("name", ["embedded_sphere_color", "embedded_min_weight", "negative"])
def test_to_dense_round_trip(name):
    """to_dense(...).extract_mesh(mw) is the sparse mesh in the dense order; unit (or dyadic) voxels at integer origins: equal bits."""
    bv, min_weight, rounds = scases.extraction_volume(name)
    v = device_volume(bv, rounds)
    lo, hi = bv.blocks.min(0), bv.blocks.max(0) + 1
    d = v.to_dense(tuple(int(x) for x in lo), tuple(int(x) for x in hi))
    assert d.dims == tuple(int(8 * (h - l)) for l, h in zip(lo, hi)) and np.allclose(d.origin, bv.origin + 8 * bv.voxel_size * lo, rtol=0, atol=0)
    sparse, dense = v.extract_mesh(min_weight), d.extract_mesh(min_weight)
    host = lambda m: tuple(None if t is None else t.cpu().numpy() for t in m)
    assert len(sparse[1]) > 100 and sref.match_meshes(host(sparse), host(dense))
    # an empty range and a range that misses every block
    assert v.to_dense((0, 0, 0), (0, 0, 0)).dims == (0, 0, 0)
    far = v.to_dense((100, 100, 100), (101, 101, 102))
    assert far.dims == (8, 8, 16) and bool((far.tsdf == 1).all()) and not bool(far.wsum.any())


def test_end_to_end_sphere():
    """The sphere from its six views: allocate all, integrate all, extract.  The faces equal the reference pipeline's."""
    from adgs import tsdf_sparse
    rv, want = scases.sphere_pipeline()
    v = tsdf_sparse.SparseTSDFVolume(1.0, trunc=cases.E2E_TRUNC, color=False, capacity=8, margin=scases.MARGIN)
    views = [((up(view.D), up(view.O), (cases.E2E_TAN, torch.from_numpy(view.pose))), dict(inv_depth=True)) for view in cases.sphere_views()]
    for args, kw in views:
        v.allocate(*args, **kw)
    assert set(map(tuple, v.block_coords.tolist())) == set(map(tuple, rv.blocks.tolist()))
    nb = v.num_blocks
    for args, kw in views:
        v.integrate(*args, allocate=False, **kw)
    assert v.num_blocks == nb
    rows = [rv.blocks.tolist().index(b) for b in v.block_coords.tolist()]
    T, W, _ = rv.pool()
    assert np.array_equal(v.wsum.cpu().numpy(), W[rows]) and np.abs(v.tsdf.cpu().numpy().astype(np.float64) - T[rows]).max() <= 2.0 ** -22
    got = v.extract_mesh(min_weight=1.0)
    check_mesh(got, want, rv, "sphere, six views")
    # closed wherever the dense reference mesh is (tests/test_tsdf_sparse_ref.py), every directed edge once, positive signed volume
    faces = got[1].cpu().numpy()
    twice, unmatched, _ = ref.edge_stats(faces)
    assert twice == 0 and unmatched == ref.edge_stats(ref.extract(cases.sphere_fused()[0], 1.0)[1])[1]
    assert ref.signed_volume(got[0].cpu().numpy(), faces) > 0


def test_interleaved_allocation_is_another_volume():
    """The documented order dependence: with allocate=True view by view, a block allocated by a later view never saw the earlier views.  The
    blocks are the same as with all allocations first; no point has seen more, and some have seen less."""
    name = "noweight"
    first, interleaved = new_volume(name), new_volume(name)
    views = [view_args(view, name) for view in cases.views(name)]
    for args, kw in views:
        first.allocate(*args, **{k: v for k, v in kw.items() if k != "image"})
    for args, kw in views:
        first.integrate(*args, allocate=False, **kw)
        interleaved.integrate(*args, allocate=True, **kw)
    assert torch.equal(torch.sort(first.keys).values, interleaved.keys)
    rows = first.slots[torch.searchsorted(first.keys, interleaved.keys[torch.argsort(interleaved.slots)])].long()      # first's row of each of interleaved's
    assert bool((interleaved.wsum <= first.wsum[rows]).all()) and bool((interleaved.wsum < first.wsum[rows]).any())


def test_truncated_allocation_through_the_abi():
    """adgs_sparse_tsdf_allocate_view with less scratch than the view has candidates: the emit pass drops candidates, the sort is given the cap
    and a device-side count, and the call returns 1 with counts[1] = what it needs.  It must leave the table it read, block_coords[:NB] and the pool
    alone (its outputs hold no result then); the call with exactly counts[1] candidates gives what a call with ample room gives."""
    import ctypes
    from adgs import _lib, tsdf, tsdf_sparse
    name = "base"
    views = cases.views(name)
    v = new_volume(name)
    args, kw = view_args(views[0], name, image=False)
    assert v.allocate(*args, **kw) > 0                          # a table that is not empty: the candidates are filtered against it
    NB, room = v.num_blocks, v.num_blocks + 4096
    (depth, opacity, camera), kw = view_args(views[1], name, image=False)
    H, W, tan, pose, mo, nr, md, d, o, _, w = tsdf._view_arguments("test", v.device, False, depth, opacity, camera, None, kw["weight"], kw["min_opacity"],
                                                                   kw["max_depth"], kw["near"])
    view = tsdf.make_view_desc(H, W, kw["inv_depth"], tan, mo, nr, md, v.trunc, v.max_weight, pose)
    keys, slots = v.keys.clone(), v.slots.clone()
    pool = [t.clone() for t in (v.tsdf, v.wsum, v.color)]

    def call(max_candidates):
        keys_out = torch.full((room,), -1, dtype=torch.int64, device="cuda")
        slots_out = torch.full((room,), -1, dtype=torch.int32, device="cuda")
        coords = torch.full((room, 3), -77, dtype=torch.int32, device="cuda")
        coords[:NB] = v.block_coords
        temp = torch.empty(int(_lib.lib().adgs_sparse_tsdf_allocate_temp_bytes(H * W, max_candidates)), dtype=torch.uint8, device="cuda")
        counts = (ctypes.c_longlong * 4)(-1, -1, -1, -1)
        desc = tsdf_sparse.make_sparse_volume_desc(NB, v.capacity, room, v.voxel_size, v.origin)
        code = _lib.call("adgs_sparse_tsdf_allocate_view", v.device, ctypes.byref(desc), ctypes.byref(view), v.margin, d.data_ptr(), o.data_ptr(), w.data_ptr(),
                         keys.data_ptr(), slots.data_ptr(), keys_out.data_ptr(), slots_out.data_ptr(), coords.data_ptr(), max_candidates, temp.data_ptr(), counts)
        # whatever the outcome, the call only reads these
        assert torch.equal(keys, v.keys) and torch.equal(slots, v.slots) and torch.equal(coords[:NB], v.block_coords)
        for a, b in zip(pool, (v.tsdf, v.wsum, v.color)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        return code, [int(x) for x in counts], keys_out, slots_out, coords

    code, counts, _, _, _ = call(1)
    print("max_candidates = 1 with %d blocks in the table: code %d, counts %s" % (NB, code, counts))
    assert code == 1 and counts[3] == 1 and counts[1] > 1
    found = counts[1]
    code, exact, keys_exact, slots_exact, coords_exact = call(found)
    assert code == 0 and exact[1] == found and exact[3] == 0
    code, ample, keys_ample, slots_ample, coords_ample = call(4 * found + 4096)
    assert code == 0 and ample[1] == found and ample[3] == 0
    new = ample[0]
    assert new > 0 and exact[0] == new and exact[2] == ample[2]
    assert torch.equal(keys_exact[:NB + new], keys_ample[:NB + new]) and torch.equal(slots_exact[:NB + new], slots_ample[:NB + new])
    assert torch.equal(coords_exact[NB:NB + new], coords_ample[NB:NB + new])
    # and that is what the volume makes of the view
    args, kw = view_args(views[1], name, image=False)
    assert v.allocate(*args, **kw) == new
    assert torch.equal(v.keys, keys_ample[:NB + new]) and torch.equal(v.slots, slots_ample[:NB + new]) and torch.equal(v.block_coords, coords_ample[:NB + new])


@pytest.mark.parametrize("per_wave", [1, 0])
def test_allocation_retries_with_the_room_the_call_asks_for(monkeypatch, per_wave):
    """SparseTSDFVolume with a scratch floor of 27 candidates (one per wave of the 36 x 48 views; per_wave = 1) or of a single one (per_wave = 0)
    instead of 4096: the first call of a view with more candidates than that is told there is no room, and the retry with found + found // 4
    gives the volume an unpatched one builds.  The last view has 23 candidates once the first three are in the table, so only the floor of 1 sends
    every view through the retry."""
    from adgs import _lib, tsdf_sparse
    name = "base"
    views = [view_args(view, name, image=False) for view in cases.views(name)]
    plain, tight = new_volume(name), new_volume(name)
    for args, kw in views:
        plain.allocate(*args, **kw)
    monkeypatch.setattr(tsdf_sparse, "MIN_CANDIDATES", 1)
    monkeypatch.setattr(tsdf_sparse, "CANDIDATES_PER_WAVE", per_wave)
    log, real = [], _lib.call

    def recording(symbol, *a):
        code = real(symbol, *a)
        if symbol == "adgs_sparse_tsdf_allocate_view":
            log.append((code, int(a[-3]), int(a[-1][1])))       # return code, max_candidates, counts[1]
        return code
    monkeypatch.setattr(_lib, "call", recording)
    floor = max(1, per_wave * -(-cases.H * cases.W // 64))
    retried = 0
    for n, (args, kw) in enumerate(views):
        del log[:]
        tight._max_candidates = 0                               # forget the scratch the last view needed: every view starts from the floor
        new = tight.allocate(*args, **kw)
        print("view %d: %d new blocks; (code, max_candidates, candidates) per call: %s" % (n, new, log))
        found = log[0][2]
        if found > floor:
            assert log == [(1, floor, found), (0, found + found // 4, found)] and tight._max_candidates == found + found // 4
            retried += 1
        else:
            assert log == [(0, floor, found)] and tight._max_candidates == 0
    assert retried == len(views) if per_wave == 0 else retried >= 1
    assert tight.num_blocks == plain.num_blocks > 100 and tight.skipped_samples == plain.skipped_samples
    assert torch.equal(tight.keys, plain.keys) and torch.equal(tight.slots, plain.slots) and torch.equal(tight.block_coords, plain.block_coords)
