"""What the block-sparse TSDF volume (include/adgs_sparse_tsdf.h, adgs.tsdf_sparse) promises without a GPU: the entry points are declared,
exported by the cross-compiled library and bound; the descriptor equals the header's; malformed calls are refused on the host, with a
message, before anything is launched (the pointers are made up and never followed); empty problems return 0; the scratch of the extraction
is bounded in terms of the number of blocks; the Python surface refuses malformed arguments and CPU tensors.  The numerics are in
tests/test_gpu_tsdf_sparse.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_tsdf_abi import IDENTITY, struct_fields  # noqa: E402

# symbol -> (return type, number of parameters)
ENTRIES = {"adgs_sparse_tsdf_allocate_temp_bytes": ("size_t", 2), "adgs_sparse_tsdf_allocate_view": ("int", 15), "adgs_sparse_tsdf_allocate_blocks": ("int", 11),
           "adgs_sparse_tsdf_integrate": ("int", 11), "adgs_sparse_tsdf_extract_temp_bytes": ("size_t", 1), "adgs_sparse_tsdf_extract_owner_bytes": ("size_t", 1),
           "adgs_sparse_tsdf_extract_count": ("int", 9), "adgs_sparse_tsdf_extract_emit": ("int", 14)}
P = 0x1000
INF, NAN = float("inf"), float("nan")
MAXB = 1 << 22


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, tsdf_sparse
    header = open(os.path.join(ROOT, "include", "adgs_sparse_tsdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()
    declared = re.findall(r"\b(int|size_t)\s+(adgs_sparse_tsdf_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, header).group(1))
    assert define("ADGS_SPARSE_TSDF_BLOCK") == tsdf_sparse.BLOCK == 8 and define("ADGS_SPARSE_TSDF_BLOCK_POINTS") == tsdf_sparse.BLOCK_POINTS == 512
    assert define("ADGS_SPARSE_TSDF_MAX_BLOCKS") == tsdf_sparse.MAX_BLOCKS == MAXB and define("ADGS_SPARSE_TSDF_COORD_LIMIT") == tsdf_sparse.COORD_LIMIT == 1 << 20
    assert define("ADGS_SPARSE_TSDF_MAX_STEPS") == tsdf_sparse.MAX_STEPS and define("ADGS_SPARSE_TSDF_OWNER_BYTES_PER_BLOCK") == 4 * 512
    fields = struct_fields(code, "adgs_sparse_tsdf_volume")
    assert [(n, t) for n, t in fields] == [(n, t) for n, t in tsdf_sparse.SparseTsdfVolumeDesc._fields_]
    assert ctypes.sizeof(tsdf_sparse.SparseTsdfVolumeDesc) == sum(ctypes.sizeof(t) for _, t in fields) == 32
    assert [f[0] for f in tsdf_sparse.SparseTsdfVolumeDesc._fields_] == ["struct_bytes", "num_blocks", "capacity", "table_capacity", "voxel_size", "origin"]
    # the dense header is untouched by the new entries (tests/test_tsdf_abi.py pins its set)
    assert "sparse" not in open(os.path.join(ROOT, "include", "adgs_tsdf.h")).read()
    # block keys: z-major, 21 bits per coordinate
    k = tsdf_sparse.block_keys(torch.tensor([[0, 0, 0], [-1, 2, -3], [(1 << 20) - 1, -(1 << 20), 0]]))
    L = 1 << 20
    assert k.tolist() == [(L << 42) | (L << 21) | L, ((L - 3) << 42) | ((L + 2) << 21) | (L - 1), (L << 42) | (2 * L - 1)]


def vol_desc(nb=5, cap=8, table=16, vs=0.25, origin=(0.0, 1.0, -2.0), struct_bytes=None):
    from adgs import tsdf_sparse
    d = tsdf_sparse.make_sparse_volume_desc(nb, cap, table, vs, origin)
    if struct_bytes is not None:
        d.struct_bytes = struct_bytes
    return d


def view_desc(H=8, W=16, inv=1, tx=0.5, ty=0.4, mo=0.5, near=0.2, md=INF, trunc=1.0, mw=64.0, pose=IDENTITY, view_bytes=None):
    from adgs import tsdf
    d = tsdf.make_view_desc(H, W, inv, (tx, ty), mo, near, md, trunc, mw, pose)
    if view_bytes is not None:
        d.struct_bytes = view_bytes
    return d


BAD_VOLUMES = [dict(struct_bytes=0), dict(struct_bytes=28), dict(struct_bytes=-1), dict(nb=-1), dict(cap=-1), dict(table=-1), dict(nb=MAXB + 1, cap=MAXB + 1),
               dict(cap=MAXB + 1), dict(table=MAXB + 1), dict(nb=2 ** 31 - 1, cap=2 ** 31 - 1)]
BAD_VOLUMES += [dict(vs=bad) for bad in (0.0, -0.5, INF, -INF, NAN)]
BAD_VOLUMES += [dict(origin=(0.0,) * i + (bad,) + (0.0,) * (2 - i)) for i in range(3) for bad in (INF, -INF, NAN)]
BAD_POOL = [dict(nb=9, cap=8)]                                  # more blocks than the pool has rows: refused wherever the pool is given
BAD_VIEWS = [dict(view_bytes=0), dict(view_bytes=140), dict(view_bytes=-1), dict(H=-1), dict(W=-1), dict(H=65536, W=32768), dict(H=2 ** 31 - 1, W=2)]
BAD_VIEWS += [{k: b} for k in ("tx", "ty", "trunc") for b in (0.0, -0.5, INF, -INF, NAN)]
BAD_VIEWS += [dict(mo=b) for b in (0.0, -0.5, 1.5, INF, NAN)] + [dict(mw=b) for b in (0.0, -1.0, NAN)] + [dict(near=b) for b in (-0.1, INF, -INF, NAN)]
BAD_VIEWS += [dict(pose=IDENTITY[:i] + [b] + IDENTITY[i + 1:]) for i in (0, 8, 11) for b in (INF, NAN)]
BAD_VIEWS += [dict(trunc=16.5)]                                 # 66 voxels of 0.25: more than ADGS_SPARSE_TSDF_MAX_STEPS


def check_refusals(name, f, bad):
    from adgs import _lib
    for kw in bad:
        assert f(**kw) < 0, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_malformed_allocating_calls_are_refused_on_the_host():
    from adgs import _lib
    lib = _lib.lib()
    counts4 = lambda: (ctypes.c_longlong * 4)(7, 7, 7, 7)

    def view(no_vol=False, no_view=False, margin=2.0, depth=P, opacity=P, weight=P, keys=P, slots=P, keys_out=P, slots_out=P, coords=P, cand=4096, temp=P,
             counts=True, vol=None, **vw):
        return lib.adgs_sparse_tsdf_allocate_view(None if no_vol else ctypes.byref(vol_desc(**(vol or {}))), None if no_view else ctypes.byref(view_desc(**vw)),
                                                  margin, depth, opacity, weight, keys, slots, keys_out, slots_out, coords, cand, temp,
                                                  counts4() if counts else None, None)

    bad = [dict(no_vol=True), dict(no_view=True), dict(depth=None), dict(opacity=None), dict(keys=None), dict(slots=None), dict(keys_out=None),
           dict(slots_out=None), dict(coords=None), dict(temp=None), dict(counts=False)]
    bad += [dict(vol=kw) for kw in BAD_VOLUMES] + BAD_VIEWS
    bad += [dict(margin=b) for b in (-0.1, 4.5, INF, NAN)] + [dict(cand=b) for b in (0, -1, 2 ** 31)]
    check_refusals("adgs_sparse_tsdf_allocate_view", view, bad)
    # an empty view is not an error and launches nothing; neither a weight nor (for an empty volume) a table is required
    for kw in (dict(H=0), dict(W=0), dict(H=0, weight=None), dict(W=0, vol=dict(nb=0), keys=None, slots=None), dict(H=0, margin=0.0), dict(H=0, margin=4.0)):
        assert view(**kw) == 0, kw

    def blocks(no_vol=False, coords_in=P, M=3, keys=P, slots=P, keys_out=P, slots_out=P, coords=P, temp=P, counts=True, **vol):
        return lib.adgs_sparse_tsdf_allocate_blocks(None if no_vol else ctypes.byref(vol_desc(**vol)), coords_in, M, keys, slots, keys_out, slots_out, coords, temp,
                                                    counts4() if counts else None, None)

    bad = [dict(no_vol=True), dict(coords_in=None), dict(keys=None), dict(slots=None), dict(keys_out=None), dict(slots_out=None), dict(coords=None),
           dict(temp=None), dict(counts=False), dict(M=-1), dict(M=2 ** 31)] + BAD_VOLUMES
    check_refusals("adgs_sparse_tsdf_allocate_blocks", blocks, bad)
    c = counts4()
    assert lib.adgs_sparse_tsdf_allocate_blocks(ctypes.byref(vol_desc()), None, 0, None, None, None, None, None, None, c, None) == 0 and list(c) == [0, 0, 0, 0]
    # the scratch: grows with the pixels and the candidates of a call, not with the volume
    small, big = lib.adgs_sparse_tsdf_allocate_temp_bytes(36 * 48, 4096), lib.adgs_sparse_tsdf_allocate_temp_bytes(1280 * 1920, 1 << 20)
    assert 24 * 4096 <= small <= 40 * 4096 + 65536 and 24 << 20 <= big <= (40 << 20) + (1 << 20)
    assert lib.adgs_sparse_tsdf_allocate_temp_bytes(-1, 4096) == 0 and lib.adgs_sparse_tsdf_allocate_temp_bytes(10, -1) == 0


def test_malformed_integrate_calls_are_refused_on_the_host():
    from adgs import _lib
    lib = _lib.lib()

    def call(no_vol=False, no_view=False, depth=P, opacity=P, image=P, weight=P, coords=P, tsdf_=P, wsum=P, color=P, vol=None, **vw):
        return lib.adgs_sparse_tsdf_integrate(None if no_vol else ctypes.byref(vol_desc(**(vol or {}))), None if no_view else ctypes.byref(view_desc(**vw)),
                                              depth, opacity, image, weight, coords, tsdf_, wsum, color, None)

    bad = [dict(no_vol=True), dict(no_view=True), dict(depth=None), dict(opacity=None), dict(coords=None), dict(tsdf_=None), dict(wsum=None),
           dict(image=None), dict(color=None)]
    bad += [dict(vol=kw) for kw in BAD_VOLUMES + BAD_POOL] + BAD_VIEWS
    check_refusals("adgs_sparse_tsdf_integrate", call, bad)
    for kw in (dict(vol=dict(nb=0)), dict(vol=dict(nb=0, cap=0, table=0)), dict(H=0), dict(W=0), dict(H=0, image=None, color=None), dict(W=0, weight=None),
               dict(vol=dict(nb=0), coords=None, tsdf_=None, wsum=None), dict(H=0, inv=0, mo=1.0, near=0.0, md=6.0, mw=INF)):
        assert call(**kw) == 0, kw


def test_malformed_extraction_calls_are_refused_on_the_host():
    from adgs import _lib
    lib = _lib.lib()
    counts3 = lambda *c: (ctypes.c_longlong * 3)(*c)

    def count(no_vol=False, keys=P, slots=P, tsdf_=P, wsum=P, mw=1.0, temp=P, counts=True, **vol):
        return lib.adgs_sparse_tsdf_extract_count(None if no_vol else ctypes.byref(vol_desc(**vol)), keys, slots, tsdf_, wsum, mw, temp,
                                                  counts3(5, 5, 5) if counts else None, None)

    def emit(no_vol=False, keys=P, slots=P, tsdf_=P, wsum=P, color=P, mw=1.0, temp=P, owners=P, counts=(9, 12, 1), vertices=P, faces=P, colors=P, **vol):
        return lib.adgs_sparse_tsdf_extract_emit(None if no_vol else ctypes.byref(vol_desc(**vol)), keys, slots, tsdf_, wsum, color, mw, temp, owners,
                                                 None if counts is None else counts3(*counts), vertices, faces, colors, None)

    shared = [dict(no_vol=True), dict(keys=None), dict(slots=None), dict(tsdf_=None), dict(wsum=None), dict(temp=None)] + BAD_VOLUMES + BAD_POOL
    shared += [dict(mw=b) for b in (0.0, -1.0, NAN, -INF)]       # an unobserved point must not count as valid
    check_refusals("adgs_sparse_tsdf_extract_count", count, shared + [dict(counts=False)])
    check_refusals("adgs_sparse_tsdf_extract_emit", emit, shared + [
        dict(counts=None), dict(counts=(-1, 0, 0)), dict(counts=(3, -2, 1)), dict(counts=(3, 2, -1)), dict(counts=(2 ** 31, 2, 1)), dict(counts=(9, 2 ** 31, 1)),
        dict(counts=(9, 12, 6)), dict(counts=(3, 1, 4)), dict(counts=(5 * 3584 + 1, 12, 1)), dict(counts=(9, 5 * 6144 + 1, 1)), dict(vertices=None),
        dict(faces=None), dict(owners=None), dict(color=None), dict(colors=None)])
    # a volume without blocks has no mesh: zero counts, nothing launched, nothing to emit
    for vol in (dict(nb=0), dict(nb=0, cap=0, table=0)):
        c = counts3(5, 5, 5)
        assert lib.adgs_sparse_tsdf_extract_count(ctypes.byref(vol_desc(**vol)), None, None, None, None, 1.0, None, c, None) == 0 and list(c) == [0, 0, 0]
        assert emit(counts=(0, 0, 0), **vol) == 0
    assert emit(counts=(0, 0, 0), keys=None, slots=None, tsdf_=None, wsum=None, temp=None, owners=None, vertices=None, faces=None, color=None, colors=None) == 0


def test_scratch_grows_with_the_blocks_only():
    from adgs import _lib
    lib = _lib.lib()
    for nb in (1, 2, 65, 4096, 100000, MAXB):
        got = lib.adgs_sparse_tsdf_extract_temp_bytes(nb)
        assert 12 * nb <= got <= 16 * nb + 4096, (nb, got)
    assert [lib.adgs_sparse_tsdf_extract_temp_bytes(n) for n in (-1, MAXB + 1)] == [0, 0]
    assert [lib.adgs_sparse_tsdf_extract_owner_bytes(n) for n in (-3, 0, 1, 7, MAXB)] == [0, 0, 2048, 14336, 2 ** 33]


def host_volume(color=True, nb=3):
    """A SparseTSDFVolume whose tensors live on the host: only good for reaching the refusals (a real one refuses to be built there)."""
    from adgs import tsdf_sparse
    v = object.__new__(tsdf_sparse.SparseTSDFVolume)
    v.origin, v.voxel_size, v.trunc, v.max_weight, v.margin, v.device = (0.0, 0.0, 0.0), 0.25, 1.0, 64.0, 2.0, torch.device("cpu")
    v._has_color, v._nb, v.skipped_samples = color, nb, 0
    v._pool = (torch.ones(4, 8, 8, 8), torch.zeros(4, 8, 8, 8), torch.zeros(4, 3, 8, 8, 8) if color else None)
    v._table, v._block_coords = (torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)), torch.zeros(8, 3, dtype=torch.int32)
    v._spare = v._temp = None
    v._max_candidates = 0
    return v


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import tsdf_sparse
    S = tsdf_sparse.SparseTSDFVolume
    for bad in (0.0, -0.1, INF, NAN):
        with pytest.raises(ValueError, match="voxel_size must be"):
            S(bad)
        with pytest.raises(ValueError, match="trunc must be"):
            S(0.1, trunc=bad)
    with pytest.raises(ValueError, match="trunc must be at most"):
        S(0.1, trunc=6.6)
    for bad in (None, 3.0, "abc", (1.0, 2.0, "x")):
        with pytest.raises(TypeError, match="origin must be"):
            S(0.1, origin=bad)
    for bad in ((1.0, 2.0), (0.0, NAN, 0.0), (0.0, 0.0, INF)):
        with pytest.raises(ValueError, match="origin must be"):
            S(0.1, origin=bad)
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="max_weight must be"):
            S(0.1, max_weight=bad)
    for bad in (4.0, True, "8", None):
        with pytest.raises(TypeError, match="capacity must be"):
            S(0.1, capacity=bad)
    for bad in (0, -1, MAXB + 1):
        with pytest.raises(ValueError, match="capacity must lie"):
            S(0.1, capacity=bad)
    for bad in (-0.5, 4.5, NAN, INF):
        with pytest.raises(ValueError, match="margin must lie"):
            S(0.1, margin=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S(0.1, device="cpu")
    # the views and properties of a volume
    vol = host_volume()
    assert vol.num_blocks == 3 and vol.capacity == 4 and vol.tsdf.shape == (3, 8, 8, 8) and vol.wsum.shape == (3, 8, 8, 8) and vol.color.shape == (3, 3, 8, 8, 8)
    assert vol.block_coords.shape == (3, 3) and vol.keys.shape == (3,) and vol.slots.shape == (3,) and host_volume(color=False).color is None
    assert vol.memory_bytes == 4 * 512 * 4 * 5 + 8 * (8 + 4 + 12)
    assert vol.tsdf.data_ptr() == vol._pool[0].data_ptr()       # views of the pool, not copies
    # allocate and integrate: the dense class's checks, before anything is launched
    d, o, img = torch.rand(8, 16), torch.rand(8, 16), torch.rand(3, 8, 16)
    pose = torch.eye(4, dtype=torch.float64)[:3]
    calls = {"allocate": lambda D=d, O=o, cam=((0.5, 0.4), pose), image=None, v=vol, **kw: v.allocate(D, O, cam, **kw),
             "integrate": lambda D=d, O=o, cam=((0.5, 0.4), pose), image=img, v=vol, **kw: v.integrate(D, O, cam, image=image, **kw)}
    for name, call in calls.items():
        for bad in (torch.rand(3, 8, 16), torch.rand(128)):
            with pytest.raises(ValueError, match="SparseTSDFVolume.%s: depth must be" % name):
                call(D=bad)
        for bad in (torch.rand(16, 8), torch.rand(8, 15)):
            with pytest.raises(ValueError, match="img_opacity must be"):
                call(O=bad)
            with pytest.raises(ValueError, match="weight must be"):
                call(weight=bad)
        with pytest.raises(TypeError, match="depth must be float32"):
            call(D=d.double())
        with pytest.raises(TypeError, match="depth must be a tensor"):
            call(D=d.numpy())
        with pytest.raises(RuntimeError, match="img_opacity is on"):
            call(O=torch.rand(8, 16, device="meta"))
        for bad in (None, 0.5, (0.5, 0.4), "ab"):
            with pytest.raises(TypeError, match="camera must be"):
                call(cam=bad)
        with pytest.raises(ValueError, match="tanfovx and tanfovy must be"):
            call(cam=((0.0, 0.4), pose))
        with pytest.raises(ValueError, match="pose must be"):
            call(cam=((0.5, 0.4), torch.eye(4)))
        for bad in (0.0, 1.5, NAN):
            with pytest.raises(ValueError, match="min_opacity must lie"):
                call(min_opacity=bad)
        for bad in (0.0, -1.0, NAN):
            with pytest.raises(ValueError, match="max_depth must be"):
                call(max_depth=bad)
        for bad in (-0.1, NAN, INF):
            with pytest.raises(ValueError, match="near must be"):
                call(near=bad)
        for kw in ({}, dict(weight=torch.ones(8, 16), inv_depth=False), dict(D=d[None], O=o[None])):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**kw)
    for bad in (torch.rand(8, 16), torch.rand(3, 8, 15)):
        with pytest.raises(ValueError, match="image must be"):
            calls["integrate"](image=bad)
    with pytest.raises(ValueError, match="image must be given exactly when"):
        calls["integrate"](image=None)
    with pytest.raises(ValueError, match="image must be given exactly when"):
        calls["integrate"](v=host_volume(color=False))
    with pytest.raises(RuntimeError, match="no CPU path"):
        calls["integrate"](allocate=False)
    # allocate_blocks
    for bad in ([[0, 0, 0]], None):
        with pytest.raises(TypeError, match="coords must be a tensor"):
            vol.allocate_blocks(bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(1, 3, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="coords must be"):
            vol.allocate_blocks(bad)
    for bad in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64)):
        with pytest.raises(TypeError, match="coords must be int32"):
            vol.allocate_blocks(bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.allocate_blocks(torch.zeros(2, 3, dtype=torch.int32))
    # extract_mesh, reserve, to_dense
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="min_weight must be > 0"):
            vol.extract_mesh(min_weight=bad)
    for bad in (4.0, True, None):
        with pytest.raises(TypeError, match="capacity must be"):
            vol.reserve(bad)
    for bad in (-1, MAXB + 1):
        with pytest.raises(ValueError, match="capacity must lie"):
            vol.reserve(bad)
    vol.reserve(2)                                              # never shrinks
    assert vol.capacity == 4
    for bad in ((0, 0), (0, 0, 0.5), (True, 0, 0), 3):
        with pytest.raises(TypeError, match="three integers"):
            vol.to_dense(bad, (1, 1, 1))
    for lo, hi in (((1, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 1, (1 << 20) + 1)), ((-(1 << 20) - 1, 0, 0), (0, 1, 1))):
        with pytest.raises(ValueError, match="lo_block <= hi_block"):
            vol.to_dense(lo, hi)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.to_dense((0, 0, 0), (1, 1, 1))
    assert "ORDER-DEPENDENT" in tsdf_sparse.__doc__ and "allocate=False" in tsdf_sparse.__doc__
