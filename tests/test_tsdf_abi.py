"""What the TSDF fusion and mesh extraction (include/adgs_tsdf.h, adgs.tsdf) promise without a GPU: the entry points are declared,
exported by the cross-compiled library and bound; the two descriptors equal the header's; malformed calls are refused on the host, with a
message, before anything is launched; empty problems return 0; the scratch bound of the header holds; the Python surface refuses
malformed arguments and CPU tensors.  The numerics are in tests/test_gpu_tsdf.py."""
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

# symbol -> (return type, number of parameters)
ENTRIES = {"adgs_tsdf_integrate": ("int", 10), "adgs_tsdf_extract_temp_bytes": ("size_t", 1), "adgs_tsdf_extract_owner_bytes": ("size_t", 1),
           "adgs_tsdf_extract_count": ("int", 7), "adgs_tsdf_extract_emit": ("int", 12)}
CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}


def struct_fields(code, name):
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            for n in names.split(","):
                m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", n)
                fields.append((m.group(1), CTYPES[ctype] * int(m.group(2)) if m.group(2) else CTYPES[ctype]))
    return fields


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, tsdf
    header = open(os.path.join(ROOT, "include", "adgs_tsdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_tsdf_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define\s+ADGS_TSDF_CHUNK\s+(\d+)", header).group(1)) == tsdf.CHUNK == 256
    assert int(re.search(r"#define\s+ADGS_TSDF_OWNER_BYTES_PER_CHUNK\s+(\d+)", header).group(1)) == 4 * tsdf.CHUNK
    # the descriptors: the same fields, types and order; no hidden padding
    for cname, cls, size in (("adgs_tsdf_volume", tsdf.TsdfVolumeDesc, 32), ("adgs_tsdf_view", tsdf.TsdfViewDesc, 144)):
        fields = struct_fields(code, cname)
        assert [(n, t) for n, t in fields] == [(n, t) for n, t in cls._fields_], cname
        assert ctypes.sizeof(cls) == sum(ctypes.sizeof(t) for _, t in fields) == size, cname
    assert [f[0] for f in tsdf.TsdfVolumeDesc._fields_] == ["struct_bytes", "nx", "ny", "nz", "voxel_size", "origin"]
    assert [f[0] for f in tsdf.TsdfViewDesc._fields_] == ["struct_bytes", "H", "W", "inv_depth", "tanfovx", "tanfovy", "min_opacity", "near",
                                                          "max_depth", "trunc", "max_weight", "reserved", "pose"]
    assert tsdf.TsdfViewDesc.pose.offset == 48


IDENTITY = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.1, 0, 0.3]
P = 0x1000
INF, NAN = float("inf"), float("nan")


def vol_desc(dims=(8, 6, 5), vs=0.25, origin=(0.0, 1.0, -2.0), struct_bytes=None):
    from adgs import tsdf
    d = tsdf.make_volume_desc(dims, vs, origin)
    if struct_bytes is not None:
        d.struct_bytes = struct_bytes
    return d


BAD_VOLUMES = [dict(struct_bytes=0), dict(struct_bytes=28), dict(struct_bytes=-1), dict(dims=(-1, 6, 5)), dict(dims=(8, -6, 5)), dict(dims=(8, 6, -5)),
               dict(dims=(2048, 1024, 1024)), dict(dims=(2 ** 31 - 1, 2, 1)), dict(dims=(65536, 65536, 1)), dict(dims=(2 ** 16, 2 ** 15, 2)),
               dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))]
BAD_VOLUMES += [dict(vs=bad) for bad in (0.0, -0.5, INF, -INF, NAN)]
BAD_VOLUMES += [dict(origin=(0.0,) * i + (bad,) + (0.0,) * (2 - i)) for i in range(3) for bad in (INF, -INF, NAN)]


def test_malformed_integrate_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib, tsdf
    lib = _lib.lib()
    name = "adgs_tsdf_integrate"

    def call(no_vol=False, no_view=False, depth=P, opacity=P, image=P, weight=P, tsdf_=P, wsum=P, color=P, vol=None, H=8, W=16, inv=1, tx=0.5, ty=0.4,
             mo=0.5, near=0.2, md=INF, trunc=1.0, mw=64.0, pose=IDENTITY, view_bytes=None):
        v = vol_desc(**(vol or {}))
        d = tsdf.make_view_desc(H, W, inv, (tx, ty), mo, near, md, trunc, mw, pose)
        if view_bytes is not None:
            d.struct_bytes = view_bytes
        return lib.adgs_tsdf_integrate(None if no_vol else ctypes.byref(v), None if no_view else ctypes.byref(d), depth, opacity, image, weight, tsdf_,
                                       wsum, color, None)

    bad = [dict(no_vol=True), dict(no_view=True), dict(depth=None), dict(opacity=None), dict(tsdf_=None), dict(wsum=None),
           dict(view_bytes=0), dict(view_bytes=140), dict(view_bytes=-1), dict(H=-1), dict(W=-1), dict(H=-8, W=-16), dict(H=65536, W=32768),
           dict(H=2 ** 31 - 1, W=2), dict(image=None), dict(color=None)]
    bad += [dict(vol=kw) for kw in BAD_VOLUMES]
    bad += [{k: b} for k in ("tx", "ty", "trunc") for b in (0.0, -0.5, INF, -INF, NAN)]
    bad += [dict(mo=b) for b in (0.0, -0.5, 1.5, INF, NAN)]
    bad += [dict(mw=b) for b in (0.0, -1.0, NAN)]
    bad += [dict(near=b) for b in (-0.1, INF, -INF, NAN)]
    bad += [dict(pose=IDENTITY[:i] + [b] + IDENTITY[i + 1:]) for i in (0, 8, 11) for b in (INF, NAN)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert _lib.last_error().startswith(name + ": "), (kw, _lib.last_error())
    # an empty problem is not an error and launches nothing; neither an image with a colour volume nor a weight is required
    for kw in (dict(vol=dict(dims=(0, 6, 5))), dict(vol=dict(dims=(8, 0, 5))), dict(vol=dict(dims=(8, 6, 0))), dict(vol=dict(dims=(0, 0, 0))),
               dict(H=0), dict(W=0), dict(H=0, W=0, vol=dict(dims=(0, 0, 0))), dict(H=0, image=None, color=None), dict(W=0, weight=None),
               dict(H=0, inv=0, mo=1.0, near=0.0, md=6.0, mw=INF)):
        assert call(**kw) == 0, kw


def test_malformed_extraction_calls_are_refused_on_the_host():
    from adgs import _lib
    lib = _lib.lib()
    counts3 = lambda *c: (ctypes.c_longlong * 3)(*c)

    def count(no_vol=False, tsdf_=P, wsum=P, mw=1.0, temp=P, counts=True, **vol):
        v = vol_desc(**vol)
        return lib.adgs_tsdf_extract_count(None if no_vol else ctypes.byref(v), tsdf_, wsum, mw, temp, counts3(5, 5, 5) if counts else None, None)

    def emit(no_vol=False, tsdf_=P, wsum=P, color=P, mw=1.0, temp=P, owners=P, counts=(9, 12, 1), vertices=P, faces=P, colors=P, **vol):
        v = vol_desc(**vol)
        return lib.adgs_tsdf_extract_emit(None if no_vol else ctypes.byref(v), tsdf_, wsum, color, mw, temp, owners,
                                          None if counts is None else counts3(*counts), vertices, faces, colors, None)

    shared = [dict(no_vol=True), dict(tsdf_=None), dict(wsum=None), dict(temp=None)] + BAD_VOLUMES
    calls = {"adgs_tsdf_extract_count": [(count, kw) for kw in shared + [dict(counts=False)]],
             "adgs_tsdf_extract_emit": [(emit, kw) for kw in shared + [
                 dict(counts=None), dict(counts=(-1, 0, 0)), dict(counts=(3, -2, 1)), dict(counts=(3, 2, -1)), dict(counts=(2 ** 31, 2, 1)),
                 dict(counts=(9, 2 ** 31, 1)), dict(counts=(9, 12, 2)), dict(counts=(3, 1, 4), dims=(40, 40, 40)), dict(vertices=None), dict(faces=None),
                 dict(owners=None), dict(color=None), dict(colors=None)]]}
    for name, cases_ in calls.items():
        for f, kw in cases_:
            assert f(**kw) < 0, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
    # lattices without a cell return zero counts and launch nothing; a mesh of nothing has nothing to emit
    for dims in ((0, 6, 5), (8, 0, 5), (0, 0, 0), (1, 1, 1), (5, 1, 7), (1, 9, 9), (9, 9, 1)):
        c = counts3(5, 5, 5)
        v = vol_desc(dims=dims)
        assert lib.adgs_tsdf_extract_count(ctypes.byref(v), P, P, 1.0, P, c, None) == 0 and list(c) == [0, 0, 0], dims
        assert emit(dims=dims, counts=(0, 0, 0)) == 0
    assert emit(counts=(0, 0, 0), owners=None, vertices=None, faces=None, color=None, colors=None) == 0


def test_scratch_grows_with_the_chunks_only():
    from adgs import _lib
    lib = _lib.lib()
    for dims in ((1, 1, 1), (41, 17, 38), (300, 5, 4), (1024, 256, 512), (1290, 1290, 1290)):
        v = vol_desc(dims=dims)
        chunks = -(-dims[0] * dims[1] * dims[2] // 256)
        got = lib.adgs_tsdf_extract_temp_bytes(ctypes.byref(v))
        assert 12 * chunks <= got <= 16 * chunks + 4096, (dims, got)
    assert lib.adgs_tsdf_extract_temp_bytes(None) == 0
    assert lib.adgs_tsdf_extract_temp_bytes(ctypes.byref(vol_desc(dims=(2048, 1024, 1024)))) == 0
    assert [lib.adgs_tsdf_extract_owner_bytes(n) for n in (-3, 0, 1, 7, 2 ** 23)] == [0, 0, 1024, 7168, 2 ** 33]


class Cam:
    FoVx, FoVy = 1.2, 0.8
    world_view_transform = torch.eye(4)


def host_volume(color=True, dims=(8, 6, 5)):
    """A TSDFVolume whose tensors live on the host: only good for reaching the refusals (a real one refuses to be built there)."""
    from adgs import tsdf
    v = object.__new__(tsdf.TSDFVolume)
    v.origin, v.voxel_size, v.dims, v.trunc, v.max_weight, v.device = (0.0, 0.0, 0.0), 0.25, dims, 1.0, 64.0, torch.device("cpu")
    nx, ny, nz = dims
    v.tsdf, v.wsum = torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx)
    v.color = torch.zeros(3, nz, ny, nx) if color else None
    return v


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import tsdf
    # the volume
    for bad in (None, 3.0, "abc", (1.0, 2.0, "x")):
        with pytest.raises(TypeError, match="origin must be"):
            tsdf.TSDFVolume(bad, 0.1, (4, 4, 4))
    for bad in ((1.0, 2.0), (0.0, NAN, 0.0), (0.0, 0.0, INF)):
        with pytest.raises(ValueError, match="origin must be"):
            tsdf.TSDFVolume(bad, 0.1, (4, 4, 4))
    for bad in (0.0, -0.1, INF, NAN):
        with pytest.raises(ValueError, match="voxel_size must be"):
            tsdf.TSDFVolume((0, 0, 0), bad, (4, 4, 4))
        with pytest.raises(ValueError, match="trunc must be"):
            tsdf.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), trunc=bad)
    for bad in (4, (4, 4), (4.0, 4, 4), (True, 4, 4), "444"):
        with pytest.raises(TypeError, match="dims must be"):
            tsdf.TSDFVolume((0, 0, 0), 0.1, bad)
    for bad in ((-1, 4, 4), (2048, 1024, 1024)):
        with pytest.raises(ValueError, match="dims must be"):
            tsdf.TSDFVolume((0, 0, 0), 0.1, bad)
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="max_weight must be"):
            tsdf.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), max_weight=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tsdf.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        tsdf.TSDFVolume.around(torch.rand(10, 3), 0.1, margin=0.2)
    for bad in (torch.rand(10), torch.rand(10, 2), torch.rand(0, 3), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="points must be"):
            tsdf.TSDFVolume.around(bad, 0.1)
    with pytest.raises(ValueError, match="points must be finite"):
        tsdf.TSDFVolume.around(torch.tensor([[0.0, NAN, 0.0]]), 0.1)
    with pytest.raises(ValueError, match="margin must be"):
        tsdf.TSDFVolume.around(torch.rand(10, 3), 0.1, margin=-1.0)
    # camera_pose: the transposition of multiview.relative_pose
    V = torch.arange(16.0).reshape(4, 4)
    pose = tsdf.camera_pose(V)
    assert pose.dtype == torch.float64 and pose.device.type == "cpu" and torch.equal(pose, V.double().T[:3])
    Cam2 = type("Cam2", (), dict(world_view_transform=V))
    assert torch.equal(tsdf.camera_pose(Cam2()), pose)
    from adgs import multiview
    assert torch.allclose(multiview.relative_pose(torch.eye(4), V + torch.eye(4)), tsdf.camera_pose(V + torch.eye(4)))
    for bad in (None, torch.eye(3), object()):
        with pytest.raises(ValueError, match="camera must be"):
            tsdf.camera_pose(bad)
    # integrate
    vol = host_volume()
    d, o, img = torch.rand(8, 16), torch.rand(8, 16), torch.rand(3, 8, 16)
    pose = torch.eye(4, dtype=torch.float64)[:3]

    def call(D=d, O=o, cam=((0.5, 0.4), pose), image=img, v=vol, **kw):
        return v.integrate(D, O, cam, image=image, **kw)

    for bad in (torch.rand(3, 8, 16), torch.rand(128), torch.rand(1, 1, 8, 16)):
        with pytest.raises(ValueError, match="depth must be"):
            call(D=bad)
    for bad in (torch.rand(16, 8), torch.rand(3, 8, 16), torch.rand(8, 15)):
        with pytest.raises(ValueError, match="img_opacity must be"):
            call(O=bad)
        with pytest.raises(ValueError, match="weight must be"):
            call(weight=bad)
    for bad in (torch.rand(8, 16), torch.rand(1, 8, 16), torch.rand(3, 8, 15), torch.rand(4, 8, 16)):
        with pytest.raises(ValueError, match="image must be"):
            call(image=bad)
    with pytest.raises(ValueError, match="image must be given exactly when"):
        call(image=None)
    with pytest.raises(ValueError, match="image must be given exactly when"):
        call(v=host_volume(color=False))
    for name, key, like in (("depth", "D", d), ("img_opacity", "O", o), ("image", "image", img)):
        with pytest.raises(TypeError, match=name + " must be float32"):
            call(**{key: like.double()})
        with pytest.raises(TypeError, match=name + " must be a tensor"):
            call(**{key: like.numpy()})
    for name, key, like in (("img_opacity", "O", o), ("image", "image", img)):
        with pytest.raises(RuntimeError, match=name + " is on"):
            call(**{key: torch.rand(*like.shape, device="meta")})
    with pytest.raises(TypeError, match="weight must be a tensor"):
        call(weight=1.0)
    with pytest.raises(RuntimeError, match="weight is on"):
        call(weight=torch.ones(8, 16, device="meta"))
    for bad in (None, 0.5, (0.5, 0.4), ((0.5, 0.4), pose.numpy()), "ab", object()):
        with pytest.raises(TypeError, match="camera must be"):
            call(cam=bad)
    for bad in (None, 0.5, (0.5,), "ab"):
        with pytest.raises(TypeError, match="FoVx / FoVy or a"):
            call(cam=(bad, pose))
    for bad in ((0.0, 0.4), (0.5, -0.4), (INF, 0.4), (0.5, NAN)):
        with pytest.raises(ValueError, match="tanfovx and tanfovy must be"):
            call(cam=(bad, pose))
    for bad in (torch.eye(4), torch.rand(12), torch.rand(4, 3), torch.eye(4, dtype=torch.int64)[:3]):
        with pytest.raises(ValueError, match="pose must be"):
            call(cam=((0.5, 0.4), bad))
    with pytest.raises(RuntimeError, match="pose must be a host tensor"):
        call(cam=((0.5, 0.4), torch.rand(3, 4, device="meta")))
    nonfinite = pose.clone()
    nonfinite[1, 3] = NAN
    with pytest.raises(ValueError, match="pose must be finite"):
        call(cam=((0.5, 0.4), nonfinite))
    for bad in (0.0, -0.1, 1.5, NAN, INF):
        with pytest.raises(ValueError, match="min_opacity must lie"):
            call(min_opacity=bad)
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="max_depth must be"):
            call(max_depth=bad)
    for bad in (-0.1, NAN, INF):
        with pytest.raises(ValueError, match="near must be"):
            call(near=bad)
    for kw in ({}, dict(D=d[None], O=o[None], cam=(Cam(), pose)), dict(cam=Cam()), dict(weight=torch.ones(8, 16), inv_depth=False),
               dict(weight=torch.ones(1, 8, 16), min_opacity=1.0, max_depth=6.0, near=0.0), dict(cam=((0.5, 0.4), pose.float())),
               dict(v=host_volume(color=False), image=None), dict(D=torch.rand(0, 16), O=torch.rand(0, 16), image=torch.rand(3, 0, 16))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(**kw)
    with pytest.raises(ValueError, match="min_weight must be"):
        vol.extract_mesh(min_weight=NAN)
