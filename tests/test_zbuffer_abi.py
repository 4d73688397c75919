"""What the mesh z-buffer (include/adgs_zbuffer.h, adgs.zbuffer, adgs.mesh.keep_faces) promises without a GPU: the entry points are declared,
exported by the cross-compiled library and bound with the declared arity; malformed calls are refused on the host, with a message, before
anything is launched; empty problems return 0; the scratch bound of the header holds; the Python surface refuses malformed arguments and
CPU tensors.  The numerics are in tests/test_gpu_zbuffer.py."""
import ctypes
import math
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
ENTRIES = {"adgs_zbuffer_temp_bytes": ("size_t", 3), "adgs_zbuffer_draw": ("int", 11), "adgs_zbuffer_interpolate": ("int", 11),
           "adgs_zbuffer_count_faces": ("int", 8), "adgs_zbuffer_keep_faces_count": ("int", 7)}
P = 0x1000
BIG = 2 ** 31 - 1
POSE = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_zbuffer.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_zbuffer_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    assert {k for k in _lib.SIGNATURES if k.startswith("adgs_zbuffer_")} == set(ENTRIES)
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
        if ret == "int":
            assert args[-1] is ctypes.c_void_p                  # the stream


def test_the_view_mirror_has_the_layout_of_the_header():
    from adgs import zbuffer
    header = open(os.path.join(ROOT, "include", "adgs_zbuffer.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} adgs_zbuffer_view;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in zbuffer.ZbufferViewDesc._fields_]
    assert ctypes.sizeof(zbuffer.ZbufferViewDesc) == 6 * 4 + 3 * 8 + 4 + 4 + 12 * 8 and zbuffer.ZbufferViewDesc.pose.offset % 8 == 0


def refused(_lib, name, f, cases_):
    for kw in cases_:
        assert f(**kw) < 0, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointers are never followed."""
    from adgs import _lib, zbuffer
    lib = _lib.lib()

    def view(H=29, W=37, tan=(0.7, 0.55), pose=POSE, near=0.2, max_depth=math.inf, cull=0, small_max=0, stages=0, short=0):
        v = zbuffer.make_view_desc(H, W, tan, pose, near, max_depth, cull, small_max, stages)
        v.struct_bytes -= short
        return ctypes.byref(v)

    def draw(V=9, F=4, vertices=P, faces=P, temp=P, face=P, depth=P, normal=P, counts=P, null_view=False, **kw):
        return lib.adgs_zbuffer_draw(None if null_view else view(**kw), V, F, vertices, faces, temp, face, depth, normal, counts, None)

    def interp(V=9, F=4, vertices=P, faces=P, face_map=P, C=3, attributes=P, out=P, null_view=False, **kw):
        return lib.adgs_zbuffer_interpolate(None if null_view else view(**kw), V, F, vertices, faces, face_map, C, attributes, 0.0, out, None)

    def count(H=29, W=37, F=4, face_map=P, scratch=P, views=P, pixels=P):
        return lib.adgs_zbuffer_count_faces(H, W, F, face_map, scratch, views, pixels, None)

    def keep(V=9, F=4, faces=P, face_keep=P, temp=P, counts=True):
        return lib.adgs_zbuffer_keep_faces_count(V, F, faces, face_keep, temp, (ctypes.c_longlong * 3)(5, 5, 5) if counts else None, None)

    nan, inf = math.nan, math.inf
    bad_pose = [tuple(x if k != j else bad for k, x in enumerate(POSE)) for j, bad in ((0, nan), (5, inf), (11, -inf))]
    views_ = [dict(null_view=True), dict(short=8), dict(short=200), dict(H=-1), dict(W=-1), dict(H=65536, W=32768), dict(H=BIG, W=2),
              dict(near=0.0), dict(near=-0.2), dict(near=nan), dict(near=inf), dict(tan=(0.0, 0.55)), dict(tan=(0.7, -1.0)), dict(tan=(nan, 0.55)),
              dict(tan=(0.7, inf)), dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=nan), dict(cull=2), dict(cull=-1),
              dict(small_max=-1), dict(small_max=4097), dict(stages=16), dict(stages=-1)] + [dict(pose=p) for p in bad_pose]
    sizes = [dict(V=-1), dict(F=-1), dict(V=-BIG - 1)]
    refused(_lib, "adgs_zbuffer_draw", draw, views_ + sizes + [dict(vertices=None), dict(faces=None), dict(temp=None), dict(face=None), dict(depth=None),
                                                              dict(counts=None)])
    refused(_lib, "adgs_zbuffer_interpolate", interp, views_ + sizes + [dict(C=-1), dict(vertices=None), dict(faces=None), dict(face_map=None),
                                                                       dict(attributes=None), dict(out=None)])
    refused(_lib, "adgs_zbuffer_count_faces", count, [dict(H=-1), dict(W=-1), dict(F=-1), dict(H=65536, W=32768), dict(face_map=None), dict(scratch=None),
                                                      dict(views=None), dict(pixels=None)])
    refused(_lib, "adgs_zbuffer_keep_faces_count", keep, sizes + [dict(faces=None), dict(face_keep=None), dict(temp=None), dict(counts=False),
                                                                 dict(V=0, temp=None)])

    # empty problems return 0 and launch nothing (no pointer is followed)
    assert draw(H=0) == 0 and draw(W=0) == 0 and draw(H=0, W=0, V=0, F=0, vertices=None, faces=None) == 0
    assert draw(H=0, normal=None) == 0
    assert interp(H=0) == 0 and interp(C=0, face_map=None, attributes=None, out=None, vertices=None, faces=None) == 0
    assert count(H=0) == 0 and count(W=0, face_map=None, scratch=None, views=None, pixels=None) == 0
    assert count(F=0, face_map=None, scratch=None, views=None, pixels=None) == 0
    c = (ctypes.c_longlong * 3)(5, 5, 5)
    assert lib.adgs_zbuffer_keep_faces_count(9, 0, None, None, P, c, None) == 0 and list(c) == [0, 0, 0]
    c = (ctypes.c_longlong * 3)(5, 5, 5)
    assert lib.adgs_zbuffer_keep_faces_count(0, 0, None, None, None, c, None) == 0 and list(c) == [0, 0, 0]


def test_scratch_bound_of_the_header():
    from adgs import _lib
    lib = _lib.lib()
    for H, W, F in ((0, 0, 0), (1, 1, 1), (29, 37, 0), (96, 128, 340), (1280, 1920, 564_968), (1280, 1920, 4_100_000), (1, BIG, 3), (BIG, 1, BIG),
                    (46340, 46340, BIG)):
        got = lib.adgs_zbuffer_temp_bytes(H, W, F)
        assert 8 * H * W + 4 * F <= got <= 8 * H * W + 4 * F + 2048, (H, W, F, got)
    f = lib.adgs_zbuffer_temp_bytes
    assert [f(-1, 5, 5), f(5, -1, 5), f(5, 5, -1), f(65536, 32768, 5), f(2 ** 31, 1, 5), f(5, 5, 2 ** 31)] == [0] * 6


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import mesh, zbuffer
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(9, 3)
    pose = torch.eye(4, dtype=torch.float64)[:3]
    cam = ((0.7, 0.55), pose)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    render = lambda faces=f, vertices=v, camera=cam, size=(29, 37), **kw: zbuffer.render_mesh(vertices, faces, camera, size, **kw)
    with pytest.raises(TypeError, match=r"faces must be int32.*\.int\(\)"):
        render(f.long())
    with pytest.raises(TypeError, match="faces must be a tensor"):
        render(f.numpy())
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.int32), torch.zeros(1, 4, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"faces must be \[F, 3\]"):
            render(bad)
    with pytest.raises(TypeError, match="vertices must be float32"):
        render(vertices=v.double())
    with pytest.raises(ValueError, match=r"vertices must be \[V, 3\]"):
        render(vertices=torch.zeros(9, 4))
    with pytest.raises(RuntimeError, match="vertices is on"):
        render(vertices=meta(v))
    with pytest.raises(TypeError, match="camera must be"):
        render(camera=None)
    with pytest.raises(ValueError, match="tanfovx and tanfovy must be finite"):
        render(camera=((0.0, 0.55), pose))
    with pytest.raises(ValueError, match=r"pose must be a floating-point \[3, 4\]"):
        render(camera=((0.7, 0.55), torch.eye(4)))
    with pytest.raises(ValueError, match="pose must be finite"):
        render(camera=((0.7, 0.55), pose * float("nan")))
    for bad in ((29,), 29, None):
        with pytest.raises(TypeError, match="size must be"):
            render(size=bad)
    with pytest.raises(TypeError, match="size must be two integers"):
        render(size=(29.0, 37))
    for bad in ((-1, 37), (65536, 32768)):
        with pytest.raises(ValueError, match="size must be >= 0"):
            render(size=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="near must be finite and > 0"):
            render(near=bad)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_depth must be > 0"):
            render(max_depth=bad)
    with pytest.raises(ValueError, match="cull must be"):
        render(cull="front")
    # everything else is fine: the device is asked last
    with pytest.raises(RuntimeError, match="no CPU path"):
        render()
    with pytest.raises(RuntimeError, match="no CPU path"):
        render(torch.zeros(0, 3, dtype=torch.int32), normals=True, cull="back", max_depth=30.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        zbuffer.visible_faces(v, f, [cam], (29, 37))
    with pytest.raises(RuntimeError, match="no CPU path"):
        zbuffer.FaceVisibility(4, "cpu")
    with pytest.raises(ValueError, match="num_faces must lie"):
        zbuffer.FaceVisibility(-1)
    with pytest.raises(TypeError, match="num_faces must be an integer"):
        zbuffer.FaceVisibility(4.0)

    r = zbuffer.MeshRender(torch.zeros(29, 37, dtype=torch.int32), torch.zeros(29, 37), None, torch.zeros(5, dtype=torch.int64), (29, 37),
                           zbuffer.make_view_desc(29, 37, (0.7, 0.55), POSE, 0.2, math.inf))
    with pytest.raises(TypeError, match="render must be the MeshRender"):
        zbuffer.interpolate(None, v, f, v)
    with pytest.raises(ValueError, match=r"attributes must be \[V, C\]"):
        zbuffer.interpolate(r, v, f, torch.zeros(8, 3))
    with pytest.raises(TypeError, match="attributes must be float32"):
        zbuffer.interpolate(r, v, f, v.double())
    with pytest.raises(TypeError, match="attributes must be a tensor"):
        zbuffer.interpolate(r, v, f, v.numpy())
    with pytest.raises(RuntimeError, match="attributes are on"):
        zbuffer.interpolate(r, v, f, meta(v))
    with pytest.raises(RuntimeError, match="no CPU path"):
        zbuffer.interpolate(r, v, f, v)

    keep = torch.ones(4, dtype=torch.bool)
    for bad in (torch.ones(3, dtype=torch.bool), torch.ones(4), None, keep.numpy()):
        with pytest.raises(ValueError, match=r"keep must be a bool \[F\]"):
            mesh.keep_faces(bad, v, f)
    with pytest.raises(TypeError, match="faces must be int32"):
        mesh.keep_faces(keep, v, f.long())
    with pytest.raises(ValueError, match=r"colors must be \[9, 3\]"):
        mesh.keep_faces(keep, v, f, colors=torch.zeros(8, 3))
    with pytest.raises(TypeError, match="normals must be float32"):
        mesh.keep_faces(keep, v, f, normals=v.double())
    with pytest.raises(RuntimeError, match="keep is on"):
        mesh.keep_faces(meta(keep), v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.keep_faces(keep, v, f, colors=v, normals=v)
