"""What the mesh clean-up (include/adgs_mesh.h, adgs.mesh) promises without a GPU: the entry points are declared, exported by the
cross-compiled library and bound with the declared arity; malformed calls are refused on the host, with a message, before anything is
launched; empty problems return 0; the scratch bounds of the header hold; the Python surface refuses malformed arguments and CPU tensors.
The numerics are in tests/test_gpu_mesh.py."""
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
ENTRIES = {"adgs_mesh_label_temp_bytes": ("size_t", 2), "adgs_mesh_label": ("int", 7), "adgs_mesh_table": ("int", 12),
           "adgs_mesh_keep_temp_bytes": ("size_t", 2), "adgs_mesh_keep_count": ("int", 9), "adgs_mesh_keep_emit": ("int", 13),
           "adgs_mesh_normals_temp_bytes": ("size_t", 2), "adgs_mesh_vertex_normals": ("int", 7)}
P = 0x1000
BIG = 2 ** 31 - 1


def counts2(*c):
    return (ctypes.c_longlong * 2)(*c)


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_mesh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_mesh_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    assert {k for k in _lib.SIGNATURES if k.startswith("adgs_mesh_")} == set(ENTRIES)
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
        if ret == "int":
            assert args[-1] is ctypes.c_void_p                  # the stream


def refused(lib, _lib, name, f, cases_):
    for kw in cases_:
        assert f(**kw) < 0, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointers are never followed."""
    from adgs import _lib
    lib = _lib.lib()

    def label(V=9, F=4, faces=P, temp=P, vc=P, counts=True):
        return lib.adgs_mesh_label(V, F, faces, temp, vc, counts2(5, 5) if counts else None, None)

    def table(V=9, F=4, C=3, faces=P, vertices=P, vc=P, temp=P, root=P, nf=P, nv=P, area=P):
        return lib.adgs_mesh_table(V, F, C, faces, vertices, vc, temp, root, nf, nv, area, None)

    def count(V=9, F=4, C=3, faces=P, vc=P, keep=P, temp=P, counts=True):
        return lib.adgs_mesh_keep_count(V, F, C, faces, vc, keep, temp, counts2(5, 5) if counts else None, None)

    def emit(V=9, F=4, faces=P, vertices=P, colors=P, normals=P, temp=P, counts=(6, 2), vo=P, fo=P, co=P, no=P):
        return lib.adgs_mesh_keep_emit(V, F, faces, vertices, colors, normals, temp, None if counts is None else counts2(*counts), vo, fo, co, no, None)

    def normals(V=9, F=4, vertices=P, faces=P, temp=P, out=P):
        return lib.adgs_mesh_vertex_normals(V, F, vertices, faces, temp, out, None)

    sizes = [dict(V=-1), dict(F=-1), dict(V=-9, F=-4), dict(V=-BIG - 1)]
    refused(lib, _lib, "adgs_mesh_label", label, sizes + [dict(faces=None), dict(temp=None), dict(vc=None), dict(counts=False)])
    refused(lib, _lib, "adgs_mesh_table", table, sizes + [dict(C=-1), dict(C=10), dict(faces=None), dict(vc=None), dict(temp=None), dict(root=None),
                                                         dict(nf=None), dict(nv=None), dict(area=None), dict(vertices=None)])
    refused(lib, _lib, "adgs_mesh_keep_count", count, sizes + [dict(C=-1), dict(C=10), dict(faces=None), dict(vc=None), dict(keep=None), dict(temp=None),
                                                              dict(counts=False)])
    refused(lib, _lib, "adgs_mesh_keep_emit", emit, sizes + [dict(counts=None), dict(counts=(-1, 0)), dict(counts=(3, -1)), dict(counts=(10, 2)),
                                                             dict(counts=(6, 5)), dict(counts=(2 ** 31, 2)), dict(faces=None), dict(vertices=None),
                                                             dict(temp=None), dict(vo=None), dict(fo=None), dict(colors=None), dict(co=None),
                                                             dict(normals=None), dict(no=None)])
    refused(lib, _lib, "adgs_mesh_vertex_normals", normals, sizes + [dict(vertices=None), dict(faces=None), dict(temp=None), dict(out=None)])

    # empty problems return 0 and launch nothing (no pointer is followed)
    c = counts2(5, 5)
    assert lib.adgs_mesh_label(0, 0, None, None, None, c, None) == 0 and list(c) == [0, 0]
    assert table(V=0, F=0, C=0, faces=None, vertices=None, vc=None, temp=None, root=None, nf=None, nv=None, area=None) == 0
    assert table(C=0, root=None, nf=None, nv=None) == 0
    assert table(V=0, F=0, C=0) == 0
    c = counts2(5, 5)
    assert lib.adgs_mesh_keep_count(0, 0, 0, None, None, None, None, c, None) == 0 and list(c) == [0, 0]
    assert emit(V=0, F=0, counts=(0, 0), faces=None, vertices=None, colors=None, normals=None, temp=None, vo=None, fo=None, co=None, no=None) == 0
    assert emit(counts=(0, 0), vo=None, fo=None) == 0           # nothing kept: nothing to write
    assert normals(V=0, F=0, vertices=None, faces=None, temp=None, out=None) == 0
    assert normals(V=0, F=4, vertices=None, out=None) == 0      # no vertex: no normal
    # faces over no vertices at all: every one of them is outside, known without reading any
    c = counts2(5, 5)
    assert lib.adgs_mesh_label(0, 4, P, None, None, c, None) < 0 and list(c) == [0, 4]
    assert _lib.last_error() == "adgs_mesh_label: 4 faces index outside the 0 vertices"


def test_scratch_bounds_of_the_header():
    from adgs import _lib
    lib = _lib.lib()
    for V, F in ((0, 0), (1, 1), (7, 0), (5002, 5000), (368_000, 565_000), (2_000_000, 4_100_000), (BIG, 3), (3, BIG), (BIG, BIG)):
        got = lib.adgs_mesh_label_temp_bytes(V, F)
        assert 4 * V <= got <= 4 * V + V // 256 + 8192, (V, F, got)
        got = lib.adgs_mesh_keep_temp_bytes(V, F)
        assert 4 * (V + F) <= got <= 4 * (V + F) + (V + F) // 256 + 16384, (V, F, got)
        got = lib.adgs_mesh_normals_temp_bytes(V, F)
        assert 48 * F <= got <= 48 * F + F + 16384, (V, F, got)
    # the labelling scratch does not grow with F, the normals' not with V
    assert lib.adgs_mesh_label_temp_bytes(1000, 0) == lib.adgs_mesh_label_temp_bytes(1000, BIG)
    assert lib.adgs_mesh_normals_temp_bytes(0, 1000) == lib.adgs_mesh_normals_temp_bytes(BIG, 1000)
    for f in (lib.adgs_mesh_label_temp_bytes, lib.adgs_mesh_keep_temp_bytes, lib.adgs_mesh_normals_temp_bytes):
        assert [f(-1, 5), f(5, -1), f(2 ** 31, 5), f(5, 2 ** 31)] == [0, 0, 0, 0]


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import mesh
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(9, 3)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    calls = {"connected_components": lambda faces: mesh.connected_components(faces, 9), "vertex_normals": lambda faces: mesh.vertex_normals(v, faces),
             "remove_small_components": lambda faces: mesh.remove_small_components(v, faces)}
    for name, call in calls.items():
        with pytest.raises(TypeError, match=r"faces must be int32.*\.int\(\)"):
            call(f.long())
        with pytest.raises(TypeError, match="faces must be int32"):
            call(f.float())
        with pytest.raises(TypeError, match="faces must be a tensor"):
            call(f.numpy())
        for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32),
                    torch.zeros(1, 4, 3, dtype=torch.int32)):
            with pytest.raises(ValueError, match=r"faces must be \[F, 3\]"):
                call(bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(torch.zeros(0, 3, dtype=torch.int32))
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="num_vertices must lie"):
            mesh.connected_components(f, bad)
    for bad in (9.0, None, True):
        with pytest.raises(TypeError, match="num_vertices must be an integer"):
            mesh.connected_components(f, bad)
    # the other arguments are checked before the device, hence before any launch
    fm = f
    with pytest.raises(ValueError, match=r"vertices must be \[9, 3\]"):
        mesh.connected_components(fm, 9, vertices=torch.zeros(8, 3))
    with pytest.raises(TypeError, match="vertices must be float32"):
        mesh.connected_components(fm, 9, vertices=v.double())
    with pytest.raises(RuntimeError, match="vertices is on"):
        mesh.connected_components(fm, 9, vertices=meta(v))
    for bad in (torch.zeros(9), torch.zeros(9, 4), torch.zeros(3, 9)):
        with pytest.raises(ValueError, match=r"vertices must be \[V, 3\]"):
            mesh.vertex_normals(bad, fm)
    with pytest.raises(TypeError, match="vertices must be a tensor"):
        mesh.vertex_normals(v.numpy(), fm)
    with pytest.raises(TypeError, match="comps must be"):
        mesh.keep_components(None, torch.zeros(0, dtype=torch.bool), v, f)
    # select: host-side argument checks, and the rule itself on host tensors (torch operations only)
    n = torch.tensor([500, 40, 60, 60, 7, 300, 60, 55], dtype=torch.int32)
    comps = mesh.Components(torch.zeros(9, dtype=torch.int32), torch.arange(8, dtype=torch.int32), n, n, None)
    assert len(comps) == 8
    assert comps.select(3, 50).tolist() == [True, False, True, True, False, True, True, False]
    assert comps.select().tolist() == (n >= 50).tolist() and comps.select(50, 0).all() and comps.select(1, 0).tolist() == [True] + [False] * 7
    assert comps.select(2, 400).tolist() == [True] + [False] * 7
    with pytest.raises(ValueError, match="min_area needs the areas"):
        comps.select(min_area=1.0)
    with pytest.raises(ValueError, match="largest must be"):
        comps.select(0)
    with pytest.raises(TypeError, match="min_faces must be an integer"):
        comps.select(3, 2.5)
    comps.area = torch.arange(8.0, dtype=torch.float64)
    assert comps.select(8, 0, min_area=3.0).tolist() == [False] * 3 + [True] * 5
    with pytest.raises(ValueError, match=r"colors must be \[9, 3\]"):
        mesh.remove_small_components(v, f, colors=torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.keep_components(comps, torch.ones(8, dtype=torch.bool), v, f)
    for bad in (torch.ones(7, dtype=torch.bool), torch.ones(8), None):
        with pytest.raises(ValueError, match="keep must be a bool"):
            mesh.keep_components(comps, bad, v, fm)
