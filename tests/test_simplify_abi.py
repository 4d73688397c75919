"""What the simplification (include/adgs_simplify.h, adgs.simplify) promises without a GPU: the entry points are declared, exported by the
cross-compiled library and bound with the declared arity; malformed calls are refused on the host, with a message, before anything is
launched; empty problems return 0; the scratch bounds of the header hold; the Python surface refuses malformed arguments and CPU tensors.
The numerics are in tests/test_gpu_simplify.py."""
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
ENTRIES = {"adgs_simplify_cluster_temp_bytes": ("size_t", 2), "adgs_simplify_cluster": ("int", 10), "adgs_simplify_cluster_emit": ("int", 13),
           "adgs_simplify_place_temp_bytes": ("size_t", 2), "adgs_simplify_place": ("int", 18)}
P = 0x1000
BIG = 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")


def counts9(*c):
    return (ctypes.c_longlong * 9)(*(c + (0,) * (9 - len(c))))


def origin3(*o):
    return (ctypes.c_float * 3)(*o)


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_simplify.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_simplify_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    assert {k for k in _lib.SIGNATURES if k.startswith("adgs_simplify_")} == set(ENTRIES)
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
        if ret == "int":
            assert args[-1] is ctypes.c_void_p                  # the stream
    # the mesh header keeps its own set: nothing of this feature is declared there
    assert "adgs_simplify" not in open(os.path.join(ROOT, "include", "adgs_mesh.h")).read()


def refused(_lib, name, f, cases_):
    for kw in cases_:
        assert f(**kw) == -1, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointers are never followed."""
    from adgs import _lib
    lib = _lib.lib()
    org = origin3(0, 0, 0)

    def cluster(V=9, F=4, vertices=P, faces=P, cell=0.5, origin=org, temp=P, vc=P, counts=True):
        return lib.adgs_simplify_cluster(V, F, vertices, faces, cell, origin, temp, vc, counts9(5, 5, 5) if counts else None, None)

    def emit(V=9, F=4, faces=P, vc=P, temp=P, counts=(6, 2, 7), root=P, nv=P, starts=P, members=P, fo=P, src=P):
        return lib.adgs_simplify_cluster_emit(V, F, faces, vc, temp, None if counts is None else counts9(*counts), root, nv, starts, members, fo, src, None)

    def place(V=9, F=4, V2=6, M=7, vertices=P, faces=P, colors=P, vc=P, starts=P, members=P, cell=0.5, origin=org, placement=1, lam=1e-3, temp=P,
              vo=P, co=P):
        return lib.adgs_simplify_place(V, F, V2, M, vertices, faces, colors, vc, starts, members, cell, origin, placement, lam, temp, vo, co, None)

    sizes = [dict(V=-1), dict(F=-1), dict(V=-9, F=-4), dict(V=-BIG - 1)]
    cells = [dict(cell=0.0), dict(cell=-1.0), dict(cell=NAN), dict(cell=INF), dict(origin=None), dict(origin=origin3(0, NAN, 0)),
             dict(origin=origin3(INF, 0, 0))]
    refused(_lib, "adgs_simplify_cluster", cluster, sizes + cells + [dict(vertices=None), dict(faces=None), dict(temp=None), dict(vc=None),
                                                                    dict(counts=False)])
    refused(_lib, "adgs_simplify_cluster_emit", emit, sizes + [dict(counts=None), dict(counts=(-1, 0, 0)), dict(counts=(3, -1, 3)), dict(counts=(10, 2, 10)),
                                                              dict(counts=(6, 5, 7)), dict(counts=(6, 2, 5)), dict(counts=(6, 2, 10)),
                                                              dict(counts=(2 ** 31, 2, 2 ** 31)), dict(faces=None), dict(vc=None), dict(temp=None),
                                                              dict(root=None), dict(nv=None), dict(starts=None), dict(members=None), dict(fo=None),
                                                              dict(src=None)])
    refused(_lib, "adgs_simplify_place", place, sizes + cells + [dict(V2=-1), dict(V2=10, M=10), dict(M=5), dict(M=10), dict(placement=2), dict(placement=-1),
                                                                dict(lam=0.0), dict(lam=-1e-3), dict(lam=NAN), dict(lam=INF), dict(vertices=None),
                                                                dict(faces=None), dict(vc=None), dict(starts=None), dict(members=None), dict(temp=None),
                                                                dict(vo=None), dict(colors=None), dict(co=None), dict(V=BIG, F=BIG)])

    # empty problems return 0 and launch nothing (no pointer is followed)
    c = counts9(5, 5, 5, 5, 5, 5, 5, 5, 5)
    assert lib.adgs_simplify_cluster(0, 0, None, None, 0.5, org, None, None, c, None) == 0 and list(c) == [0] * 9
    assert emit(V=0, F=0, counts=(0, 0, 0), faces=None, vc=None, temp=None, root=None, nv=None, starts=None, members=None, fo=None, src=None) == 0
    assert place(V=0, F=0, V2=0, M=0, vertices=None, faces=None, colors=None, vc=None, starts=None, members=None, temp=None, vo=None, co=None) == 0
    assert place(V2=0, M=0, vo=None, co=None, colors=None) == 0   # nothing in the output: nothing to write
    # faces over no vertices at all: every one of them is outside, known without reading any
    c = counts9(5, 5, 5)
    assert lib.adgs_simplify_cluster(0, 4, None, P, 0.5, org, None, None, c, None) == -2 and list(c) == [0, 0, 0, 0, 0, 4, 0, 0, 0]
    assert _lib.last_error() == "adgs_simplify_cluster: 4 faces index outside the 0 vertices"


def test_scratch_bounds_of_the_header():
    from adgs import _lib
    lib = _lib.lib()
    for V, F in ((0, 0), (1, 1), (7, 0), (5002, 5000), (368_000, 565_000), (2_000_000, 4_100_000), (BIG, 3), (3, BIG), (BIG, BIG)):
        got = lib.adgs_simplify_cluster_temp_bytes(V, F)
        assert 28 * V + 24 * F + 16 * max(V, F) <= got <= 45 * (V + F) + 65536, (V, F, got)
        got = lib.adgs_simplify_place_temp_bytes(V, F)
        assert 48 * F <= got <= 49 * F + 16384, (V, F, got)
    assert lib.adgs_simplify_place_temp_bytes(0, 1000) == lib.adgs_simplify_place_temp_bytes(BIG, 1000)
    for f in (lib.adgs_simplify_cluster_temp_bytes, lib.adgs_simplify_place_temp_bytes):
        assert [f(-1, 5), f(5, -1), f(2 ** 31, 5), f(5, 2 ** 31)] == [0, 0, 0, 0]


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import simplify
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(9, 3)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    cl = simplify.Clustering(z(9), z(5), z(5), z(6), z(6), z(2, 3), z(2), {}, 0.5, (0.0, 0.0, 0.0))
    assert len(cl) == 5
    calls = {"cluster_vertices": lambda faces, vertices=v, **kw: simplify.cluster_vertices(vertices, faces, kw.pop("cell_size", 0.5), **kw),
             "place_vertices": lambda faces, vertices=v, **kw: simplify.place_vertices(cl, vertices, faces, **kw),
             "simplify_mesh": lambda faces, vertices=v, **kw: simplify.simplify_mesh(vertices, faces, **dict({"cell_size": 0.5}, **kw))}
    for name, call in calls.items():
        with pytest.raises(TypeError, match=r"%s: faces must be int32.*\.int\(\)" % name):
            call(f.long())
        with pytest.raises(TypeError, match="faces must be int32"):
            call(f.float())
        with pytest.raises(TypeError, match="faces must be a tensor"):
            call(f.numpy())
        for bad in (z(4), z(4, 4), z(3, 4), z(1, 4, 3)):
            with pytest.raises(ValueError, match=r"faces must be \[F, 3\]"):
                call(bad)
        for bad in (torch.zeros(9), torch.zeros(9, 4), torch.zeros(3, 9)):
            with pytest.raises(ValueError, match=r"vertices must be \[(V|9), 3\]"):
                call(f, vertices=bad)
        with pytest.raises(TypeError, match="vertices must be float32"):
            call(f, vertices=v.double())
        with pytest.raises(TypeError, match="vertices must be a tensor"):
            call(f, vertices=v.numpy())
        with pytest.raises(RuntimeError, match="vertices is on"):
            call(f, vertices=meta(v))
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(z(0, 3))
    for name in ("cluster_vertices", "simplify_mesh"):
        for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-60, 1e60):
            with pytest.raises(ValueError, match="%s: cell_size must be a positive finite" % name):
                calls[name](f, cell_size=bad)
        for bad in (None, "1", True):
            with pytest.raises(TypeError, match="cell_size must be a number"):
                calls[name](f, cell_size=bad)
        for bad in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float("nan"), 0.0)):
            with pytest.raises(ValueError, match="origin must be"):
                calls[name](f, origin=bad)
        for bad in (None, 1.0, ("a", "b", "c")):
            with pytest.raises(TypeError, match="origin must be three numbers"):
                calls[name](f, origin=bad)
    for name in ("place_vertices", "simplify_mesh"):
        for bad in ("Quadric", "median", None, 1):
            with pytest.raises(ValueError, match="placement must be 'quadric' or 'average'"):
                calls[name](f, placement=bad)
        for bad in (0.0, -1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="regularization must be a positive finite"):
                calls[name](f, regularization=bad)
        with pytest.raises(TypeError, match="regularization must be a number"):
            calls[name](f, regularization=None)
        with pytest.raises(ValueError, match=r"colors must be \[9, 3\]"):
            calls[name](f, colors=torch.zeros(8, 3))
        with pytest.raises(TypeError, match="colors must be float32"):
            calls[name](f, colors=v.double())
    with pytest.raises(TypeError, match="clustering must be"):
        simplify.place_vertices(None, v, f)
    with pytest.raises(TypeError):                              # cell_size is keyword-only and required
        simplify.simplify_mesh(v, f)
    with pytest.raises(TypeError):
        simplify.simplify_mesh(v, f, None, 0.5)
