"""What the adjacency and the smoothing (include/adgs_smooth.h, adgs.smooth) promise without a GPU: the entry points are declared, exported by
the cross-compiled library and bound with the declared arity; malformed calls are refused on the host, with a message, before anything is
launched; empty problems return 0; the scratch bounds of the header hold; the Python surface refuses malformed arguments and CPU tensors.
The numerics are in tests/test_gpu_smooth.py."""
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
ENTRIES = {"adgs_smooth_adjacency_temp_bytes": ("size_t", 2), "adgs_smooth_adjacency_count": ("int", 7), "adgs_smooth_adjacency_emit": ("int", 7),
           "adgs_smooth_steps_temp_bytes": ("size_t", 2), "adgs_smooth_steps": ("int", 12)}
P = 0x1000
BIG = 2 ** 31 - 1
MOST = (2 ** 31 - 1) // 6                                       # the largest F with 6 F < 2^31
NAN, INF = float("nan"), float("inf")


def counts7(*c):
    return (ctypes.c_longlong * 7)(*(c + (0,) * (7 - len(c))))


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_smooth.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_smooth_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    assert {k for k in _lib.SIGNATURES if k.startswith("adgs_smooth_")} == set(ENTRIES)
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
        if ret == "int":
            assert args[-1] is ctypes.c_void_p                  # the stream
    # the mesh and the simplification headers keep their own sets: nothing of this feature is declared there
    for other in ("adgs_mesh.h", "adgs_simplify.h"):
        assert "adgs_smooth" not in open(os.path.join(ROOT, "include", other)).read()


def refused(_lib, name, f, cases_):
    for kw in cases_:
        assert f(**kw) == -1, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointers are never followed."""
    from adgs import _lib
    lib = _lib.lib()

    def count(V=9, F=4, faces=P, temp=P, boundary=P, counts=True):
        return lib.adgs_smooth_adjacency_count(V, F, faces, temp, boundary, counts7(5, 5, 5) if counts else None, None)

    def emit(V=9, F=4, temp=P, counts=(16,), starts=P, neighbors=P):
        return lib.adgs_smooth_adjacency_emit(V, F, temp, None if counts is None else counts7(*counts), starts, neighbors, None)

    def steps(V=9, N=16, vertices=P, starts=P, neighbors=P, fixed=P, steps=2, s_even=0.5, s_odd=-0.53, temp=P, out=2 * P):
        return lib.adgs_smooth_steps(V, N, vertices, starts, neighbors, fixed, steps, s_even, s_odd, temp, out, None)

    sizes = [dict(V=-1), dict(F=-1), dict(V=-9, F=-4), dict(V=-BIG - 1), dict(F=MOST + 1), dict(F=BIG)]
    refused(_lib, "adgs_smooth_adjacency_count", count, sizes + [dict(faces=None), dict(temp=None), dict(boundary=None), dict(counts=False)])
    refused(_lib, "adgs_smooth_adjacency_emit", emit, sizes + [dict(counts=None), dict(counts=(-2,)), dict(counts=(15,)), dict(counts=(26,)),
                                                               dict(counts=(2 ** 33,)), dict(V=0, counts=(2,)), dict(temp=None), dict(starts=None),
                                                               dict(neighbors=None)])
    refused(_lib, "adgs_smooth_steps", steps, [dict(V=-1), dict(N=-1), dict(V=-BIG - 1), dict(steps=-1), dict(steps=20001), dict(s_even=NAN),
                                               dict(s_odd=INF), dict(s_even=-INF), dict(vertices=None), dict(starts=None), dict(neighbors=None),
                                               dict(temp=None), dict(out=None), dict(out=P)])

    # empty problems return 0 and launch nothing (no pointer is followed)
    c = counts7(5, 5, 5, 5, 5, 5, 5)
    assert lib.adgs_smooth_adjacency_count(0, 0, None, None, None, c, None) == 0 and list(c) == [0] * 7
    assert emit(V=0, F=0, counts=(0,), temp=None, starts=None, neighbors=None) == 0
    assert emit(V=0, F=4, counts=(0,), temp=None, starts=None, neighbors=None) == 0
    assert steps(V=0, N=0, vertices=None, starts=None, neighbors=None, fixed=None, temp=None, out=None) == 0
    assert steps(V=0, N=0, steps=0, vertices=None, starts=None, neighbors=None, fixed=None, temp=None, out=None) == 0
    # faces over no vertices at all: every one of them is outside, known without reading any
    c = counts7(5, 5, 5)
    assert lib.adgs_smooth_adjacency_count(0, 4, P, None, None, c, None) == -2 and list(c) == [0, 4, 0, 0, 0, 0, 0]
    assert _lib.last_error() == "adgs_smooth_adjacency_count: 4 faces index outside the 0 vertices"


def test_scratch_bounds_of_the_header():
    from adgs import _lib
    lib = _lib.lib()
    for V, F in ((0, 0), (1, 1), (7, 0), (5002, 5000), (368_000, 565_000), (2_000_000, 4_100_000), (BIG, 3), (3, BIG), (BIG, BIG), (3, MOST), (BIG, MOST)):
        got = lib.adgs_smooth_adjacency_temp_bytes(V, F)
        if F > MOST:
            assert got == 0, (V, F, got)                        # 6 F >= 2^31
        else:
            assert 144 * F <= got <= 148 * F + 16384, (V, F, got)
        got = lib.adgs_smooth_steps_temp_bytes(V, F)
        assert 64 * V <= got <= 64 * V + 1024, (V, F, got)
    assert lib.adgs_smooth_adjacency_temp_bytes(0, 1000) == lib.adgs_smooth_adjacency_temp_bytes(BIG, 1000)
    assert lib.adgs_smooth_steps_temp_bytes(1000, 0) == lib.adgs_smooth_steps_temp_bytes(1000, BIG)
    for f in (lib.adgs_smooth_adjacency_temp_bytes, lib.adgs_smooth_steps_temp_bytes):
        assert [f(-1, 5), f(5, -1), f(2 ** 31, 5), f(5, 2 ** 31)] == [0, 0, 0, 0]
    assert lib.adgs_smooth_adjacency_temp_bytes(5, MOST + 1) == 0


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import smooth
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(9, 3)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    adj = smooth.Adjacency(z(10), z(16), torch.zeros(9, dtype=torch.bool), {})
    assert len(adj) == 8 and adj.degree().shape == (9,) and adj.degree().dtype == torch.int32
    calls = {"mesh_adjacency": lambda faces, **kw: smooth.mesh_adjacency(faces, kw.pop("num_vertices", 9), **kw),
             "smooth_mesh": lambda faces, vertices=v, **kw: smooth.smooth_mesh(vertices, faces, **kw)}
    for name, call in calls.items():
        with pytest.raises(TypeError, match=r"%s: faces must be int32.*\.int\(\)" % name):
            call(f.long())
        with pytest.raises(TypeError, match="faces must be int32"):
            call(f.float())
        with pytest.raises(TypeError, match="%s: faces must be a tensor" % name):
            call(f.numpy())
        for bad in (z(4), z(4, 4), z(3, 4), z(1, 4, 3)):
            with pytest.raises(ValueError, match=r"%s: faces must be \[F, 3\]" % name):
                call(bad)
        with pytest.raises(RuntimeError, match="%s: tensors must be on a HIP device; there is no CPU path" % name):
            call(f)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(z(0, 3))
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match=r"mesh_adjacency: num_vertices must lie in \[0, 2\^31\)"):
            calls["mesh_adjacency"](f, num_vertices=bad)
    for bad in (None, 9.0, True, "9"):
        with pytest.raises(TypeError, match="mesh_adjacency: num_vertices must be an integer"):
            calls["mesh_adjacency"](f, num_vertices=bad)
    call = calls["smooth_mesh"]
    for bad in (torch.zeros(9), torch.zeros(9, 4), torch.zeros(3, 9)):
        with pytest.raises(ValueError, match=r"smooth_mesh: vertices must be \[V, 3\]"):
            call(f, vertices=bad)
    with pytest.raises(TypeError, match="smooth_mesh: vertices must be float32"):
        call(f, vertices=v.double())
    with pytest.raises(TypeError, match="vertices must be a tensor"):
        call(f, vertices=v.numpy())
    with pytest.raises(RuntimeError, match="vertices is on"):
        call(f, vertices=meta(v))
    for bad in (-1, 10001):
        with pytest.raises(ValueError, match=r"smooth_mesh: iterations must lie in \[0, 10000\]"):
            call(f, iterations=bad)
    for bad in (None, 2.0, True, "2"):
        with pytest.raises(TypeError, match="smooth_mesh: iterations must be an integer"):
            call(f, iterations=bad)
    for bad in ("Taubin", "cotangent", None, 1):
        with pytest.raises(ValueError, match="smooth_mesh: method must be 'taubin' or 'laplacian'"):
            call(f, method=bad)
    for bad in ("Fixed", "pinned", None, True):
        with pytest.raises(ValueError, match="smooth_mesh: boundary must be 'fixed' or 'free'"):
            call(f, boundary=bad)
    for bad in (0.0, -0.5, 1.5, NAN, INF):
        with pytest.raises(ValueError, match=r"smooth_mesh: lam must be a finite number in \(0, 1\]"):
            call(f, lam=bad)
    for bad in (0.0, 0.53, -1.6, NAN, -INF):
        with pytest.raises(ValueError, match=r"smooth_mesh: mu must be a finite number in \[-1.5, 0\)"):
            call(f, mu=bad)
    for bad in (None, "0.5", True):
        with pytest.raises(TypeError, match="smooth_mesh: lam must be a number"):
            call(f, lam=bad)
        with pytest.raises(TypeError, match="smooth_mesh: mu must be a number"):
            call(f, mu=bad)
    for bad in (torch.zeros(8, dtype=torch.bool), torch.zeros(9, dtype=torch.uint8), torch.zeros(9, 1, dtype=torch.bool), [False] * 9):
        with pytest.raises(ValueError, match=r"smooth_mesh: fixed must be a bool \[V\] = \[9\] tensor"):
            call(f, fixed=bad)
    with pytest.raises(RuntimeError, match="smooth_mesh: fixed is on"):
        call(f, fixed=meta(torch.zeros(9, dtype=torch.bool)))
    with pytest.raises(TypeError, match="smooth_mesh: adjacency must be the Adjacency of mesh_adjacency"):
        call(f, adjacency=(adj.starts, adj.neighbors))
    with pytest.raises(ValueError, match="smooth_mesh: the adjacency is of 9 vertices, vertices has 8"):
        call(f, vertices=torch.zeros(8, 3), adjacency=adj)
    with pytest.raises(RuntimeError, match="smooth_mesh: the adjacency is on"):
        call(f, adjacency=smooth.Adjacency(meta(adj.starts), meta(adj.neighbors), meta(adj.boundary), {}))
    with pytest.raises(RuntimeError, match="no CPU path"):     # a matching adjacency on the host does not make a CPU path
        call(f, adjacency=adj)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(f, iterations=0)
