"""What the geometry evaluation (include/adgs_geometry.h, adgs.geometry) promises without a GPU: the entry points are declared, exported by the
cross-compiled library and bound with the declared arity; malformed calls are refused on the host, with a message, before anything is
launched; empty problems return 0; the scratch bounds of the header hold; the Python surface refuses malformed arguments and CPU tensors.
The numerics are in tests/test_gpu_geometry.py."""
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
ENTRIES = {"adgs_geometry_grid_temp_bytes": ("size_t", 1), "adgs_geometry_grid_plan": ("int", 8), "adgs_geometry_grid_build": ("int", 11),
           "adgs_geometry_nearest_temp_bytes": ("size_t", 1), "adgs_geometry_nearest": ("int", 15), "adgs_geometry_face_areas": ("int", 6),
           "adgs_geometry_sample": ("int", 11), "adgs_geometry_stats_temp_bytes": ("size_t", 1), "adgs_geometry_distance_stats": ("int", 8)}
P = 0x1000
BIG = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")


def f3(*v):
    return (ctypes.c_float * 3)(*v)


def i3(*v):
    return (ctypes.c_int * 3)(*v)


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_geometry.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    declared = re.findall(r"\b(int|size_t)\s+(adgs_geometry_\w+)\s*\(([^)]*)\)\s*;", code)
    assert {d[1]: (d[0], len(d[2].split(","))) for d in declared} == ENTRIES
    assert {k for k in _lib.SIGNATURES if k.startswith("adgs_geometry_")} == set(ENTRIES)
    for name, (ret, n) in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t) and len(args) == n, name
        assert getattr(lib, name) is not None
        if ret == "int":
            assert args[-1] is ctypes.c_void_p                  # the stream


def refused(_lib, name, f, cases_, needle=None):
    for kw in cases_:
        assert f(**kw) < 0, (name, kw)
        assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
        if needle:
            assert needle in _lib.last_error(), (name, kw, _lib.last_error())


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up device pointers are never followed."""
    from adgs import _lib
    lib = _lib.lib()
    fin = ctypes.c_longlong(0)

    def plan(M=9, points=P, cell=0.5, temp=P, origin=True, dims=True, finite=True):
        return lib.adgs_geometry_grid_plan(M, points, cell, temp, f3() if origin else None, i3() if dims else None, ctypes.byref(fin) if finite else None, None)

    def build(M=9, points=P, cell=0.5, origin=(0, 0, 0), dims=(4, 4, 4), temp=P, records=P, keys=P, starts=P, counts=P):
        return lib.adgs_geometry_grid_build(M, points, cell, None if origin is None else f3(*origin), None if dims is None else i3(*dims), temp, records,
                                            keys, starts, counts, None)

    def nearest(M=9, N=5, queries=P, md=0.5, cell=0.5, origin=(0, 0, 0), dims=(4, 4, 4), records=P, keys=P, starts=P, counts=P, temp=P, d2=P, idx=P):
        return lib.adgs_geometry_nearest(M, N, queries, md, cell, None if origin is None else f3(*origin), None if dims is None else i3(*dims), records,
                                         keys, starts, counts, temp, d2, idx, None)

    def areas(V=9, F=4, vertices=P, faces=P, out=P):
        return lib.adgs_geometry_face_areas(V, F, vertices, faces, out, None)

    def sample(V=9, F=4, n=5, vertices=P, faces=P, cdf=P, total=2.0, seed=0, points=P, face=P):
        return lib.adgs_geometry_sample(V, F, n, vertices, faces, cdf, total, seed, points, face, None)

    def stats(N=5, d2=P, taus=(0.1, 0.2), md=0.5, temp=P, out=P, nt=None):
        arr = None if taus is None else (ctypes.c_double * max(len(taus), 1))(*taus)
        return lib.adgs_geometry_distance_stats(N, d2, len(taus or ()) if nt is None else nt, arr, md, temp, out, None)

    bad_cell = [dict(cell=v) for v in (0.0, -1.0, INF, NAN)]
    refused(_lib, "adgs_geometry_grid_plan", plan, [dict(M=-1), dict(M=-BIG - 1), dict(points=None), dict(temp=None), dict(origin=False), dict(dims=False),
                                                     dict(finite=False)] + bad_cell)
    refused(_lib, "adgs_geometry_grid_plan", plan, bad_cell, "cell_size must be finite and positive")
    refused(_lib, "adgs_geometry_grid_build", build, [dict(M=-1), dict(points=None), dict(temp=None), dict(records=None), dict(keys=None), dict(starts=None),
                                                      dict(counts=None), dict(origin=None), dict(dims=None), dict(origin=(NAN, 0, 0)), dict(dims=(-1, 4, 4))]
            + bad_cell)
    for name, f in (("adgs_geometry_grid_build", build), ("adgs_geometry_nearest", nearest)):
        refused(_lib, name, f, [dict(dims=(2 ** 21 + 1, 4, 4)), dict(dims=(4, 2 ** 21 + 1, 4)), dict(dims=(4, 4, BIG))], "enlarge cell_size")
        assert "at most 2^21" in _lib.last_error()
    refused(_lib, "adgs_geometry_nearest", nearest, [dict(M=-1), dict(N=-1), dict(queries=None), dict(d2=None), dict(idx=None), dict(records=None),
                                                     dict(keys=None), dict(starts=None), dict(counts=None), dict(temp=None), dict(origin=None), dict(dims=None)]
            + bad_cell)
    refused(_lib, "adgs_geometry_nearest", nearest, [dict(md=v) for v in (0.0, -0.5, INF, NAN)], "max_dist must be finite and positive")
    # R = ceil(max_dist (1 + 2^-20) / cell_size) > 8
    refused(_lib, "adgs_geometry_nearest", nearest, [dict(md=4.0, cell=0.5), dict(md=4.5, cell=0.5), dict(md=1e6, cell=1e-3)], "enlarge cell_size")
    assert nearest(N=0, md=3.9, cell=0.5) == 0                  # R = 8 passes
    refused(_lib, "adgs_geometry_face_areas", areas, [dict(V=-1), dict(F=-1), dict(vertices=None), dict(faces=None), dict(out=None)])
    refused(_lib, "adgs_geometry_sample", sample, [dict(V=-1), dict(F=-1), dict(n=-1), dict(F=0), dict(total=0.0), dict(total=-1.0), dict(total=INF),
                                                   dict(total=NAN), dict(vertices=None), dict(faces=None), dict(cdf=None), dict(points=None), dict(face=None)])
    refused(_lib, "adgs_geometry_sample", sample, [dict(F=0)], "no face")
    refused(_lib, "adgs_geometry_sample", sample, [dict(total=0.0), dict(total=NAN)], "total area")
    refused(_lib, "adgs_geometry_distance_stats", stats, [dict(N=-1), dict(d2=None), dict(temp=None), dict(out=None), dict(taus=(0.1,) * 5), dict(nt=-1),
                                                          dict(taus=None, nt=2), dict(taus=(0.1, 0.0)), dict(taus=(NAN,)), dict(taus=(INF,)), dict(md=0.0),
                                                          dict(md=NAN), dict(md=INF)])

    # empty problems return 0 and launch nothing (no pointer is followed)
    o, d = f3(5, 5, 5), i3(5, 5, 5)
    fin.value = 5
    assert lib.adgs_geometry_grid_plan(0, None, 0.5, None, o, d, ctypes.byref(fin), None) == 0
    assert list(o) == [0, 0, 0] and list(d) == [0, 0, 0] and fin.value == 0
    assert build(M=0, points=None, temp=None, records=None, keys=None, starts=None, dims=(0, 0, 0)) == 0
    assert nearest(N=0, queries=None, d2=None, idx=None, temp=None) == 0
    assert nearest(M=0, N=0, queries=None, d2=None, idx=None, temp=None, records=None, keys=None, starts=None, counts=None, dims=(0, 0, 0)) == 0
    assert areas(F=0, vertices=None, faces=None, out=None) == 0 and areas(V=0, F=0) == 0
    assert sample(n=0, vertices=None, faces=None, cdf=None, points=None, face=None) == 0
    assert sample(n=0, F=0, total=0.0) == 0                     # nothing asked of an empty mesh


def test_scratch_bounds_of_the_header():
    from adgs import _lib
    lib = _lib.lib()
    for n in (0, 1, 257, 5000, 20000, 1_000_000, 10_000_000, BIG):
        got = lib.adgs_geometry_grid_temp_bytes(n)
        assert 28 * n <= got <= 30 * n + 65536, (n, got)
        got = lib.adgs_geometry_nearest_temp_bytes(n)
        assert 24 * n <= got <= 26 * n + 65536, (n, got)
        got = lib.adgs_geometry_stats_temp_bytes(n)
        assert 1024 * 6 * 8 <= got <= 65536, (n, got)
    assert lib.adgs_geometry_stats_temp_bytes(1) == lib.adgs_geometry_stats_temp_bytes(BIG)
    for f in (lib.adgs_geometry_grid_temp_bytes, lib.adgs_geometry_nearest_temp_bytes, lib.adgs_geometry_stats_temp_bytes):
        assert [f(-1), f(2 ** 31), f(2 ** 40)] == [0, 0, 0]


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import geometry as geo
    pts = torch.zeros(9, 3)
    f = torch.zeros(4, 3, dtype=torch.int32)
    v = torch.zeros(9, 3)
    cdf = torch.ones(4, dtype=torch.float64)
    d2 = torch.zeros(5)
    point_calls = {"PointGrid": lambda p: geo.PointGrid(p, 0.5), "evaluate_points pred": lambda p: geo.evaluate_points(p, pts, (0.1,), 0.5),
                   "evaluate_points gt": lambda p: geo.evaluate_points(pts, p, (0.1,), 0.5), "evaluate_mesh gt": lambda p: geo.evaluate_mesh(v, f, p, (0.1,), 0.5)}
    for name, call in point_calls.items():
        with pytest.raises(TypeError, match="must be float32"):
            call(pts.double())
        with pytest.raises(TypeError, match="must be a tensor"):
            call(pts.numpy())
        for bad in (torch.zeros(9), torch.zeros(9, 4), torch.zeros(3, 9), torch.zeros(1, 9, 3)):
            with pytest.raises(ValueError, match=r"must be \[n, 3\]"):
                call(bad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(pts)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="cell_size must be finite and positive"):
            geo.PointGrid(pts, bad)
        with pytest.raises(ValueError, match="max_dist must be finite and positive"):
            geo.evaluate_points(pts, pts, (0.1,), bad)
        with pytest.raises(ValueError, match="max_dist must be finite and positive"):
            geo.distance_stats(d2, (0.1,), bad)
    for bad in ("0.5", None, True):
        with pytest.raises(TypeError, match="cell_size must be a number"):
            geo.PointGrid(pts, bad)
    # an empty set on either side
    for a, b in ((torch.zeros(0, 3), pts), (pts, torch.zeros(0, 3))):
        with pytest.raises(ValueError, match="an empty point set"):
            geo.evaluate_points(a, b, (0.1,), 0.5)
    with pytest.raises(ValueError, match="an empty point set"):
        geo.evaluate_mesh(v, f, pts, (0.1,), 0.5, samples=0)
    # thresholds
    with pytest.raises(ValueError, match="at most 4 thresholds"):
        geo.evaluate_points(pts, pts, (0.1,) * 5, 0.5)
    with pytest.raises(ValueError, match="exceeds max_dist"):
        geo.evaluate_points(pts, pts, (0.1, 0.6), 0.5)
    with pytest.raises(ValueError, match="threshold must be finite and positive"):
        geo.distance_stats(d2, (0.0,), 0.5)
    with pytest.raises(TypeError, match="thresholds must be a sequence"):
        geo.distance_stats(d2, ("a",), 0.5)
    with pytest.raises(TypeError, match="dist2 must be float32"):
        geo.distance_stats(d2.double(), (0.1,), 0.5)
    with pytest.raises(ValueError, match=r"dist2 must be \[N\]"):
        geo.distance_stats(torch.zeros(5, 1), (0.1,), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geo.distance_stats(d2, (0.1,), 0.5)
    # the mesh side
    mesh_calls = {"face_areas": lambda faces: geo.face_areas(v, faces), "sample_surface": lambda faces: geo.sample_surface(v, faces, 10),
                  "sample_from_cdf": lambda faces: geo.sample_from_cdf(v, faces, cdf, 10), "evaluate_mesh": lambda faces: geo.evaluate_mesh(v, faces, pts, (0.1,), 0.5)}
    for name, call in mesh_calls.items():
        with pytest.raises(TypeError, match=r"faces must be int32.*\.int\(\)"):
            call(f.long())
        with pytest.raises(ValueError, match=r"faces must be \[F, 3\]"):
            call(torch.zeros(4, 4, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(f)
    with pytest.raises(TypeError, match="vertices must be float32"):
        geo.face_areas(v.double(), f)
    with pytest.raises(TypeError, match="cdf must be float64"):
        geo.sample_from_cdf(v, f, cdf.float(), 10)
    for bad in (torch.ones(3, dtype=torch.float64), torch.ones(4, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"cdf must be \[F\] = \[4\]"):
            geo.sample_from_cdf(v, f, bad, 10)
    with pytest.raises(TypeError, match="cdf must be a tensor"):
        geo.sample_from_cdf(v, f, [1.0] * 4, 10)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="n must lie"):
            geo.sample_surface(v, f, bad)
    with pytest.raises(TypeError, match="n must be an integer"):
        geo.sample_surface(v, f, 10.0)
    with pytest.raises(TypeError, match="seed must be an integer"):
        geo.sample_from_cdf(v, f, cdf, 10, seed=-1)
    with pytest.raises(ValueError, match="no face to sample from"):
        geo.sample_surface(v, torch.zeros(0, 3, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match="no face to sample from"):
        geo.sample_from_cdf(v, torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, dtype=torch.float64), 10)
    # the search radius the host computes
    assert geo.search_radius(0.25, 0.25) == 2 and geo.search_radius(0.25, 0.25 * 1.001) == 1 and geo.search_radius(0.25, 0.1) == 3
    assert geo.search_radius(4.0, 0.5) == 9


def test_a_threshold_equal_to_max_dist_is_accepted_whichever_way_max_dist_rounds():
    """thresholds are 'each <= max_dist' against max_dist AS GIVEN: 0.16 and 0.7 round DOWN to float32, 0.1 and 0.3 up, 0.25 is exact.  The
    checks pass and the call ends at the device check, the last one; a threshold above max_dist is refused before it."""
    from adgs import geometry as geo
    pts, d2 = torch.zeros(9, 3), torch.zeros(5)
    f, v = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(9, 3)
    for md in (0.16, 0.7, 0.1, 0.3, 0.25):
        assert (geo._f32(md) < md) == (md in (0.16, 0.7))
        for call in (lambda t: geo.distance_stats(d2, t, md), lambda t: geo.evaluate_points(pts, pts, t, md), lambda t: geo.evaluate_mesh(v, f, pts, t, md)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call((md / 2, md))
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(md)
            with pytest.raises(ValueError, match="exceeds max_dist"):
                call((md * (1 + 2.0 ** -50),))
    # what distance_stats is handed by evaluate_points: the float32 value itself is a valid max_dist for a threshold up to it
    with pytest.raises(RuntimeError, match="no CPU path"):
        geo.distance_stats(d2, (geo._f32(0.16),), geo._f32(0.16))
