"""What the multi-view geometric consistency loss (include/adgs_multiview_geo.h, adgs.multiview) promises without a GPU: the two entry
points are declared, exported by the cross-compiled library and bound; the work-size constant and the descriptor equal the header's;
malformed calls are refused on the host, with a message, before anything is launched; empty problems return 0; the Python surface refuses
malformed arguments and CPU tensors.  The numerics are in tests/test_gpu_multiview_geo.py."""
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

# symbol -> number of parameters, the stream included
ENTRIES = {"adgs_multiview_geo_forward": 11, "adgs_multiview_geo_backward": 13}


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, multiview
    header = open(os.path.join(ROOT, "include", "adgs_multiview_geo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    for name, n in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert getattr(lib, name) is not None
    size = eval(re.search(r"#define\s+ADGS_MULTIVIEW_GEO_WORK_DOUBLES\s+\(([\d\s*+]+)\)", header).group(1))
    loss_header = open(os.path.join(ROOT, "include", "adgs_loss.h")).read()
    slots = int(re.search(r"#define\s+ADGS_LOSS_SLOTS\s+(\d+)", loss_header).group(1))
    assert size == multiview.MULTIVIEW_GEO_WORK_DOUBLES == slots * 2 + 4 and slots == multiview.SLOTS
    # the descriptor: the same fields in the same order, all four bytes wide
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*adgs_multiview_geo_desc\s*;", code, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            assert ctype in ("int", "float"), stmt
            fields += [n.strip().split("[")[0] for n in names.split(",")]
    assert fields == [f[0] for f in multiview.MultiviewGeoDesc._fields_]
    assert fields == ["struct_bytes", "H", "W", "Hn", "Wn", "inv_depth", "tanfovx", "tanfovy", "tanfovx_n", "tanfovy_n", "min_opacity",
                      "max_pixel_error", "pose"]
    assert ctypes.sizeof(multiview.MultiviewGeoDesc) == 4 * (len(fields) - 1 + 12) == 96


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib, multiview
    lib = _lib.lib()
    p = 0x1000
    inf, nan = float("inf"), float("nan")
    identity = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.1, 0, 0.3]

    def desc(H=8, W=16, Hn=6, Wn=12, inv=1, tx=0.5, ty=0.4, txn=0.6, tyn=0.3, mo=0.5, mpe=1.0, pose=identity, struct_bytes=None):
        d = multiview.make_geo_desc(H, W, Hn, Wn, inv, (tx, ty), (txn, tyn), mo, mpe, pose)
        if struct_bytes is not None:
            d.struct_bytes = struct_bytes
        return d

    def fwd(no_desc=False, depth=p, opacity=p, nd=p, no=p, weight=p, work=p, loss=p, err=p, gw=p, **kw):
        d = desc(**kw)
        return lib.adgs_multiview_geo_forward(None if no_desc else ctypes.byref(d), depth, opacity, nd, no, weight, work, loss, err, gw, None)

    def bwd(no_desc=False, depth=p, opacity=p, nd=p, no=p, weight=p, work=p, g_loss=p, gd=p, go=p, gnd=p, gno=p, **kw):
        d = desc(**kw)
        return lib.adgs_multiview_geo_backward(None if no_desc else ctypes.byref(d), depth, opacity, nd, no, weight, work, g_loss, gd, go, gnd, gno, None)

    shared = [dict(no_desc=True), dict(depth=None), dict(opacity=None), dict(nd=None), dict(no=None), dict(work=None),
              dict(struct_bytes=0), dict(struct_bytes=92), dict(struct_bytes=-1),
              dict(H=-1), dict(W=-1), dict(Hn=-1), dict(Wn=-2), dict(H=-8, W=-16), dict(H=65536, W=32768), dict(H=2 ** 31 - 1, W=2),
              dict(Hn=65536, Wn=32768), dict(Hn=3, Wn=2 ** 30)]
    shared += [{k: bad} for k in ("tx", "ty", "txn", "tyn") for bad in (0.0, -0.5, inf, -inf, nan)]
    shared += [dict(mo=bad) for bad in (0.0, -0.5, 1.5, inf, nan)]
    shared += [dict(mpe=bad) for bad in (0.0, -1.0, inf, -inf, nan)]
    shared += [dict(pose=identity[:i] + [bad] + identity[i + 1:]) for i in (0, 8, 11) for bad in (inf, nan)]
    calls = {"adgs_multiview_geo_forward": [(fwd, kw) for kw in shared + [dict(loss=None)]],
             "adgs_multiview_geo_backward": [(bwd, kw) for kw in shared + [dict(g_loss=None)]]}
    assert set(calls) == set(ENTRIES)
    for name, cases in calls.items():
        for f, kw in cases:
            assert f(**kw) < 0, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
    # an empty problem is not an error and launches nothing; neither a weight nor the per-pixel outputs are required
    for f in (fwd, bwd):
        assert f(H=0) == 0 and f(W=0) == 0 and f(Hn=0) == 0 and f(Wn=0) == 0 and f(H=0, W=0, Hn=0, Wn=0) == 0
        assert f(H=0, weight=None, inv=0, mo=1.0, mpe=50.0) == 0
    assert fwd(Hn=0, err=None, gw=None) == 0 and bwd(W=0, gd=None, go=None, gnd=None, gno=None) == 0
    # a backward that is asked for nothing has nothing to launch
    assert bwd(gd=None, go=None, gnd=None, gno=None) == 0 and bwd(gd=None, go=None, gnd=None, gno=None, weight=None) == 0


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import multiview

    class Cam:
        FoVx, FoVy = 1.2, 0.8

    d, o = torch.rand(8, 16), torch.rand(8, 16)
    dn, on = torch.rand(6, 12), torch.rand(6, 12)
    tan, tan_n = (0.5, 0.4), (0.6, 0.3)
    pose = torch.eye(4, dtype=torch.float64)[:3]
    for f in (multiview.geometric_consistency_loss, multiview.reprojection_errors):
        def call(D=d, O=o, cam=tan, Dn=dn, On=on, cam_n=tan_n, P=pose, **kw):
            return f(D, O, cam, Dn, On, cam_n, P, **kw)
        for bad in (torch.rand(3, 8, 16), torch.rand(128), torch.rand(1, 1, 8, 16)):
            with pytest.raises(ValueError, match="depth must be"):
                call(D=bad)
        for bad in (torch.rand(16, 8), torch.rand(3, 8, 16), torch.rand(8, 15), torch.rand(128), torch.rand(1, 1, 8, 16)):
            with pytest.raises(ValueError, match="img_opacity must be"):
                call(O=bad)
            with pytest.raises(ValueError, match="weight must be"):
                call(weight=bad)
        for bad in (torch.rand(3, 6, 12), torch.rand(72), torch.rand(1, 1, 6, 12)):
            with pytest.raises(ValueError, match="nbr_depth must be"):
                call(Dn=bad)
        for bad in (torch.rand(12, 6), torch.rand(8, 16), torch.rand(3, 6, 12), torch.rand(72), torch.rand(1, 1, 6, 12)):
            with pytest.raises(ValueError, match="nbr_opacity must be"):
                call(On=bad)
        for name, key, like in (("depth", "D", d), ("img_opacity", "O", o), ("nbr_depth", "Dn", dn), ("nbr_opacity", "On", on)):
            with pytest.raises(TypeError, match=name + " must be float32"):
                call(**{key: like.double()})
            with pytest.raises(TypeError, match=name + " must be a tensor"):
                call(**{key: like.numpy()})
        for name, key, like in (("img_opacity", "O", o), ("nbr_depth", "Dn", dn), ("nbr_opacity", "On", on)):
            with pytest.raises(RuntimeError, match=name + " is on"):
                call(**{key: torch.rand(*like.shape, device="meta")})
        with pytest.raises(TypeError, match="weight must be float32"):
            call(weight=torch.ones(8, 16, dtype=torch.bool))
        with pytest.raises(TypeError, match="weight must be a tensor"):
            call(weight=1.0)
        with pytest.raises(RuntimeError, match="weight is on"):
            call(weight=torch.ones(8, 16, device="meta"))
        for key in ("cam", "cam_n"):
            for bad in (None, 0.5, (0.5,), (0.5, 0.4, 0.3), "ab", object()):
                with pytest.raises(TypeError, match="FoVx / FoVy or a"):
                    call(**{key: bad})
            for bad in ((0.0, 0.4), (0.5, -0.4), (float("inf"), 0.4), (0.5, float("nan"))):
                with pytest.raises(ValueError, match="tanfovx and tanfovy must be"):
                    call(**{key: bad})
        for bad in (torch.eye(4), torch.rand(12), torch.rand(4, 3), torch.eye(4, dtype=torch.int64)[:3]):
            with pytest.raises(ValueError, match="pose must be"):
                call(P=bad)
        with pytest.raises(TypeError, match="pose must be a tensor"):
            call(P=pose.numpy())
        with pytest.raises(RuntimeError, match="pose must be a host tensor"):
            call(P=torch.rand(3, 4, device="meta"))
        nonfinite = pose.clone()
        nonfinite[1, 3] = float("nan")
        with pytest.raises(ValueError, match="pose must be finite"):
            call(P=nonfinite)
        for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="min_opacity must lie"):
                call(min_opacity=bad)
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="max_pixel_error must be"):
                call(max_pixel_error=bad)
        for kw in ({}, dict(D=d[None], O=o[None], Dn=dn[None], On=on[None], cam=Cam(), cam_n=Cam()), dict(weight=torch.ones(8, 16), inv_depth=False),
                   dict(weight=torch.ones(1, 8, 16), min_opacity=1.0, max_pixel_error=25.0), dict(P=pose.float()),
                   dict(D=torch.rand(0, 16), O=torch.rand(0, 16)), dict(Dn=torch.rand(6, 0), On=torch.rand(6, 0))):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**kw)
