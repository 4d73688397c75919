"""What the normal-map prior (include/adgs_normals.h, adgs.normals) promises without a GPU: the five entry points are declared, exported by
the cross-compiled library and bound; the work-size constant equals the header's; malformed calls are refused on the host, with a message,
before anything is launched; the Python surface refuses malformed arguments and CPU tensors.  The numerics are in tests/test_gpu_normals.py."""
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
ENTRIES = {"adgs_gaussian_normals_forward": 10, "adgs_gaussian_normals_backward": 10, "adgs_normal_consistency_forward": 13,
           "adgs_normal_consistency_backward": 16, "adgs_depth_to_normal": 10}


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, normals
    header = open(os.path.join(ROOT, "include", "adgs_normals.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    for name, n in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert getattr(lib, name) is not None
    size = eval(re.search(r"#define\s+ADGS_NORMAL_WORK_DOUBLES\s+\(([\d\s*+]+)\)", header).group(1))
    loss_header = open(os.path.join(ROOT, "include", "adgs_loss.h")).read()
    slots = int(re.search(r"#define\s+ADGS_LOSS_SLOTS\s+(\d+)", loss_header).group(1))
    assert size == normals.NORMAL_WORK_DOUBLES == slots * 2 + 4 and slots == normals.SLOTS


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib
    lib = _lib.lib()
    p = 0x1000
    inf, nan = float("inf"), float("nan")
    gfwd = lambda N=8, scales=p, rot=p, means=p, view=p, mask=None, stride=3, c0=0, out=p: \
        lib.adgs_gaussian_normals_forward(N, scales, rot, means, view, mask, stride, c0, out, None)
    gbwd = lambda N=8, scales=p, rot=p, means=p, view=p, g=p, stride=3, c0=0, out=p: \
        lib.adgs_gaussian_normals_backward(N, scales, rot, means, view, g, stride, c0, out, None)
    gshared = [dict(scales=None), dict(rot=None), dict(means=None), dict(view=None), dict(out=None), dict(N=-1), dict(stride=2), dict(stride=0),
               dict(stride=-3), dict(c0=-1), dict(stride=3, c0=1), dict(stride=4, c0=2), dict(stride=32, c0=30), dict(stride=33), dict(stride=33, c0=30)]
    cfwd = lambda H=8, W=16, normal=p, depth=p, opacity=p, weight=p, tx=0.5, ty=0.4, inv=1, mo=0.5, work=p, loss=p: \
        lib.adgs_normal_consistency_forward(H, W, normal, depth, opacity, weight, tx, ty, inv, mo, work, loss, None)
    cbwd = lambda H=8, W=16, normal=p, depth=p, opacity=p, weight=p, tx=0.5, ty=0.4, inv=1, mo=0.5, work=p, g_loss=p, gn=p, gd=p, go=p: \
        lib.adgs_normal_consistency_backward(H, W, normal, depth, opacity, weight, tx, ty, inv, mo, work, g_loss, gn, gd, go, None)
    d2n = lambda H=8, W=16, depth=p, opacity=p, tx=0.5, ty=0.4, inv=1, mo=0.5, out=p: \
        lib.adgs_depth_to_normal(H, W, depth, opacity, tx, ty, inv, mo, out, None)
    view = [dict(depth=None), dict(opacity=None), dict(H=-1), dict(W=-1), dict(H=-8, W=-16), dict(H=65536, W=32768), dict(H=2 ** 31 - 1, W=2),
            dict(tx=0.0), dict(tx=-0.5), dict(tx=inf), dict(tx=nan), dict(ty=0.0), dict(ty=-0.4), dict(ty=inf), dict(ty=-inf), dict(ty=nan),
            dict(mo=0.0), dict(mo=-0.5), dict(mo=1.5), dict(mo=inf), dict(mo=nan)]
    calls = {"adgs_gaussian_normals_forward": [(gfwd, kw) for kw in gshared + [dict(mask=p, c0=0), dict(mask=p, stride=8, c0=0)]],
             "adgs_gaussian_normals_backward": [(gbwd, kw) for kw in gshared + [dict(g=None)]],
             "adgs_normal_consistency_forward": [(cfwd, kw) for kw in view + [dict(normal=None), dict(work=None), dict(loss=None)]],
             "adgs_normal_consistency_backward": [(cbwd, kw) for kw in view + [dict(normal=None), dict(work=None), dict(g_loss=None)]],
             "adgs_depth_to_normal": [(d2n, kw) for kw in view + [dict(out=None)]]}
    assert set(calls) == set(ENTRIES)
    for name, cases in calls.items():
        for f, kw in cases:
            assert f(**kw) < 0, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
    # an empty problem is not an error and launches nothing; neither a mask nor a weight is required
    for f in (gfwd, gbwd):
        assert f(N=0) == 0 and f(N=0, stride=32, c0=29) == 0
    assert gfwd(N=0, mask=p, stride=4, c0=1) == 0
    for f in (cfwd, cbwd, d2n):
        assert f(H=0) == 0 and f(W=0) == 0 and f(H=0, W=0) == 0 and f(H=0, inv=0, mo=1.0) == 0
    assert cfwd(H=0, weight=None) == 0 and cbwd(W=0, weight=None, gn=None, gd=None, go=None) == 0
    # a backward that is asked for nothing has nothing to launch
    assert cbwd(gn=None, gd=None, go=None) == 0


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import normals
    f = normals.gaussian_normals
    s, q, x, v = torch.rand(8, 3), torch.rand(8, 4), torch.rand(8, 3), torch.eye(4)
    for bad in (torch.rand(8, 3), torch.rand(8), torch.rand(4, 8), torch.rand(2, 8, 4)):
        with pytest.raises(ValueError, match="rotations must be"):
            f(s, bad, x, v)
    with pytest.raises(TypeError, match="rotations must be float32"):
        f(s, q.double(), x, v)
    with pytest.raises(TypeError, match="rotations must be a tensor"):
        f(s, q.numpy(), x, v)
    for bad in (torch.rand(7, 3), torch.rand(8, 4), torch.rand(8)):
        with pytest.raises(ValueError, match="scales must be"):
            f(bad, q, x, v)
        with pytest.raises(ValueError, match="means3D must be"):
            f(s, q, bad, v)
    with pytest.raises(TypeError, match="scales must be float32"):
        f(s.half(), q, x, v)
    with pytest.raises(TypeError, match="means3D must be a tensor"):
        f(s, q, None, v)
    with pytest.raises(RuntimeError, match="means3D is on"):
        f(s, q, torch.rand(8, 3, device="meta"), v)
    for bad in (torch.eye(3), torch.rand(16), torch.rand(1, 4, 4)):
        with pytest.raises(ValueError, match="viewmatrix must be"):
            f(s, q, x, bad)
    with pytest.raises(TypeError, match="viewmatrix must be float32"):
        f(s, q, x, v.double())
    with pytest.raises(TypeError, match="viewmatrix must be a tensor"):
        f(s, q, x, v.numpy())
    for bad in (torch.rand(7), torch.rand(8, 2), torch.rand(1, 8)):
        with pytest.raises(ValueError, match="mask must be"):
            f(s, q, x, v, mask=bad)
    with pytest.raises(TypeError, match="mask must be float32"):
        f(s, q, x, v, mask=torch.ones(8, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask must be a tensor"):
        f(s, q, x, v, mask=1.0)
    for args, kw in (((s, q, x, v), {}), ((s, q, x, v), dict(mask=torch.ones(8))), ((s, q, x, v), dict(mask=torch.ones(8, 1))),
                     ((s[:0], q[:0], x[:0], v), {})):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(*args, **kw)

    class Cam:
        FoVx, FoVy = 1.2, 0.8

    f = normals.normal_consistency_loss
    n, d, o = torch.rand(3, 8, 16), torch.rand(8, 16), torch.rand(8, 16)
    tan = (0.5, 0.4)
    for bad in (torch.rand(8, 16), torch.rand(1, 8, 16), torch.rand(4, 8, 16), torch.rand(1, 3, 8, 16)):
        with pytest.raises(ValueError, match="img_normal must be"):
            f(bad, d, o, tan)
    with pytest.raises(TypeError, match="img_normal must be float32"):
        f(n.double(), d, o, tan)
    with pytest.raises(TypeError, match="img_normal must be a tensor"):
        f(n.numpy(), d, o, tan)
    for bad in (torch.rand(16, 8), torch.rand(3, 8, 16), torch.rand(8, 15), torch.rand(128), torch.rand(1, 1, 8, 16)):
        with pytest.raises(ValueError, match="depth must be"):
            f(n, bad, o, tan)
        with pytest.raises(ValueError, match="img_opacity must be"):
            f(n, d, bad, tan)
        with pytest.raises(ValueError, match="weight must be"):
            f(n, d, o, tan, weight=bad)
    for name, args in (("depth", lambda b: (n, b, o, tan)), ("img_opacity", lambda b: (n, d, b, tan))):
        with pytest.raises(TypeError, match=name + " must be float32"):
            f(*args(d.double()))
        with pytest.raises(TypeError, match=name + " must be a tensor"):
            f(*args(d.numpy()))
        with pytest.raises(RuntimeError, match=name + " is on"):
            f(*args(torch.rand(8, 16, device="meta")))
    with pytest.raises(TypeError, match="weight must be float32"):
        f(n, d, o, tan, weight=torch.ones(8, 16, dtype=torch.bool))
    with pytest.raises(TypeError, match="weight must be a tensor"):
        f(n, d, o, tan, weight=1.0)
    with pytest.raises(RuntimeError, match="weight is on"):
        f(n, d, o, tan, weight=torch.ones(8, 16, device="meta"))
    for bad in (None, 0.5, (0.5,), (0.5, 0.4, 0.3), "ab", object()):
        with pytest.raises(TypeError, match="FoVx / FoVy or a"):
            f(n, d, o, bad)
    for bad in ((0.0, 0.4), (0.5, -0.4), (float("inf"), 0.4), (0.5, float("nan"))):
        with pytest.raises(ValueError, match="tanfovx and tanfovy must be"):
            f(n, d, o, bad)
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_opacity must lie"):
            f(n, d, o, tan, min_opacity=bad)
    for args, kw in (((n, d, o, tan), {}), ((n, d[None], o[None], Cam()), {}), ((n, d, o[None], tan), dict(weight=torch.ones(8, 16), inv_depth=False)),
                     ((n, d, o, tan), dict(weight=torch.ones(1, 8, 16), min_opacity=1.0)), ((torch.rand(3, 0, 16), torch.rand(0, 16), torch.rand(0, 16), tan), {})):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(*args, **kw)

    f = normals.depth_to_normal
    for bad in (torch.rand(3, 8, 16), torch.rand(128), torch.rand(1, 1, 8, 16)):
        with pytest.raises(ValueError, match="depth must be"):
            f(bad, o, *tan)
    for bad in (torch.rand(16, 8), torch.rand(8, 15), torch.rand(3, 8, 16)):
        with pytest.raises(ValueError, match="img_opacity must be"):
            f(d, bad, *tan)
    with pytest.raises(TypeError, match="depth must be float32"):
        f(d.double(), o, *tan)
    with pytest.raises(TypeError, match="img_opacity must be a tensor"):
        f(d, o.numpy(), *tan)
    with pytest.raises(RuntimeError, match="img_opacity is on"):
        f(d, torch.rand(8, 16, device="meta"), *tan)
    with pytest.raises(ValueError, match="tanfovx and tanfovy must be"):
        f(d, o, 0.0, 0.4)
    with pytest.raises(ValueError, match="min_opacity must lie"):
        f(d, o, *tan, min_opacity=0.0)
    for args, kw in (((d, o) + tan, {}), ((d[None], o) + tan, dict(inv_depth=False)), ((torch.rand(0, 16), torch.rand(0, 16)) + tan, {})):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(*args, **kw)
