"""What the depth smoothness term (include/adgs_loss.h, adgs.loss.depth_smoothness_loss) promises without a GPU: both entry points are declared,
exported by the cross-compiled library and bound; the work-size constant equals the header's; malformed calls are refused on the host,
with a message, before anything is launched; the Python surface refuses malformed arguments and CPU tensors.  The numerics are in
tests/test_gpu_depth_smooth.py."""
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
ENTRIES = {"adgs_depth_smooth_forward": 12, "adgs_depth_smooth_backward": 13}


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, loss
    header = open(os.path.join(ROOT, "include", "adgs_loss.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    for name, n in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert getattr(lib, name) is not None
    size = eval(re.search(r"#define\s+ADGS_SMOOTH_WORK_DOUBLES\s+\(([\d\s*+]+)\)", header).group(1))
    slots = int(re.search(r"#define\s+ADGS_LOSS_SLOTS\s+(\d+)", header).group(1))
    assert size == loss.SMOOTH_WORK_DOUBLES == slots * 8 + 8 and slots == loss.SLOTS


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib
    lib = _lib.lib()
    p = 0x1000
    inf, nan = float("inf"), float("nan")
    # (H, W, C, depth, guide, weight, order, normalize, gamma), then work, loss | work, g_loss, dL_ddepth
    fwd = lambda H=8, W=16, C=3, depth=p, guide=p, weight=p, order=1, normalize=1, gamma=1.0, work=p, loss=p: \
        lib.adgs_depth_smooth_forward(H, W, C, depth, guide, weight, order, normalize, gamma, work, loss, None)
    bwd = lambda H=8, W=16, C=3, depth=p, guide=p, weight=p, order=1, normalize=1, gamma=1.0, work=p, g_loss=p, out=p: \
        lib.adgs_depth_smooth_backward(H, W, C, depth, guide, weight, order, normalize, gamma, work, g_loss, out, None)
    shared = [dict(depth=None), dict(work=None), dict(H=-1), dict(W=-1), dict(H=-8, W=-16), dict(H=65536, W=32768), dict(H=2 ** 31 - 1, W=2),
              dict(order=0), dict(order=3), dict(order=-1), dict(C=-1), dict(C=9), dict(C=0), dict(C=0, guide=p, weight=None), dict(C=1, guide=None),
              dict(C=8, guide=None), dict(gamma=-0.5), dict(gamma=inf), dict(gamma=-inf), dict(gamma=nan)]
    calls = {"adgs_depth_smooth_forward": [(fwd, kw) for kw in shared + [dict(loss=None)]],
             "adgs_depth_smooth_backward": [(bwd, kw) for kw in shared + [dict(g_loss=None), dict(out=None)]]}
    assert set(calls) == set(ENTRIES)
    for name, cases in calls.items():
        for f, kw in cases:
            assert f(**kw) < 0, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
    # an empty problem is not an error and launches nothing; neither a weight nor a guide is required
    for f in (fwd, bwd):
        assert f(H=0) == 0 and f(W=0) == 0 and f(H=0, W=0) == 0
        assert f(H=0, C=0, guide=None, weight=None) == 0
        assert f(H=0, order=2, normalize=0, gamma=0.0) == 0


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import loss
    f = loss.depth_smoothness_loss
    d, img = torch.rand(8, 16), torch.rand(3, 8, 16)
    for bad in (torch.rand(3, 8, 16), torch.rand(128), torch.rand(1, 1, 8, 16), torch.rand(2, 8, 16)):
        with pytest.raises(ValueError, match="depth must be"):
            f(bad)
    for bad in (d.double(), d.half(), d > 0.5):
        with pytest.raises(TypeError, match="depth must be float32"):
            f(bad)
    with pytest.raises(TypeError, match="depth must be a tensor"):
        f(d.numpy())
    for bad in (torch.rand(8, 16), torch.rand(3, 16, 8), torch.rand(3, 8, 15), torch.rand(9, 8, 16), torch.rand(0, 8, 16), torch.rand(1, 3, 8, 16)):
        with pytest.raises(ValueError, match="image must be"):
            f(d, bad)
    for bad in (img.double(), img.half(), (img * 255).to(torch.uint8)):
        with pytest.raises(TypeError, match="image must be float32"):
            f(d, bad)
    with pytest.raises(TypeError, match="image must be a tensor"):
        f(d, img.numpy())
    with pytest.raises(RuntimeError, match="image is on"):
        f(d, torch.rand(3, 8, 16, device="meta"))
    for bad in (torch.ones(16, 8), torch.ones(3, 8, 16), torch.ones(8, 15), torch.ones(128)):
        with pytest.raises(ValueError, match="weight must be"):
            f(d, img, bad)
    for bad in (torch.ones(8, 16, dtype=torch.float64), torch.ones(8, 16, dtype=torch.bool), torch.ones(8, 16, dtype=torch.float16)):
        with pytest.raises(TypeError, match="weight must be float32"):
            f(d, img, bad)
    with pytest.raises(TypeError, match="weight must be a tensor"):
        f(d, img, 1.0)
    with pytest.raises(RuntimeError, match="weight is on"):
        f(d, img, torch.ones(8, 16, device="meta"))
    for bad in (0, 3, -1, 1.5, None):
        with pytest.raises(ValueError, match="order must be 1 or 2"):
            f(d, img, order=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="edge_gamma must be"):
            f(d, img, edge_gamma=bad)
    # well-formed arguments: the CPU tensors themselves are refused
    for args, kw in (((d,), {}), ((d[None],), {}), ((d, img), {}), ((d, img, torch.ones(8, 16)), dict(order=2)), ((d, None, torch.ones(1, 8, 16)), dict(normalize=False)),
                     ((d, img[:1]), dict(edge_gamma=0.0)), ((torch.rand(0, 16),), {})):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(*args, **kw)
