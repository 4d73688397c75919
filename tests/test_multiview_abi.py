"""What the multi-view photometric consistency loss (include/adgs_multiview.h, adgs.multiview) promises without a GPU: the two entry
points are declared, exported by the cross-compiled library and bound; the work-size constant and the descriptor equal the header's;
malformed calls are refused on the host, with a message, before anything is launched; empty problems return 0; the Python surface refuses
malformed arguments and CPU tensors.  The numerics are in tests/test_gpu_multiview.py."""
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
ENTRIES = {"adgs_multiview_ncc_forward": 14, "adgs_multiview_ncc_backward": 15}


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, multiview
    header = open(os.path.join(ROOT, "include", "adgs_multiview.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    for name, n in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert getattr(lib, name) is not None
    size = eval(re.search(r"#define\s+ADGS_MULTIVIEW_WORK_DOUBLES\s+\(([\d\s*+]+)\)", header).group(1))
    loss_header = open(os.path.join(ROOT, "include", "adgs_loss.h")).read()
    slots = int(re.search(r"#define\s+ADGS_LOSS_SLOTS\s+(\d+)", loss_header).group(1))
    assert size == multiview.MULTIVIEW_WORK_DOUBLES == slots * 2 + 4 and slots == multiview.SLOTS
    assert int(re.search(r"#define\s+ADGS_MULTIVIEW_MAX_RADIUS\s+(\d+)", header).group(1)) == multiview.MAX_RADIUS == 3
    # the descriptor: the same fields in the same order, all four bytes wide
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*adgs_multiview_desc\s*;", code, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            assert ctype in ("int", "float"), stmt
            fields += [n.strip().split("[")[0] for n in names.split(",")]
    assert fields == [f[0] for f in multiview.MultiviewDesc._fields_]
    assert ctypes.sizeof(multiview.MultiviewDesc) == 4 * (len(fields) - 1 + 12) == 108


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib, multiview
    lib = _lib.lib()
    p = 0x1000
    inf, nan = float("inf"), float("nan")
    identity = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.1, 0, 0.3]

    def desc(H=8, W=16, Hn=6, Wn=12, radius=3, inv=1, tx=0.5, ty=0.4, txn=0.6, tyn=0.3, mo=0.5, mc=0.1, me=0.9, eps=1e-8, pose=identity,
             struct_bytes=None):
        d = multiview.make_desc(H, W, Hn, Wn, radius, inv, (tx, ty), (txn, tyn), mo, mc, me, eps, pose)
        if struct_bytes is not None:
            d.struct_bytes = struct_bytes
        return d

    def fwd(no_desc=False, normal=p, depth=p, opacity=p, ref=p, nbr=p, weight=p, samples=p, S=5, work=p, loss=p, e=p, valid=p, **kw):
        d = desc(**kw)
        return lib.adgs_multiview_ncc_forward(None if no_desc else ctypes.byref(d), normal, depth, opacity, ref, nbr, weight, samples, S, work, loss, e, valid, None)

    def bwd(no_desc=False, normal=p, depth=p, opacity=p, ref=p, nbr=p, weight=p, samples=p, S=5, work=p, g_loss=p, gn=p, gd=p, go=p, **kw):
        d = desc(**kw)
        return lib.adgs_multiview_ncc_backward(None if no_desc else ctypes.byref(d), normal, depth, opacity, ref, nbr, weight, samples, S, work, g_loss, gn, gd, go, None)

    shared = [dict(no_desc=True), dict(normal=None), dict(depth=None), dict(opacity=None), dict(ref=None), dict(nbr=None), dict(samples=None), dict(work=None),
              dict(struct_bytes=0), dict(struct_bytes=104), dict(struct_bytes=-1),
              dict(H=-1), dict(W=-1), dict(Hn=-1), dict(Wn=-2), dict(H=-8, W=-16), dict(H=65536, W=32768), dict(H=2 ** 31 - 1, W=2),
              dict(Hn=65536, Wn=32768), dict(Hn=3, Wn=2 ** 30), dict(S=-1), dict(S=-2 ** 31),
              dict(radius=0), dict(radius=4), dict(radius=-1), dict(radius=49)]
    shared += [{k: bad} for k in ("tx", "ty", "txn", "tyn") for bad in (0.0, -0.5, inf, -inf, nan)]
    shared += [{k: bad} for k in ("mo", "mc", "me") for bad in (0.0, -0.5, 1.5, inf, nan)]
    shared += [dict(eps=bad) for bad in (0.0, -1e-8, inf, nan)]
    shared += [dict(pose=identity[:i] + [bad] + identity[i + 1:]) for i in (0, 8, 11) for bad in (inf, nan)]
    calls = {"adgs_multiview_ncc_forward": [(fwd, kw) for kw in shared + [dict(loss=None)]],
             "adgs_multiview_ncc_backward": [(bwd, kw) for kw in shared + [dict(g_loss=None)]]}
    assert set(calls) == set(ENTRIES)
    for name, cases in calls.items():
        for f, kw in cases:
            assert f(**kw) < 0, (name, kw)
            assert _lib.last_error().startswith(name + ": "), (name, kw, _lib.last_error())
    # an empty problem is not an error and launches nothing; neither a weight nor the per-sample outputs are required
    for f in (fwd, bwd):
        assert f(S=0) == 0 and f(H=0) == 0 and f(W=0) == 0 and f(Hn=0) == 0 and f(Wn=0) == 0 and f(H=0, W=0, Hn=0, Wn=0, S=0) == 0
        assert f(S=0, weight=None, radius=1, inv=0, mo=1.0, mc=1.0, me=1.0) == 0
    assert fwd(S=0, e=None, valid=None) == 0 and bwd(S=0, gn=None, gd=None, go=None) == 0
    # a backward that is asked for nothing has nothing to launch
    assert bwd(gn=None, gd=None, go=None) == 0 and bwd(gn=None, gd=None, go=None, weight=None) == 0


def test_python_surface_refuses_malformed_arguments_and_cpu_tensors():
    from adgs import multiview

    class Cam:
        FoVx, FoVy = 1.2, 0.8

    n, d, o = torch.rand(3, 8, 16), torch.rand(8, 16), torch.rand(8, 16)
    ir, inb = torch.rand(8, 16), torch.rand(6, 12)
    tan, tan_n = (0.5, 0.4), (0.6, 0.3)
    pose = torch.eye(4, dtype=torch.float64)[:3]
    s = torch.tensor([40, 41, 57], dtype=torch.int32)
    for f in (multiview.photometric_consistency_loss, multiview.patch_errors):
        def call(N=n, D=d, O=o, cam=tan, ref=ir, nbr=inb, cam_n=tan_n, P=pose, idx=s, **kw):
            return f(N, D, O, cam, ref, nbr, cam_n, P, idx, **kw)
        for bad in (torch.rand(8, 16), torch.rand(1, 8, 16), torch.rand(4, 8, 16), torch.rand(1, 3, 8, 16)):
            with pytest.raises(ValueError, match="img_normal must be"):
                call(N=bad)
        with pytest.raises(TypeError, match="img_normal must be float32"):
            call(N=n.double())
        with pytest.raises(TypeError, match="img_normal must be a tensor"):
            call(N=n.numpy())
        for bad in (torch.rand(16, 8), torch.rand(3, 8, 16), torch.rand(8, 15), torch.rand(128), torch.rand(1, 1, 8, 16)):
            with pytest.raises(ValueError, match="depth must be"):
                call(D=bad)
            with pytest.raises(ValueError, match="img_opacity must be"):
                call(O=bad)
            with pytest.raises(ValueError, match="ref_gray must be"):
                call(ref=bad)
            with pytest.raises(ValueError, match="weight must be"):
                call(weight=bad)
        for bad in (torch.rand(3, 6, 12), torch.rand(72), torch.rand(1, 1, 6, 12)):
            with pytest.raises(ValueError, match="nbr_gray must be"):
                call(nbr=bad)
        for name, key in (("depth", "D"), ("img_opacity", "O"), ("ref_gray", "ref"), ("nbr_gray", "nbr")):
            with pytest.raises(TypeError, match=name + " must be float32"):
                call(**{key: d.double()})
            with pytest.raises(TypeError, match=name + " must be a tensor"):
                call(**{key: d.numpy()})
            with pytest.raises(RuntimeError, match=name + " is on"):
                call(**{key: torch.rand(8, 16, device="meta")})
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
        for bad in (s.float(), s.long(), s.double(), s.bool()):
            with pytest.raises(TypeError, match="samples must be int32"):
                call(idx=bad)
        for bad in (s[None], s.reshape(3, 1), torch.tensor(3, dtype=torch.int32)):
            with pytest.raises(ValueError, match="samples must be"):
                call(idx=bad)
        with pytest.raises(TypeError, match="samples must be a tensor"):
            call(idx=[40, 41])
        with pytest.raises(RuntimeError, match="samples is on"):
            call(idx=torch.zeros(3, dtype=torch.int32, device="meta"))
        for bad in (0, 4, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="radius must be 1, 2 or 3"):
                call(radius=bad)
        for key in ("min_opacity", "min_cos", "max_error"):
            for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
                with pytest.raises(ValueError, match=key + " must lie"):
                    call(**{key: bad})
        for kw in ({}, dict(D=d[None], O=o[None], cam=Cam(), cam_n=Cam()), dict(weight=torch.ones(8, 16), inv_depth=False, radius=1),
                   dict(weight=torch.ones(1, 8, 16), min_opacity=1.0, radius=2), dict(idx=s[:0]), dict(P=pose.float()),
                   dict(N=torch.rand(3, 0, 16), D=torch.rand(0, 16), O=torch.rand(0, 16), ref=torch.rand(0, 16))):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**kw)


def test_host_helpers():
    """gray, relative_pose and sample_pixels are torch code: they run anywhere."""
    from adgs import multiview
    img = torch.rand(3, 5, 7)
    assert torch.allclose(multiview.gray(img), 0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2])
    with pytest.raises(ValueError, match="gray"):
        multiview.gray(torch.rand(5, 7))

    class Cam:
        pass

    def camera(Rt):
        c = Cam()
        c.world_view_transform = Rt.T.contiguous().float()        # the transposed matrix the rasterizer receives
        return c

    def rigid(seed):
        g = torch.Generator().manual_seed(seed)
        A = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
        if torch.linalg.det(A) < 0:
            A[:, 0] = -A[:, 0]
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = A, torch.randn(3, generator=g, dtype=torch.float64)
        return M

    A_r, A_n = rigid(1), rigid(2)
    rel = multiview.relative_pose(camera(A_r), camera(A_n))
    assert rel.dtype == torch.float64 and tuple(rel.shape) == (3, 4) and rel.device.type == "cpu"
    Xw = torch.randn(10, 3, dtype=torch.float64)
    Xr, Xn = Xw @ A_r[:3, :3].T + A_r[:3, 3], Xw @ A_n[:3, :3].T + A_n[:3, 3]
    assert float((Xr @ rel[:, :3].T + rel[:, 3] - Xn).abs().max()) < 1e-5      # the matrices were float32
    assert float((multiview.relative_pose(camera(A_r), camera(A_r)) - torch.eye(4, dtype=torch.float64)[:3]).abs().max()) < 1e-6
    with pytest.raises(ValueError, match="relative_pose"):
        multiview.relative_pose(torch.eye(3), camera(A_n))

    mask = torch.zeros(12, 20)
    mask[:, 5:] = 1.0
    for radius, n in ((0, 1000), (3, 1000), (2, 17), (3, 0)):
        idx = multiview.sample_pixels(mask, n, radius, generator=torch.Generator().manual_seed(3))
        y, x = idx.long() // 20, idx.long() % 20
        candidates = (12 - 2 * radius) * (20 - max(5, radius) - radius)
        assert idx.dtype == torch.int32 and idx.numel() == min(n, candidates) and torch.unique(idx).numel() == idx.numel()
        assert bool(((x >= max(5, radius)) & (x < 20 - radius) & (y >= radius) & (y < 12 - radius)).all())
    assert multiview.sample_pixels(mask[None], 5, 6).numel() == 0                # no pixel is six from the border of a 12-row mask
    with pytest.raises(ValueError, match="sample_pixels"):
        multiview.sample_pixels(torch.zeros(3, 4, 5), 3, 1)
