"""The fused evaluation pass on the GPU (adgs.metrics over include/adgs_metrics.h) against the float64 reference of tests/metrics_ref.py.

Shapes (C, H, W); the kernel's tiles are 32 x 16: (3,1,1) a single pixel; (3,5,70) an image lower than the window's halo; (3,16,32)
exactly one tile; (3,17,33) one pixel over in both directions: four tiles, three of them partial; (3,37,53) an interior case with
partial tiles (3 W = 159 is no multiple of 4: the 8-bit rows start at every alignment); (1,40,24) one channel; (3,48,200) several
interior tiles, 3 W a multiple of 4.  The inputs are those of tests/golden/metrics_golden.npz: unclipped, one element in eight
outside [0, 1].

Tolerances against the float64 reference: l1 1e-6 and ssim 1e-5 are the project's own (tests/test_gpu_loss.py); psnr and
psnr_channel_mean 1e-5 dB: the kernel forms x - y and its square in float32 (relative error at most 3 * 2^-24 = 1.8e-7, i.e. 8e-7 dB)
and sums in double; mse the same bound as a relative error, 1e-5 ln(10) / 10 = 2.3e-6.  The 8-bit images are compared bit for bit."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import metrics_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 1), (3, 5, 70), (3, 16, 32), (3, 17, 33), (3, 37, 53), (1, 40, 24), (3, 48, 200)]
WRAP = (3, 17, 4097)                      # 129 x 2 = 258 tiles, the fewest over the 256 slot rows with partial tiles on both axes; not in the golden file
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "metrics_golden.npz"))
L1_TOL, SSIM_TOL, PSNR_TOL = 1e-6, 1e-5, 1e-5
MSE_REL = PSNR_TOL * math.log(10.0) / 10.0
TSX, TSY = 32, 16


def name_of(shape):
    return "%dx%dx%d" % shape


@functools.lru_cache(maxsize=None)
def inputs(shape):
    n = name_of(shape)
    if shape == WRAP:                     # the golden file's recipe (tests/golden/make_metrics_golden.py)
        g = torch.Generator().manual_seed(sum(shape))
        gt = torch.rand(*shape, generator=g)
        return gt + 0.15 * torch.randn(*shape, generator=g), gt
    return torch.from_numpy(GOLDEN[n + "/img"]), torch.from_numpy(GOLDEN[n + "/gt"])


@functools.lru_cache(maxsize=None)
def masks_of(shape, regions):
    """1: a soft mask; 4: all zero, all ones, soft, non-zero only in the last (bottom right) tile"""
    _, H, W = shape
    soft = torch.rand(H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    if regions == 1:
        return soft[None].contiguous()
    last = torch.zeros(H, W)
    last[(H - 1) // TSY * TSY:, (W - 1) // TSX * TSX:] = 0.25 + 0.75 * soft[(H - 1) // TSY * TSY:, (W - 1) // TSX * TSX:]
    return torch.stack([torch.zeros(H, W), torch.ones(H, W), soft, last])


@functools.lru_cache(maxsize=None)
def reference(shape, regions, quantized=False):
    """computed once per case, shared, never modified"""
    img, gt = inputs(shape)
    return ref.metrics(img, gt, masks_of(shape, regions) if regions else None, quantized=quantized)


def evaluate(img, gt, masks=None, quantize=False, u8=None):
    from adgs import metrics
    ev = metrics.Evaluator(1, regions=0 if masks is None else masks.shape[0], quantize=quantize)
    index, out = ev.add(img.cuda(), gt.cuda(), None if masks is None else masks.cuda(), u8=u8)
    assert index == 0
    return ev.results(), (None if out is None else out.cpu()), ev


def check_region(tag, got, want, view=0):
    if want["weight"] == 0:
        assert got["weight"][view] == 0 and all(math.isnan(got[k][view]) for k in ("l1", "mse", "psnr", "psnr_channel_mean", "ssim")), tag
        return
    figs = {k: abs(got[k][view] - want[k]) for k in ("l1", "ssim", "psnr", "psnr_channel_mean")}
    figs["mse_rel"] = abs(got["mse"][view] / want["mse"] - 1.0)
    print("%s: |l1| %.2e (%.0e)  |ssim| %.2e (%.0e)  |psnr| %.2e  |psnr_channel_mean| %.2e (%.0e dB)  mse rel %.2e (%.1e)" % (
        tag, figs["l1"], L1_TOL, figs["ssim"], SSIM_TOL, figs["psnr"], figs["psnr_channel_mean"], PSNR_TOL, figs["mse_rel"], MSE_REL))
    assert abs(got["weight"][view] - want["weight"]) <= 1e-9 * want["weight"], tag
    assert figs["l1"] <= L1_TOL and figs["ssim"] <= SSIM_TOL, tag
    assert figs["psnr"] <= PSNR_TOL and figs["psnr_channel_mean"] <= PSNR_TOL and figs["mse_rel"] <= MSE_REL, tag


@pytest.mark.parametrize("regions", [0, 1, 4])
@pytest.mark.parametrize("shape", SHAPES + [WRAP])
def test_metrics_against_the_reference(shape, regions):
    img, gt = inputs(shape)
    res, _, ev = evaluate(img, gt, masks_of(shape, regions) if regions else None)
    want = reference(shape, regions)
    assert len(res) == 1 + regions == len(want)
    for r in range(1 + regions):
        check_region("%s region %d of %d" % (shape, r, regions), res[r], want[r])
        assert res[r]["count"] == (1 if want[r]["weight"] > 0 else 0)
        for k in ("l1", "mse", "psnr", "psnr_channel_mean", "ssim"):
            if want[r]["weight"] > 0:
                assert res[r]["mean"][k] == res[r][k][0] and res[r][k].dtype == np.float64
            else:
                assert math.isnan(res[r]["mean"][k])
    if regions == 4:
        # the all-ones mask is region 0's row (the sums differ in the order of their atomic additions only)
        for k in ("l1", "mse", "psnr", "psnr_channel_mean", "ssim", "weight"):
            assert abs(res[2][k][0] - res[0][k][0]) <= 1e-12 * abs(res[0][k][0])
        assert want[4]["weight"] > 0
    assert not ev.work.any()                                   # the finishing kernel leaves the work buffer zero


def test_the_golden_values_of_the_reference_itself():
    """the reference's own float32 results (tests/golden/make_metrics_golden.py), with the CPU test's caps as tolerances"""
    for shape in SHAPES:
        res, _, _ = evaluate(*inputs(shape))
        n = name_of(shape)
        for k, tol in (("psnr", 1e-4), ("psnr_channel_mean", 1e-4), ("ssim", SSIM_TOL), ("l1", L1_TOL)):
            assert abs(res[0][k][0] - float(GOLDEN[n + "/" + k])) <= tol, (shape, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_quantized_metrics(shape):
    img, gt = inputs(shape)
    m = masks_of(shape, 1)
    res, _, _ = evaluate(img, gt, m, quantize=True)
    want = reference(shape, 1, True)
    for r in range(2):
        check_region("%s quantized region %d" % (shape, r), res[r], want[r])
    if shape == (3, 48, 200):
        assert abs(want[0]["psnr"] - reference(shape, 1)[0]["psnr"]) > 10 * PSNR_TOL      # the quantisation is visible at this tolerance (2.9e-4 dB)


@pytest.mark.parametrize("shape", SHAPES)
def test_identical_images(shape):
    _, gt = inputs(shape)
    res, _, _ = evaluate(gt, gt, masks_of(shape, 1))
    for r in range(2):
        assert res[r]["l1"][0] == 0.0 and res[r]["mse"][0] == 0.0
        assert res[r]["psnr"][0] == math.inf and res[r]["psnr_channel_mean"][0] == math.inf and res[r]["mean"]["psnr"] == math.inf
        assert abs(res[r]["ssim"][0] - 1.0) <= 1e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_is_that_of_the_training_loss(shape):
    from adgs import loss
    img, gt = inputs(shape)
    res, _, _ = evaluate(img, gt)
    with torch.no_grad():
        want = loss.ssim(img.cuda().clamp(0, 1), gt.cuda().clamp(0, 1)).item()
    assert abs(res[0]["ssim"][0] - want) <= 1e-6


@pytest.mark.parametrize("mode", ["round", "truncate"])
def test_eight_bit_images_bit_for_bit(mode):
    from adgs import metrics
    cases = [inputs(s)[0] for s in SHAPES] + [ref.planted_image()[0], ref.planted_image()[0][:1].contiguous()]
    for img in cases:
        want = ref.to_u8(img, mode)
        for quantize in (False, True):                         # the bytes are those of the unquantised image either way
            _, got, _ = evaluate(img, img.flip(2).contiguous(), quantize=quantize, u8=mode)
            assert got.dtype == torch.uint8 and got.shape == want.shape == (img.shape[1], img.shape[2], img.shape[0])
            assert torch.equal(got, want), (tuple(img.shape), mode, quantize, int((got != want).sum()))
        assert torch.equal(metrics.to8b(img.cuda(), mode).cpu(), want)
    img, n = ref.planted_image()
    got = metrics.to8b(img.cuda(), mode).cpu().permute(2, 0, 1).reshape(-1)[:n]
    assert got[-5:].tolist() == ([0, 255, 0, 255, 255] if mode == "round" else [0, 255, 0, 255, 254])


def test_eight_bit_rows_do_not_touch_their_neighbours():
    """an 8-bit image written into the middle of a larger buffer, at an odd byte offset: the bytes around it keep their value"""
    from adgs import _lib, metrics
    shape = (3, 37, 53)
    img, gt = inputs(shape)
    C, H, W = shape
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.full((H * W * C + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ev = metrics.Evaluator(1)
    a, b = img.cuda(), gt.cuda()
    desc = metrics.MetricsDesc(ctypes.sizeof(metrics.MetricsDesc), C, H, W, 0, 0, 1)
    _lib.call("adgs_metrics_accumulate", dev, ctypes.byref(desc), a.data_ptr(), b.data_ptr(), None, ev.work.data_ptr(), ev.table.data_ptr(), 0, buf.data_ptr() + 29)
    out = buf.cpu()
    assert (out[:29] == 0xAB).all() and (out[29 + H * W * C:] == 0xAB).all()
    assert torch.equal(out[29:29 + H * W * C].reshape(H, W, C), ref.to_u8(img, "round"))


def test_six_views_in_a_row_reset_and_capacity():
    from adgs import metrics
    shapes = [(3, 17, 33), (3, 37, 53), (3, 5, 70), (3, 48, 200), (3, 16, 32), (3, 1, 1)]
    ev = metrics.Evaluator(6, regions=4)
    for k, s in enumerate(shapes):
        img, gt = inputs(s)
        index, out = ev.add(img.cuda(), gt.cuda(), list(masks_of(s, 4).cuda()), u8="truncate" if k % 2 else None)
        assert index == k and (out is None) == (k % 2 == 0)
    assert len(ev) == 6
    res = ev.results()
    assert not ev.work.any()
    for k, s in enumerate(shapes):
        single, _, _ = evaluate(*inputs(s), masks_of(s, 4))
        for r in range(5):
            check_region("view %d region %d" % (k, r), res[r], reference(s, 4)[r], view=k)
            for key in ("l1", "mse", "ssim", "weight"):
                a, b = res[r][key][k], single[r][key][0]
                assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)
    assert res[1]["count"] == 0 and math.isnan(res[1]["mean"]["psnr"]) and res[0]["count"] == 6
    for r in (0, 2, 3, 4):
        for key in ("l1", "psnr", "psnr_channel_mean", "ssim"):
            assert abs(res[r]["mean"][key] - np.mean([reference(s, 4)[r][key] for s in shapes])) <= {"l1": L1_TOL, "ssim": SSIM_TOL}.get(key, PSNR_TOL)
    with pytest.raises(RuntimeError, match="capacity"):
        ev.add(inputs(shapes[0])[0].cuda(), inputs(shapes[0])[1].cuda(), masks_of(shapes[0], 4).cuda())
    ev.reset()
    assert len(ev) == 0 and not ev.table.any() and ev.results()[0]["count"] == 0
    img, gt = inputs(shapes[1])
    assert ev.add(img.cuda(), gt.cuda(), masks_of(shapes[1], 4).cuda())[0] == 0
    check_region("after reset", ev.results()[3], reference(shapes[1], 4)[3])


def test_add_refuses_what_does_not_fit():
    from adgs import metrics
    img, gt = (t.cuda() for t in inputs((3, 17, 33)))
    m = masks_of((3, 17, 33), 1).cuda()
    ev = metrics.Evaluator(2, regions=1)
    for bad, exc in ((lambda: ev.add(img, gt[:, :16], m), ValueError), (lambda: ev.add(img[:2], gt[:2], m), ValueError),
                     (lambda: ev.add(img[0], gt[0], m), ValueError), (lambda: ev.add(img.double(), gt.double(), m), TypeError),
                     (lambda: ev.add(img, gt.half(), m), TypeError), (lambda: ev.add(img.cpu(), gt, m), RuntimeError),
                     (lambda: ev.add(img, gt.cpu(), m), RuntimeError), (lambda: ev.add(img, gt), ValueError),
                     (lambda: ev.add(img, gt, torch.cat([m, m])), ValueError), (lambda: ev.add(img, gt, m[:, :5]), ValueError),
                     (lambda: ev.add(img, gt, m > 0.5), TypeError), (lambda: ev.add(img, gt, m.cpu()), RuntimeError),
                     (lambda: ev.add(img, gt, m, u8="nearest"), ValueError)):
        with pytest.raises(exc):
            bad()
    assert len(ev) == 0 and not ev.table.any() and not ev.work.any()
    with pytest.raises(ValueError):
        metrics.Evaluator(2, regions=5)
    with pytest.raises(ValueError):
        metrics.Evaluator(0)


def test_native_validation_errors_raise():
    from adgs import _lib, metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    img, gt = (t.cuda() for t in inputs((3, 17, 33)))
    m = masks_of((3, 17, 33), 1).cuda()
    ev = metrics.Evaluator(1, regions=1)
    out = torch.full((17, 33, 3), 7, dtype=torch.uint8, device=dev)

    def call(view=0, struct_bytes=ctypes.sizeof(metrics.MetricsDesc), masks=m.data_ptr(), **kw):
        f = dict(channels=3, H=17, W=33, regions=1, quantize=0, u8_mode=1)
        f.update(kw)
        d = metrics.MetricsDesc(struct_bytes, f["channels"], f["H"], f["W"], f["regions"], f["quantize"], f["u8_mode"])
        _lib.call("adgs_metrics_accumulate", dev, ctypes.byref(d), img.data_ptr(), gt.data_ptr(), masks, ev.work.data_ptr(), ev.table.data_ptr(), view, out.data_ptr())
    for kw in (dict(channels=2), dict(regions=5), dict(masks=None), dict(view=-1), dict(H=0), dict(W=0), dict(struct_bytes=8)):
        with pytest.raises(RuntimeError, match="adgs_metrics_accumulate failed: adgs_metrics_accumulate: "):
            call(**kw)
    torch.cuda.synchronize()
    assert (out == 7).all() and not ev.table.any() and not ev.work.any()      # nothing was launched


def test_drop_in_psnr_and_mse():
    from adgs import metrics
    img, gt = torch.from_numpy(GOLDEN["dropin/img"]).cuda(), torch.from_numpy(GOLDEN["dropin/gt"]).cuda()
    for a, b, tag, shape in ((img, gt, "batch", (2, 1)), (img[0], gt[0], "image", (3, 1))):
        p, m = metrics.psnr(a, b), metrics.mse(a, b)
        assert tuple(p.shape) == tuple(m.shape) == shape
        assert np.abs(p.cpu().numpy().astype(np.float64) - GOLDEN["dropin/psnr_" + tag]).max() <= 1e-4
        assert np.abs(m.cpu().numpy().astype(np.float64) / GOLDEN["dropin/mse_" + tag] - 1).max() <= 1e-5
    # ... and the Evaluator gives both of the reference's PSNRs for the same pair
    res, _, _ = evaluate(img[0].cpu(), gt[0].cpu())
    assert abs(res[0]["psnr"][0] - metrics.psnr(img[0][None], gt[0][None]).item()) <= 1e-4
    assert abs(res[0]["psnr_channel_mean"][0] - metrics.psnr(img[0], gt[0]).mean().item()) <= 1e-4


def test_evaluation_loop_of_the_example():
    """examples/evaluate.py's loop on a 160 x 96 scene of 2 000 Gaussians: the metrics are those of the same renders through the reference"""
    import types
    from adgs import synthetic
    from examples import evaluate as example
    from gaussian_renderer import render
    W, H, focal = 160, 96, 120.0
    dev = torch.device("cuda", torch.cuda.current_device())
    sc = synthetic.make_scene(2000, W, H, focal, sh_degree=3, seed=0, n_objects=2)
    cams = [(synthetic.make_camera(W, H, focal, cam_seed=k or None), 0.2 + 0.2 * k) for k in range(3)]
    model, env_map, views = example.build(sc, cams, dev, env_res=64)
    res, render_time, all_time, frame = example.render_set(views, model, env_map)
    assert len(res) == 3 and res[0]["count"] == 3 and 0 < render_time <= all_time
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    for k, view in enumerate(views):
        with torch.no_grad():
            image = render(view, model, env_map, pipe, scaling_modifier=example.EVAL_SCALING)["render"]
        want = ref.metrics(image.cpu(), view.original_image.cpu(), torch.stack([view.semantic, view.sky]).cpu())
        for r in range(3):
            check_region("example view %d region %s" % (k, example.REGION_NAMES[r]), res[r], want[r], view=k)
        assert want[0]["psnr"] < 60 and want[2]["weight"] > 0      # the evaluated render is not the ground truth; there is sky
    assert torch.equal(frame.cpu(), ref.to_u8(image.cpu(), "round"))
    assert any(res[1]["weight"] > 0)                            # some view sees an object
