"""The colour fit on the GPU (adgs.colorcorrect over include/adgs_colorcorrect.h) against the float64 reference of
tests/colorcorrect_ref.py.

Shapes (H, W); the accumulate launch has one workgroup of 256 threads per 256 pixels, at most 512, and 64 slot rows: (1,1) a single
pixel; (3,5) less than a wave; (16,32) two workgroups; (17,33), (37,53) partial last workgroups, odd sizes; (48,200) 38 workgroups;
(131,137) 71 workgroups -- more than slot rows, so two workgroups add into one row.

Inputs: the unclipped noise images of tests/golden/metrics_golden.npz where it has the shape, and a NEAR-GREY pair from a seed: luma
uniform in [0.1, 0.9] plus per-channel noise of sigma 0.01, the render 0.8 gt + 0.07 plus the same noise, every eighth pixel pushed
outside [0, 1] in both, on alternating sides.  Its Gram matrices have condition numbers around 1e9: in float32 they are not positive
definite.

Tolerances.  Corrected image: 1e-6 on every element against the reference's float32 image -- the float32 rounding of the output
(6e-8) plus the order effects of the double sums and the solve, which measured 2e-9 on the CPU at condition 1.7e9 (a permuted 64-chunk
summation); it is also the project's L1 tolerance.  Support: 1e-9 relative.  The warps are not compared: they are ill-conditioned by
design, only what they do to the image counts.  So that no mask bit can differ between the two sides, every case asserts that the
reference's own condition number is at most 1e10 and that no value it computed lies within 2e-8 (ten times the measured order effect)
of a threshold of the `unclipped` predicate; the seeds below were chosen on the CPU, with the reference alone, to meet both."""
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

from tests import colorcorrect_ref as ref  # noqa: E402
from tests import metrics_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (16, 32), (17, 33), (37, 53), (48, 200), (131, 137)]
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "metrics_golden.npz"))
SEEDS = {(1, 1): 0, (3, 5): 0, (16, 32): 0, (17, 33): 0, (37, 53): 0, (48, 200): 0, (131, 137): 0}      # near-grey: see the docstring
CASES = [(s, kind) for s in SHAPES for kind in ("noise", "grey") if kind == "grey" or "3x%dx%d/img" % s in GOLDEN.files]
MODELS = ("affine", "quadratic")
ITERS = (1, 2, 5)
WEIGHTS = (None, "soft", "corner", "zero")
IMAGE_TOL, SUPPORT_REL = 1e-6, 1e-9
COND_MAX, MARGIN_MIN = 1e10, 2e-8
PSNR_TOL, SSIM_TOL = 1e-5, 1e-5            # those of tests/test_gpu_metrics.py


def near_grey(shape, seed):
    H, W = shape
    rng = np.random.RandomState(seed)
    luma = rng.uniform(0.1, 0.9, size=(1, H, W))
    gt = luma + 0.01 * rng.randn(3, H, W)
    img = 0.8 * gt + 0.07 + 0.01 * rng.randn(3, H, W)
    pix = np.arange(H * W).reshape(H, W)
    out, above = pix % 8 == 7, (pix // 8) % 2 == 0         # saturated in the render and in the photograph alike: a lamp, a shadow
    for t in (img, gt):
        far = rng.uniform(0.05, 0.5, size=(3, H, W))
        t[:, out & above] = 1.0 + far[:, out & above]
        t[:, out & ~above] = -far[:, out & ~above]
    return img.astype(np.float32), gt.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    if kind == "grey":
        return near_grey(shape, SEEDS[shape])
    return GOLDEN["3x%dx%d/img" % shape], GOLDEN["3x%dx%d/gt" % shape]


@functools.lru_cache(maxsize=None)
def weight_of(shape, which):
    """soft: uniform in [0, 1); corner: non-zero only in the bottom-right 32 x 16 pixels; zero: nothing to fit"""
    H, W = shape
    soft = np.random.RandomState(H * 1000 + W).uniform(size=(H, W)).astype(np.float32)
    if which is None or which == "soft":
        return None if which is None else soft
    w = np.zeros((H, W), np.float32)
    if which == "corner":
        w[max(H - 16, 0):, max(W - 32, 0):] = 0.25 + 0.75 * soft[max(H - 16, 0):, max(W - 32, 0):]
    return w


@functools.lru_cache(maxsize=None)
def reference(shape, kind, model, iters, which):
    """computed once per case, shared, never modified"""
    img, gt = inputs(shape, kind)
    return ref.color_correct(img, gt, weight_of(shape, which), model=model, iters=iters)


def well_posed(shape, kind):
    """what the seeds were chosen for: -> (largest cond, smallest margin) over every crossed case of the shape"""
    res = [reference(shape, kind, m, it, w) for m in MODELS for it in ITERS for w in WEIGHTS]
    return max(r["cond"] for r in res), min(r["margin"] for r in res)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape,kind", CASES)
def test_corrected_image_and_support_against_the_reference(shape, kind, model):
    from adgs import colorcorrect
    img, gt = inputs(shape, kind)
    fitter = colorcorrect.ColorFitter()
    d_img, d_gt = dev(img), dev(gt)
    clipped = np.clip(img, np.float32(0), np.float32(1))
    for iters in ITERS:
        for which in WEIGHTS:
            tag = "%s %s %s iters %d weight %s" % (shape, kind, model, iters, which)
            want = reference(shape, kind, model, iters, which)
            warp = fitter.fit(d_img, d_gt, dev(weight_of(shape, which)), model=model, iters=iters)
            got = colorcorrect.apply(d_img, warp)
            assert not fitter.work.any(), tag                  # every finishing launch leaves the work buffer zero
            assert got.dtype == torch.float32 and tuple(got.shape) == img.shape and warp.iters == iters and warp.model == model
            warps, support = warp.host()
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want["image"].astype(np.float64)).max())
            rel = float(np.abs(support - want["support"]).max() / max(want["support"].max(), 1e-300))
            print("%s: cond %.2e  margin %.2e  |image| %.2e (%.0e)  support rel %.2e (%.0e)" % (
                tag, want["cond"], want["margin"], err, IMAGE_TOL, rel, SUPPORT_REL))
            assert want["cond"] <= COND_MAX and want["margin"] >= MARGIN_MIN, tag
            assert err <= IMAGE_TOL, tag
            assert np.all(np.abs(support - want["support"]) <= SUPPORT_REL * want["support"]), tag
            assert warps.shape == (iters, 3, 10) and np.isfinite(warps).all(), tag
            if model == "affine":
                assert not warps[:, :, 3:9].any(), tag
            if which == "zero":
                assert not support.any() and all(np.array_equal(warps[k], np.eye(3, 10)) for k in range(iters)), tag
                assert np.array_equal(got.cpu().numpy(), clipped), tag      # bit for bit
            # a second call on the same buffers
            again = colorcorrect.apply(d_img, fitter.fit(d_img, d_gt, dev(weight_of(shape, which)), model=model, iters=iters))
            assert float((again - got).abs().max()) <= IMAGE_TOL, tag


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape,kind", CASES)
def test_metrics_of_the_corrected_image(shape, kind, model):
    """color_correct(image, gt)[0] through the Evaluator against the reference's corrected image through tests/metrics_ref.py.  An
    image within d = 1e-6 of another has, to first order, a PSNR within (20 / ln 10) d / rmse of the other's: the bound is the
    Evaluator's own tolerance plus that term, from the reference's own rmse; the SSIM bound is its tolerance plus the same term."""
    from adgs import colorcorrect, metrics
    img, gt = inputs(shape, kind)
    want_img = reference(shape, kind, model, 5, None)
    assert want_img["cond"] <= COND_MAX and want_img["margin"] >= MARGIN_MIN
    corrected, warp = colorcorrect.color_correct(dev(img), dev(gt), model=model)
    assert warp.iters == 5 and warp.eps == 0.5 / 255
    ev = metrics.Evaluator(2)
    ev.add(dev(img), dev(gt))
    ev.add(corrected, dev(gt))
    got = ev.results()[0]
    want = metrics_ref.metrics(torch.from_numpy(want_img["image"]), torch.from_numpy(gt))[0]
    raw = metrics_ref.metrics(torch.from_numpy(img), torch.from_numpy(gt))[0]
    rmse = math.sqrt(want["mse"])
    first_order = (20.0 / math.log(10.0)) * IMAGE_TOL / rmse if rmse > 0 else math.inf
    print("%s %s %s: raw psnr %.4f  cc_psnr %.4f (reference %.4f, bound %.2e)  cc_ssim %.6f (reference %.6f)" % (
        shape, kind, model, got["psnr"][0], got["psnr"][1], want["psnr"], PSNR_TOL + first_order, got["ssim"][1], want["ssim"]))
    if rmse > 0:
        assert abs(got["psnr"][1] - want["psnr"]) <= PSNR_TOL + first_order
        assert abs(got["ssim"][1] - want["ssim"]) <= SSIM_TOL + first_order
    else:                                                        # a fit without residual (one pixel): an image within 1e-6 of the ground truth
        assert got["psnr"][1] >= -20.0 * math.log10(IMAGE_TOL) and got["ssim"][1] >= 1.0 - SSIM_TOL
    if kind == "grey":
        gain = want["psnr"] - raw["psnr"]
        assert gain > 0                                          # the reference removes the exposure mismatch ...
        assert got["psnr"][1] > got["psnr"][0]                   # ... and so does the GPU: at least half of the reference's gain
        assert got["psnr"][1] - got["psnr"][0] >= 0.5 * gain or math.isinf(gain)      # (an infinite one: the 120 dB asserted above)


def test_non_contiguous_inputs_give_the_result_of_their_contiguous_copies():
    from adgs import colorcorrect
    shape = (37, 53)
    H, W = shape
    img, gt = inputs(shape, "grey")
    w = weight_of(shape, "soft")
    wide_img, wide_gt = torch.zeros(3, H, 2 * W, device="cuda"), torch.zeros(H, W, 3, device="cuda")
    wide_img[:, :, ::2] = dev(img)
    wide_gt[:] = dev(gt).permute(1, 2, 0)
    wide_w = torch.zeros(W, H, device="cuda")
    wide_w[:] = dev(w).t()
    a, b, c = wide_img[:, :, ::2], wide_gt.permute(2, 0, 1), wide_w.t()
    assert not a.is_contiguous() and not b.is_contiguous() and not c.is_contiguous()
    got, _ = colorcorrect.color_correct(a, b, weight=c)
    want, _ = colorcorrect.color_correct(dev(img), dev(gt), weight=dev(w))
    assert got.is_contiguous() and float((got - want).abs().max()) <= IMAGE_TOL
    assert float((got.cpu() - torch.from_numpy(reference(shape, "grey", "quadratic", 5, "soft")["image"])).abs().max()) <= IMAGE_TOL


def test_a_warp_applies_to_another_image():
    """apply() takes any image of the warp's device: the warp of one view on the reference's restatement of x -> clip(phi(x) . W)"""
    from adgs import colorcorrect
    shape = (17, 33)
    img, gt = inputs(shape, "grey")
    other = inputs(shape, "noise")[0]
    for model in MODELS:
        warp = colorcorrect.fit(dev(img), dev(gt), model=model, iters=2)
        warps, _ = warp.host()
        x = np.clip(other, np.float32(0), np.float32(1)).astype(np.float64).reshape(3, -1)
        for k in range(2):
            x = np.clip(warps[k] @ ref.features(x, model), 0.0, 1.0)
        got = colorcorrect.apply(dev(other), warp).cpu().numpy()
        assert np.abs(got.astype(np.float64) - x.reshape(other.shape)).max() <= 1e-7      # the float32 rounding of the output


def test_evaluation_loop_of_the_example_with_colour_correction():
    """examples/evaluate.py --color-correct on a 160 x 96 scene: the raw figures are those of the loop without the flag, and the "cc"
    figures those of the colour-corrected renders through an Evaluator of their own"""
    import types
    from adgs import colorcorrect, metrics, synthetic
    from examples import evaluate as example
    from gaussian_renderer import render
    W, H, focal = 160, 96, 120.0
    device = torch.device("cuda", torch.cuda.current_device())
    sc = synthetic.make_scene(2000, W, H, focal, sh_degree=3, seed=0, n_objects=2)
    cams = [(synthetic.make_camera(W, H, focal, cam_seed=k or None), 0.2 + 0.2 * k) for k in range(2)]
    model, env_map, views = example.build(sc, cams, device, env_res=64)
    plain, _, _, _ = example.render_set(views, model, env_map)
    res, _, _, frame = example.render_set(views, model, env_map, color_correct=True)
    assert len(res) == 3 and frame is not None and all("cc" not in region for region in plain)
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    ev = metrics.Evaluator(2, regions=2)
    for view in views:
        with torch.no_grad():
            image = render(view, model, env_map, pipe, scaling_modifier=example.EVAL_SCALING)["render"]
        ev.add(colorcorrect.color_correct(image, view.original_image)[0], view.original_image, masks=(view.semantic, view.sky))
    want = ev.results()
    for r in range(3):
        for k in ("psnr", "ssim", "l1"):
            for a, b in ((res[r][k], plain[r][k]), (res[r]["cc"][k], want[r][k])):      # the raw figures are those without the flag
                assert all((math.isnan(u) and math.isnan(v)) or abs(u - v) <= 1e-5 for u, v in zip(a, b)), (r, k)
    print("example: psnr %.4f  cc_psnr %.4f" % (res[0]["mean"]["psnr"], res[0]["cc"]["mean"]["psnr"]))
