"""The float64 reference of the colour fit (tests/colorcorrect_ref.py) checked against what the definition implies, without a GPU: an
exact warp is recovered, a fully clipped image gives the identity, pixels of weight zero do not exist for the fit, and one iteration
never makes the fitted pixels worse."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests import colorcorrect_ref as ref  # noqa: E402

EPS = 0.5 / 255


def dyadic_image(seed, H=24, W=40):
    """values k / 64, k = 8 .. 40: with the dyadic coefficients below, every product and sum of the warps is exact in float32, so `gt`
    is an exact warp of `image` although both are float32"""
    rng = np.random.RandomState(seed)
    return (rng.randint(8, 41, size=(3, H, W)) / 64.0).astype(np.float32)


def exact_warp(image, model):
    r, g, b = image.astype(np.float64)
    if model == "affine":
        out = [0.5 * r + 0.25 * g + 0.125 * b + 0.0625, 0.125 * r + 0.75 * g + 0.03125, 0.25 * g + 0.5 * b + 0.125]
    else:
        out = [0.5 * r + 0.25 * g * g + 0.125 * r * b + 0.125, 0.75 * g + 0.25 * r * r - 0.125 * g * b + 0.0625, 0.5 * b + 0.5 * r * g + 0.25 * b * b + 0.03125]
    out = np.stack(out)
    gt = out.astype(np.float32)
    assert np.array_equal(gt.astype(np.float64), out)                      # exactly representable
    assert out.min() > EPS and out.max() < 1 - EPS and image.min() > EPS and image.max() < 1 - EPS
    return gt


@pytest.mark.parametrize("model", ["affine", "quadratic"])
def test_an_exact_warp_is_recovered_in_one_iteration(model):
    """The ridge pulls the solution towards the identity by about ridge / (smallest eigenvalue of G) -- 1e-6 at the default 1e-6, for
    this image -- so the exactness is asked at ridge 1e-13, where that pull (1e-13) and the solve's own error (condition 1e5 x 2^-53)
    are both far below the 1e-9 asserted."""
    image = dyadic_image(1)
    gt = exact_warp(image, model)
    res = ref.color_correct(image, gt, model=model, iters=1, ridge=1e-13)
    assert np.abs(res["image64"] - gt.astype(np.float64)).max() <= 1e-9
    assert np.all(res["support"] == image.shape[1] * image.shape[2])
    assert res["cond"] < 1e8
    if model == "affine":
        assert not res["warps"][:, :, 3:9].any()


def test_every_pixel_clipped_gives_exactly_the_identity():
    image = np.full((3, 7, 9), 1.5, np.float32)
    gt = dyadic_image(2, 7, 9)
    for model in ("affine", "quadratic"):
        res = ref.color_correct(image, gt, model=model, iters=3)
        assert not res["support"].any()
        for k in range(3):
            assert np.array_equal(res["warps"][k], np.eye(3, ref.FEATURES))
        assert np.array_equal(res["image"], np.ones((3, 7, 9), np.float32))      # clip(image), bit for bit


def test_pixels_under_zero_weight_change_no_bit_of_the_warps():
    rng = np.random.RandomState(3)
    gt = rng.uniform(-0.1, 1.1, size=(3, 19, 23)).astype(np.float32)
    image = (0.8 * gt + 0.07 + 0.02 * rng.randn(3, 19, 23)).astype(np.float32)
    weight = rng.uniform(0, 1, size=(19, 23)).astype(np.float32)
    weight[rng.uniform(size=(19, 23)) < 0.4] = 0.0
    dead = weight == 0
    image2, gt2 = image.copy(), gt.copy()
    image2[:, dead] = rng.uniform(-0.5, 1.5, size=(3, int(dead.sum()))).astype(np.float32)
    gt2[:, dead] = rng.uniform(-0.5, 1.5, size=(3, int(dead.sum()))).astype(np.float32)
    for model in ("affine", "quadratic"):
        a = ref.color_correct(image, gt, weight, model=model, iters=4)
        b = ref.color_correct(image2, gt2, weight, model=model, iters=4)
        assert np.array_equal(a["warps"], b["warps"]) and np.array_equal(a["support"], b["support"])
        assert np.array_equal(a["image"][:, ~dead], b["image"][:, ~dead])
        assert a["support"].min() > 0


@pytest.mark.parametrize("model", ["affine", "quadratic"])
def test_one_iteration_does_not_make_the_fitted_pixels_worse(model):
    """W minimises sum m (phi . W - y)^2 + ridge |W - e_c|^2, and at W = e_c that is the uncorrected error: the corrected error is not
    above it (the clip moves a value towards y, which lies in [0, 1]).  The margin allowed for the ridge is ridge |e_c|^2 = ridge."""
    rng = np.random.RandomState(4)
    ridge = 1e-6
    gt = rng.uniform(-0.1, 1.1, size=(3, 21, 34)).astype(np.float32)
    image = (0.7 * gt + 0.1 + 0.05 * rng.randn(3, 21, 34)).astype(np.float32)
    weight = rng.uniform(0, 1, size=(21, 34)).astype(np.float32)
    res = ref.color_correct(image, gt, weight, model=model, iters=1, ridge=ridge)
    x0, y = np.clip(image, 0, 1).astype(np.float64), np.clip(gt, 0, 1).astype(np.float64)
    eps = float(np.float32(EPS))
    ok = lambda z: (z >= eps) & (z <= 1 - eps)
    for c in range(3):
        m = weight.astype(np.float64) * (ok(x0[c]) & ok(y[c]))
        assert abs(m.sum() - res["support"][0, c]) <= 1e-9 * m.sum()
        before, after = (m * (x0[c] - y[c]) ** 2).sum(), (m * (res["image64"][c] - y[c]) ** 2).sum()
        assert after <= before + ridge * 1.0
        assert after < 0.5 * before                            # ... and this pair has an exposure mismatch to remove
