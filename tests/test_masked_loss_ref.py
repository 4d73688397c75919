"""tests/masked_loss_ref.py pinned without a GPU: with a weight of ones it is the unweighted loss of the golden vectors, it is the region
metric of tests/metrics_ref.py, its autograd gradients agree with central differences, and its BCE and LiDAR expressions are the plain
torch ones."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import masked_loss_ref as ref
from tests import metrics_ref

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_golden.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files if not k.startswith("depth")})


@pytest.mark.parametrize("case", CASES)
def test_weight_of_ones_is_the_unweighted_golden_loss(case):
    """the tolerances of tests/test_gpu_loss.py:22-27 for these fixtures"""
    img, gt = torch.tensor(GOLD[case + "/img"]), torch.tensor(GOLD[case + "/gt"])
    l1, s, g1, g2 = ref.l1_ssim_grads(img, gt, torch.ones(img.shape[-2:]))
    assert abs(l1 - float(GOLD[case + "/l1"])) <= 1e-6 and abs(s - float(GOLD[case + "/ssim"])) <= 1e-5
    np.testing.assert_allclose(g1.numpy(), GOLD[case + "/g_l1"], rtol=1e-6, atol=1e-9)
    want = GOLD[case + "/g_ssim"]
    np.testing.assert_allclose(g2.numpy(), want, rtol=0, atol=1e-4 * np.abs(want).max())


@pytest.mark.parametrize("C", [1, 3])
def test_equals_the_region_metric_of_the_evaluation_reference(C):
    g = torch.Generator().manual_seed(5 + C)
    H, W = 23, 41
    gt = torch.rand(C, H, W, generator=g)
    img = (gt + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    masks = torch.stack([(torch.rand(H, W, generator=g) > 0.5).float(), torch.rand(H, W, generator=g)])
    m = metrics_ref.metrics(img, gt, masks)
    for r in range(2):
        l1, s = ref.l1_ssim(img, gt, masks[r])
        np.testing.assert_allclose(float(l1), m[1 + r]["l1"], rtol=1e-12)
        np.testing.assert_allclose(float(s), m[1 + r]["ssim"], rtol=1e-12)
    l1, s = ref.l1_ssim(img, gt, torch.ones(1, H, W))                  # [1, H, W] is accepted; ones = the whole image
    np.testing.assert_allclose([float(l1), float(s)], [m[0]["l1"], m[0]["ssim"]], rtol=1e-12)


def test_gradients_against_central_differences():
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(3, 7, 9, generator=g, dtype=torch.float64)
    img = (gt + 0.2 * torch.randn(3, 7, 9, generator=g, dtype=torch.float64)).clamp(0.05, 0.95)
    w = torch.rand(7, 9, generator=g, dtype=torch.float64)
    w[2:4] = 0
    _, _, g1, g2 = ref.l1_ssim_grads(img, gt, w)
    h = 1e-6
    fd = torch.zeros(2, *img.shape, dtype=torch.float64)
    for i in range(img.numel()):
        e = torch.zeros(img.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(img.shape)
        hi, lo = ref.l1_ssim(img + e, gt, w), ref.l1_ssim(img - e, gt, w)
        for k in range(2):
            fd[k].reshape(-1)[i] = (float(hi[k]) - float(lo[k])) / (2 * h)
    # |img - gt| >= 1e-3 here except by accident: no kink inside a step of 1e-6
    assert float((img - gt).abs().min()) > 10 * h
    np.testing.assert_allclose(g1.numpy(), fd[0].numpy(), rtol=0, atol=1e-8)
    np.testing.assert_allclose(g2.numpy(), fd[1].numpy(), rtol=0, atol=1e-7 * float(g2.abs().max()) + 1e-9)
    assert float(g1[:, 2:4].abs().max()) == 0.0                        # no L1 gradient where the weight is zero


def test_zero_weight_gives_zero_loss_and_zero_gradient():
    g = torch.Generator().manual_seed(2)
    img, gt = torch.rand(2, 3, 6, 8, generator=g), torch.rand(2, 3, 6, 8, generator=g)
    l1, s, g1, g2 = ref.l1_ssim_grads(img, gt, torch.zeros(6, 8))
    assert l1 == 0.0 and s == 0.0 and not g1.any() and not g2.any() and g1.shape == img.shape
    v, gp = ref.value_and_grad(lambda p: ref.bce_clip(p, (gt[0, 0] > 0.5).float(), 1e-3, 1 - 1e-3, 0, 0, torch.zeros(6, 8)), img[0, 0])
    assert v == 0.0 and not gp.any()
    v, gd = ref.value_and_grad(lambda d: ref.lidar_depth(d, gt[0, 0], torch.zeros(6, 8), False), img[0, 0])
    assert v == 0.0 and not gd.any()


def test_bce_and_lidar_expressions_against_plain_torch():
    g = torch.Generator().manual_seed(3)
    H, W = 9, 13
    pred = torch.rand(H, W, generator=g, dtype=torch.float64) * 0.9 + 0.05
    tgt = (torch.rand(H, W, generator=g) > 0.6).double()
    w = torch.rand(H, W, generator=g, dtype=torch.float64)
    lo, hi = 1e-3, 1 - 1e-3
    # the object term (positive_target) and the sky term (invert) of train.py:95-103, unweighted: the mean
    np.testing.assert_allclose(float(ref.bce_clip(pred, tgt * 3, lo, hi, 0, 1)), float(F.binary_cross_entropy(pred.clamp(lo, hi), tgt)), rtol=1e-13)
    np.testing.assert_allclose(float(ref.bce_clip(pred, tgt, lo, hi, 1, 0)), float(F.binary_cross_entropy(1 - pred.clamp(lo, hi), tgt)), rtol=1e-13)
    # weighted: torch's own per-element weight, renormalised by the sum of weights
    want = F.binary_cross_entropy(1 - pred.clamp(lo, hi), tgt, weight=w, reduction="sum") / w.sum()
    np.testing.assert_allclose(float(ref.bce_clip(pred, tgt, lo, hi, 1, 0, w)), float(want), rtol=1e-13)
    depth = torch.rand(H, W, generator=g, dtype=torch.float64) * 50 + 1
    lidar = torch.rand(H, W, generator=g, dtype=torch.float64) * 50 + 1
    mask = torch.rand(H, W, generator=g) > 0.7
    lidar[0, :5] = 0                                                    # masked pixels without a return
    mask[0, :5] = True
    v = mask & (lidar > 0)
    np.testing.assert_allclose(float(ref.lidar_depth(depth, lidar, mask, False)), float((depth[v] - lidar[v]).abs().mean()), rtol=1e-13)
    np.testing.assert_allclose(float(ref.lidar_depth(depth, lidar, mask, True)), float((depth[v] - 1 / lidar[v]).abs().mean()), rtol=1e-13)
    val, grad = ref.value_and_grad(lambda d: ref.lidar_depth(d, lidar, mask, True), depth)
    assert np.isfinite(val) and bool(torch.isfinite(grad).all()) and not grad[~v].any()
