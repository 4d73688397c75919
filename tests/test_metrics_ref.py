"""tests/metrics_ref.py (float64) against tests/golden/metrics_golden.npz, the values of the reference's own psnr / ssim / l1_loss
(tests/golden/make_metrics_golden.py).  The reference computes in float32, so its distance from the float64 restatement is a
measurement: GOLDEN_TABLE records it per case, the test allows 4 x that figure and never more than 1e-4 dB (PSNR) or 1e-6 (SSIM, L1).
Also what the restatement promises on its own: the region sums, the quantisation and the two 8-bit conversions at their ties."""
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

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "metrics_golden.npz"))
# case: |float32 reference - float64 restatement| of (psnr [dB], psnr_channel_mean [dB], ssim, l1), measured on the CPU
GOLDEN_TABLE = {
    "3x1x1": (2.10e-07, 3.17e-07, 6.73e-08, 1.25e-09),
    "3x5x70": (1.75e-07, 2.31e-07, 2.04e-08, 4.52e-09),
    "3x16x32": (1.76e-07, 1.08e-06, 3.77e-09, 3.26e-09),
    "3x17x33": (1.41e-06, 1.21e-07, 1.88e-08, 8.44e-09),
    "3x37x53": (5.19e-07, 9.40e-07, 4.56e-08, 5.37e-09),
    "1x40x24": (1.00e-06, 1.00e-06, 1.76e-08, 6.56e-09),
    "3x48x200": (9.52e-07, 5.08e-07, 9.41e-08, 3.10e-09),
}
KEYS = ("psnr", "psnr_channel_mean", "ssim", "l1")
CAPS = (1e-4, 1e-4, 1e-6, 1e-6)


def case(name):
    return torch.from_numpy(GOLDEN[name + "/img"]), torch.from_numpy(GOLDEN[name + "/gt"])


@pytest.mark.parametrize("name", sorted(GOLDEN_TABLE))
def test_restatement_equals_the_reference(name):
    img, gt = case(name)
    assert ((img < 0) | (img > 1)).any()                       # the stored render is unclipped
    m = ref.metrics(img, gt)[0]
    for key, recorded, cap in zip(KEYS, GOLDEN_TABLE[name], CAPS):
        err = abs(m[key] - float(GOLDEN[name + "/" + key]))
        tol = min(4 * recorded, cap)
        print("%s %s: %.9g, reference %.9g, diff %.3e, tolerance %.3e" % (name, key, m[key], float(GOLDEN[name + "/" + key]), err, tol))
        assert err <= tol


def test_golden_covers_the_table_and_the_two_psnrs_differ():
    assert {k.split("/")[0] for k in GOLDEN.files} == set(GOLDEN_TABLE) | {"dropin"}
    # the channels of these images are alike, so the two definitions lie close: still 30 x the tolerance they are told apart with
    assert abs(float(GOLDEN["3x37x53/psnr"]) - float(GOLDEN["3x37x53/psnr_channel_mean"])) > 3e-4


def test_drop_in_psnr_and_mse_keep_the_reference_shapes():
    from adgs import metrics
    img, gt = torch.from_numpy(GOLDEN["dropin/img"]), torch.from_numpy(GOLDEN["dropin/gt"])
    for a, b, tag, shape in ((img, gt, "batch", (2, 1)), (img[0], gt[0], "image", (3, 1))):
        p, m = metrics.psnr(a, b), metrics.mse(a, b)
        assert tuple(p.shape) == tuple(m.shape) == shape == GOLDEN["dropin/psnr_" + tag].shape
        assert np.abs(p.numpy().astype(np.float64) - GOLDEN["dropin/psnr_" + tag]).max() <= 1e-4
        assert np.abs(m.numpy().astype(np.float64) / GOLDEN["dropin/mse_" + tag] - 1).max() <= 1e-5
    # psnr(a[None], b[None]) is render.py's PSNR, psnr(a, b).mean() train.py's: the restatement's two forms
    want = ref.metrics(img[0], gt[0])[0]
    assert abs(metrics.psnr(img[0][None], gt[0][None]).item() - want["psnr"]) <= 1e-4
    assert abs(metrics.psnr(img[0], gt[0]).mean().item() - want["psnr_channel_mean"]) <= 1e-4


def test_region_sums():
    img, gt = case("3x17x33")
    H, W = img.shape[1:]
    gen = torch.Generator().manual_seed(3)
    soft = torch.rand(H, W, generator=gen)
    half = torch.zeros(H, W)
    half[:, : W // 2] = 1.0
    whole, ones, zero, s, left = ref.metrics(img, gt, torch.stack([torch.ones(H, W), torch.zeros(H, W), soft, half]))
    for k in KEYS + ("mse",):
        assert ones[k] == whole[k] and math.isnan(zero[k])
    assert zero["weight"] == 0.0 and abs(s["weight"] - float(soft.double().sum())) < 1e-9
    # a binary mask is the metric of the pixels it keeps
    x, y = ref.clip(img).double()[:, :, : W // 2], ref.clip(gt).double()[:, :, : W // 2]
    assert abs(left["l1"] - float((x - y).abs().mean())) < 1e-12
    assert abs(left["mse"] - float(((x - y) ** 2).mean())) < 1e-12
    assert abs(left["ssim"] - float(ref.ssim_map(ref.clip(img).double(), ref.clip(gt).double())[:, :, : W // 2].mean())) < 1e-12
    # identical images
    same = ref.metrics(gt, gt)[0]
    assert same["l1"] == 0.0 and same["psnr"] == math.inf and same["psnr_channel_mean"] == math.inf and abs(same["ssim"] - 1.0) < 1e-12


def test_eight_bit_conversions_at_the_ties():
    img, n = ref.planted_image()
    flat = img.reshape(-1)[:n].double()
    r = ref.to_u8(img, "round").permute(2, 0, 1).reshape(-1)[:n].long()
    t = ref.to_u8(img, "truncate").permute(2, 0, 1).reshape(-1)[:n].long()
    assert r.dtype == t.dtype and ref.to_u8(img, "round").shape == (img.shape[1], img.shape[2], 3)
    assert r[-5:].tolist() == [0, 255, 0, 255, 255] and t[-5:].tolist() == [0, 255, 0, 255, 254]
    # exact arithmetic would give round(x * 255) / floor(x * 255): the float32 two-step result is within one level, and differs somewhere
    exact_r = torch.floor(flat.clamp(0, 1) * 255 + 0.5).long().clamp(max=255)
    assert (r - exact_r).abs().max() <= 1
    assert (r[:768] != exact_r[:768]).any()                    # the ties are decided by float32 rounding: the case a fused multiply-add misses
    # the quantised image is the rounded byte over 255
    q = ref.quantize(img).reshape(-1)[:n]
    assert torch.equal(q, r.float() / 255.0)
    m_q, m_c = ref.metrics(img, img, quantized=True)[0], ref.metrics(img, img)[0]
    assert m_c["l1"] == 0.0 and 0.0 < m_q["l1"] <= 0.5 / 255 + 1e-7
