"""Float64 torch-CPU restatement of the evaluation pass (adgs.metrics, include/adgs_metrics.h): the clipping of render.py:54-56, the
optional 8-bit quantisation of the render, L1 / MSE / SSIM (11x11 Gaussian window, sigma 1.5, zero padding: utils/loss_utils.py:26-66)
with both PSNR forms (render.py:59: the whole image; train.py:258: the mean of the per-channel PSNRs), the weighted region sums, and the
two 8-bit conversions in float32 exactly as the libraries write them (torchvision.utils.save_image; render.py:39 to8b, in numpy)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def clip(x):
    return x.clamp(0.0, 1.0)


def quantize(image):
    """The value a PNG written by save_image holds, as a float32 tensor: floor(x * 255 + 0.5) / 255 of the clipped float32 image, every
    operation rounded to float32 on its own."""
    x = clip(image.float())
    return torch.floor(x * 255.0 + 0.5) / 255.0


def window():
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    return g[:, None] * g[None, :]


def ssim_map(x, y):
    """[C, H, W] float64 -> the SSIM map, [C, H, W]"""
    C = x.shape[0]
    w = window()[None, None].expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=C)[0]
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def _psnr(mse):
    return math.inf if mse == 0 else 10.0 * math.log10(1.0 / mse)


def metrics(image, gt, masks=None, quantized=False):
    """image, gt: [C, H, W] float32, unclipped; masks: [R, H, W] weights or None.  Returns a list over the regions (0: the whole image)
    of {"l1", "mse", "psnr", "psnr_channel_mean", "ssim", "weight"} as Python floats; every metric is NaN where a region has no weight."""
    x = (quantize(image) if quantized else clip(image.float())).double()
    y = clip(gt.float()).double()
    C, H, W = x.shape
    d = x - y
    smap = ssim_map(x, y)
    weights = [torch.ones(H, W, dtype=torch.float64)] + ([] if masks is None else [m.double() for m in masks])
    out = []
    for w in weights:
        n = float(w.sum())
        if n == 0:
            out.append({k: math.nan for k in ("l1", "mse", "psnr", "psnr_channel_mean", "ssim")} | {"weight": 0.0})
            continue
        sq = [float((w * d[c] ** 2).sum()) for c in range(C)]
        mse = sum(sq) / (C * n)
        out.append({"l1": float((w * d.abs()).sum()) / (C * n), "mse": mse, "psnr": _psnr(mse),
                    "psnr_channel_mean": sum(_psnr(s / n) for s in sq) / C, "ssim": float((w * smap).sum()) / (C * n), "weight": n})
    return out


def to_u8(image, mode):
    """[C, H, W] float32 -> [H, W, C] uint8.  "round": torchvision.utils.save_image (`grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0)
    .to("cpu", torch.uint8)`) of the clipped image, restated; "truncate": render.py:39,68 to8b on the permuted numpy array."""
    x = clip(image.float())
    if mode == "round":
        return x.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).contiguous()
    if mode == "truncate":
        return torch.from_numpy((255.0 * np.clip(torch.permute(x, (1, 2, 0)).numpy(), 0, 1)).astype(np.uint8))
    raise ValueError(mode)


def planted_image():
    """float32((k + 0.5) / 255) and its two float32 neighbours for every k (where a fused multiply-add would round differently), and the
    values at and beyond the clip bounds"""
    t = torch.tensor([(k + 0.5) / 255 for k in range(256)], dtype=torch.float32)
    vals = torch.cat([t, torch.nextafter(t, torch.tensor(0.0)), torch.nextafter(t, torch.tensor(2.0)),
                      torch.tensor([0.0, 1.0, -0.3, 1.7]), torch.nextafter(torch.tensor([1.0]), torch.tensor(0.0))])
    n = vals.numel()                                           # 773
    W = 53
    H = (n + 3 * W - 1) // (3 * W)
    img = torch.zeros(3 * H * W)
    img[:n] = vals
    return img.reshape(3, H, W), n
