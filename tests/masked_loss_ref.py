"""Float64 torch-CPU restatement of the weighted training losses (adgs.loss with `weight=`, include/adgs_loss.h) and of the sparse metric
depth term.  With P planes (the product of the leading dimensions of [..., C, H, W] times C) and Sw the sum of the [H, W] weight:

    L1_w   = sum_planes sum_pixels w |image - gt| / (P Sw)
    SSIM_w = sum_planes sum_pixels w ssim_map     / (P Sw)

ssim_map is the unweighted map (11x11 Gaussian window, sigma 1.5, zero padding), written as tests/metrics_ref.py writes it; Sw = 0 gives 0.
Gradients come from autograd.  `dtype` is float64 everywhere except where a test measures what float32 alone costs."""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    return (g[:, None] * g[None, :]).to(dtype)


def ssim_map(x, y):
    """[P, H, W] -> the SSIM map, [P, H, W]"""
    P = x.shape[0]
    w = window(x.dtype)[None, None].expand(P, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=P)[0]
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def l1_ssim(image, gt, weight, dtype=torch.float64):
    """image, gt: [..., C, H, W]; weight: [H, W] or [1, H, W] -> (L1_w, SSIM_w) as 0-d tensors of `dtype`, differentiable w.r.t. image"""
    H, W = image.shape[-2:]
    x, y = image.to(dtype).reshape(-1, H, W), gt.to(dtype).reshape(-1, H, W)
    w = weight.to(dtype).reshape(H, W)
    sw = w.sum()
    if float(sw) == 0:
        zero = (x * 0).sum()
        return zero, zero.clone()
    n = x.shape[0] * sw
    return (w * (x - y).abs()).sum() / n, (w * ssim_map(x, y)).sum() / n


def l1_ssim_grads(image, gt, weight, dtype=torch.float64):
    """-> (L1_w, SSIM_w, dL1_w/dimage, dSSIM_w/dimage): two floats and two tensors of image's shape"""
    x = image.detach().to(dtype).clone().requires_grad_(True)
    l1, s = l1_ssim(x, gt, weight, dtype)
    g1, = torch.autograd.grad(l1, x, retain_graph=True)
    g2, = torch.autograd.grad(s, x)
    return float(l1.detach()), float(s.detach()), g1, g2


def bce_clip(pred, target, lo, hi, invert, positive_target, weight=None, dtype=torch.float64):
    """sum w bce / sum w of q = clip(pred, lo, hi) (1 - clip with invert) against t = target ((target > 0) with positive_target), the
    logarithms clamped at -100 as torch.nn.functional.binary_cross_entropy does; 0 when sum w = 0"""
    p, t = pred.to(dtype), target.to(dtype).reshape(pred.shape)
    w = torch.ones_like(p) if weight is None else weight.to(dtype).reshape(pred.shape)
    c = p.clamp(lo, hi)
    q = 1 - c if invert else c
    t = (t > 0).to(dtype) if positive_target else t
    bce = -(t * q.log().clamp_min(-100) + (1 - t) * (1 - q).log().clamp_min(-100))
    sw = w.sum()
    return (p * 0).sum() if float(sw) == 0 else (w * bce).sum() / sw


def lidar_depth(depth, lidar, mask, inv_depth, dtype=torch.float64):
    """sum_valid m |depth - target| / sum_valid m; valid: m > 0 and lidar > 0; target = lidar or 1 / lidar; 0 when nothing is valid"""
    d, l = depth.to(dtype), lidar.to(dtype).reshape(depth.shape)
    m = mask.to(dtype).reshape(depth.shape)
    valid = (m > 0) & (l > 0)
    m = torch.where(valid, m, torch.zeros_like(m))
    safe = torch.where(valid, l, torch.ones_like(l))
    target = 1 / safe if inv_depth else safe
    sm = m.sum()
    return (d * 0).sum() if float(sm) == 0 else (m * (d - target).abs()).sum() / sm


def value_and_grad(fn, x, dtype=torch.float64):
    """(fn(x) as a float, its gradient) for x converted to `dtype`"""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    v = fn(x)
    g, = torch.autograd.grad(v, x)
    return float(v.detach()), g
