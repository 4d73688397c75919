"""Inputs of tests/test_gpu_normals.py, generated on the CPU with seeded generators (shared with the float32 check of
tests/test_normals_ref.py)."""
import functools

import torch

from tests import normals_ref as ref

TAN = (0.47, 0.31)
LARGE, LARGE_TAN = (161, 1025), (2.0, 0.35)
WEIGHTS = (None, "ones", "zeros", "binary", "fractional", "zero_rows", "corner_pixel")
OPACITIES = ("above", "mixed", "holes", "zero_column", "below")
DEPTHS = ("noisy", "smooth")
# (depth kind, opacity kind, weight kind, inv_depth) of the large shape
LARGE_CASES = (("smooth", "mixed", "fractional", True), ("noisy", "holes", None, False), ("smooth", "above", "binary", False))


def make_weight(kind, H, W):
    g = torch.Generator().manual_seed(1000 + H * 31 + W)
    if kind is None:
        return None
    if kind == "ones":
        return torch.ones(H, W)
    if kind == "zeros":
        return torch.zeros(H, W)
    if kind == "binary":
        return (torch.rand(H, W, generator=g) > 0.4).float()
    if kind == "fractional":
        return torch.rand(H, W, generator=g)
    if kind == "zero_rows":                                    # the ego vehicle: the bottom rows, from a row inside a tile
        w = torch.ones(H, W)
        w[H - max(H // 3, 1):] = 0
        return w
    if kind == "corner_pixel":                                 # the only weighted pixel is never valid: sum v = 0
        w = torch.zeros(H, W)
        w[H - 1, W - 1] = 0.75
        return w
    raise ValueError(kind)


def make_opacity(kind, H, W):
    """Never within 0.1 of min_opacity = 0.5."""
    g = torch.Generator().manual_seed(2000 + H * 37 + W)
    hi, lo = 0.6 + 0.4 * torch.rand(H, W, generator=g), 0.1 + 0.3 * torch.rand(H, W, generator=g)
    if kind == "above":
        return hi
    if kind == "below":
        return lo
    if kind == "mixed":
        return torch.where(torch.rand(H, W, generator=g) < 0.15, lo, hi)
    if kind == "holes":                                        # holes across the borders of the 32 x 16 tiles
        o = hi.clone()
        for y0 in range(14, H, 16):
            for x0 in range(30, W, 32):
                o[y0:y0 + 4, x0:x0 + 5] = lo[y0:y0 + 4, x0:x0 + 5]
        o[: min(2, H), : min(3, W)] = lo[: min(2, H), : min(3, W)]
        return o
    if kind == "zero_column":                                  # nothing rendered at x = 31 .. 32: D = 0 there as well
        o = hi.clone()
        o[:, 31:33] = 0
        if W <= 31:
            o[:, W // 2] = 0
        return o
    raise ValueError(kind)


def make_z(kind, H, W):
    g = torch.Generator().manual_seed(3000 + H * 41 + W)
    if kind == "noisy":
        return 4 + 20 * torch.rand(H, W, generator=g)
    y, x = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    return 12 + 3 * torch.sin(x / 7) + 2 * torch.cos(y / 5) + 0.004 * x + 0.01 * y


@functools.lru_cache(maxsize=None)
def maps(H, W, depth_kind, opacity_kind, inv_depth):
    """float32 (normal [3, H, W], depth [H, W], opacity [H, W]) as the rasterizer would render them."""
    z, O = make_z(depth_kind, H, W), make_opacity(opacity_kind, H, W)
    D = (O / z if inv_depth else O * z).float()
    g = torch.Generator().manual_seed(4000 + H * 43 + W)
    N = torch.randn(3, H, W, generator=g) * O
    return N, D, O


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def float32_errors(H, W, tan, case, split=False):
    """What float32 itself holds on one case: (max |n_d32 - n_d64|, the largest of the three gradients' max |g32 - g64| / max |g64|)."""
    dk, ok, wk, inv = case
    N, D, O = maps(H, W, dk, ok, inv)
    w = make_weight(wk, H, W)
    n64, _ = ref.depth_normals(D.double(), O.double(), *tan, inv_depth=inv)
    n32, _ = ref.depth_normals(D, O, *tan, inv_depth=inv, split=split)
    r64 = ref.normal_consistency_with_grads(N, D, O, *tan, weight=w, inv_depth=inv)
    r32 = ref.normal_consistency_with_grads(N, D, O, *tan, weight=w, inv_depth=inv, dtype=torch.float32, split=split)
    return float((n32.double() - n64).abs().max()), max(rel(a, b) for a, b in zip(r32[1:], r64[1:]))
