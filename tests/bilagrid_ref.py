"""Reference of the bilateral-grid slice (include/adgs_bilagrid.h), written from the definition: a restatement with explicit
corners, weights and hand-derived gradients (torch tensors, any float dtype; the tests use float64), and the same function as
torch's own 5-D grid_sample followed by the affine map (differentiable through autograd).  Nothing here touches the HIP library."""
import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)


def identity_grid(L, Hg, Wg, dtype=torch.float64):
    g = torch.zeros(12, L, Hg, Wg, dtype=dtype)
    g[[0, 5, 10]] = 1.0
    return g


def gray_of(image):
    return LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]


def _axis(n, cells, dtype):
    """cell and fraction of the n pixel centres along an axis of `cells` nodes"""
    g = (torch.arange(n, dtype=dtype) + 0.5) / n * (cells - 1)
    c = torch.clamp(torch.floor(g), max=cells - 2)
    return c.long(), g - c


def _taps(grid, image):
    L, Hg, Wg = grid.shape[1:]
    H, W = image.shape[1:]
    dt = image.dtype
    x0, fx = _axis(W, Wg, dt)
    y0, fy = _axis(H, Hg, dt)
    x0, fx = x0[None, :].expand(H, W), fx[None, :].expand(H, W)
    y0, fy = y0[:, None].expand(H, W), fy[:, None].expand(H, W)
    v = gray_of(image) * (L - 1)
    gz = torch.clamp(v, 0, L - 1)
    z0 = torch.clamp(torch.floor(gz), max=L - 2)
    fz = gz - z0
    slope = ((v >= 0) & (v <= L - 1)).to(dt)
    return (x0, y0, z0.long()), (fx, fy, fz), slope


def _corners(grid, cells, fracs):
    """yields (flat index into [L Hg Wg], x-y weight, z weight, dz) of the 8 corners, each [H, W]"""
    L, Hg, Wg = grid.shape[1:]
    (x0, y0, z0), (fx, fy, fz) = cells, fracs
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                yield ((z0 + dz) * Hg + (y0 + dy)) * Wg + (x0 + dx), (fx if dx else 1 - fx) * (fy if dy else 1 - fy), (fz if dz else 1 - fz), dz


def affine_field(grid, image):
    """A [12, H, W] and dA/dgz [12, H, W] (the slope inside the cell [z0, z0 + 1])"""
    cells, fracs, _ = _taps(grid, image)
    flat = grid.reshape(12, -1)
    A = torch.zeros(12, *image.shape[1:], dtype=image.dtype)
    dA = torch.zeros_like(A)
    for idx, wxy, wz, dz in _corners(grid, cells, fracs):
        val = flat[:, idx.reshape(-1)].reshape(12, *idx.shape)
        A += wxy * wz * val
        dA += (1 if dz else -1) * wxy * val
    return A, dA


def slice_forward(grid, image):
    """grid [12, L, Hg, Wg], image [3, H, W] -> out [3, H, W]"""
    A, _ = affine_field(grid, image)
    r, g, b = image
    return torch.stack([A[4 * i] * r + A[4 * i + 1] * g + A[4 * i + 2] * b + A[4 * i + 3] for i in range(3)])


def slice_backward(grid, image, d_out):
    """(dL/dgrid [12, L, Hg, Wg], dL/dimage [3, H, W]) for the upstream gradient d_out [3, H, W]"""
    L = grid.shape[1]
    cells, fracs, slope = _taps(grid, image)
    A, dA = affine_field(grid, image)
    r, g, b = image
    m = [r, g, b, torch.ones_like(r)]
    d_grid = torch.zeros(12, grid[0].numel(), dtype=grid.dtype)
    for idx, wxy, wz, _ in _corners(grid, cells, fracs):
        for i in range(3):
            for j in range(4):
                d_grid[4 * i + j].index_add_(0, idx.reshape(-1), (wxy * wz * d_out[i] * m[j]).reshape(-1))
    through_z = sum(d_out[i] * (dA[4 * i] * r + dA[4 * i + 1] * g + dA[4 * i + 2] * b + dA[4 * i + 3]) for i in range(3)) * slope * (L - 1)
    d_image = torch.stack([sum(d_out[i] * A[4 * i + k] for i in range(3)) + LUMA[k] * through_z for k in range(3)])
    return d_grid.reshape(grid.shape), d_image


def grid_sample_form(grid, image):
    """The same function through F.grid_sample (bilinear, border padding, align_corners=True) at (x, y, gray) * 2 - 1."""
    H, W = image.shape[1:]
    dt = image.dtype
    x = ((torch.arange(W, dtype=dt) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=dt) + 0.5) / H)[:, None].expand(H, W)
    coords = torch.stack([x, y, gray_of(image)], dim=-1) * 2 - 1
    A = F.grid_sample(grid[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    r, g, b = image
    return torch.stack([A[4 * i] * r + A[4 * i + 1] * g + A[4 * i + 2] * b + A[4 * i + 3] for i in range(3)])


def total_variation(grids):
    """grids [N, 12, L, Hg, Wg]: (1 / N) sum_n sum_axis mean over channels and adjacent pairs of (difference)^2"""
    tv = 0
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        d = grids.narrow(axis, 1, n - 1) - grids.narrow(axis, 0, n - 1)
        tv = tv + (d * d).mean(dim=(1, 2, 3, 4)).sum()
    return tv / grids.shape[0]


def total_variation_grad(grids):
    """d total_variation / d grids by hand: every element gathers from its two neighbours along each axis"""
    N = grids.shape[0]
    out = torch.zeros_like(grids)
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        d = grids.narrow(axis, 1, n - 1) - grids.narrow(axis, 0, n - 1)
        w = 2.0 / (N * d[0].numel())
        out.narrow(axis, 1, n - 1).add_(w * d)
        out.narrow(axis, 0, n - 1).sub_(w * d)
    return out


def knot_mask(image, L, tol=1e-4):
    """pixels with |gray (L - 1) - k| <= tol for an integer k in 1 .. L - 1: the luma slope is discontinuous there"""
    v = gray_of(image.double()) * (L - 1)
    k = torch.round(v)
    return ((v - k).abs() <= tol) & (k >= 1) & (k <= L - 1)


GRIDS = ((2, 2, 2), (3, 5, 7), (8, 4, 4), (8, 16, 16))
IMAGES = ((1, 1), (3, 5), (16, 64), (37, 121), (48, 200), (28, 110))


def make_case(L, Hg, Wg, H, W, seed, N=3):
    """The inputs of one comparison, generated in float32 (what the kernels are given; the references widen them): image uniform in
    [-0.2, 1.3] with three planted pixels where the image has room for them -- exactly zero, gray = 2.0 (above the grid's range) and a
    negative gray --, grids = identity + 0.3 N(0, 1), and a random upstream gradient N(0.5, 1).  Returns (grids [N, 12, L, Hg, Wg], image, d_out,
    planted flat pixel indices)."""
    gen = torch.Generator().manual_seed(seed)
    image = torch.rand(3, H, W, generator=gen, dtype=torch.float32) * 1.5 - 0.2
    n = H * W
    planted = []
    if n >= 3:
        planted = [0, n // 2, n - 1]
        flat = image.reshape(3, n)
        flat[:, planted[0]] = 0.0
        flat[:, planted[1]] = 2.0
        flat[:, planted[2]] = -0.15
    grids = identity_grid(L, Hg, Wg, torch.float32)[None] + 0.3 * torch.randn(N, 12, L, Hg, Wg, generator=gen, dtype=torch.float32)
    d_out = torch.randn(3, H, W, generator=gen, dtype=torch.float32) + 0.5        # off zero mean: sums of it are well-conditioned
    return grids, image, d_out, planted
