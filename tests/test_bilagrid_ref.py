"""The bilateral-grid reference against itself (no GPU): the restatement of include/adgs_bilagrid.h in tests/bilagrid_ref.py
against torch's grid_sample and autograd in float64, and the loader's view of the new entry points."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import bilagrid_ref as ref  # noqa: E402

CASES = [((8, 16, 16), (37, 121)), ((2, 2, 2), (16, 64)), ((3, 5, 7), (48, 200)), ((8, 4, 4), (3, 5))]


def _case(grid, image, seed=7):
    grids, img, d_out, planted = ref.make_case(*grid, *image, seed)
    return grids[1].double(), img.double(), d_out.double(), planted


@pytest.mark.parametrize("grid,image", CASES)
def test_forward_matches_grid_sample(grid, image):
    g, img, _, _ = _case(grid, image)
    a, b = ref.slice_forward(g, img), ref.grid_sample_form(g, img)
    assert (a - b).abs().max().item() < 1e-13


@pytest.mark.parametrize("grid,image", CASES)
def test_gradients_match_autograd(grid, image):
    g, img, d_out, planted = _case(grid, image)
    L = grid[0]
    gg, ii = g.clone().requires_grad_(True), img.clone().requires_grad_(True)
    (ref.grid_sample_form(gg, ii) * d_out).sum().backward()
    d_grid, d_image = ref.slice_backward(g, img, d_out)
    assert (d_grid - gg.grad).abs().max().item() < 1e-12 * max(1.0, gg.grad.abs().max().item())
    # the luma slope is discontinuous at the knots; at gray == 0 exactly torch takes the outer one-sided slope (0), the definition the inner
    v = ref.gray_of(img) * (L - 1)
    masked = ref.knot_mask(img, L) | (v == 0)
    assert masked.sum().item() <= max(1, 0.002 * masked.numel())
    err = (d_image - ii.grad).abs().amax(dim=0)
    assert err[~masked].max().item() < 1e-12 * max(1.0, ii.grad.abs().max().item())
    # the planted pixels above and below the range carry no luma slope and are compared
    flat = (~masked).reshape(-1)
    assert flat[planted[1]] and flat[planted[2]]


@pytest.mark.parametrize("N,grid", [(1, (2, 2, 2)), (3, (8, 16, 16)), (2, (3, 5, 7))])
def test_total_variation_matches_autograd(N, grid):
    gen = torch.Generator().manual_seed(3)
    grids = torch.randn(N, 12, *grid, generator=gen, dtype=torch.float64).requires_grad_(True)
    tv = ref.total_variation(grids)
    tv.backward()
    assert (ref.total_variation_grad(grids.detach()) - grids.grad).abs().max().item() < 1e-14
    # one image, one axis, by hand: mean over the 12 channels and the pairs of (difference)^2
    g0 = grids.detach()
    by_hand = sum(((g0[:, :, 1:] - g0[:, :, :-1]) ** 2).mean().item() if a == 2 else
                  ((g0[:, :, :, 1:] - g0[:, :, :, :-1]) ** 2).mean().item() if a == 3 else
                  ((g0[..., 1:] - g0[..., :-1]) ** 2).mean().item() for a in (2, 3, 4))
    assert abs(tv.item() - by_hand) < 1e-12 * by_hand


def test_identity_grid_returns_the_image():
    _, img, _, _ = _case((8, 16, 16), (37, 121))
    out = ref.slice_forward(ref.identity_grid(8, 16, 16), img)
    assert (out - img).abs().max().item() < 1e-15
    assert (ref.grid_sample_form(ref.identity_grid(8, 16, 16), img) - img).abs().max().item() < 1e-15


def test_library_exports_the_bilagrid_entry_points():
    from adgs import _lib
    lib = _lib.lib()
    for name in ("adgs_bilagrid_slice_forward", "adgs_bilagrid_slice_backward", "adgs_bilagrid_tv_forward", "adgs_bilagrid_tv_backward"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype is _lib.c_i
