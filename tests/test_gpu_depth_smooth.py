"""The edge-aware depth smoothness term (adgs.loss.depth_smoothness_loss, csrc/depth_smooth.hip) on the GPU against tests/depth_smooth_ref.py
(float64 torch-CPU, autograd): values at rtol 1e-5, gradients at atol = 1e-4 max|ref| (the tolerances of tests/test_gpu_loss.py and
tests/test_gpu_masked_loss.py for this kernel family), no element exempt.

The kernels work on 32 x 16 tiles (x by y) with a halo of 1 (order 1) or 2 (order 2); the shapes are the smallest at which that stencil can go
wrong: axes with no pair or triple; exactly one tile; one-pixel partial tiles, where terms straddle both tile borders; the order-2 halo crossing a
border; several partial tiles; and 11 x 33 = 363 workgroups, more than the 256 slot rows.  Every small shape runs the full product of
order x normalize x guide {none, C = 1, C = 3} x edge_gamma {0, 1, 4} x weight kind x upstream gradient {1, -1.3} (edge_gamma only matters
with a guide); the 165 k pixel shape runs every weight kind and every guide once per order.  A reference is computed once per case and
shared by both upstream gradients (the gradient is linear in it)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import depth_smooth_ref as ref

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (16, 32), (17, 33), (16, 64), (18, 66), (37, 121)]
LARGE = (161, 1025)
WEIGHTS = (None, "ones", "zeros", "binary", "fractional", "zero_rows", "corner_pixel")
GUIDES = [(0, 1.0)] + [(C, gamma) for C in (1, 3) for gamma in (0.0, 1.0, 4.0)]          # (channels, edge_gamma)
UPSTREAM = (1.0, -1.3)


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
    if kind == "zero_rows":                                    # the ego vehicle: the bottom rows (from a row inside a tile, so triples straddle the cut)
        w = torch.ones(H, W)
        w[H - max(H // 3, 1):] = 0
        return w
    if kind == "corner_pixel":
        w = torch.zeros(H, W)
        w[H - 1, W - 1] = 0.75
        return w
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def inputs(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    return 0.05 + 0.3 * torch.rand(H, W, generator=g), torch.rand(3, H, W, generator=g)


def run_gpu(d, img, w, order, normalize, gamma, upstream=1.0):
    from adgs import loss
    x = d.cuda().requires_grad_(True)
    L = loss.depth_smoothness_loss(x, None if img is None else img.cuda(), None if w is None else w.cuda(), order=order, normalize=normalize, edge_gamma=gamma)
    (L * upstream).backward()
    return L.item(), x.grad.cpu().double().numpy()


def check_case(H, W, order, normalize, C, gamma, kind):
    d, img3 = inputs(H, W)
    img, w = (img3[:C] if C else None), make_weight(kind, H, W)
    rL, rg = ref.value_and_grad(d, img, w, order, normalize, gamma)
    rL, rg = float(rL), rg.numpy()
    what = dict(shape=(H, W), order=order, normalize=normalize, C=C, gamma=gamma, weight=kind)
    for up in UPSTREAM:
        L, g = run_gpu(d, img, w, order, normalize, gamma, up)
        assert abs(L - rL) <= 1e-5 * abs(rL), (what, L, rL)
        assert np.isfinite(g).all(), what
        np.testing.assert_allclose(g, up * rg, rtol=0, atol=1e-4 * np.abs(rg).max() * abs(up), err_msg=str((what, up)))
        if kind == "zeros":
            assert L == 0.0 and not g.any(), what
        if w is not None and not normalize:
            assert not g[w.numpy() == 0].any(), what          # exactly zero wherever the weight is


@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_values_and_gradients(shape, order):
    for normalize, (C, gamma), kind in itertools.product((False, True), GUIDES, WEIGHTS):
        check_case(*shape, order, normalize, C, gamma, kind)


@pytest.mark.parametrize("order", (1, 2))
def test_more_workgroups_than_slot_rows(order):
    """161 x 1025: 11 x 33 = 363 workgroups of 32 x 16 pixels; every weight kind and every guide once"""
    cases = [(True, 3, 1.0, "fractional"), (False, 3, 4.0, "binary"), (True, 1, 1.0, "zero_rows"), (False, 0, 1.0, None), (True, 0, 1.0, "ones"),
             (True, 1, 0.0, "zeros"), (False, 3, 1.0, "corner_pixel")]
    for normalize, C, gamma, kind in cases:
        check_case(*LARGE, order, normalize, C, gamma, kind)


def dyadic_depth(H, W):
    """multiples of 1/256: every difference, product with a unit weight and partial sum is exact, whatever order the workgroups add in"""
    g = torch.Generator().manual_seed(H + W)
    return torch.randint(1, 64, (H, W), generator=g).float() / 256


@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("normalize", (False, True))
def test_exact_answers(order, normalize):
    H, W = 18, 66
    _, img = inputs(H, W)
    w = make_weight("fractional", H, W)
    # constant depth
    for kw in (dict(img=None, w=None), dict(img=img, w=w)):
        L, g = run_gpu(torch.full((H, W), 0.375), order=order, normalize=normalize, gamma=1.0, **kw)
        assert L == 0.0 and not g.any()
    # a dyadic plane: free at order 2, with and without guide and weight
    y, x = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    plane = (3 + 0.25 * x + 0.5 * y) / 64
    if order == 2:
        for kw in (dict(img=None, w=None), dict(img=img, w=w)):
            L, g = run_gpu(plane, order=2, normalize=normalize, gamma=1.0, **kw)
            assert L == 0.0 and not g.any()
    # edge_gamma = 0 with a guide is no guide
    d = dyadic_depth(H, W)
    L0, g0 = run_gpu(d, img, None, order, normalize, 0.0)
    L1, g1 = run_gpu(d, None, None, order, normalize, 1.0)
    assert L0 == L1 and np.array_equal(g0, g1)
    assert L0 == pytest.approx(float(ref.value_and_grad(d, None, None, order, normalize)[0]), rel=1e-6)


def test_squares_along_x():
    """d(y, x) = x^2, columns counted from 1, order 1, no normalisation: W + 1 exactly (tests/test_depth_smooth_ref.py); counted from 0: W - 1"""
    for H, W in ((17, 33), (4, 9)):
        x = torch.arange(1, W + 1, dtype=torch.float32)
        L, _ = run_gpu((x * x).expand(H, W).contiguous(), None, None, 1, False, 1.0)
        assert L == W + 1
        x0 = torch.arange(W, dtype=torch.float32)
        assert run_gpu((x0 * x0).expand(H, W).contiguous(), None, None, 1, False, 1.0)[0] == W - 1


@pytest.mark.parametrize("order", (1, 2))
def test_normalised_loss_ignores_the_scale_of_the_depth(order):
    """Doubling a float is exact and so is every float product and double sum of doubled terms: what remains is the 1e-7 added to the mean
    (2.5e-7 relative at a mean of 0.2) and the final rounding to float (6e-8): 1e-6 relative, as for the reference."""
    d, img = inputs(37, 121)
    w = make_weight("fractional", 37, 121)
    L1, _ = run_gpu(d, img, w, order, True, 1.0)
    L2, _ = run_gpu(2 * d, img, w, order, True, 1.0)
    assert abs(L2 - L1) <= 1e-6 * L1


def test_depth_layouts_repeated_backward_and_weighted_total():
    from adgs import loss
    H, W = 17, 33
    _, img = inputs(H, W)
    d, img, w = dyadic_depth(H, W).cuda(), img.cuda(), make_weight("binary", H, W).cuda()
    for order in (1, 2):
        a, b = d.clone().requires_grad_(True), d[None].clone().requires_grad_(True)
        La, Lb = (loss.depth_smoothness_loss(t, img, w, order=order) for t in (a, b))
        assert Lb.shape == () and torch.equal(La, Lb)
        La.backward(retain_graph=True)
        first = a.grad.clone()
        a.grad = None
        La.backward()                                              # a second backward of the same forward
        Lb.backward()
        assert torch.equal(first, a.grad) and b.grad.shape == (1, H, W) and torch.equal(b.grad[0], a.grad)
    # composes with weighted_total
    x = d.clone().requires_grad_(True)
    s1, s2 = loss.depth_smoothness_loss(x, img, w, order=1), loss.depth_smoothness_loss(x, img, order=2, normalize=False)
    total = loss.weighted_total([(0.1, s1), (0.05, s2)])
    assert total.item() == pytest.approx(0.1 * s1.item() + 0.05 * s2.item(), rel=1e-6)
    total.backward()
    g1, g2 = (ref.value_and_grad(d.cpu(), img.cpu(), ww, order, nz)[1] for ww, order, nz in ((w.cpu(), 1, True), (None, 2, False)))
    want = (0.1 * g1 + 0.05 * g2).numpy()
    np.testing.assert_allclose(x.grad.cpu().double().numpy(), want, rtol=0, atol=1e-4 * np.abs(want).max())
    # an empty image: zero, and an empty gradient
    e = torch.zeros(0, 5, device="cuda", requires_grad=True)
    Le = loss.depth_smoothness_loss(e)
    Le.backward()
    assert Le.item() == 0.0 and e.grad.shape == (0, 5)


def test_work_buffer_convention():
    """Through the library entry points: the slot rows are zero again after the forward, the totals sit behind them, and the backward reads them."""
    from adgs import _lib, loss
    H, W = 37, 121
    d, img = inputs(H, W)
    w = make_weight("fractional", H, W)
    dev = torch.device("cuda", torch.cuda.current_device())
    dd, gi, gw = d.cuda(), img.cuda(), w.cuda()
    work = torch.zeros(loss.SMOOTH_WORK_DOUBLES, dtype=torch.float64, device=dev)
    out, gl, grad = torch.empty(1, device=dev), torch.full((1,), -1.3, device=dev), torch.empty(H, W, device=dev)
    for order in (1, 2):
        for _ in range(2):                                         # the second forward finds the rows as the first one left them
            _lib.call("adgs_depth_smooth_forward", dev, H, W, 3, dd.data_ptr(), gi.data_ptr(), gw.data_ptr(), order, 1, 1.0, work.data_ptr(), out.data_ptr())
        _lib.call("adgs_depth_smooth_backward", dev, H, W, 3, dd.data_ptr(), gi.data_ptr(), gw.data_ptr(), order, 1, 1.0, work.data_ptr(), gl.data_ptr(), grad.data_ptr())
        rows, tot = work[:loss.SLOTS * 8].cpu(), work[loss.SLOTS * 8:].cpu().numpy()
        assert not rows.any()
        rL, rg = ref.value_and_grad(d, img, w, order, True, 1.0)
        wd = w.double()
        assert tot[0] == pytest.approx(float((wd * d.double()).sum()), rel=1e-6) and tot[1] == pytest.approx(float(wd.sum()), rel=1e-12)
        assert tot[6] == pytest.approx(1.0 / (float((wd * d.double()).sum() / wd.sum()) + 1e-7), rel=1e-6)
        assert tot[7] == pytest.approx(float(rL), rel=1e-5) and float(out) == pytest.approx(float(rL), rel=1e-5)
        np.testing.assert_allclose(grad.cpu().double().numpy(), -1.3 * rg.numpy(), rtol=0, atol=1.3e-4 * float(rg.abs().max()))
