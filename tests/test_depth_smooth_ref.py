"""Pins tests/depth_smooth_ref.py, the float64 yardstick of the depth smoothness kernels: autograd against central finite differences, the
closed-form gradient of include/adgs_loss.h against autograd, and answers known exactly."""
import itertools

import pytest
import torch

from tests import depth_smooth_ref as ref


def case(H, W, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = (0.05 + 0.3 * torch.rand(H, W, generator=g)).double()
    img = torch.rand(C, H, W, generator=g).double()
    w = (0.25 + 0.75 * torch.rand(H, W, generator=g)).double()
    return d, img, w


@pytest.mark.parametrize("order,normalize", list(itertools.product((1, 2), (False, True))))
def test_autograd_matches_central_differences(order, normalize):
    """5 x 7, random depth: every |delta| is far above the step, so no sign changes inside it."""
    d, img, w = case(5, 7)
    kw = dict(image=img, weight=w, order=order, normalize=normalize, edge_gamma=2.0)
    _, g = ref.value_and_grad(d, **kw)
    h = 1e-6
    for y, x in itertools.product(range(5), range(7)):
        e = torch.zeros_like(d)
        e[y, x] = h
        fd = (ref.loss(d + e, **kw) - ref.loss(d - e, **kw)) / (2 * h)
        assert abs(float(fd) - float(g[y, x])) <= 1e-7 * max(1.0, float(g.abs().max())), (y, x, float(fd), float(g[y, x]))


@pytest.mark.parametrize("shape", [(17, 33), (1, 7), (7, 1), (2, 2), (3, 3), (1, 1)])
@pytest.mark.parametrize("order,normalize,guided,weighted", list(itertools.product((1, 2), (False, True), (False, True), (False, True))))
def test_closed_form_gradient_matches_autograd(shape, order, normalize, guided, weighted):
    d, img, w = case(*shape, seed=3)
    kw = dict(image=img if guided else None, weight=w if weighted else None, order=order, normalize=normalize, edge_gamma=2.0)
    L, g = ref.value_and_grad(d, **kw)
    Lc, gc = ref.closed_form(d, **kw)
    assert float(L) == float(Lc)
    assert float((g - gc).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max()))


@pytest.mark.parametrize("order,normalize", list(itertools.product((1, 2), (False, True))))
def test_constant_depth_is_free(order, normalize):
    d, img, w = case(9, 11)
    L, g = ref.value_and_grad(torch.full((9, 11), 0.375), img, w, order, normalize, 1.0)
    assert float(L) == 0.0 and float(g.abs().max()) == 0.0


def test_squares_along_x_order_one():
    """d(y, x) = x^2 with the columns counted from 1: |delta| = 2 x + 1 for x = 1 .. W - 1, whose mean is W + 1; nothing along y.
    (With the columns counted from 0 the same image gives W - 1.)"""
    for H, W in ((4, 9), (17, 33)):
        x = torch.arange(1, W + 1, dtype=torch.float64)
        L, _ = ref.value_and_grad((x * x).expand(H, W), order=1, normalize=False)
        assert float(L) == W + 1
        x0 = torch.arange(W, dtype=torch.float64)
        assert float(ref.value_and_grad((x0 * x0).expand(H, W), order=1, normalize=False)[0]) == W - 1


@pytest.mark.parametrize("normalize", (False, True))
def test_dyadic_plane_is_free_at_order_two(normalize):
    d, img, w = case(18, 66)
    y, x = torch.meshgrid(torch.arange(18.0), torch.arange(66.0), indexing="ij")
    plane = ((3 + 0.25 * x + 0.5 * y) / 64).float()
    for kw in (dict(), dict(image=img, weight=w)):
        L, g = ref.value_and_grad(plane, order=2, normalize=normalize, **kw)
        assert float(L) == 0.0 and float(g.abs().max()) == 0.0
    assert float(ref.value_and_grad(plane, order=1, normalize=normalize)[0]) > 0          # order 1 does penalise the slant


@pytest.mark.parametrize("order,normalize", list(itertools.product((1, 2), (False, True))))
def test_gamma_zero_is_no_guide(order, normalize):
    d, img, w = case(13, 17)
    L0, g0 = ref.value_and_grad(d, img, w, order, normalize, 0.0)
    L1, g1 = ref.value_and_grad(d, None, w, order, normalize, 1.0)
    assert float(L0) == float(L1) and torch.equal(g0, g1)


@pytest.mark.parametrize("order", (1, 2))
def test_normalised_loss_ignores_the_scale_of_the_depth(order):
    """to 1e-6 relative, not exactly: the 1e-7 added to the mean does not scale"""
    d, img, w = case(13, 17)
    L1, _ = ref.value_and_grad(d, img, w, order, True, 1.0)
    L2, _ = ref.value_and_grad(2 * d, img, w, order, True, 1.0)
    assert abs(float(L2) - float(L1)) <= 1e-6 * float(L1)
    assert float(ref.value_and_grad(2 * d, img, w, order, False, 1.0)[0]) == pytest.approx(2 * float(ref.value_and_grad(d, img, w, order, False, 1.0)[0]), rel=1e-14)


def test_zero_weight_and_short_axes():
    d, img, w = case(5, 7)
    L, g = ref.value_and_grad(d, img, torch.zeros(5, 7), 2, True, 1.0)
    assert float(L) == 0.0 and float(g.abs().max()) == 0.0
    for order, shape in ((1, (1, 1)), (2, (2, 2)), (2, (1, 2))):
        assert float(ref.value_and_grad(0.1 + torch.rand(*shape), order=order)[0]) == 0.0
    # one axis too short: the other one alone
    row = (0.1 + torch.rand(1, 7)).double()
    assert float(ref.value_and_grad(row, order=2, normalize=False)[0]) == pytest.approx(float((row[0, :-2] - 2 * row[0, 1:-1] + row[0, 2:]).abs().mean()), rel=1e-14)
