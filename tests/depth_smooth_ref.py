"""The edge-aware depth smoothness term of include/adgs_loss.h (adgs_depth_smooth_forward) in float64 torch on the CPU, differentiated by
autograd: the yardstick of tests/test_gpu_depth_smooth.py, pinned by tests/test_depth_smooth_ref.py.

    Sw = sum w,  m = sum w d / Sw,  s = 1 / (m + 1e-7) with normalize, else 1
    order 1, x axis, x + 1 < W:       delta = d(x) - d(x+1),            v = w(x) w(x+1),         a = exp(-gamma (1/C) sum_c |I_c(x) - I_c(x+1)|)
    order 2, x axis, 1 <= x <= W - 2: delta = d(x-1) - 2 d(x) + d(x+1),  v = w(x-1) w(x) w(x+1),
                                      a = exp(-gamma (1/(2C)) sum_c (|I_c(x) - I_c(x-1)| + |I_c(x+1) - I_c(x)|))
    S = sum v a |delta|,  V = sum v  per axis (0 for an axis with V = 0);  L = s (S_x / V_x + S_y / V_y);  Sw = 0 gives L = 0

The differences are taken on the UN-normalised depth and s multiplies the total (differences of d * s lose the exact zeros of a plane to rounding).
Inputs may be float32: they are converted to float64 first, so delta has the sign the kernels' double-precision delta has."""
import torch


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _axis_terms(d, img, w, order, gamma, dim):
    """(delta, v, a) of every term along `dim` of the [H, W] planes (the guide is [C, H, W]: its `dim` is shifted by one), or None."""
    n = d.shape[dim]
    if n <= order:
        return None
    cut = lambda t, k, dm=dim: t.narrow(dm, k, n - order)
    if order == 1:
        delta = cut(d, 0) - cut(d, 1)
        v = cut(w, 0) * cut(w, 1)
        e = None if img is None else (cut(img, 0, dim + 1) - cut(img, 1, dim + 1)).abs().mean(0)
    else:
        delta = cut(d, 0) - 2.0 * cut(d, 1) + cut(d, 2)
        v = cut(w, 0) * cut(w, 1) * cut(w, 2)
        e = None if img is None else ((cut(img, 1, dim + 1) - cut(img, 0, dim + 1)).abs() + (cut(img, 2, dim + 1) - cut(img, 1, dim + 1)).abs()).mean(0) / 2.0
    a = torch.ones_like(v) if e is None else torch.exp(-gamma * e)
    return delta, v, a


def loss(d, image=None, weight=None, order=1, normalize=True, edge_gamma=1.0):
    """L as a float64 scalar tensor; d is a float64 [H, W] tensor (differentiable), image [C, H, W] and weight [H, W] float64 constants."""
    w = torch.ones_like(d) if weight is None else weight
    sw = w.sum()
    if float(sw) == 0.0:
        return d.sum() * 0.0
    s = 1.0 / ((w * d).sum() / sw + 1e-7) if normalize else 1.0
    total = d.sum() * 0.0
    for dim in (1, 0):
        terms = _axis_terms(d, image, w, order, edge_gamma, dim)
        if terms is None:
            continue
        delta, v, a = terms
        V = v.sum()
        if float(V) != 0.0:
            total = total + (v * a * delta.abs()).sum() / V
    return s * total


def value_and_grad(depth, image=None, weight=None, order=1, normalize=True, edge_gamma=1.0):
    """(L, dL/dd) as float64 CPU tensors ([] and [H, W]) by autograd; depth [H, W] or [1, H, W] of any float dtype."""
    d = _f64(depth).reshape(depth.shape[-2:]).clone().requires_grad_(True)
    L = loss(d, _f64(image), _f64(weight), order, normalize, edge_gamma)
    (g,) = torch.autograd.grad(L, d)
    return L.detach(), g


def closed_form(depth, image=None, weight=None, order=1, normalize=True, edge_gamma=1.0):
    """(L, dL/dd) with the gradient written out as the kernels compute it:
    dL/dd_p = s (G_p - [normalize] (w_p / Sw) L),  G_p = sum over the terms that contain p of coefficient sign(delta) v a / V."""
    d, img, w = _f64(depth).reshape(depth.shape[-2:]), _f64(image), _f64(weight)
    w = torch.ones_like(d) if w is None else w
    L = loss(d, img, w, order, normalize, edge_gamma)
    sw = w.sum()
    G = torch.zeros_like(d)
    if float(sw) == 0.0:
        return L, G
    s = 1.0 / ((w * d).sum() / sw + 1e-7) if normalize else 1.0
    for dim in (1, 0):
        terms = _axis_terms(d, img, w, order, edge_gamma, dim)
        if terms is None:
            continue
        delta, v, a = terms
        V = v.sum()
        if float(V) == 0.0:
            continue
        c = torch.sign(delta) * v * a / V
        n = d.shape[dim] - order
        for k, coeff in enumerate((1.0, -1.0) if order == 1 else (1.0, -2.0, 1.0)):
            G.narrow(dim, k, n).add_(coeff * c)
    return L, s * (G - (w / sw * L if normalize else 0.0))
