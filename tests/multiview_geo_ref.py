"""The definition of include/adgs_multiview_geo.h (the depth reprojection error between two renders) in float64 torch on the CPU,
differentiated by autograd: the yardstick of tests/test_gpu_multiview_geo.py, pinned by tests/test_multiview_geo_ref.py.  Inputs are
converted to float64 first (float32 maps, and the pose, the four tanfov values and the thresholds rounded to float32, as the C ABI
receives them); dtype=torch.float32 evaluates the same chain in float32 instead (the float32 restatement).

    r(x, y) = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)
    the pixel of m in a view of size (W, H): ((m.x / m.z) / tanfovx W / 2 + (W - 1) / 2, (m.y / m.z) / tanfovy H / 2 + (H - 1) / 2)
    1. z = O / D (inv_depth) or D / O;  X = z r(p);  Y = R X + t;  (u, v) = the neighbour's pixel of Y
    2. xi = min(floor(u), Wn - 2), fx = u - xi, the same in v; z_c = On_c / Dn_c or Dn_c / On_c at the four corners;
       top = z00 + fx (z01 - z00), bot likewise, zh = top + fy (bot - top)
    3. Y' = Y / Y.z zh    4. X' = R^T (Y' - t)    5. (x', y') = the reference view's pixel of X'
    6. err = sqrt((x' - x)^2 + (y' - y)^2), derivative 0 at err == 0
    valid: O >= min_opacity, D > 0, Y.z > 1e-6, 0 <= u <= Wn - 1, 0 <= v <= Hn - 1, the four corners On_c >= min_opacity and Dn_c > 0,
    X'.z > 1e-6, err < max_pixel_error (piecewise constant);  g = exp(-err) detached;  L = sum w v g err / sum w v, 0 when the
    denominator is 0.

Validity is decided in a first pass without gradients; the differentiable chain then runs over the pixels that pass every gate before
the error, so no gradient goes through a gate and none through an invalid pixel."""
import collections

import torch

from tests.multiview_ref import _f64, f32, pose12, ray_xy

MARGINS = ("opacity", "mz", "border", "nbr_opacity", "xz", "error")
Result = collections.namedtuple("Result", "L err valid geo gw margins")


def pixel_of(mx, my, mz, H, W, tan):
    return (mx / mz) / tan[0] * (W / 2) + (W - 1) / 2, (my / mz) / tan[1] * (H / 2) + (H - 1) / 2


def cell(u, v, Hn, Wn):
    """The bilinear cell of (u, v) inside [0, Wn - 1] x [0, Hn - 1]: (xi, yi, x1, y1, fx, fy)."""
    xi = u.detach().floor().long().clamp(0, max(Wn - 2, 0))
    yi = v.detach().floor().long().clamp(0, max(Hn - 2, 0))
    x1, y1 = (xi + 1).clamp(max=Wn - 1), (yi + 1).clamp(max=Hn - 1)
    return xi, yi, x1, y1, u - xi.to(u.dtype), v - yi.to(v.dtype)


def project(Ds, Os, x, y, view, inv_depth, dtype):
    """Step 1 for the pixels (x, y) with D, O [P]: (rx, ry, Y [3 x P], u, v)."""
    H, W, Hn, Wn, tan, tan_n, R, t = view
    z = Os / Ds if inv_depth else Ds / Os
    rx, ry = ray_xy(x, y, H, W, tan, dtype)
    X = (z * rx, z * ry, z)
    Y = [R[i, 0] * X[0] + R[i, 1] * X[1] + R[i, 2] * X[2] + t[i] for i in range(3)]
    u, v = pixel_of(Y[0], Y[1], Y[2], Hn, Wn, tan_n)
    return Y, u, v


def round_trip(Ds, Os, Dn, On, x, y, view, inv_depth, dtype):
    """Steps 1 to 6 for pixels that land inside the neighbour's image: (err, dx, dy, X'.z)."""
    H, W, Hn, Wn, tan, tan_n, R, t = view
    Y, u, v = project(Ds, Os, x, y, view, inv_depth, dtype)
    xi, yi, x1, y1, fx, fy = cell(u, v, Hn, Wn)
    zn = On / Dn if inv_depth else Dn / On
    z00, z01, z10, z11 = zn[yi, xi], zn[yi, x1], zn[y1, xi], zn[y1, x1]
    top, bot = z00 + fx * (z01 - z00), z10 + fx * (z11 - z10)
    zh = top + fy * (bot - top)
    Yp = (Y[0] / Y[2] * zh, Y[1] / Y[2] * zh, zh)
    q = [Yp[i] - t[i] for i in range(3)]
    Xp = [R[0, i] * q[0] + R[1, i] * q[1] + R[2, i] * q[2] for i in range(3)]
    xp, yp = pixel_of(Xp[0], Xp[1], Xp[2], H, W, tan)
    dx, dy = xp - x.to(dtype), yp - y.to(dtype)
    sq = dx * dx + dy * dy
    pos = sq.detach() > 0
    err = torch.where(pos, torch.where(pos, sq, torch.ones_like(sq)).sqrt(), torch.zeros_like(sq))     # derivative 0 at err == 0
    return err, dx, dy, Xp[2]


def evaluate(D, O, tan, Dn, On, tan_n, pose, weight=None, inv_depth=True, min_opacity=0.5, max_pixel_error=1.0, dtype=torch.float64, frozen=None):
    """-> Result(L, err [H, W], valid [H, W], geo [H, W], gw [H, W], margins [H, W, 6]).  D, O [H, W] and Dn, On [Hn, Wn] may be leaves of
    `dtype` that require grad (L is then differentiable); everything else is a constant.  err is the error where every gate before the
    last holds (geo), else 0; gw = valid exp(-err).  margins[..., j] (MARGINS): O - min_opacity, Y.z - 1e-6, the distance of (u, v) to
    the neighbour's border in pixels, the smallest On_c - min_opacity of the four corners, X'.z - 1e-6, |err - max_pixel_error|; +inf
    where an earlier gate has already failed (the later ones are not evaluated).  frozen: a Result whose valid and gw replace this
    evaluation's (for finite differences of the function autograd differentiates)."""
    D, O, Dn, On = (t if t.dtype == dtype and t.requires_grad else _f64(t).to(dtype) for t in (D, O, Dn, On))
    D, O, Dn, On = (t.reshape(t.shape[-2:]) for t in (D, O, Dn, On))
    H, W = D.shape
    Hn, Wn = Dn.shape
    R, t = pose12(pose)
    view = (H, W, Hn, Wn, (f32(tan[0]), f32(tan[1])), (f32(tan_n[0]), f32(tan_n[1])), R.to(dtype), t.to(dtype))
    min_opacity, max_pixel_error = f32(min_opacity), f32(max_pixel_error)
    y, x = (g.reshape(-1) for g in torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij"))
    P = H * W
    inf = torch.full((P,), float("inf"), dtype=torch.float64)
    Df, Of = D.reshape(-1), O.reshape(-1)
    with torch.no_grad():
        m_op = (Of.detach() - min_opacity).double()
        ok = (Of >= min_opacity) & (Df > 0)
        one = torch.ones_like(Df)
        Y, u, v = project(torch.where(ok, Df, one), torch.where(ok, Of, one), x, y, view, inv_depth, dtype)
        m_mz = torch.where(ok, (Y[2] - 1e-6).double(), inf)
        ok = ok & (Y[2] > 1e-6)
        border = torch.minimum(torch.minimum(u, Wn - 1 - u), torch.minimum(v, Hn - 1 - v))
        m_border = torch.where(ok, border.double(), inf)
        ok = ok & (u >= 0) & (u <= Wn - 1) & (v >= 0) & (v <= Hn - 1)
        us, vs = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
        xi, yi, x1, y1, _, _ = cell(us, vs, Hn, Wn)
        corners = ((yi, xi), (yi, x1), (y1, xi), (y1, x1))
        On_min = torch.stack([On.detach()[c] for c in corners]).min(0).values
        Dn_min = torch.stack([Dn.detach()[c] for c in corners]).min(0).values
        m_nop = torch.where(ok, (On_min - min_opacity).double(), inf)
        ok = ok & (On_min >= min_opacity) & (Dn_min > 0)
    k = ok.nonzero().reshape(-1)
    err = torch.zeros(P, dtype=dtype)
    geo = torch.zeros(P, dtype=torch.bool)
    valid = torch.zeros(P, dtype=torch.bool)
    gw = torch.zeros(P, dtype=dtype)
    m_xz, m_err = inf.clone(), inf.clone()
    L = torch.zeros((), dtype=dtype)
    if k.numel():
        ek, _, _, xz = round_trip(Df[k], Of[k], Dn, On, x[k], y[k], view, inv_depth, dtype)
        m_xz[k] = (xz.detach() - 1e-6).double()
        front = xz.detach() > 1e-6
        k, ek = k[front], ek[front]
        geo[k] = True
        err = err.index_put((k,), ek)
        m_err[k] = (ek.detach() - max_pixel_error).abs().double()
        valid[k] = ek.detach() < max_pixel_error
        gw[k] = torch.where(valid[k], torch.exp(-ek.detach()), torch.zeros_like(ek.detach()))
        if frozen is not None:
            valid, gw = frozen.valid.reshape(-1), frozen.gw.reshape(-1).to(dtype)
        w = torch.ones(k.numel(), dtype=dtype) if weight is None else _f64(weight).to(dtype).reshape(-1)[k]
        den = (w * valid[k].to(dtype)).sum()
        if float(den) > 0:
            L = (w * gw[k] * ek).sum() / den
    margins = torch.stack([m_op, m_mz, m_border, m_nop, m_xz, m_err], dim=1)
    return Result(L, err.reshape(H, W), valid.reshape(H, W), geo.reshape(H, W), gw.reshape(H, W), margins.reshape(H, W, len(MARGINS)))


def with_grads(D, O, tan, Dn, On, *args, **kw):
    """evaluate() of float32 maps, with (gD, gO [H, W], gDn, gOn [Hn, Wn]) of L in the evaluation's dtype: -> (Result, grads)."""
    dtype = kw.get("dtype", torch.float64)
    leaves = [_f64(t).reshape(t.shape[-2:]).to(dtype).requires_grad_(True) for t in (D, O, Dn, On)]
    res = evaluate(leaves[0], leaves[1], tan, leaves[2], leaves[3], *args, **kw)
    if res.L.requires_grad:
        res.L.backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]
    return res._replace(L=res.L.detach(), err=res.err.detach()), grads


def near_gate(margins, tol=1e-3):
    """[H, W] bool: a pixel whose margin to any evaluated gate is below tol."""
    return (margins.abs() < tol).any(dim=-1)
