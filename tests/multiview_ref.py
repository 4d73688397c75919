"""The definition of include/adgs_multiview.h (the plane-warped patch NCC) in float64 torch on the CPU, differentiated by autograd: the
yardstick of tests/test_gpu_multiview.py, pinned by tests/test_multiview_ref.py.  Inputs are converted to float64 first (float32 maps, and
the pose, the four tanfov values and the thresholds rounded to float32, as the C ABI receives them); dtype=torch.float32 evaluates the
same chain in float32 instead (the float32 restatement).

    r(x, y) = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)
    z = O / D (inv_depth) or D / O;  Nh = N / sqrt(N . N + 1e-12);  r0 = r(p);  c0 = Nh . r0
    tap k at q = p + (dx, dy), row-major over (dy, dx):  s_k = (Nh . r(q)) / (z c0);  m_k = R r(q) + t s_k
    u = (m.x / m.z) / tanfovx_n Wn / 2 + (Wn - 1) / 2,  v likewise;  b_k = bilinear I_n(u, v);  a_k = I_r(q)
    C = sum a b - Sa Sb / T, Va = sum a^2 - Sa^2 / T, Vb likewise;  e = 1 - C^2 / (Va Vb + eps)
    valid: index in the image, radius <= x0 < W - radius (y likewise), O >= min_opacity, D > 0, -c0 >= min_cos |r0|, every tap m.z > 1e-6 and
    0 <= u <= Wn - 1, 0 <= v <= Hn - 1, e < max_error (piecewise constant);  L = sum w v e / sum w v, 0 when the denominator is 0.

Validity is decided in a first pass without gradients; the differentiable chain then runs over the samples that pass every gate before
the error, so no gradient goes through a gate and none through an invalid sample."""
import collections

import torch

MARGINS = ("opacity", "cos", "border", "mz", "error")
Result = collections.namedtuple("Result", "L e valid geo margins")


def f32(x):
    """x rounded to float32, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def pose12(pose):
    """[3, 4] (R | t) -> (R [3, 3], t [3]) in float64, rounded to float32 first."""
    p = pose.detach().to("cpu", torch.float64).float().double()
    return p[:, :3].contiguous(), p[:, 3].contiguous()


def tap_offsets(radius):
    """(dx [T], dy [T]) row-major over (dy, dx)."""
    r = torch.arange(-radius, radius + 1)
    dy, dx = torch.meshgrid(r, r, indexing="ij")
    return dx.reshape(-1), dy.reshape(-1)


def ray_xy(x, y, H, W, tan, dtype=torch.float64):
    """The x and y components of the pixel-centre rays of integer pixel tensors (formed in float64, handed out as `dtype`)."""
    rx = ((2 * x.double() + 1) / W - 1) * tan[0]
    ry = ((2 * y.double() + 1) / H - 1) * tan[1]
    return rx.to(dtype), ry.to(dtype)


def bilinear(I, u, v):
    """I [Hn, Wn] at (u, v) inside [0, Wn - 1] x [0, Hn - 1]: xi = min(floor(u), Wn - 2), fx = u - xi, the same in v."""
    Hn, Wn = I.shape
    xi = u.detach().floor().long().clamp(0, max(Wn - 2, 0))
    yi = v.detach().floor().long().clamp(0, max(Hn - 2, 0))
    x1, y1 = (xi + 1).clamp(max=Wn - 1), (yi + 1).clamp(max=Hn - 1)
    fx, fy = u - xi.to(u.dtype), v - yi.to(v.dtype)
    i00, i01, i10, i11 = I[yi, xi], I[yi, x1], I[y1, xi], I[y1, x1]
    top, bot = i00 + fx * (i01 - i00), i10 + fx * (i11 - i10)
    return top + fy * (bot - top)


def warp(Ns, Ds, Os, x0, y0, view, radius, inv_depth, dtype=torch.float64):
    """The geometry of the samples at integer pixels (x0, y0) with N [S, 3], D, O [S]: a dict of z, Nh, c0, |r0| [S] and s, mz, u, v
    [S, T].  view = (H, W, Hn, Wn, tan, tan_n, R, t)."""
    H, W, Hn, Wn, tan, tan_n, R, t = view
    R, t = R.to(dtype), t.to(dtype)
    z = Os / Ds if inv_depth else Ds / Os
    Nh = Ns / (Ns * Ns).sum(-1, keepdim=True).add(1e-12).sqrt()
    r0x, r0y = ray_xy(x0, y0, H, W, tan, dtype)
    c0 = Nh[:, 0] * r0x + Nh[:, 1] * r0y + Nh[:, 2]
    r0n = (r0x * r0x + r0y * r0y + 1).sqrt()
    dx, dy = tap_offsets(radius)
    qx, qy = x0[:, None] + dx[None], y0[:, None] + dy[None]
    rqx, rqy = ray_xy(qx, qy, H, W, tan, dtype)
    s = (Nh[:, 0:1] * rqx + Nh[:, 1:2] * rqy + Nh[:, 2:3]) / (z * c0)[:, None]
    m = [R[i, 0] * rqx + R[i, 1] * rqy + R[i, 2] + t[i] * s for i in range(3)]
    u = (m[0] / m[2]) / tan_n[0] * (Wn / 2) + (Wn - 1) / 2
    v = (m[1] / m[2]) / tan_n[1] * (Hn / 2) + (Hn - 1) / 2
    return dict(z=z, Nh=Nh, c0=c0, r0n=r0n, s=s, mz=m[2], u=u, v=v, qx=qx, qy=qy, rqx=rqx, rqy=rqy)


def patch_error(a, b, eps):
    """PGSR's lncc over the last dimension: 1 - C^2 / (Va Vb + eps) from un-normalised sums."""
    T = a.shape[-1]
    Sa, Sb = a.sum(-1), b.sum(-1)
    C = (a * b).sum(-1) - Sa * Sb / T
    Va = (a * a).sum(-1) - Sa * Sa / T
    Vb = (b * b).sum(-1) - Sb * Sb / T
    return 1 - C * C / (Va * Vb + eps)


def evaluate(N, D, O, tan, ref_gray, nbr_gray, tan_n, pose, samples, weight=None, radius=3, inv_depth=True, min_opacity=0.5, min_cos=0.1,
             max_error=0.9, eps=1e-8, dtype=torch.float64):
    """-> Result(L, e [S], valid [S], geo [S], margins [S, 5]).  N [3, H, W], D, O [H, W] may be float64 leaves that require grad (L is
    then differentiable); everything else is a constant.  e is the error where every gate before the last holds (geo), else 0.
    margins[:, j] (MARGINS): O - min_opacity, -c0 / |r0| - min_cos, the smallest tap distance to the neighbour's border in pixels, the
    smallest m.z, |e - max_error|; +inf where an earlier gate has already failed (the later ones are not evaluated)."""
    N, D, O = (t if t.dtype == dtype and t.requires_grad else _f64(t).to(dtype) for t in (N, D, O))
    D, O = D.reshape(D.shape[-2:]), O.reshape(O.shape[-2:])
    Ir, In = _f64(ref_gray).to(dtype), _f64(nbr_gray).to(dtype)
    H, W = D.shape
    Hn, Wn = In.shape
    R, t = pose12(pose)
    view = (H, W, Hn, Wn, (f32(tan[0]), f32(tan[1])), (f32(tan_n[0]), f32(tan_n[1])), R, t)
    min_opacity, min_cos, max_error, eps = f32(min_opacity), f32(min_cos), f32(max_error), f32(eps)
    idx = samples.detach().cpu().long()
    S = idx.numel()
    inf = torch.full((S,), float("inf"), dtype=torch.float64)
    in_range = (idx >= 0) & (idx < H * W)
    safe = torch.where(in_range, idx, torch.zeros_like(idx))
    y0, x0 = safe // W, safe % W
    inner = in_range & (x0 >= radius) & (x0 < W - radius) & (y0 >= radius) & (y0 < H - radius)
    with torch.no_grad():
        Nd, Dd, Od = N.detach().reshape(3, -1)[:, safe].T, D.detach().reshape(-1)[safe], O.detach().reshape(-1)[safe]
        g = warp(Nd, Dd, Od, x0, y0, view, radius, inv_depth, dtype)
        m_op = torch.where(inner, (Od - min_opacity).double(), inf)
        ok = inner & (Od >= min_opacity) & (Dd > 0)
        m_cos = torch.where(ok, (-g["c0"] / g["r0n"] - min_cos).double(), inf)
        ok = ok & (-g["c0"] >= min_cos * g["r0n"])
        m_mz = torch.where(ok, g["mz"].min(-1).values.double(), inf)
        ok = ok & (g["mz"] > 1e-6).all(-1)
        u, v = g["u"], g["v"]
        border = torch.minimum(torch.minimum(u, Wn - 1 - u), torch.minimum(v, Hn - 1 - v)).min(-1).values
        m_border = torch.where(ok, border.double(), inf)
        geo = ok & ((u >= 0) & (u <= Wn - 1) & (v >= 0) & (v <= Hn - 1)).all(-1)
    k = geo.nonzero().reshape(-1)
    e = torch.zeros(S, dtype=dtype)
    valid = torch.zeros(S, dtype=torch.bool)
    m_err = inf.clone()
    L = torch.zeros((), dtype=dtype)
    if k.numel():
        sk = safe[k]
        gk = warp(N.reshape(3, -1)[:, sk].T, D.reshape(-1)[sk], O.reshape(-1)[sk], x0[k], y0[k], view, radius, inv_depth, dtype)
        a = Ir[gk["qy"], gk["qx"]]
        b = bilinear(In, gk["u"], gk["v"])
        ek = patch_error(a, b, eps)
        e = e.index_put((k,), ek)
        valid[k] = ek.detach() < max_error
        m_err[k] = (ek.detach() - max_error).abs().double()
        w = torch.ones(k.numel(), dtype=dtype) if weight is None else _f64(weight).to(dtype).reshape(-1)[sk]
        wv = w * valid[k].to(dtype)
        den = wv.sum()
        if float(den) > 0:
            L = (wv * ek).sum() / den
    return Result(L, e, valid, geo, torch.stack([m_op, m_cos, m_border, m_mz, m_err], dim=1))


def with_grads(N, D, O, *args, **kw):
    """evaluate() of float32 maps, with (gN [3, H, W], gD [H, W], gO [H, W]) of L in the evaluation's dtype: -> (Result, grads)."""
    dtype = kw.get("dtype", torch.float64)
    leaves = [_f64(t).to(dtype).requires_grad_(True) for t in (N, D.reshape(D.shape[-2:]), O.reshape(O.shape[-2:]))]
    res = evaluate(*leaves, *args, **kw)
    if res.L.requires_grad:
        res.L.backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]
    return res._replace(L=res.L.detach(), e=res.e.detach()), grads


def near_gate(margins, tol=1e-3):
    """[S] bool: a sample whose margin to any evaluated gate is below tol."""
    return (margins.abs() < tol).any(dim=1)
