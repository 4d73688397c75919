"""The two definitions of include/adgs_normals.h in float64 torch on the CPU, differentiated by autograd: the yardstick of
tests/test_gpu_normals.py, pinned by tests/test_normals_ref.py.  The *_with_grads entry and the Gaussian normals convert float32 inputs to float64 first; the map
functions evaluate in the dtype of the tensors they are given (float32 tensors: the float32 restatement).

Gaussian normal (per row):  qh = q / |q|, q = (w, x, y, z);  k = argmin of the three scales, the lowest index on ties;  n_w = R(qh)[:, k];
    n_c[j] = m[j] n_w.x + m[4 + j] n_w.y + m[8 + j] n_w.z  (m: the transposed view matrix, flattened);  p_c the same of the mean plus m[12 + j];
    out = n_c if n_c . p_c <= 0 else -n_c.

Consistency:  z = O / D (inv_depth) or D / O;  r(x, y) = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1);  P = z r;
    t_x = P(x + 1, y) - P(x - 1, y),  t_y = P(x, y + 1) - P(x, y - 1),  c = t_y x t_x,  n_d = c / sqrt(c . c + 1e-30),
    Nh = N / sqrt(N . N + 1e-12),  e = 1 - Nh . n_d;  m = interior and (O >= min_opacity and D > 0) at the pixel and its four neighbours;
    v = weight m;  L = sum v e / sum v, 0 when sum v = 0."""
import torch


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def rotation_matrix(qh):
    """R [N, 3, 3] of normalised quaternions [N, 4] (w, x, y, z)."""
    w, x, y, z = qh.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def shortest_axis(scales):
    """Index of the smallest scale per row, the lowest index on ties."""
    s = scales
    k = torch.zeros(s.shape[0], dtype=torch.long)
    best = s[:, 0].clone()
    for j in (1, 2):
        less = s[:, j] < best
        k[less] = j
        best = torch.where(less, s[:, j], best)
    return k


def gaussian_normals_parts(scales, rotations, means3D, viewmatrix):
    """(n_c un-flipped [N, 3], p_c [N, 3], k [N]) in float64; `rotations` may carry requires_grad (float64)."""
    s, p, m = _f64(scales), _f64(means3D), _f64(viewmatrix).reshape(4, 4)
    q = rotations if rotations.dtype == torch.float64 else _f64(rotations)
    R = rotation_matrix(q / q.norm(dim=-1, keepdim=True))
    k = shortest_axis(s)
    n_w = R[torch.arange(s.shape[0]), :, k]
    n_c = n_w @ m[:3, :3]                      # n_c[j] = sum_a n_w[a] m[4 a + j]
    p_c = p @ m[:3, :3] + m[3, :3]
    return n_c, p_c, k


def gaussian_normals(scales, rotations, means3D, viewmatrix):
    n_c, p_c, _ = gaussian_normals_parts(scales, rotations, means3D, viewmatrix)
    flip = (n_c.detach() * p_c).sum(-1) > 0
    return torch.where(flip[:, None], -n_c, n_c)


def rays(H, W, tanfovx, tanfovy, dtype=torch.float64):
    """[3, H, W]: the rasterizer's pixel-centre rays (formed in float64, handed out as `dtype`)."""
    x = ((2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1) * float(tanfovx)
    y = ((2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1) * float(tanfovy)
    return torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64)]).to(dtype)


def validity(depth, opacity, min_opacity):
    """m [H, W] bool."""
    ok = (opacity >= float(min_opacity)) & (depth > 0)
    H, W = ok.shape
    m = torch.zeros(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        m[1:-1, 1:-1] = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
    return m


def depth_normals(depth, opacity, tanfovx, tanfovy, inv_depth=True, min_opacity=0.5, split=False):
    """(m n_d [3, H, W], m [H, W]); depth / opacity: float64 [H, W] tensors (may require grad).  Float32 tensors are evaluated in
    float32 throughout: the float32 restatement whose error says what float32 itself can hold.  split: the tangents as (z+ - z-) r + (z+ + z-) dr, the form the
    header prescribes for float32 (the same numbers in exact arithmetic), instead of the difference of the two points."""
    H, W = depth.shape
    m = validity(depth.detach(), opacity.detach(), min_opacity)
    ok = (opacity.detach() >= float(min_opacity)) & (depth.detach() > 0)
    safe_d, safe_o = torch.where(ok, depth, torch.ones_like(depth)), torch.where(ok, opacity, torch.ones_like(opacity))
    z = safe_o / safe_d if inv_depth else safe_d / safe_o
    P = z[None] * rays(H, W, tanfovx, tanfovy, depth.dtype)
    n_d = torch.zeros(3, H, W, dtype=depth.dtype)
    if H >= 3 and W >= 3:
        if split:
            r = rays(H, W, tanfovx, tanfovy, depth.dtype)[:, 1:-1, 1:-1]
            dr = torch.tensor([2 * float(tanfovx) / W, 2 * float(tanfovy) / H], dtype=depth.dtype)
            zx, sx = z[1:-1, 2:] - z[1:-1, :-2], z[1:-1, 2:] + z[1:-1, :-2]
            zy, sy = z[2:, 1:-1] - z[:-2, 1:-1], z[2:, 1:-1] + z[:-2, 1:-1]
            t_x = torch.stack([zx * r[0] + sx * dr[0], zx * r[1], zx])
            t_y = torch.stack([zy * r[0], zy * r[1] + sy * dr[1], zy])
        else:
            t_x = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
            t_y = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
        c = torch.cross(t_y, t_x, dim=0)
        inner = c / torch.sqrt((c * c).sum(0, keepdim=True) + 1e-30)
        n_d = torch.nn.functional.pad(inner, (1, 1, 1, 1))
    return torch.where(m[None], n_d, torch.zeros_like(n_d)), m


def normal_consistency(normal, depth, opacity, tanfovx, tanfovy, weight=None, inv_depth=True, min_opacity=0.5, split=False):
    """L (float64 scalar); normal [3, H, W], depth / opacity [H, W]: float64 tensors (may require grad)."""
    n_d, m = depth_normals(depth, opacity, tanfovx, tanfovy, inv_depth, min_opacity, split)
    nh = normal / torch.sqrt((normal * normal).sum(0, keepdim=True) + 1e-12)
    e = 1.0 - (nh * n_d).sum(0)
    v = m.to(normal.dtype) * (1.0 if weight is None else weight.detach().to("cpu", normal.dtype).reshape(m.shape))
    sv = v.sum()
    if float(sv) <= 0:
        return (normal.sum() + depth.sum() + opacity.sum()) * 0.0
    return (torch.where(m, v * e, torch.zeros_like(e))).sum() / sv


def normal_consistency_with_grads(normal, depth, opacity, tanfovx, tanfovy, weight=None, inv_depth=True, min_opacity=0.5, dtype=torch.float64, split=False):
    """(L, dL/dnormal, dL/ddepth, dL/dopacity) in float64 from float32 or float64 inputs (dtype=torch.float32: the float32 restatement)."""
    n, d, o = (t.detach().to("cpu", dtype).clone().requires_grad_(True) for t in (normal, depth.reshape(depth.shape[-2:]), opacity.reshape(opacity.shape[-2:])))
    L = normal_consistency(n, d, o, tanfovx, tanfovy, weight, inv_depth, min_opacity, split)
    L.backward()
    return L.detach(), n.grad, d.grad, o.grad
