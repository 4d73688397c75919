"""The normal-map geometry prior on the HIP path (include/adgs_normals.h): per-Gaussian camera-space normals for the rasterizer's
semantic channels, the normals of a rendered depth map, and the consistency loss between the two (2DGS, GOF, PGSR and the street-scene
trainers built on them).

`gaussian_normals` builds the [N, 3] (or, with the object mask, [N, 4]) tensor `gaussian_renderer.render()` hands to the rasterizer as
`semantic` under pipe.render_normals, in one kernel with an analytic backward to the rotations; `normal_consistency_loss` ties the blended
normal map to the surface the rendered depth describes, one stencil pass forward and one gather backward; `depth_to_normal` is the
forward-only depth normal map for visualisation and evaluation.  There is no CPU fallback.
"""
import math

import torch

from . import _lib
from .loss import SLOTS, _check_weight, _g1, _ptr, _scalar, _work

NORMAL_WORK_DOUBLES = 256 * 2 + 4        # ADGS_NORMAL_WORK_DOUBLES


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotations, scales, means3D, viewmatrix, mask):
        N = rotations.shape[0]
        c0 = 0 if mask is None else 1
        out = torch.empty((N, c0 + 3), dtype=torch.float32, device=rotations.device)
        if N:
            _lib.call("adgs_gaussian_normals_forward", out.device, N, scales.data_ptr(), rotations.data_ptr(), means3D.data_ptr(), viewmatrix.data_ptr(),
                      _ptr(mask), c0 + 3, c0, out.data_ptr())
        ctx.c0 = c0
        ctx.save_for_backward(rotations, scales, means3D, viewmatrix)
        return out

    @staticmethod
    def backward(ctx, g_out):
        rotations, scales, means3D, viewmatrix = ctx.saved_tensors
        N = rotations.shape[0]
        g = g_out.contiguous().float()
        g_rot = torch.empty_like(rotations)
        if N:
            _lib.call("adgs_gaussian_normals_backward", g.device, N, scales.data_ptr(), rotations.data_ptr(), means3D.data_ptr(), viewmatrix.data_ptr(),
                      g.data_ptr(), ctx.c0 + 3, ctx.c0, g_rot.data_ptr())
        return g_rot, None, None, None, None


def _check_rows(t, name, cols, N, device, who):
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if t.dim() != 2 or t.shape[1] != cols or (N is not None and t.shape[0] != N):
        raise ValueError("%s: %s must be [N, %d]%s, got %s" % (who, name, cols, "" if N is None else " with N = %d" % N, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    if device is not None and t.device != device:
        raise RuntimeError("%s: %s is on %s, rotations on %s" % (who, name, t.device, device))


def gaussian_normals(scales, rotations, means3D, viewmatrix, mask=None):
    """The camera-space normal of every Gaussian, oriented towards the camera: column k of R(q / |q|), k the shortest of the three scales
    (the lowest index on ties), rotated by the view matrix and negated where it points away from the camera (n_c . p_c > 0).

    scales [N, 3] (activated), rotations [N, 4] (w, x, y, z; any non-zero length), means3D [N, 3]: float32.  viewmatrix: the [4, 4] float32
    world-to-view matrix as the rasterizer receives it (transposed: GaussianRasterizationSettings.viewmatrix).  mask: an optional [N] or
    [N, 1] float32 column (the object mask) that becomes column 0 of the result.  Returns [N, 3], or [N, 4] with the mask: the rasterizer's
    `semantic` tensor in one pass.  The gradient goes to `rotations` only: the choice of the axis and the flip are piecewise constant."""
    who = "gaussian_normals"
    _check_rows(rotations, "rotations", 4, None, None, who)
    N, device = rotations.shape[0], rotations.device
    _check_rows(scales, "scales", 3, N, device, who)
    _check_rows(means3D, "means3D", 3, N, device, who)
    if not torch.is_tensor(viewmatrix):
        raise TypeError("%s: viewmatrix must be a tensor, got %s" % (who, type(viewmatrix).__name__))
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError("%s: viewmatrix must be [4, 4], got %s" % (who, tuple(viewmatrix.shape)))
    if viewmatrix.dtype != torch.float32:
        raise TypeError("%s: viewmatrix must be float32, got %s" % (who, viewmatrix.dtype))
    if viewmatrix.device != device:
        raise RuntimeError("%s: viewmatrix is on %s, rotations on %s" % (who, viewmatrix.device, device))
    m = None
    if mask is not None:
        if not torch.is_tensor(mask):
            raise TypeError("%s: mask must be a tensor, got %s" % (who, type(mask).__name__))
        if tuple(mask.shape) not in ((N,), (N, 1)):
            raise ValueError("%s: mask must be [N] or [N, 1] with N = %d, got %s" % (who, N, tuple(mask.shape)))
        if mask.dtype != torch.float32:
            raise TypeError("%s: mask must be float32, got %s" % (who, mask.dtype))
        if mask.device != device:
            raise RuntimeError("%s: mask is on %s, rotations on %s" % (who, mask.device, device))
        m = mask.detach().reshape(N).contiguous()
    if not rotations.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    return _GaussianNormals.apply(rotations.contiguous(), scales.detach().contiguous(), means3D.detach().contiguous(), viewmatrix.detach().contiguous(), m)


def _tanfov(camera_or_tanfov, who):
    if hasattr(camera_or_tanfov, "FoVx") and hasattr(camera_or_tanfov, "FoVy"):
        tx, ty = math.tan(0.5 * float(camera_or_tanfov.FoVx)), math.tan(0.5 * float(camera_or_tanfov.FoVy))
    else:
        try:
            tx, ty = camera_or_tanfov
            tx, ty = float(tx), float(ty)
        except (TypeError, ValueError):
            raise TypeError("%s: expected a camera with FoVx / FoVy or a (tanfovx, tanfovy) pair, got %r" % (who, camera_or_tanfov)) from None
    if not (0.0 < tx < float("inf") and 0.0 < ty < float("inf")):
        raise ValueError("%s: tanfovx and tanfovy must be finite and > 0, got %r, %r" % (who, tx, ty))
    return tx, ty


def _check_map(t, name, H, W, device, who):
    """A [H, W] or [1, H, W] float32 map; H, W None: this map defines them."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    ok = t.dim() in (2, 3) and t.numel() == t.shape[-2] * t.shape[-1] if H is None else tuple(t.shape) in ((H, W), (1, H, W))
    if not ok:
        raise ValueError("%s: %s must be [H, W] or [1, H, W]%s, got %s" % (who, name, "" if H is None else " = [%d, %d]" % (H, W), tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    if device is not None and t.device != device:
        raise RuntimeError("%s: %s is on %s, depth on %s" % (who, name, t.device, device))


def _min_opacity(min_opacity, who):
    mo = float(min_opacity)
    if not (0.0 < mo <= 1.0):
        raise ValueError("%s: min_opacity must lie in (0, 1], got %r" % (who, min_opacity))
    return mo


def depth_to_normal(depth, img_opacity, tanfovx, tanfovy, inv_depth=True, min_opacity=0.5):
    """The normals [3, H, W] of the surface a rendered depth map describes, facing the camera (a fronto-parallel plane gives (0, 0, -1)):
    the normalised cross product of the central differences of the unprojected expected depth z = O / D (inv_depth) or D / O.  Zero on the
    one-pixel border and wherever the pixel or one of its four neighbours has O < min_opacity or D <= 0.  Forward only."""
    who = "depth_to_normal"
    _check_map(depth, "depth", None, None, None, who)
    H, W = depth.shape[-2:]
    _check_map(img_opacity, "img_opacity", H, W, depth.device, who)
    tx, ty = _tanfov((tanfovx, tanfovy), who)
    mo = _min_opacity(min_opacity, who)
    if not depth.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    d, o = depth.detach().contiguous().reshape(H, W), img_opacity.detach().contiguous().reshape(H, W)
    out = torch.empty((3, H, W), dtype=torch.float32, device=d.device)
    if d.numel():
        _lib.call("adgs_depth_to_normal", d.device, H, W, d.data_ptr(), o.data_ptr(), tx, ty, int(bool(inv_depth)), mo, out.data_ptr())
    return out


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal, depth, opacity, w, view):
        H, W = normal.shape[-2:]
        n, d, o = normal.contiguous(), depth.contiguous().reshape(H, W), opacity.contiguous().reshape(H, W)
        ctx.args, ctx.shapes = (H, W), (depth.shape, opacity.shape)
        ctx.view, ctx.has_w = view, w is not None
        out = _scalar(n.device, n.numel())
        work, ctx.token = _work(n.device, NORMAL_WORK_DOUBLES)        # the backward reads sum v from `work`
        if n.numel():
            _lib.call("adgs_normal_consistency_forward", n.device, H, W, n.data_ptr(), d.data_ptr(), o.data_ptr(), _ptr(w), *view, work.data_ptr(), out.data_ptr())
        ctx.token.done()
        ctx.save_for_backward(n, d, o, work, *([w] if w is not None else []))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        n, d, o, work, *rest = ctx.saved_tensors
        w = rest[0] if ctx.has_w else None
        need = ctx.needs_input_grad[:3]
        g_n = torch.empty_like(n) if need[0] else None
        g_d = torch.empty_like(d) if need[1] else None
        g_o = torch.empty_like(o) if need[2] else None
        gl = _g1(g_loss)
        if n.numel() and any(need):
            _lib.call("adgs_normal_consistency_backward", n.device, *ctx.args, n.data_ptr(), d.data_ptr(), o.data_ptr(), _ptr(w), *ctx.view, work.data_ptr(),
                      gl.data_ptr(), _ptr(g_n), _ptr(g_d), _ptr(g_o))
        return (g_n, None if g_d is None else g_d.reshape(ctx.shapes[0]), None if g_o is None else g_o.reshape(ctx.shapes[1]), None, None)


def normal_consistency_loss(img_normal, depth, img_opacity, camera_or_tanfov, weight=None, inv_depth=True, min_opacity=0.5):
    """The depth-normal consistency term: mean over the valid pixels of 1 - Nh . n_d, with Nh the normalised blended normal map
    (render()'s 'img_normal' under pipe.render_normals) and n_d the normal of the rendered depth (depth_to_normal).

    img_normal: float32 [3, H, W]; depth, img_opacity: float32 [H, W] or [1, H, W] as render() returns them (`inv_depth` = pipe.inv_depth);
    camera_or_tanfov: a camera with FoVx / FoVy or a (tanfovx, tanfovy) pair; weight: an optional supervision weight (see
    adgs.loss.l1_ssim), a constant.  A pixel is valid when it is not on the one-pixel border and it and its four neighbours have
    O >= min_opacity and D > 0;  loss = sum v e / sum v with v = weight x valid, 0 with zero gradients when sum v = 0 (decided on the
    device).  Gradients go to whichever of the three maps require them; the backward is one gather launch (include/adgs_normals.h)."""
    who = "normal_consistency_loss"
    if not torch.is_tensor(img_normal):
        raise TypeError("%s: img_normal must be a tensor, got %s" % (who, type(img_normal).__name__))
    if img_normal.dim() != 3 or img_normal.shape[0] != 3:
        raise ValueError("%s: img_normal must be [3, H, W], got %s" % (who, tuple(img_normal.shape)))
    if img_normal.dtype != torch.float32:
        raise TypeError("%s: img_normal must be float32, got %s" % (who, img_normal.dtype))
    H, W = img_normal.shape[-2:]
    device = img_normal.device
    _check_map(depth, "depth", H, W, None, who)
    if depth.device != device:
        raise RuntimeError("%s: depth is on %s, img_normal on %s" % (who, depth.device, device))
    _check_map(img_opacity, "img_opacity", H, W, device, who)
    tx, ty = _tanfov(camera_or_tanfov, who)
    mo = _min_opacity(min_opacity, who)
    w = None if weight is None else _check_weight(weight, H, W, device, who)
    if not img_normal.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    return _NormalConsistency.apply(img_normal, depth, img_opacity, w, (tx, ty, int(bool(inv_depth)), mo))
