"""The multi-view photometric consistency term on the HIP path (include/adgs_multiview.h): PGSR's plane-warped patch NCC.

Every other geometry term of this package constrains one view at a time.  This one ties the surface a reference view renders -- the
local plane its depth and normal describe at a pixel -- to what a NEIGHBOURING training image saw: the plane induces a homography into
the neighbour, a (2 radius + 1)^2 patch of the reference grey image is warped through it, and the squared normalised cross-correlation
with the neighbour's grey image is the error.  One render, not two: the neighbour contributes its ground-truth image and its pose.

    rel = relative_pose(cam, nbr)                                   # once per camera pair, at load time
    pkg = render(cam, model, None, pipe)                            # pipe.render_normals = True
    idx = sample_pixels(static_mask, 102400, radius=3)
    L = photometric_consistency_loss(pkg["img_normal"], pkg["depth"], pkg["img_opacity"], cam, gray(cam.original_image),
                                     gray(nbr.original_image), nbr, rel, idx, weight=static_mask, inv_depth=pipe.inv_depth)

One wave per sample and one tap per lane, forward in one launch plus the finish, backward in one launch that recomputes the taps; no
[S, T] tensor exists.  There is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import SLOTS, _check_weight, _g1, _ptr, _scalar, _work
from .normals import _check_map, _min_opacity, _tanfov

MULTIVIEW_WORK_DOUBLES = 256 * 2 + 4        # ADGS_MULTIVIEW_WORK_DOUBLES
MAX_RADIUS = 3                              # ADGS_MULTIVIEW_MAX_RADIUS
EPS = 1e-8                                  # PGSR's lncc


class MultiviewDesc(ctypes.Structure):
    """adgs_multiview_desc (include/adgs_multiview.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("Hn", ctypes.c_int), ("Wn", ctypes.c_int),
                ("radius", ctypes.c_int), ("inv_depth", ctypes.c_int), ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float),
                ("tanfovx_n", ctypes.c_float), ("tanfovy_n", ctypes.c_float), ("min_opacity", ctypes.c_float), ("min_cos", ctypes.c_float),
                ("max_error", ctypes.c_float), ("eps", ctypes.c_float), ("pose", ctypes.c_float * 12)]


def make_desc(H, W, Hn, Wn, radius, inv_depth, tan, tan_n, min_opacity, min_cos, max_error, eps, pose):
    """An adgs_multiview_desc; pose: 12 numbers, R row-major then t."""
    return MultiviewDesc(ctypes.sizeof(MultiviewDesc), H, W, Hn, Wn, radius, int(bool(inv_depth)), tan[0], tan[1], tan_n[0], tan_n[1],
                         min_opacity, min_cos, max_error, eps, (ctypes.c_float * 12)(*pose))


def gray(image):
    """0.299 R + 0.587 G + 0.114 B of a [3, H, W] image -> [H, W]."""
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("gray: image must be a [3, H, W] tensor")
    return 0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]


def relative_pose(cam_ref, cam_nbr):
    """The [3, 4] float64 HOST tensor (R | t) with X_n = R X_r + t, from the reference camera's frame to the neighbour's, built from the
    two `world_view_transform`s.  Those are the transposed (row-vector) matrices the rasterizer receives, so A = V.T maps world to camera
    and rel = A_n inv(A_r), formed in float64.  This READS THE TWO MATRICES BACK from the device: call it once per camera pair when the
    cameras are loaded, not per iteration."""
    A = []
    for name, cam in (("cam_ref", cam_ref), ("cam_nbr", cam_nbr)):
        V = getattr(cam, "world_view_transform", cam)
        if not torch.is_tensor(V) or tuple(V.shape) != (4, 4):
            raise ValueError("relative_pose: %s must be a camera with a [4, 4] world_view_transform (or that matrix)" % name)
        A.append(V.detach().to("cpu", torch.float64).T)
    rel = A[1] @ torch.linalg.inv(A[0])
    return rel[:3, :4].contiguous()


def sample_pixels(mask, n, radius, generator=None):
    """Up to `n` unique int32 linear indices y * W + x, on the mask's device, of pixels with mask > 0 that lie at least `radius` from the
    border of the [H, W] (or [1, H, W]) mask; fewer when the mask has fewer such pixels.  Torch operations (a permutation of the
    candidates); `generator` must live on the mask's device."""
    if not torch.is_tensor(mask) or mask.dim() not in (2, 3) or mask.numel() != mask.shape[-2] * mask.shape[-1]:
        raise ValueError("sample_pixels: mask must be an [H, W] or [1, H, W] tensor")
    n, radius = int(n), int(radius)
    if n < 0 or radius < 0:
        raise ValueError("sample_pixels: n and radius must be >= 0")
    H, W = mask.shape[-2:]
    inner = torch.zeros((H, W), dtype=torch.bool, device=mask.device)
    if H > 2 * radius and W > 2 * radius:
        inner[radius:H - radius, radius:W - radius] = mask.reshape(H, W)[radius:H - radius, radius:W - radius] > 0
    cand = inner.reshape(-1).nonzero().reshape(-1)
    pick = torch.randperm(cand.numel(), device=mask.device, generator=generator)[:n]
    return cand[pick].to(torch.int32)


def _gray_map(t, name, H, W, device, who):
    _check_map(t, name, H, W, None, who)
    if t.device != device:
        raise RuntimeError("%s: %s is on %s, img_normal on %s" % (who, name, t.device, device))
    return t.detach().contiguous().reshape(t.shape[-2:])


def _prepare(who, img_normal, depth, img_opacity, camera_or_tanfov, ref_gray, nbr_gray, nbr_camera_or_tanfov, pose, samples, weight, radius,
             inv_depth, min_opacity, min_cos, max_error):
    """The checks every entry shares -> (desc arguments, the constant tensors): decided from the arguments alone, nothing is read back."""
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
    tan = _tanfov(camera_or_tanfov, who)
    ref = _gray_map(ref_gray, "ref_gray", H, W, device, who)
    _check_map(nbr_gray, "nbr_gray", None, None, None, who)
    nbr = _gray_map(nbr_gray, "nbr_gray", *nbr_gray.shape[-2:], device, who)
    tan_n = _tanfov(nbr_camera_or_tanfov, who)
    if not torch.is_tensor(pose):
        raise TypeError("%s: pose must be a tensor (relative_pose), got %s" % (who, type(pose).__name__))
    if tuple(pose.shape) != (3, 4) or not pose.dtype.is_floating_point:
        raise ValueError("%s: pose must be a floating-point [3, 4] tensor (R | t), got %s %s" % (who, pose.dtype, tuple(pose.shape)))
    if pose.device.type != "cpu":
        raise RuntimeError("%s: pose must be a host tensor (relative_pose), it is on %s" % (who, pose.device))
    p = pose.detach().to(torch.float64)
    pose12 = p[:, :3].reshape(-1).tolist() + p[:, 3].tolist()
    if not all(abs(x) < float("inf") for x in pose12):
        raise ValueError("%s: pose must be finite" % who)
    if not torch.is_tensor(samples):
        raise TypeError("%s: samples must be a tensor, got %s" % (who, type(samples).__name__))
    if samples.dim() != 1:
        raise ValueError("%s: samples must be [S], got %s" % (who, tuple(samples.shape)))
    if samples.dtype != torch.int32:
        raise TypeError("%s: samples must be int32 linear pixel indices, got %s" % (who, samples.dtype))
    if samples.device != device:
        raise RuntimeError("%s: samples is on %s, img_normal on %s" % (who, samples.device, device))
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError("%s: radius must be 1, 2 or 3, got %r" % (who, radius))
    mo = _min_opacity(min_opacity, who)
    mc, me = float(min_cos), float(max_error)
    if not (0.0 < mc <= 1.0):
        raise ValueError("%s: min_cos must lie in (0, 1], got %r" % (who, min_cos))
    if not (0.0 < me <= 1.0):
        raise ValueError("%s: max_error must lie in (0, 1], got %r" % (who, max_error))
    w = None if weight is None else _check_weight(weight, H, W, device, who)
    if not img_normal.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    desc = (H, W, nbr.shape[0], nbr.shape[1], radius, bool(inv_depth), tan, tan_n, mo, mc, me, EPS, pose12)
    return desc, (ref, nbr, samples.detach().contiguous(), w)


class _MultiviewNcc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal, depth, opacity, desc, consts):
        ref, nbr, samples, w = consts
        H, W = normal.shape[-2:]
        n, d, o = normal.contiguous(), depth.contiguous().reshape(H, W), opacity.contiguous().reshape(H, W)
        S = samples.numel()
        ctx.launched = bool(S and n.numel() and nbr.numel())
        ctx.desc, ctx.S, ctx.shapes, ctx.has_w = desc, S, (depth.shape, opacity.shape), w is not None
        out = _scalar(n.device, ctx.launched)
        work, ctx.token = _work(n.device, MULTIVIEW_WORK_DOUBLES)        # the backward reads sum w v from `work`
        if ctx.launched:
            _lib.call("adgs_multiview_ncc_forward", n.device, ctypes.byref(make_desc(*desc)), n.data_ptr(), d.data_ptr(), o.data_ptr(), ref.data_ptr(),
                      nbr.data_ptr(), _ptr(w), samples.data_ptr(), S, work.data_ptr(), out.data_ptr(), None, None)
        ctx.token.done()
        ctx.save_for_backward(n, d, o, work, ref, nbr, samples, *([w] if w is not None else []))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        n, d, o, work, ref, nbr, samples, *rest = ctx.saved_tensors
        w = rest[0] if ctx.has_w else None
        need = ctx.needs_input_grad[:3]
        new = torch.empty_like if ctx.launched else torch.zeros_like      # the native call zero-fills what it is given
        g_n = new(n) if need[0] else None
        g_d = new(d) if need[1] else None
        g_o = new(o) if need[2] else None
        gl = _g1(g_loss)
        if ctx.launched and any(need):
            _lib.call("adgs_multiview_ncc_backward", n.device, ctypes.byref(make_desc(*ctx.desc)), n.data_ptr(), d.data_ptr(), o.data_ptr(), ref.data_ptr(),
                      nbr.data_ptr(), _ptr(w), samples.data_ptr(), ctx.S, work.data_ptr(), gl.data_ptr(), _ptr(g_n), _ptr(g_d), _ptr(g_o))
        return (g_n, None if g_d is None else g_d.reshape(ctx.shapes[0]), None if g_o is None else g_o.reshape(ctx.shapes[1]), None, None)


def photometric_consistency_loss(img_normal, depth, img_opacity, camera_or_tanfov, ref_gray, nbr_gray, nbr_camera_or_tanfov, pose, samples,
                                 weight=None, radius=3, inv_depth=True, min_opacity=0.5, min_cos=0.1, max_error=0.9):
    """The multi-view photometric consistency term: the weighted mean over the valid samples of 1 - NCC^2 between a patch of the
    reference grey image and the neighbour's grey image under the homography of the rendered local plane (include/adgs_multiview.h).

    img_normal: float32 [3, H, W]; depth, img_opacity: float32 [H, W] or [1, H, W], as render() returns them under pipe.render_normals
    (`inv_depth` = pipe.inv_depth); camera_or_tanfov: the reference camera (FoVx / FoVy) or a (tanfovx, tanfovy) pair; ref_gray [H, W]
    and nbr_gray [Hn, Wn]: float32 grey images (gray()), constants -- the neighbour has its own size and nbr_camera_or_tanfov; pose:
    relative_pose(cam, nbr), a [3, 4] host tensor; samples: int32 [S] linear pixel indices (sample_pixels), indices outside the image
    or too close to its border are invalid samples, a pixel listed twice counts twice; weight: an optional supervision weight (see
    adgs.loss.l1_ssim), a constant.  A sample is valid when O >= min_opacity and D > 0, the normal faces the camera (-Nh . r0 >=
    min_cos |r0|), every tap lands inside the neighbour's image in front of its camera, and the error is below max_error;
    loss = sum w v e / sum w v, 0 with zero gradients when no sample is valid (decided on the device).  Gradients go to whichever of
    img_normal, depth, img_opacity require them, at the sampled pixels only."""
    desc, consts = _prepare("photometric_consistency_loss", img_normal, depth, img_opacity, camera_or_tanfov, ref_gray, nbr_gray, nbr_camera_or_tanfov,
                            pose, samples, weight, radius, inv_depth, min_opacity, min_cos, max_error)
    return _MultiviewNcc.apply(img_normal, depth, img_opacity, desc, consts)


def patch_errors(img_normal, depth, img_opacity, camera_or_tanfov, ref_gray, nbr_gray, nbr_camera_or_tanfov, pose, samples, weight=None,
                 radius=3, inv_depth=True, min_opacity=0.5, min_cos=0.1, max_error=0.9):
    """(e [S] float32, valid [S] bool) of the same arguments, forward only: e is the patch error wherever every gate before the last
    holds (0 elsewhere), valid includes e < max_error.  For visualisation and tests."""
    desc, (ref, nbr, samples, w) = _prepare("patch_errors", img_normal, depth, img_opacity, camera_or_tanfov, ref_gray, nbr_gray, nbr_camera_or_tanfov,
                                            pose, samples, weight, radius, inv_depth, min_opacity, min_cos, max_error)
    H, W = img_normal.shape[-2:]
    n = img_normal.detach().contiguous()
    d, o = depth.detach().contiguous().reshape(H, W), img_opacity.detach().contiguous().reshape(H, W)
    S = samples.numel()
    launched = bool(S and n.numel() and nbr.numel())
    e = (torch.empty if launched else torch.zeros)(S, dtype=torch.float32, device=n.device)
    valid = (torch.empty if launched else torch.zeros)(S, dtype=torch.uint8, device=n.device)
    if launched:
        loss = _scalar(n.device, True)
        work, token = _work(n.device, MULTIVIEW_WORK_DOUBLES)
        _lib.call("adgs_multiview_ncc_forward", n.device, ctypes.byref(make_desc(*desc)), n.data_ptr(), d.data_ptr(), o.data_ptr(), ref.data_ptr(),
                  nbr.data_ptr(), _ptr(w), samples.data_ptr(), S, work.data_ptr(), loss.data_ptr(), e.data_ptr(), valid.data_ptr())
        token.done()
    return e, valid.bool()


# ---- the geometric term (include/adgs_multiview_geo.h): the depth reprojection error between two renders ----
#
#     pkg, pkg_n = render(cam, model, None, pipe), render(nbr, model, None, pipe)      # the same time stamp
#     L_geo = geometric_consistency_loss(pkg["depth"], pkg["img_opacity"], cam, pkg_n["depth"], pkg_n["img_opacity"], nbr, rel,
#                                        weight=static_mask, inv_depth=pipe.inv_depth)
#     err, geo_weight = reprojection_errors(...the same arguments...)                  # exp(-err) where the round trip closes, else 0
#     idx = sample_pixels(static_mask * geo_weight, 102400, radius=3)
#     L_ncc = photometric_consistency_loss(..., idx, weight=static_mask * geo_weight)

MULTIVIEW_GEO_WORK_DOUBLES = 256 * 2 + 4    # ADGS_MULTIVIEW_GEO_WORK_DOUBLES


class MultiviewGeoDesc(ctypes.Structure):
    """adgs_multiview_geo_desc (include/adgs_multiview_geo.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("Hn", ctypes.c_int), ("Wn", ctypes.c_int),
                ("inv_depth", ctypes.c_int), ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("tanfovx_n", ctypes.c_float),
                ("tanfovy_n", ctypes.c_float), ("min_opacity", ctypes.c_float), ("max_pixel_error", ctypes.c_float), ("pose", ctypes.c_float * 12)]


def make_geo_desc(H, W, Hn, Wn, inv_depth, tan, tan_n, min_opacity, max_pixel_error, pose):
    """An adgs_multiview_geo_desc; pose: 12 numbers, R row-major then t."""
    return MultiviewGeoDesc(ctypes.sizeof(MultiviewGeoDesc), H, W, Hn, Wn, int(bool(inv_depth)), tan[0], tan[1], tan_n[0], tan_n[1], min_opacity,
                            max_pixel_error, (ctypes.c_float * 12)(*pose))


def _pose12(pose, who):
    if not torch.is_tensor(pose):
        raise TypeError("%s: pose must be a tensor (relative_pose), got %s" % (who, type(pose).__name__))
    if tuple(pose.shape) != (3, 4) or not pose.dtype.is_floating_point:
        raise ValueError("%s: pose must be a floating-point [3, 4] tensor (R | t), got %s %s" % (who, pose.dtype, tuple(pose.shape)))
    if pose.device.type != "cpu":
        raise RuntimeError("%s: pose must be a host tensor (relative_pose), it is on %s" % (who, pose.device))
    p = pose.detach().to(torch.float64)
    pose12 = p[:, :3].reshape(-1).tolist() + p[:, 3].tolist()
    if not all(abs(x) < float("inf") for x in pose12):
        raise ValueError("%s: pose must be finite" % who)
    return pose12


def _prepare_geo(who, depth, img_opacity, camera_or_tanfov, nbr_depth, nbr_opacity, nbr_camera_or_tanfov, pose, weight, inv_depth, min_opacity,
                 max_pixel_error):
    """The checks both entries share -> (desc arguments, the weight): decided from the arguments alone, nothing is read back."""
    _check_map(depth, "depth", None, None, None, who)
    H, W = depth.shape[-2:]
    device = depth.device
    _check_map(img_opacity, "img_opacity", H, W, device, who)
    tan = _tanfov(camera_or_tanfov, who)
    _check_map(nbr_depth, "nbr_depth", None, None, device, who)
    Hn, Wn = nbr_depth.shape[-2:]
    _check_map(nbr_opacity, "nbr_opacity", Hn, Wn, device, who)
    tan_n = _tanfov(nbr_camera_or_tanfov, who)
    pose12 = _pose12(pose, who)
    mo = _min_opacity(min_opacity, who)
    me = float(max_pixel_error)
    if not (0.0 < me < float("inf")):
        raise ValueError("%s: max_pixel_error must be finite and > 0, got %r" % (who, max_pixel_error))
    w = None if weight is None else _check_weight(weight, H, W, device, who)
    if not depth.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    return (H, W, Hn, Wn, bool(inv_depth), tan, tan_n, mo, me, pose12), w


class _MultiviewGeo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, opacity, nbr_depth, nbr_opacity, desc, w):
        H, W, Hn, Wn = desc[:4]
        d, o = depth.contiguous().reshape(H, W), opacity.contiguous().reshape(H, W)
        dn, on = nbr_depth.contiguous().reshape(Hn, Wn), nbr_opacity.contiguous().reshape(Hn, Wn)
        ctx.launched = bool(d.numel() and dn.numel())
        ctx.desc, ctx.has_w = desc, w is not None
        ctx.shapes = (depth.shape, opacity.shape, nbr_depth.shape, nbr_opacity.shape)
        out = _scalar(d.device, ctx.launched)
        work, ctx.token = _work(d.device, MULTIVIEW_GEO_WORK_DOUBLES)     # the backward reads sum w v from `work`
        if ctx.launched:
            _lib.call("adgs_multiview_geo_forward", d.device, ctypes.byref(make_geo_desc(*desc)), d.data_ptr(), o.data_ptr(), dn.data_ptr(), on.data_ptr(),
                      _ptr(w), work.data_ptr(), out.data_ptr(), None, None)
        ctx.token.done()
        ctx.save_for_backward(d, o, dn, on, work, *([w] if w is not None else []))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        d, o, dn, on, work, *rest = ctx.saved_tensors
        w = rest[0] if ctx.has_w else None
        need = ctx.needs_input_grad[:4]
        new = torch.empty_like if ctx.launched else torch.zeros_like      # the native call writes every element of what it is given
        grads = [new(t) if n else None for t, n in zip((d, o, dn, on), need)]
        gl = _g1(g_loss)
        if ctx.launched and any(need):
            _lib.call("adgs_multiview_geo_backward", d.device, ctypes.byref(make_geo_desc(*ctx.desc)), d.data_ptr(), o.data_ptr(), dn.data_ptr(),
                      on.data_ptr(), _ptr(w), work.data_ptr(), gl.data_ptr(), *[_ptr(g) for g in grads])
        return (*[None if g is None else g.reshape(s) for g, s in zip(grads, ctx.shapes)], None, None)


def geometric_consistency_loss(depth, img_opacity, camera_or_tanfov, nbr_depth, nbr_opacity, nbr_camera_or_tanfov, pose, weight=None,
                               inv_depth=True, min_opacity=0.5, max_pixel_error=1.0):
    """The multi-view geometric consistency term (include/adgs_multiview_geo.h): every pixel of the reference view is lifted with the
    rendered depth, projected into the neighbour, re-lifted with the depth the neighbour rendered there (bilinear) and projected back;
    err is the distance in pixels between where it started and where it lands, and loss = sum w v exp(-err) err / sum w v with
    exp(-err) a constant of the differentiation; 0 with zero gradients when no pixel is valid (decided on the device).

    depth, img_opacity: float32 [H, W] or [1, H, W], as render() returns them (`inv_depth` = pipe.inv_depth); nbr_depth, nbr_opacity:
    the same of the NEIGHBOUR'S OWN RENDER, [Hn, Wn] or [1, Hn, Wn] -- its own size and nbr_camera_or_tanfov; the cameras: FoVx / FoVy
    or a (tanfovx, tanfovy) pair; pose: relative_pose(cam, nbr), a [3, 4] host tensor; weight: an optional [H, W] supervision weight
    (see adgs.loss.l1_ssim), a constant.  A pixel is valid when O >= min_opacity and D > 0, it lands inside the neighbour's image in
    front of its camera, the four corners it samples there have On >= min_opacity and Dn > 0, the re-lifted point is in front of the
    reference camera, and err < max_pixel_error.  Gradients go to whichever of the four maps require them: the reference view's are
    deterministic to the bit, the neighbour's are sums of float atomics.  Render the neighbour under torch.no_grad() to skip them."""
    who = "geometric_consistency_loss"
    desc, w = _prepare_geo(who, depth, img_opacity, camera_or_tanfov, nbr_depth, nbr_opacity, nbr_camera_or_tanfov, pose, weight, inv_depth,
                           min_opacity, max_pixel_error)
    return _MultiviewGeo.apply(depth, img_opacity, nbr_depth, nbr_opacity, desc, w)


def reprojection_errors(depth, img_opacity, camera_or_tanfov, nbr_depth, nbr_opacity, nbr_camera_or_tanfov, pose, weight=None, inv_depth=True,
                        min_opacity=0.5, max_pixel_error=1.0):
    """(err [H, W], geo_weight [H, W]) float32 of the same arguments, forward only: err is the reprojection error in pixels wherever
    every gate before the last holds (0 elsewhere); geo_weight = exp(-err) at the valid pixels (err < max_pixel_error included), 0
    elsewhere.  geo_weight is what to multiply into the `weight=` of photometric_consistency_loss and to hand to sample_pixels: it keeps
    occluded and inconsistent pixels out of the photometric term, as upstream does.  `weight` does not enter either map."""
    who = "reprojection_errors"
    desc, w = _prepare_geo(who, depth, img_opacity, camera_or_tanfov, nbr_depth, nbr_opacity, nbr_camera_or_tanfov, pose, weight, inv_depth,
                           min_opacity, max_pixel_error)
    H, W, Hn, Wn = desc[:4]
    d, o = depth.detach().contiguous().reshape(H, W), img_opacity.detach().contiguous().reshape(H, W)
    dn, on = nbr_depth.detach().contiguous().reshape(Hn, Wn), nbr_opacity.detach().contiguous().reshape(Hn, Wn)
    launched = bool(d.numel() and dn.numel())
    err, gw = ((torch.empty if launched else torch.zeros)((H, W), dtype=torch.float32, device=d.device) for _ in range(2))
    if launched:
        loss = _scalar(d.device, True)
        work, token = _work(d.device, MULTIVIEW_GEO_WORK_DOUBLES)
        _lib.call("adgs_multiview_geo_forward", d.device, ctypes.byref(make_geo_desc(*desc)), d.data_ptr(), o.data_ptr(), dn.data_ptr(), on.data_ptr(),
                  _ptr(w), work.data_ptr(), loss.data_ptr(), err.data_ptr(), gw.data_ptr())
        token.done()
    return err, gw


def nearest_cameras(cameras, k=1, max_angle=math.radians(30.0), min_distance=0.0, max_distance=1.5):
    """For every camera of the sequence, the indices of up to `k` OTHER cameras to use as its neighbours: a list of lists of int.  A
    candidate qualifies when the angle between the two viewing directions is <= max_angle (radians) and the distance between the two
    centres lies in (min_distance, max_distance]; the qualifying ones are ordered by distance, then by index.  A driving rig moves
    along its viewing direction, so the angle alone cannot rank neighbours; a stationary ego gives a zero baseline, which min_distance
    excludes.  Directions and centres come from the `world_view_transform`s, read as relative_pose reads them (A = V.T maps world to
    camera: the centre is -R^T t, the viewing direction the third row of R).  Host torch in float64; this READS THE MATRICES BACK from
    the device: call it once, when the cameras are loaded."""
    cameras = list(cameras)
    k = int(k)
    max_angle, min_distance, max_distance = float(max_angle), float(min_distance), float(max_distance)
    if k < 0:
        raise ValueError("nearest_cameras: k must be >= 0")
    if not (0.0 <= max_angle <= math.pi) or not (0.0 <= min_distance <= max_distance < float("inf")):
        raise ValueError("nearest_cameras: max_angle must lie in [0, pi] and 0 <= min_distance <= max_distance < inf")
    centres, dirs = [], []
    for i, cam in enumerate(cameras):
        V = getattr(cam, "world_view_transform", cam)
        if not torch.is_tensor(V) or tuple(V.shape) != (4, 4):
            raise ValueError("nearest_cameras: cameras[%d] must be a camera with a [4, 4] world_view_transform (or that matrix)" % i)
        A = V.detach().to("cpu", torch.float64).T
        R, t = A[:3, :3], A[:3, 3]
        centres.append(-R.T @ t)
        dirs.append(R[2] / R[2].norm())
    if not cameras:
        return []
    C, Z = torch.stack(centres), torch.stack(dirs)
    dist = (C[:, None] - C[None]).norm(dim=-1)
    angle = torch.acos((Z @ Z.T).clamp(-1.0, 1.0))
    ok = (angle <= max_angle) & (dist > min_distance) & (dist <= max_distance)
    ok.fill_diagonal_(False)
    out = []
    for i in range(len(cameras)):
        cand = sorted((float(dist[i, j]), j) for j in ok[i].nonzero().reshape(-1).tolist())
        out.append([j for _, j in cand[:k]])
    return out
