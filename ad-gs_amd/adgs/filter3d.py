"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1) on the HIP path (include/adgs_filter3d.h): the
"3D half" next to the rasterizer's anti-aliased 2D filter.  Every Gaussian gets a low-pass filter whose size comes from the highest
sampling rate (focal length / depth) any training camera has of it, so that optimisation cannot shrink a Gaussian below the
sampling limit of the cameras that see it.  Opt-in:

    model.compute_3d_filter(train_cameras)      # before the first iteration, after every densification, every 100 iterations
    pipe.filter_3d = True                       # gaussian_renderer.render() then rasterizes apply(scales, opacity, model.filter_3D)

`compute_3d_filter` is one streaming pass over the positions per group of cameras (the published trainer: a Python loop over the
cameras with about twenty element-wise kernels over all Gaussians each); `apply` is one fused kernel with an analytic backward.
There is no CPU fallback.
"""
import ctypes
import math
import warnings

import torch

from . import _lib

CAMERA_FLOATS = 16          # ADGS_FILTER3D_CAMERA_FLOATS


class CameraRecord(ctypes.Structure):
    """One camera of adgs_filter3d_accumulate: p_cam = R p + t (R row-major), focal lengths and image size in pixels."""
    _fields_ = [("R", ctypes.c_float * 9), ("t", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("W", ctypes.c_float), ("H", ctypes.c_float)]


def _need_cuda(who, **tensors):
    for name, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("%s: %s must be a tensor on a HIP device; there is no CPU path" % (who, name))


def camera_records(cameras, device):
    """[C, 16] fp32 on `device` from objects with the reference Camera's attributes (world_view_transform -- the transposed,
    row-vector matrix: R is its upper-left block transposed, t its last row --, FoVx, FoVy, image_width, image_height)."""
    cameras = list(cameras)
    device = torch.device(device)
    if not cameras:
        return torch.zeros(0, CAMERA_FLOATS, dtype=torch.float32, device=device)
    view = torch.stack([c.world_view_transform.detach().to(device=device, dtype=torch.float32) for c in cameras])
    intr = torch.tensor([[c.image_width / (2.0 * math.tan(0.5 * c.FoVx)), c.image_height / (2.0 * math.tan(0.5 * c.FoVy)),
                          float(c.image_width), float(c.image_height)] for c in cameras], dtype=torch.float64).float().to(device)
    return torch.cat([view[:, :3, :3].transpose(1, 2).reshape(-1, 9), view[:, 3, :3], intr], dim=1).contiguous()


def accumulate(xyz, cams, rate, row0=0, rows=None, init=False):
    """rate[row] = max(0 if init else rate[row], the sampling rates of `cams` [C, 16]) for the rows [row0, row0 + rows) of xyz [N, 3];
    in place on rate [N] (or [N, 1]), which is returned."""
    _need_cuda("filter3d.accumulate", xyz=xyz, cams=cams, rate=rate)
    N = xyz.shape[0]
    rows = N - row0 if rows is None else rows
    if xyz.dim() != 2 or xyz.shape[1] != 3 or rate.numel() != N or cams.dim() != 2 or cams.shape[1] != CAMERA_FLOATS:
        raise ValueError("filter3d.accumulate: xyz [N,3], cams [C,16], rate [N]; got %s, %s, %s" % (tuple(xyz.shape), tuple(cams.shape), tuple(rate.shape)))
    if row0 < 0 or rows < 0 or row0 + rows > N:
        raise ValueError("filter3d.accumulate: rows [%d, %d) of %d" % (row0, row0 + rows, N))
    for name, t in (("xyz", xyz), ("cams", cams), ("rate", rate)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != xyz.device:
            raise ValueError("filter3d.accumulate: %s must be contiguous fp32 on %s" % (name, xyz.device))
    if cams.shape[0] == 0:          # no camera: nothing to take a maximum over
        if init:
            rate.view(-1)[row0:row0 + rows].zero_()
        return rate
    _lib.call("adgs_filter3d_accumulate", xyz.device, xyz.data_ptr(), int(row0), int(rows), cams.data_ptr(), cams.shape[0], rate.data_ptr(), int(bool(init)))
    return rate


def finalize(rate, out=None):
    """filter [N, 1] from rates [N]: sqrt(0.2) / rate, the largest of those for rows no camera saw, zeros when none was seen."""
    _need_cuda("filter3d.finalize", rate=rate)
    if rate.dtype != torch.float32 or not rate.is_contiguous():
        raise ValueError("filter3d.finalize: rate must be contiguous fp32")
    N = rate.numel()
    out = torch.empty(N, 1, dtype=torch.float32, device=rate.device) if out is None else out
    work = torch.empty(1, dtype=torch.int32, device=rate.device)
    _lib.call("adgs_filter3d_finalize", rate.device, rate.data_ptr(), N, out.data_ptr(), work.data_ptr())
    return out


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacity, filter_3d):
        _need_cuda("filter3d.apply", scales=scales, opacity=opacity, filter_3D=filter_3d)
        P = scales.shape[0]
        if scales.dim() != 2 or scales.shape[1] != 3 or opacity.numel() != P or filter_3d.numel() != P:
            raise ValueError("filter3d.apply: scales [P,3], opacity [P,1], filter [P,1]; got %s, %s, %s" % (
                tuple(scales.shape), tuple(opacity.shape), tuple(filter_3d.shape)))
        s, o, f = scales.contiguous().float(), opacity.contiguous().float(), filter_3d.contiguous().float()
        s_out, o_out = torch.empty_like(s), torch.empty_like(o)
        _lib.call("adgs_filter3d_apply_forward", s.device, P, s.data_ptr(), o.data_ptr(), f.data_ptr(), s_out.data_ptr(), o_out.data_ptr())
        ctx.save_for_backward(s, o, f)
        return s_out, o_out

    @staticmethod
    def backward(ctx, g_s_out, g_o_out):
        s, o, f = ctx.saved_tensors
        gs_out, go_out = g_s_out.contiguous().float(), g_o_out.contiguous().float()
        g_s, g_o = torch.empty_like(s), torch.empty_like(o)
        _lib.call("adgs_filter3d_apply_backward", s.device, s.shape[0], s.data_ptr(), o.data_ptr(), f.data_ptr(), gs_out.data_ptr(), go_out.data_ptr(),
                  g_s.data_ptr(), g_o.data_ptr())
        return g_s, g_o, None


def apply(scales, opacity, filter_3d):
    """(sqrt(s^2 + f^2), o sqrt(prod_i s_i^2 / (s_i^2 + f^2))) of activated scales [P,3], activated opacity [P,1] and filter [P,1];
    differentiable in scales and opacity, the filter receives no gradient."""
    return _Apply.apply(scales, opacity, filter_3d)


_warned_unseen = False


def compute_3d_filter(model, cameras):
    """model.filter_3D [N, 1] from the training cameras (reference Camera attributes, with `time`).  Rows that do not move with time
    -- the scene range when the model's background deformation orders are all zero -- take one launch over all cameras; the
    time-dependent rows one launch per distinct time stamp on get_deformed_xyz(t), restricted to their range.  Maxima and the minimum
    do not depend on order: every data-parallel rank computes the same filter.  Warns (once) when no camera sees any Gaussian."""
    global _warned_unseen
    cameras = list(cameras)
    with torch.no_grad():
        Ns, No = model._scene_xyz.shape[0], model._obj_xyz.shape[0]
        N = Ns + No
        device = model._scene_xyz.device if Ns else model._obj_xyz.device
        if device.type != "cuda":
            raise RuntimeError("compute_3d_filter: the model must live on a HIP device; there is no CPU path")
        order = sorted(range(len(cameras)), key=lambda i: float(cameras[i].time))
        recs = camera_records([cameras[i] for i in order], device)
        times = [float(cameras[i].time) for i in order]
        rate = torch.zeros(N, dtype=torch.float32, device=device)
        static = Ns if all(int(a) == 0 for a in model.order_args.get("background", [0] * 6)) else 0
        if static and cameras:
            accumulate(model._scene_xyz.detach().contiguous(), recs, rate[:static], init=True)
        a = 0
        while a < len(times) and N > static:
            b = a
            while b < len(times) and times[b] == times[a]:
                b += 1
            accumulate(model.get_deformed_xyz(times[a]).detach().contiguous(), recs[a:b], rate, row0=static, rows=N - static, init=(a == 0))
            a = b
        model.filter_3D = finalize(rate)
        if N and not _warned_unseen and not bool(model.filter_3D.any()):
            _warned_unseen = True
            warnings.warn("compute_3d_filter: no camera sees any Gaussian; the 3D filter is zero everywhere")
    return model.filter_3D
