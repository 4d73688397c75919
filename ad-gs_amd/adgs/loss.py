"""Photometric loss on the HIP path: drop-ins for
utils/loss_utils.py `l1_loss` (:20-21) and `ssim` (:37-68) as used at train.py:79-80.

`l1_ssim(image, gt)` evaluates both in ONE forward kernel and back-propagates both in ONE backward
kernel (adgs_l1_ssim_forward / _backward, include/adgs_loss.h); `l1_loss` / `ssim` keep the reference's
names and signatures on top of it.  Images are [..., C, H, W] fp32 on a HIP device, `gt` is a constant.
There is no CPU fallback.

Every image term takes an optional per-pixel supervision weight (`weight=`: ego vehicle, invalid borders of undistorted images, excluded
regions) -- see l1_ssim -- and `lidar_depth_loss` is the sparse metric depth term over the lidar_depth/*.npz arrays.
`depth_smoothness_loss` is the edge-aware smoothness prior (first or second order) on the rendered inverse depth.
"""
import ctypes
import threading

import torch

from . import _lib

SLOTS = 256        # ADGS_LOSS_SLOTS


class _Slice:
    """Ownership of one slice of a _WorkArena (or of nothing: a fresh buffer).  The slot is free again when the token is dropped -- at once
    for terms whose backward does not read the slice, with the autograd context for the terms whose backward does (depth, flow).  A token
    dropped before done() (a launch failed between the sum kernel and the finish kernel that re-zeroes the slot rows) marks its slice
    dirty: it is zero-filled before it is handed out again."""
    __slots__ = ("arena", "i", "clean")

    def __init__(self, arena, i):
        self.arena, self.i, self.clean = arena, i, False

    def done(self):
        self.clean = True

    def __del__(self):
        a = self.arena
        if a is not None:
            if not self.clean:
                a.dirty.add(self.i)
            a.busy[self.i] = False


class _WorkArena:
    """Zero-initialised work buffers of the loss kernels (include/adgs_loss.h) without a fill per call: the kernel that consumes a
    buffer's slot rows leaves them zero, so a buffer only has to be zeroed when it is created.  One arena per (device, stream, layout):
    N slices; a slice is busy while its _Slice token lives (a training iteration holds two across its backward: depth and flow).  When
    every slice is busy -- gradient accumulation over more terms than the ring holds -- or under stream capture (an arena created there
    would have its zero fill baked into the graph) the caller gets a fresh zero-filled buffer instead.  take() is guarded by a lock (two
    threads may share a stream)."""
    N = 64

    def __init__(self, device, doubles):
        self.buf = torch.zeros(self.N, doubles, dtype=torch.float64, device=device)
        self.busy = [False] * self.N
        self.dirty = set()
        self.next = 0
        self.lock = threading.Lock()

    def take(self):
        with self.lock:
            for k in range(self.N):
                i = (self.next + k) % self.N
                if not self.busy[i]:
                    break
            else:
                return None
            self.next = (i + 1) % self.N
            self.busy[i] = True
            spoiled = i in self.dirty
            self.dirty.discard(i)
        if spoiled:
            self.buf[i].zero_()
        return self.buf[i], _Slice(self, i)


_ARENAS = {}


def _work(device, doubles):
    """(zeroed work buffer of `doubles` doubles for one loss term, its _Slice token: call done() after the term's launches)"""
    if not torch.cuda.is_current_stream_capturing():
        key = (device, _lib.stream_ptr(device).value, doubles)
        a = _ARENAS.get(key)
        if a is None:
            if len(_ARENAS) > 48:
                _ARENAS.clear()
            a = _ARENAS[key] = _WorkArena(device, doubles)
        got = a.take()
        if got is not None:
            return got
    t = _Slice(None, -1)
    return torch.zeros(doubles, dtype=torch.float64, device=device), t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _scalar(device, launched, n=1):
    """The [n] fp32 output of a term: written by its kernels when they are launched, zeros for an empty input (no launch)."""
    return (torch.empty if launched else torch.zeros)(n, dtype=torch.float32, device=device)


def _g1(g_loss):
    """The upstream gradient of a scalar term as one contiguous fp32 element."""
    return None if g_loss is None else g_loss.reshape(1).float().contiguous()


# An image term is ONE pair of plain functions that owns the term's whole marshalling -- work slice, native call(s), done() -- over prepared contiguous
# fp32 tensors and raw output / gradient POINTERS: a standalone Function hands in a small tensor's pointer, the fused _ImageLosses node an element of its [6].
def _l1_ssim_fwd(img, ref, maps, out2):
    H, W = img.shape[-2:]
    sums, tok = _work(img.device, 2 * SLOTS)                   # spread atomics (include/adgs_loss.h); consumed by adgs_l1_ssim_means below
    if img.numel():
        _lib.call("adgs_l1_ssim_forward", img.device, img.numel() // (H * W), H, W, img.data_ptr(), ref.data_ptr(), sums.data_ptr(), *[_ptr(m) for m in maps])
        _lib.call("adgs_l1_ssim_means", img.device, sums.data_ptr(), img.numel(), out2)
    tok.done()


def _l1_ssim_bwd(img, ref, maps, g_l1, g_ssim, out):
    H, W = img.shape[-2:]
    if img.numel():
        _lib.call("adgs_l1_ssim_backward", img.device, img.numel() // (H * W), H, W, img.data_ptr(), ref.data_ptr(), *[m.data_ptr() for m in maps], g_l1, g_ssim, out)


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt):
        if not image.is_cuda or not gt.is_cuda:
            raise RuntimeError("l1_ssim: tensors must be on a HIP device; there is no CPU path")
        if image.shape != gt.shape or image.dim() < 3:
            raise ValueError("l1_ssim: image and gt must have the same [..., C, H, W] shape")
        img, ref = image.contiguous().float(), gt.contiguous().float()
        need = ctx.needs_input_grad[0]
        maps = [torch.empty_like(img) for _ in range(3)] if need else [None] * 3
        means = _scalar(img.device, img.numel(), 2)
        _l1_ssim_fwd(img, ref, maps, means.data_ptr())
        if need:
            ctx.save_for_backward(img, ref, *maps)
        return means[0], means[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        img, ref, *maps = ctx.saved_tensors
        out, gl, gs = torch.empty_like(img), _g1(g_l1), _g1(g_ssim)
        _l1_ssim_bwd(img, ref, maps, _ptr(gl), _ptr(gs), out.data_ptr())
        return out, None


L1_SSIM_WEIGHTED_WORK_DOUBLES = 256 * 3 + 4        # ADGS_L1_SSIM_WEIGHTED_WORK_DOUBLES


def _check_weight(weight, H, W, device, who):
    """A supervision weight as the kernels take it: a float32 [H, W] (or [1, H, W]) tensor on `device`, detached and contiguous.
    Decided from the arguments alone, before anything is launched; the range [0, 1] is not checked (that would be a read-back)."""
    if not torch.is_tensor(weight):
        raise TypeError("%s: weight must be a tensor, got %s" % (who, type(weight).__name__))
    if tuple(weight.shape) not in ((H, W), (1, H, W)):
        raise ValueError("%s: weight must be [H, W] or [1, H, W] = [%d, %d], got %s" % (who, H, W, tuple(weight.shape)))
    if weight.dtype != torch.float32:
        raise TypeError("%s: weight must be float32 weights in [0, 1], got %s" % (who, weight.dtype))
    if weight.device != device:
        raise RuntimeError("%s: weight is on %s, the images on %s" % (who, weight.device, device))
    return weight.detach().reshape(H, W).contiguous()


def _l1_ssim_weighted_fwd(img, ref, w, maps, out2):
    """-> (work, token): the backward reads sum w from `work`, so both live with the autograd context."""
    H, W = img.shape[-2:]
    work, tok = _work(img.device, L1_SSIM_WEIGHTED_WORK_DOUBLES)
    if img.numel():
        _lib.call("adgs_l1_ssim_weighted_forward", img.device, img.numel() // (H * W), H, W, img.data_ptr(), ref.data_ptr(), w.data_ptr(), work.data_ptr(),
                  *[_ptr(m) for m in maps], out2)
    tok.done()
    return work, tok


def _l1_ssim_weighted_bwd(img, ref, w, maps, work, g_l1, g_ssim, out):
    H, W = img.shape[-2:]
    if img.numel():
        _lib.call("adgs_l1_ssim_weighted_backward", img.device, img.numel() // (H * W), H, W, img.data_ptr(), ref.data_ptr(), w.data_ptr(),
                  *[m.data_ptr() for m in maps], work.data_ptr(), g_l1, g_ssim, out)


class _L1SSIMWeighted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, w):
        img, ref = image.contiguous().float(), gt.contiguous().float()
        need = ctx.needs_input_grad[0]
        maps = [torch.empty_like(img) for _ in range(3)] if need else [None] * 3
        means = _scalar(img.device, img.numel(), 2)
        work, tok = _l1_ssim_weighted_fwd(img, ref, w, maps, means.data_ptr())
        if need:
            ctx.token = tok
            ctx.save_for_backward(img, ref, w, work, *maps)
        return means[0], means[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        img, ref, w, work, *maps = ctx.saved_tensors
        out, gl, gs = torch.empty_like(img), _g1(g_l1), _g1(g_ssim)
        _l1_ssim_weighted_bwd(img, ref, w, maps, work, _ptr(gl), _ptr(gs), out.data_ptr())
        return out, None, None


def l1_ssim(image, gt, weight=None):
    """(mean |image - gt|, mean SSIM(image, gt)) -- both differentiable w.r.t. `image`.

    weight: an optional float32 [H, W] or [1, H, W] tensor of supervision weights on the images' device, meant to lie in [0, 1] (not
    checked); a constant, shared by every channel and every leading dimension of [..., C, H, W].  With P planes and Sw = sum(weight):
        L1_w = sum_planes sum_pixels w |image - gt| / (P Sw)          SSIM_w = sum_planes sum_pixels w ssim_map / (P Sw)
    The SSIM map is the unchanged one, computed from the UNMASKED images: the weight applies to the map, not to the images.  This is the
    region definition of adgs.metrics.Evaluator, so the loss over a region and the evaluation metric over the same region are the same
    number; the consequence is that pixels within 5 px of a masked area still influence the loss through the 11x11 window.
    Sw = 0 (decided on the device) gives (0, 0) and an all-zero gradient."""
    if weight is None:
        return _L1SSIM.apply(image, gt.detach())
    if image.dim() < 3 or image.shape != gt.shape:
        raise ValueError("l1_ssim: image and gt must have the same [..., C, H, W] shape")
    w = _check_weight(weight, image.shape[-2], image.shape[-1], image.device, "l1_ssim")
    if not image.is_cuda or not gt.is_cuda:
        raise RuntimeError("l1_ssim: tensors must be on a HIP device; there is no CPU path")
    return _L1SSIMWeighted.apply(image, gt.detach(), w)


def l1_loss(network_output, gt, weight=None):
    """utils/loss_utils.py:20-21; `weight`: see l1_ssim."""
    return l1_ssim(network_output, gt, weight)[0]


def ssim(img1, img2, window_size=11, size_average=True, weight=None):
    """utils/loss_utils.py:37-68 for the arguments AD-GS uses (11x11 window, mean over everything); `weight`: see l1_ssim."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("the HIP ssim implements window_size=11, size_average=True (train.py:80)")
    return l1_ssim(img1, img2, weight)[1]


def photometric_loss(image, gt, lambda_dssim, lambda_l1=1.0, weight=None):
    """train.py:79-80,112: (1 - lambda_dssim) * lambda_l1 * L1 + lambda_dssim * (1 - SSIM); returns (loss, Ll1, dssim_loss).
    `weight`: see l1_ssim."""
    l1, s = l1_ssim(image, gt, weight)
    dssim = 1.0 - s
    return (1.0 - lambda_dssim) * lambda_l1 * l1 + lambda_dssim * dssim, l1, dssim


DEPTH_WORK_DOUBLES = 256 * 8 + 16        # ADGS_DEPTH_WORK_DOUBLES


def _depth_fwd(p, g, m, out):
    """-> (work, token): the backward reads the fitted scale and shift from `work`, so both live with the autograd context."""
    work, tok = _work(p.device, DEPTH_WORK_DOUBLES)
    _lib.call("adgs_depth_loss_forward", p.device, p.numel(), p.data_ptr(), g.data_ptr(), _ptr(m), work.data_ptr(), out)
    tok.done()
    return work, tok


def _depth_bwd(p, g, m, work, g_loss, out):
    _lib.call("adgs_depth_loss_backward", p.device, p.numel(), p.data_ptr(), g.data_ptr(), _ptr(m), work.data_ptr(), g_loss, out)


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask):
        if not pred.is_cuda:
            raise RuntimeError("get_depth_loss: tensors must be on a HIP device; there is no CPU path")
        p, g = pred.contiguous().float(), gt.contiguous().float()
        m = None if mask is None else mask.contiguous().float()
        if p.shape != g.shape or (m is not None and m.shape != p.shape):
            raise ValueError("get_depth_loss: prediction, target and mask must have the same shape")
        out = _scalar(p.device, p.numel())
        work, ctx.token = _depth_fwd(p, g, m, out.data_ptr())
        ctx.save_for_backward(p, g, work, *([m] if m is not None else []))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        p, g, work, *rest = ctx.saved_tensors
        out, gl = torch.empty_like(p), _g1(g_loss)
        _depth_bwd(p, g, rest[0] if rest else None, work, gl.data_ptr(), out.data_ptr())
        return out, None, None


def get_depth_loss(pred, gt, mask=None):
    """utils/loss_utils.py:70-75: L1 between the scale/shift-aligned prediction (utils/depth_utils.py:3-45, closed-form least
    squares) and the target, averaged over the mask; differentiable w.r.t. `pred` through the scale and the shift.  No host
    synchronisation (the reference's `if det == 0` is one)."""
    return _DepthLoss.apply(pred, gt.detach(), None if mask is None else mask.detach())


AUX_WORK_DOUBLES = 256 * 2 + 2           # ADGS_AUX_WORK_DOUBLES


class _FlowCam:
    """K, R, T of the flow target (flow_pkg[1:4], train.py:68-71) as kernel arguments.  Tensors on the render device are handed to the
    `_devcam` entry points as device pointers (the kernels form K R and K T themselves): nothing is read back, and -- unlike a host-side
    copy keyed by storage address, which the caching allocator re-issues to the next iteration's `a.cuda()` -- nothing can go stale.
    CPU tensors go by value through the host entry points."""

    def __init__(self, K, R, T, device):
        ts = (K, R, T)
        for t, n, name in zip(ts, (9, 9, 3), "KRT"):
            if t.numel() != n:
                raise ValueError("flow camera: %s must have %d elements" % (name, n))
        self.on_device = all(t.is_cuda and t.device == device for t in ts)
        if self.on_device:
            self.keep = tuple(t.detach().contiguous().float() for t in ts)          # alive until the backward has been enqueued
            self.args = tuple(t.data_ptr() for t in self.keep)
        else:                                                                          # a tensor on another device is read back (correct, slow)
            self.keep = None
            self.args = tuple((ctypes.c_float * n)(*[float(x) for x in t.detach().reshape(-1).tolist()]) for t, n in zip(ts, (9, 9, 3)))

    def symbol(self, direction):
        return "adgs_flow_loss_%s%s" % (direction, "_devcam" if self.on_device else "")


def _flow_fwd(cam, f, fl, vis, op, dist, out):
    """-> (work, token): the backward reads the number of valid pixels from `work`, so both live with the autograd context."""
    work, tok = _work(f.device, AUX_WORK_DOUBLES)
    _lib.call(cam.symbol("forward"), f.device, fl.shape[1], fl.shape[2], f.data_ptr(), fl.data_ptr(), vis.data_ptr(), _ptr(op), *cam.args, dist, work.data_ptr(), out)
    tok.done()
    return work, tok


def _flow_bwd(cam, f, fl, vis, op, dist, work, g_loss, g_f, g_op):
    _lib.call(cam.symbol("backward"), f.device, fl.shape[1], fl.shape[2], f.data_ptr(), fl.data_ptr(), vis.data_ptr(), _ptr(op), *cam.args, dist, work.data_ptr(),
              g_loss, g_f, g_op)


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_flow, img_opacity, flow, flow_vis, K, R, T, dist):
        if not img_flow.is_cuda:
            raise RuntimeError("get_flow_loss: tensors must be on a HIP device; there is no CPU path")
        f = img_flow.contiguous().float()
        fl, vis = flow.contiguous().float(), flow_vis.contiguous().float()
        op = None if img_opacity is None else img_opacity.contiguous().float()
        H, W = fl.shape[1], fl.shape[2]
        if f.shape != (3, H, W) or fl.shape[0] != 2 or vis.shape != (H, W) or (op is not None and op.numel() != H * W):
            raise ValueError("get_flow_loss: expected img_flow [3,H,W], flow [2,H,W], flow_vis [H,W], img_opacity [H,W]")
        cam = _FlowCam(K, R, T, f.device)
        out = _scalar(f.device, H * W)
        work, ctx.token = _flow_fwd(cam, f, fl, vis, op, float(dist), out.data_ptr())
        ctx.save_for_backward(f, fl, vis, work, *([op] if op is not None else []))
        ctx.cam, ctx.dist, ctx.op_shape = cam, float(dist), None if img_opacity is None else img_opacity.shape
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        f, fl, vis, work, *rest = ctx.saved_tensors
        op = rest[0] if rest else None
        g_f = torch.empty_like(f)
        g_op = torch.empty(fl.shape[1:], dtype=torch.float32, device=f.device) if op is not None else None
        gl = _g1(g_loss)
        _flow_bwd(ctx.cam, f, fl, vis, op, ctx.dist, work, gl.data_ptr(), g_f.data_ptr(), _ptr(g_op))
        return g_f, (g_op.reshape(ctx.op_shape) if g_op is not None else None), None, None, None, None, None, None


def get_flow_loss(img_flow, flow_pkg, img_opacity=None, dist=1e-3):
    """utils/loss_utils.py:86-106: mean over the pixels with a valid flow target of the normalised L1 distance between the
    re-projected rendered flow point and the target, weighted by the accumulated opacity; flow_pkg = (_, K, R, T, flow, flow_vis)
    as in the reference (train.py:68-71).  One reduction pass + one elementwise backward; the reference's nonzero() (a host
    synchronisation) and gathers are gone.  Always returns a tensor: 0 with zero gradients where the reference returns 0.0."""
    _, K, R, T, flow, flow_vis = flow_pkg
    return _FlowLoss.apply(img_flow, img_opacity, flow.detach(), flow_vis.detach(), K, R, T, dist)


def _bce_fwd(p, t, params, out):
    """params: (lo, hi, invert, positive_target) as the native entry takes them."""
    work, tok = _work(p.device, AUX_WORK_DOUBLES)
    _lib.call("adgs_bce_clip_forward", p.device, p.numel(), p.data_ptr(), t.data_ptr(), *params, work.data_ptr(), out)
    tok.done()


def _bce_bwd(p, t, params, g_loss, out):
    _lib.call("adgs_bce_clip_backward", p.device, p.numel(), p.data_ptr(), t.data_ptr(), *params, g_loss, out)


class _BceClip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lo, hi, invert, positive_target):
        if not pred.is_cuda:
            raise RuntimeError("bce_clip_loss: tensors must be on a HIP device; there is no CPU path")
        p, t = pred.contiguous().float(), target.contiguous().float()
        if p.numel() != t.numel():
            raise ValueError("bce_clip_loss: prediction and target must have the same number of elements")
        ctx.params, ctx.shape = (float(lo), float(hi), int(bool(invert)), int(bool(positive_target))), pred.shape
        out = _scalar(p.device, p.numel())
        _bce_fwd(p, t, ctx.params, out.data_ptr())
        ctx.save_for_backward(p, t)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        p, t = ctx.saved_tensors
        out, gl = torch.empty_like(p), _g1(g_loss)
        _bce_bwd(p, t, ctx.params, gl.data_ptr(), out.data_ptr())
        return out.reshape(ctx.shape), None, None, None, None, None


def _bce_weighted_fwd(p, t, w, params, out):
    """-> (work, token): the backward reads sum w from `work`, so both live with the autograd context."""
    work, tok = _work(p.device, AUX_WORK_DOUBLES)
    _lib.call("adgs_bce_clip_weighted_forward", p.device, p.numel(), p.data_ptr(), t.data_ptr(), w.data_ptr(), *params, work.data_ptr(), out)
    tok.done()
    return work, tok


def _bce_weighted_bwd(p, t, w, params, work, g_loss, out):
    _lib.call("adgs_bce_clip_weighted_backward", p.device, p.numel(), p.data_ptr(), t.data_ptr(), w.data_ptr(), *params, work.data_ptr(), g_loss, out)


class _BceClipWeighted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, w, lo, hi, invert, positive_target):
        p, t = pred.contiguous().float(), target.contiguous().float()
        ctx.params, ctx.shape = (float(lo), float(hi), int(bool(invert)), int(bool(positive_target))), pred.shape
        out = _scalar(p.device, p.numel())
        work, ctx.token = _bce_weighted_fwd(p, t, w, ctx.params, out.data_ptr())
        ctx.save_for_backward(p, t, w, work)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        p, t, w, work = ctx.saved_tensors
        out, gl = torch.empty_like(p), _g1(g_loss)
        _bce_weighted_bwd(p, t, w, ctx.params, work, gl.data_ptr(), out.data_ptr())
        return out.reshape(ctx.shape), None, None, None, None, None, None


def bce_clip_loss(pred, target, lo=1e-3, hi=1.0 - 1e-3, invert=False, positive_target=False, weight=None):
    """mean BCE(q, t) with q = clip(pred, lo, hi) (1 - clip(...) with `invert`) and t = target ((target > 0) with `positive_target`).
    weight: an optional float32 [H, W] or [1, H, W] tensor over the H x W elements of `pred` ([H, W] or [1, H, W]): sum w bce / sum w,
    0 with a zero gradient when sum w = 0 (decided on the device)."""
    if weight is None:
        return _BceClip.apply(pred, target.detach(), lo, hi, invert, positive_target)
    if pred.dim() < 2 or pred.numel() != pred.shape[-2] * pred.shape[-1]:
        raise ValueError("bce_clip_loss: with a weight, pred must be [H, W] or [1, H, W], got %s" % (tuple(pred.shape),))
    if pred.numel() != target.numel():
        raise ValueError("bce_clip_loss: prediction and target must have the same number of elements")
    w = _check_weight(weight, pred.shape[-2], pred.shape[-1], pred.device, "bce_clip_loss")
    if not pred.is_cuda or not target.is_cuda:
        raise RuntimeError("bce_clip_loss: tensors must be on a HIP device; there is no CPU path")
    return _BceClipWeighted.apply(pred, target.detach(), w, lo, hi, invert, positive_target)


# (lo, hi, invert, positive_target) of the two BCE terms of a training iteration: obj_loss, sky_loss and the fused _ImageLosses node read these
OBJ_BCE = (1e-3, 1.0 - 1e-3, 0, 1)
SKY_BCE = (1e-3, 1.0 - 1e-3, 1, 0)


def obj_loss(img_semantic, gt_semantic, weight=None):
    """train.py:95-98: binary_cross_entropy(clip(img_semantic, 1e-3, 1 - 1e-3)[0], (gt_semantic > 0).float()); `weight`: see bce_clip_loss."""
    return bce_clip_loss(img_semantic[0] if img_semantic.dim() == 3 else img_semantic, gt_semantic, *OBJ_BCE, weight=weight)


def sky_loss(img_opacity, gt_sky, weight=None):
    """train.py:100-103: binary_cross_entropy(1 - clip(img_opacity, 1e-3, 1 - 1e-3), gt_sky); `weight`: see bce_clip_loss."""
    return bce_clip_loss(img_opacity, gt_sky, *SKY_BCE, weight=weight)


class _LidarDepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, lidar_depth, lidar_mask, inv_depth):
        d = depth.contiguous().float()
        ctx.inv_depth, ctx.shape = int(bool(inv_depth)), depth.shape
        out = _scalar(d.device, d.numel())
        work, ctx.token = _work(d.device, AUX_WORK_DOUBLES)
        if d.numel():
            _lib.call("adgs_lidar_depth_loss_forward", d.device, d.numel(), d.data_ptr(), lidar_depth.data_ptr(), lidar_mask.data_ptr(), ctx.inv_depth,
                      work.data_ptr(), out.data_ptr())
        ctx.token.done()
        ctx.save_for_backward(d, lidar_depth, lidar_mask, work)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        d, lidar_depth, lidar_mask, work = ctx.saved_tensors
        out, gl = torch.empty_like(d), _g1(g_loss)
        if d.numel():
            _lib.call("adgs_lidar_depth_loss_backward", d.device, d.numel(), d.data_ptr(), lidar_depth.data_ptr(), lidar_mask.data_ptr(), ctx.inv_depth,
                      work.data_ptr(), gl.data_ptr(), out.data_ptr())
        return out.reshape(ctx.shape), None, None, None


def lidar_depth_loss(depth, lidar_depth, lidar_mask, inv_depth=False):
    """Sparse metric depth term over the `depth` and `mask` arrays of a lidar_depth/*.npz file (scripts/kitti/kitti.py:185-188,
    scripts/waymo/waymo.py:329, scripts/nuscene/nuscene.py:90): depth is the rendered [H, W] (or [1, H, W]) depth, a pixel is valid iff
    lidar_mask > 0 and lidar_depth > 0 (a bool mask is converted), its target is lidar_depth or, with inv_depth=True, 1 / lidar_depth
    (the rasterizer renders inverse depth under pipe.inv_depth: the caller says which they rendered).
        loss = sum_valid m |depth - target| / sum_valid m
    with no scale or shift fitted (get_depth_loss is the scale/shift-invariant monocular term); 0 with a zero gradient when nothing is
    valid, decided on the device.  One reduction pass and one element-wise backward; differentiable w.r.t. `depth`."""
    for t, name in ((depth, "depth"), (lidar_depth, "lidar_depth"), (lidar_mask, "lidar_mask")):
        if not torch.is_tensor(t):
            raise TypeError("lidar_depth_loss: %s must be a tensor, got %s" % (name, type(t).__name__))
    if depth.dim() < 2 or depth.numel() != depth.shape[-2] * depth.shape[-1]:
        raise ValueError("lidar_depth_loss: depth must be [H, W] or [1, H, W], got %s" % (tuple(depth.shape),))
    if lidar_depth.numel() != depth.numel() or lidar_mask.numel() != depth.numel():
        raise ValueError("lidar_depth_loss: lidar_depth %s and lidar_mask %s must have the %d elements of depth"
                         % (tuple(lidar_depth.shape), tuple(lidar_mask.shape), depth.numel()))
    if lidar_depth.device != depth.device or lidar_mask.device != depth.device:
        raise RuntimeError("lidar_depth_loss: lidar_depth is on %s and lidar_mask on %s, depth on %s" % (lidar_depth.device, lidar_mask.device, depth.device))
    if not depth.is_cuda:
        raise RuntimeError("lidar_depth_loss: tensors must be on a HIP device; there is no CPU path")
    return _LidarDepthLoss.apply(depth, lidar_depth.detach().contiguous().float(), lidar_mask.detach().contiguous().float(), inv_depth)


SMOOTH_WORK_DOUBLES = 256 * 8 + 8        # ADGS_SMOOTH_WORK_DOUBLES


class _DepthSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, guide, w, order, normalize, gamma):
        d = depth.contiguous().reshape(depth.shape[-2:])
        H, W = d.shape
        ctx.args = (H, W, 0 if guide is None else guide.shape[0]), (order, normalize, gamma)
        ctx.shape, ctx.has = depth.shape, (guide is not None, w is not None)
        out = _scalar(d.device, d.numel())
        work, ctx.token = _work(d.device, SMOOTH_WORK_DOUBLES)        # the backward reads the totals, s and L from `work`
        if d.numel():
            _lib.call("adgs_depth_smooth_forward", d.device, *ctx.args[0], d.data_ptr(), _ptr(guide), _ptr(w), *ctx.args[1], work.data_ptr(), out.data_ptr())
        ctx.token.done()
        ctx.save_for_backward(d, work, *[t for t in (guide, w) if t is not None])
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        d, work, *rest = ctx.saved_tensors
        guide = rest.pop(0) if ctx.has[0] else None
        w = rest.pop(0) if ctx.has[1] else None
        out, gl = torch.empty_like(d), _g1(g_loss)
        if d.numel():
            _lib.call("adgs_depth_smooth_backward", d.device, *ctx.args[0], d.data_ptr(), _ptr(guide), _ptr(w), *ctx.args[1], work.data_ptr(), gl.data_ptr(), out.data_ptr())
        return out.reshape(ctx.shape), None, None, None, None, None


def depth_smoothness_loss(depth, image=None, weight=None, order=1, normalize=True, edge_gamma=1.0):
    """Edge-aware smoothness of the rendered depth: the disparity smoothness term of the self-supervised driving pipelines (Monodepth2's
    get_smooth_loss, kornia's inverse_depth_smoothness_loss), defined on what the rasterizer renders under pipe.inv_depth.

    depth: float32 [H, W] or [1, H, W], differentiable.  image: an optional float32 [C, H, W] guide (1 <= C <= 8; use the ground-truth
    image), a constant.  weight: an optional supervision weight (see l1_ssim), a constant.  With Sw = sum w, m = sum w d / Sw and
    s = 1 / (m + 1e-7) (s = 1 with normalize=False):
        order 1, along x:  delta = d(x) - d(x+1),            v = w(x) w(x+1),         a = exp(-edge_gamma mean_c |I(x) - I(x+1)|)
        order 2, along x:  delta = d(x-1) - 2 d(x) + d(x+1),  v = w(x-1) w(x) w(x+1),  a = exp(-edge_gamma mean_c (|I(x) - I(x-1)| + |I(x+1) - I(x)|) / 2)
        loss = s (sum v a |delta| / sum v  [along x]  +  the same along y)
    (a = 1 without an image).  Order 1 penalises every slanted surface; order 2 leaves planes -- whose inverse depth is affine in the pixel
    coordinates: roads, walls -- unpenalised.  The differences are taken on the un-normalised depth and s multiplies the total: the loss of the
    mean-normalised depth (it is homogeneous of degree 1), in one pass.  An axis without a term contributes 0, Sw = 0 gives 0 with a zero
    gradient, both decided on the device.  One stencil pass and a one-block finish forward, one gather backward (include/adgs_loss.h)."""
    who = "depth_smoothness_loss"
    if not torch.is_tensor(depth):
        raise TypeError("%s: depth must be a tensor, got %s" % (who, type(depth).__name__))
    if depth.dim() not in (2, 3) or depth.numel() != depth.shape[-2] * depth.shape[-1]:
        raise ValueError("%s: depth must be [H, W] or [1, H, W], got %s" % (who, tuple(depth.shape)))
    if depth.dtype != torch.float32:
        raise TypeError("%s: depth must be float32, got %s" % (who, depth.dtype))
    H, W = depth.shape[-2:]
    if order not in (1, 2):
        raise ValueError("%s: order must be 1 or 2, got %r" % (who, order))
    gamma = float(edge_gamma)
    if not (0.0 <= gamma < float("inf")):
        raise ValueError("%s: edge_gamma must be finite and >= 0, got %r" % (who, edge_gamma))
    guide = None
    if image is not None:
        if not torch.is_tensor(image):
            raise TypeError("%s: image must be a tensor, got %s" % (who, type(image).__name__))
        if image.dim() != 3 or tuple(image.shape[1:]) != (H, W) or not 1 <= image.shape[0] <= 8:
            raise ValueError("%s: image must be [C, H, W] = [1..8, %d, %d], got %s" % (who, H, W, tuple(image.shape)))
        if image.dtype != torch.float32:
            raise TypeError("%s: image must be float32, got %s" % (who, image.dtype))
        if image.device != depth.device:
            raise RuntimeError("%s: image is on %s, depth on %s" % (who, image.device, depth.device))
        guide = image.detach().contiguous()
    w = None if weight is None else _check_weight(weight, H, W, depth.device, who)
    if not depth.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    return _DepthSmooth.apply(depth, guide, w, int(order), int(bool(normalize)), gamma)


# ---------------------------------------------------------------- neighbourhood regularisers (train.py:104-113)
def _validate_near_idx(idx, N):
    """`param[obj_near_idx]` raises IndexError in the reference when an index lies outside [-N, N) (a stale obj_near_idx after a prune).
    A kernel cannot raise, so every index tensor is checked ONCE per (tensor object, in-place version, N): one min/max read-back when
    set_obj_near_idx / densify_and_prune installs a new tensor (every 10 iterations at most), none afterwards.  The record lives ON the
    tensor object (an attribute: it dies with the object and cannot be inherited by another tensor at the same address).  Skipped under
    stream capture (no read-back possible): there the kernels' own guards apply (NaN loss, no gradient for the affected groups)."""
    if idx.numel() == 0 or torch.cuda.is_current_stream_capturing():
        return
    if getattr(idx, "_adgs_validated", None) == (idx._version, N):
        return
    lo, hi = (int(v) for v in torch.aminmax(idx))
    if lo < -N or hi >= N:
        raise IndexError("obj_near_idx: index %d is out of bounds for dimension 0 with size %d (a stale neighbour index after densify / prune? "
                         "call set_obj_near_idx())" % (lo if lo < -N else hi, N))
    idx._adgs_validated = (idx._version, N)


class _GroupVar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, inner):
        if not x.is_cuda or not idx.is_cuda:
            raise RuntimeError("group variance loss: tensors must be on a HIP device; there is no CPU path")
        if idx.dim() != 2 or idx.dtype != torch.int64:
            raise ValueError("obj_near_idx must be an int64 [G, K] tensor")
        _validate_near_idx(idx, x.shape[0])
        xs, ix = x.contiguous().float(), idx.contiguous()
        N = xs.shape[0]
        D = xs.numel() // max(N, 1)
        G, K = ix.shape
        ctx.dims, ctx.shape = (N, G, K, D, int(inner)), x.shape
        work, tok = _work(xs.device, AUX_WORK_DOUBLES)
        out = _scalar(xs.device, G and D)
        if G and D:
            _lib.call("adgs_group_var_forward", xs.device, *ctx.dims, xs.data_ptr(), ix.data_ptr(), work.data_ptr(), out.data_ptr())
        tok.done()
        ctx.save_for_backward(xs, ix)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        xs, ix = ctx.saved_tensors
        out, gl = torch.zeros_like(xs), _g1(g_loss)
        if ctx.dims[1] and ctx.dims[3]:
            _lib.call("adgs_group_var_backward", xs.device, *ctx.dims, xs.data_ptr(), ix.data_ptr(), gl.data_ptr(), out.data_ptr())
        return out.reshape(ctx.shape), None, None


def reg_loss(xyz_deform_param, obj_near_idx):
    """train.py:104-106: mean(sum(var(xyz_deform_param[obj_near_idx], dim=1), dim=-1)); xyz_deform_param [N,3,C], obj_near_idx [G,K]."""
    return _GroupVar.apply(xyz_deform_param, obj_near_idx, xyz_deform_param.shape[-1])


def reg_sigma_loss(gs_time_sigma, obj_near_idx):
    """train.py:111-113: mean(sum(var(gs_time_sigma[obj_near_idx], dim=1), dim=-1)); gs_time_sigma [N,2]."""
    return _GroupVar.apply(gs_time_sigma, obj_near_idx, gs_time_sigma.shape[-1])


class _SigmaLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_sigma, frame_gap):
        if not log_sigma.is_cuda:
            raise RuntimeError("sigma_loss: tensors must be on a HIP device; there is no CPU path")
        if log_sigma.dim() != 2 or log_sigma.shape[1] != 2:
            raise ValueError("gs_time_sigma must be [N, 2]")
        ls = log_sigma.contiguous().float()
        ctx.gap = float(frame_gap)
        work, tok = _work(ls.device, AUX_WORK_DOUBLES)
        out = _scalar(ls.device, ls.shape[0])
        if ls.shape[0]:
            _lib.call("adgs_sigma_loss_forward", ls.device, ls.shape[0], ls.data_ptr(), ctx.gap, work.data_ptr(), out.data_ptr())
        tok.done()
        ctx.save_for_backward(ls)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        (ls,) = ctx.saved_tensors
        out, gl = torch.empty_like(ls), _g1(g_loss)
        if ls.shape[0]:
            _lib.call("adgs_sigma_loss_backward", ls.device, ls.shape[0], ls.data_ptr(), ctx.gap, gl.data_ptr(), out.data_ptr())
        return out, None


def sigma_loss(gs_time_sigma, frame_gap):
    """train.py:108-110: mean(|frame_gap / mean(exp(gs_time_sigma), dim=-1)|)."""
    return _SigmaLoss.apply(gs_time_sigma, frame_gap)


_WEIGHTS = {}


class _WeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        ctx.save_for_backward(weights)
        ctx.n = len(terms)
        return torch.dot(torch.stack([t.reshape(()) for t in terms]).to(weights.dtype), weights)

    @staticmethod
    def backward(ctx, g):
        (weights,) = ctx.saved_tensors
        gw = g * weights                          # one kernel; the terms' gradients are views of it
        return (None,) + tuple(gw.unbind(0))


def weighted_total(terms):
    """sum_i w_i * L_i of scalar loss terms, [(w_i, L_i), ...] -- what train.py:112-115 writes as a chain of python scalar products
    and sums (two kernels per term forward, two more backward: ~40 launches of 2 - 4 us each per iteration) as one stack, one dot
    product and one scaling in the backward.  Same value up to the order of the float32 additions."""
    terms = [(float(w), t) for w, t in terms if t is not None and not (isinstance(t, (int, float)) and t == 0)]
    if not terms:
        return 0.0
    ref = next(t for _, t in terms if torch.is_tensor(t))
    key = (tuple(w for w, _ in terms), ref.device)
    w = _WEIGHTS.get(key)
    if w is None:                                  # the lambdas are constants of a run: one upload
        if len(_WEIGHTS) > 64:
            _WEIGHTS.clear()
        w = _WEIGHTS[key] = torch.tensor(key[0], dtype=torch.float32, device=ref.device)
    ts = [t if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float32, device=ref.device) for _, t in terms]
    return _WeightedSum.apply(w, *ts)


# ---------------------------------------------------------------- the image terms of train.py:78-99 as ONE autograd node
class _ImageLosses(torch.autograd.Function):
    """L1, SSIM, depth loss, flow loss, object BCE, sky BCE -- the `_*_fwd` / `_*_bwd` pairs of the six functions above, in their order, behind
    one autograd node: six Python-level Function calls forward and six backward (each ~30 us of host time around a 5 - 90 us kernel)
    become two, so the short kernels of this section no longer wait for the host between them (tools/iteration_gaps.py: ~100 us of
    idle GPU per iteration in front of the rasterizer's backward).  Output: a [6] tensor (Ll1, ssim, depth, flow, obj, sky).
    `w`: the checked supervision weight or None; with one, L1 / SSIM and the two BCE terms are the weighted forms and the depth term takes it
    as its mask (the flow term's selection is flow_vis)."""

    @staticmethod
    def forward(ctx, image, depth, img_flow, img_opacity, img_semantic, gt_image, gt_depth, flow, flow_vis, cam, dist, gt_semantic, gt_sky, w):
        if not image.is_cuda:
            raise RuntimeError("image_losses: tensors must be on a HIP device; there is no CPU path")
        f32 = lambda t: t.contiguous().float()
        img, ref = f32(image), f32(gt_image)
        H, W = img.shape[-2:]
        if img.shape != ref.shape or img.dim() != 3:
            raise ValueError("image_losses: image and gt_image must be [C, H, W]")
        dep, gdep = f32(depth).reshape(H, W), f32(gt_depth).reshape(H, W)
        fl_img, op = f32(img_flow), f32(img_opacity).reshape(H, W)
        fl, vis = f32(flow), f32(flow_vis)
        sem = f32(img_semantic[0] if img_semantic.dim() == 3 else img_semantic).reshape(H, W)
        gsem, gsky = f32(gt_semantic).reshape(H, W), f32(gt_sky).reshape(H, W)
        if fl_img.shape != (3, H, W) or fl.shape != (2, H, W) or vis.shape != (H, W):
            raise ValueError("image_losses: expected img_flow [3,H,W], flow [2,H,W], flow_vis [H,W]")
        terms = _scalar(img.device, img.numel(), 6)
        maps = [torch.empty_like(img) for _ in range(3)]
        p0 = terms.data_ptr()
        if w is None:
            _l1_ssim_fwd(img, ref, maps, p0)
            weighted = ()
        else:
            w_ssim, tok_ssim = _l1_ssim_weighted_fwd(img, ref, w, maps, p0)
        w_depth, tok_depth = _depth_fwd(dep, gdep, w, p0 + 8)
        w_flow, tok_flow = _flow_fwd(cam, fl_img, fl, vis, op, float(dist), p0 + 12)
        if w is None:
            _bce_fwd(sem, gsem, OBJ_BCE, p0 + 16)
            _bce_fwd(op, gsky, SKY_BCE, p0 + 20)
            ctx.tokens = (tok_depth, tok_flow)
        else:
            w_obj, tok_obj = _bce_weighted_fwd(sem, gsem, w, OBJ_BCE, p0 + 16)
            w_sky, tok_sky = _bce_weighted_fwd(op, gsky, w, SKY_BCE, p0 + 20)
            weighted = (w, w_ssim, w_obj, w_sky)
            ctx.tokens = (tok_depth, tok_flow, tok_ssim, tok_obj, tok_sky)
        ctx.save_for_backward(img, ref, *maps, dep, gdep, w_depth, fl_img, fl, vis, op, w_flow, sem, gsem, gsky, *weighted)
        ctx.cam, ctx.dist = cam, float(dist)
        ctx.shapes = (image.shape, depth.shape, img_flow.shape, img_opacity.shape, img_semantic.shape)
        return terms

    @staticmethod
    def backward(ctx, g):
        img, ref, d_mu1, d_e11, d_e12, dep, gdep, w_depth, fl_img, fl, vis, op, w_flow, sem, gsem, gsky, *weighted = ctx.saved_tensors
        g = g.contiguous().float()
        p0 = g.data_ptr()
        g_img, g_dep, g_fl = torch.empty_like(img), torch.empty_like(dep), torch.empty_like(fl_img)
        g_op, g_op2, g_sem = torch.empty_like(op), torch.empty_like(op), torch.empty_like(sem)
        if weighted:
            w, w_ssim, w_obj, w_sky = weighted
            _l1_ssim_weighted_bwd(img, ref, w, (d_mu1, d_e11, d_e12), w_ssim, p0, p0 + 4, g_img.data_ptr())
        else:
            w = None
            _l1_ssim_bwd(img, ref, (d_mu1, d_e11, d_e12), p0, p0 + 4, g_img.data_ptr())
        _depth_bwd(dep, gdep, w, w_depth, p0 + 8, g_dep.data_ptr())
        _flow_bwd(ctx.cam, fl_img, fl, vis, op, ctx.dist, w_flow, p0 + 12, g_fl.data_ptr(), g_op.data_ptr())
        if weighted:
            _bce_weighted_bwd(sem, gsem, w, OBJ_BCE, w_obj, p0 + 16, g_sem.data_ptr())
            _bce_weighted_bwd(op, gsky, w, SKY_BCE, w_sky, p0 + 20, g_op2.data_ptr())
        else:
            _bce_bwd(sem, gsem, OBJ_BCE, p0 + 16, g_sem.data_ptr())
            _bce_bwd(op, gsky, SKY_BCE, p0 + 20, g_op2.data_ptr())
        g_op.add_(g_op2)                               # img_opacity feeds the flow loss and the sky loss
        s_img, s_dep, s_fl, s_op, s_sem = ctx.shapes
        if len(s_sem) == 3 and s_sem[0] > 1:           # [D_S, H, W]: only channel 0 enters the object loss (train.py:95-98)
            g_sem_out = torch.zeros(s_sem, dtype=torch.float32, device=img.device)
            g_sem_out[0].copy_(g_sem)
        else:
            g_sem_out = g_sem.reshape(s_sem)
        return (g_img.reshape(s_img), g_dep.reshape(s_dep), g_fl.reshape(s_fl), g_op.reshape(s_op), g_sem_out) + (None,) * 9


def image_losses(image, gt_image, depth, gt_depth, img_flow, flow_pkg, img_opacity, img_semantic, gt_semantic, gt_sky, dist=1e-3, weight=None):
    """The six image terms of a training iteration in one autograd node: returns (Ll1, ssim, depth_loss, flow_loss, obj_loss, sky_loss) --
    bit for bit what l1_ssim, get_depth_loss (no mask), get_flow_loss, obj_loss and sky_loss return for the same arguments
    (utils/loss_utils.py:20-106, train.py:78-99; flow_pkg = (_, K, R, T, flow, flow_vis) as in train.py:68-71).
    weight: an optional supervision weight (see l1_ssim).  With one the node returns what l1_ssim(..., weight), get_depth_loss(..., mask=weight),
    get_flow_loss, obj_loss(..., weight) and sky_loss(..., weight) return.  The flow term is unchanged: its selection comes from flow_vis,
    so fold the mask into it once at load time (`flow_vis * (weight > 0.5)`)."""
    _, K, R, T, flow, flow_vis = flow_pkg
    w = None if weight is None else _check_weight(weight, image.shape[-2], image.shape[-1], image.device, "image_losses")
    cam = _FlowCam(K, R, T, image.device)
    terms = _ImageLosses.apply(image, depth, img_flow, img_opacity, img_semantic, gt_image.detach(), gt_depth.detach(), flow.detach(), flow_vis.detach(),
                               cam, float(dist), gt_semantic.detach(), gt_sky.detach(), w)
    return tuple(terms.unbind(0))
