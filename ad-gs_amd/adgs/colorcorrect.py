"""Colour-corrected evaluation on the HIP path (include/adgs_colorcorrect.h): fit a per-image colour transform of a render to its ground
truth, by iterated least squares over the unsaturated pixels, and apply it -- what trainers that ship a bilateral grid do before they
report `cc_psnr` / `cc_ssim`.  A model trained with adgs.bilagrid absorbs per-camera exposure and white balance in the grid; evaluation
views are rendered without one, so their raw metrics count the rig's exposure mismatch as reconstruction error.

    ev, cc_ev = Evaluator(len(views)), Evaluator(len(views))
    for view in views:
        image = render(view, ...)["render"]                                   # unclipped, under torch.no_grad()
        ev.add(image, view.original_image)
        corrected, warp = color_correct(image, view.original_image)           # nothing is read back
        cc_ev.add(corrected, view.original_image)
    ev.results()[0]["mean"]["psnr"], cc_ev.results()[0]["mean"]["psnr"]       # raw and colour-corrected

The whole fit is double precision on the device (a float32 Gram matrix of a near-grey image is not positive definite); per iteration
one accumulate launch and one finishing launch, no intermediate image and no host synchronisation.  `weight` is the region definition
of Evaluator and of the weighted losses: pixels of weight 0 (ego vehicle, invalid borders) do not take part in the fit.  There is no
autograd (this is evaluation) and no CPU fallback.
"""
import ctypes

import torch

from . import _lib

FEATURES = 10          # ADGS_CC_FEATURES: [r, g, b, r^2, rg, rb, g^2, gb, b^2, 1]
MAX_ITERS = 8          # ADGS_CC_MAX_ITERS
MODELS = {"affine": 0, "quadratic": 1}
DEFAULT_EPS = 0.5 / 255
DEFAULT_RIDGE = 1e-6


class CcDesc(ctypes.Structure):
    """adgs_cc_desc (include/adgs_colorcorrect.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("model", ctypes.c_int), ("iters", ctypes.c_int),
                ("eps", ctypes.c_float), ("ridge", ctypes.c_double)]


def _desc(H, W, model, iters, eps, ridge):
    return CcDesc(ctypes.sizeof(CcDesc), H, W, model, iters, eps, ridge)


class ColorWarp:
    """The result of a fit: `warps` [iters, 3, 10] and `support` [iters, 3] (the weighted number of fitted pixels per iteration and
    channel), float64 on the device; `model`, `eps`, `iters`, `ridge` as given.  Row (k, c) maps the feature vector of iteration k's
    input colour to output channel c; an affine warp has zeros in the six quadratic columns.  The warps of a near-grey image are
    ill-conditioned by design: compare what two of them do to an image, not their entries."""

    def __init__(self, warps, support, model, eps, ridge):
        self.warps, self.support, self.model, self.eps, self.ridge = warps, support, model, float(eps), float(ridge)

    @property
    def iters(self):
        return self.warps.shape[0]

    def host(self):
        """(warps, support) as numpy float64 arrays: two device-to-host copies."""
        return self.warps.cpu().numpy(), self.support.cpu().numpy()


def _image(who, name, t):
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor" % (who, name))
    if not t.is_cuda:
        raise RuntimeError("%s: %s is on %s; needs a HIP device, there is no CPU path" % (who, name, t.device))
    if t.dim() != 3 or t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError("%s: %s must be [3, H, W] (a one-channel image has no colour to correct), got %s" % (who, name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    return t.detach().contiguous()


class ColorFitter:
    """Owns the work buffer of the fit on one device (zero between calls: every iteration's finishing launch leaves it so).  Every call
    is enqueued on the current stream of that device; use one ColorFitter from one stream at a time, as an Evaluator."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ColorFitter: needs a HIP device; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.work = torch.zeros(_lib.lib().adgs_cc_work_doubles(), dtype=torch.float64, device=device)

    def fit(self, image, gt, weight=None, model="quadratic", iters=5, eps=DEFAULT_EPS, ridge=DEFAULT_RIDGE):
        """image, gt: [3, H, W] float32 on the fitter's device, unclipped; weight: [H, W] float32 in [0, 1] or None -> ColorWarp."""
        who = "colorcorrect.fit"
        if model not in MODELS:
            raise ValueError("%s: model must be 'affine' or 'quadratic', got %r" % (who, model))
        if not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError("%s: iters must be 1 .. %d" % (who, MAX_ITERS))
        if not 0.0 <= float(eps) < 0.5:
            raise ValueError("%s: eps must be in [0, 0.5)" % who)
        if not 0.0 < float(ridge) < float("inf"):
            raise ValueError("%s: ridge must be positive and finite" % who)
        img, ref = _image(who, "image", image), _image(who, "gt", gt)
        if ref.shape != img.shape:
            raise ValueError("%s: gt %s does not have the image's shape %s" % (who, tuple(ref.shape), tuple(img.shape)))
        if img.device != self.device or ref.device != self.device:
            raise RuntimeError("%s: image on %s and gt on %s, the fitter on %s" % (who, img.device, ref.device, self.device))
        _, H, W = img.shape
        wt = None
        if weight is not None:
            if not torch.is_tensor(weight) or tuple(weight.shape) != (H, W):
                raise ValueError("%s: weight must be an [H, W] = [%d, %d] tensor" % (who, H, W))
            if weight.dtype != torch.float32:
                raise TypeError("%s: weight must be float32 in [0, 1], got %s" % (who, weight.dtype))
            if weight.device != self.device:
                raise RuntimeError("%s: weight is on %s, the image on %s" % (who, weight.device, self.device))
            wt = weight.detach().contiguous()
        iters = int(iters)
        warps = torch.empty(iters, 3, FEATURES, dtype=torch.float64, device=self.device)
        support = torch.empty(iters, 3, dtype=torch.float64, device=self.device)
        desc = _desc(H, W, MODELS[model], iters, float(eps), float(ridge))
        _lib.call("adgs_cc_fit", self.device, ctypes.byref(desc), img.data_ptr(), ref.data_ptr(), None if wt is None else wt.data_ptr(),
                  self.work.data_ptr(), warps.data_ptr(), support.data_ptr())
        return ColorWarp(warps, support, model, eps, ridge)


_fitters = {}


def _fitter(device):
    if device not in _fitters:
        _fitters[device] = ColorFitter(device)
    return _fitters[device]


def fit(image, gt, weight=None, model="quadratic", iters=5, eps=DEFAULT_EPS, ridge=DEFAULT_RIDGE):
    """ColorFitter.fit with the module's fitter of the image's device (one work buffer per device: calls from several streams at a
    time want a ColorFitter each)."""
    _image("colorcorrect.fit", "image", image)
    return _fitter(image.device).fit(image, gt, weight, model, iters, eps, ridge)


def apply(image, warp):
    """The image after all of `warp`'s iterations: [3, H, W] float32, clipped to [0, 1] (it is what goes into an Evaluator, which clips
    anyway).  Any image of the warp's device, not only the one it was fitted on."""
    who = "colorcorrect.apply"
    if not isinstance(warp, ColorWarp):
        raise TypeError("%s: warp must be a ColorWarp" % who)
    img = _image(who, "image", image)
    if warp.warps.device != img.device:
        raise RuntimeError("%s: the warp is on %s, the image on %s" % (who, warp.warps.device, img.device))
    _, H, W = img.shape
    out = torch.empty_like(img)
    desc = _desc(H, W, MODELS[warp.model], warp.iters, warp.eps, warp.ridge)
    _lib.call("adgs_cc_apply", img.device, ctypes.byref(desc), img.data_ptr(), warp.warps.data_ptr(), warp.iters, out.data_ptr())
    return out


def color_correct(image, gt, **kw):
    """(apply(image, warp), warp) with warp = fit(image, gt, **kw)."""
    warp = fit(image, gt, **kw)
    return apply(image, warp), warp
