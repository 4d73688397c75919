"""Evaluation metrics on the HIP path (include/adgs_metrics.h): what the reference's two evaluation loops do with a rendered view,
render.py:52-93 (`render_set`) and train.py:204-258 (`training_report`), as ONE pass per view and ONE read-back per loop.

    ev = Evaluator(capacity=len(views), regions=2)
    for view in views:
        image = render(view, ...)["render"]                                   # unclipped, under torch.no_grad()
        i, png = ev.add(image, view.original_image, masks=[(view.semantic > 0).float(), view.sky], u8="round")
    res = ev.results()                                                        # the only host synchronisation
    res[0]["mean"]["psnr"], res[0]["mean"]["ssim"], res[1]["psnr"][i]         # whole image; region 1 = the first mask

`add` clips both images to [0, 1] (render.py:54,56), optionally rounds the render to 8 bits first (`quantize`: the metric upstream's
metrics.py computes from the saved PNGs), and accumulates |x - y|, (x - y)^2 and the SSIM map for the whole image and for every mask.
There are TWO PSNRs in the reference and `results()` gives both:
    psnr               10 log10(1 / mse) over the whole image            psnr(render[None], gt[None])   render.py:59
    psnr_channel_mean  the mean of the three per-channel PSNRs           psnr(image, gt).mean()         train.py:258
(utils/image_utils.py:17-19 reduces over shape[0]: the batch of one there, the channels here).  The 8-bit image comes in the two
conversions the reference writes files with: "round" is torchvision.utils.save_image's `x * 255 + 0.5`, clamped, truncated (render.py:64),
"truncate" is `to8b`, `(255 * clip(x)).astype(uint8)` (render.py:39,68); both in H x W x C order, bit for bit the float32 result.

LPIPS (render.py:61-62) is out of scope: it is a pretrained network, not a formula.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_REGIONS = 4        # ADGS_METRICS_MAX_REGIONS
ROW = 8                # ADGS_METRICS_ROW
U8_MODES = {None: 0, "round": 1, "truncate": 2}
METRICS = ("l1", "mse", "psnr", "psnr_channel_mean", "ssim")


class MetricsDesc(ctypes.Structure):
    """adgs_metrics_desc (include/adgs_metrics.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("struct_bytes", "channels", "H", "W", "regions", "quantize", "u8_mode")]


def _desc(channels, H, W, regions, quantize, u8_mode):
    return MetricsDesc(ctypes.sizeof(MetricsDesc), channels, H, W, regions, 1 if quantize else 0, u8_mode)


class Evaluator:
    """The sums of up to `capacity` views, on the device until results().  `regions`: how many masks every add() brings (0 .. 4);
    `quantize`: metrics of the render rounded to 8 bits.  Every add() is enqueued on the current stream of `device` and reads nothing
    back; use one Evaluator from one stream at a time."""

    def __init__(self, capacity, regions=0, quantize=False, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("Evaluator: needs a HIP device; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(capacity) < 1:
            raise ValueError("Evaluator: capacity must be at least 1")
        if not 0 <= int(regions) <= MAX_REGIONS:
            raise ValueError("Evaluator: regions must be 0 .. %d" % MAX_REGIONS)
        self.capacity, self.regions, self.quantize, self.device = int(capacity), int(regions), bool(quantize), device
        # zero on entry, and every call's finishing kernel leaves it zero (the convention of include/adgs_loss.h)
        self.work = torch.zeros(_lib.lib().adgs_metrics_work_doubles(self.regions), dtype=torch.float64, device=device)
        self.table = torch.zeros(self.capacity, 1 + self.regions, ROW, dtype=torch.float64, device=device)
        self.channels = []

    def __len__(self):
        return len(self.channels)

    def reset(self, zero=True):
        """Forget every view: the table is zero again.  zero=False leaves the table as it is (every add() overwrites its view's rows,
        and results() reads only the rows of the views added since): a rewind without a fill kernel."""
        if zero:
            self.table.zero_()
        self.channels = []

    def _masks(self, masks, H, W):
        n = 0 if masks is None else len(masks)
        if n != self.regions:
            raise ValueError("Evaluator.add: %d masks for an Evaluator of %d regions" % (n, self.regions))
        if n == 0:
            return None
        if not torch.is_tensor(masks):
            if any(not torch.is_tensor(m) or tuple(m.shape) != (H, W) for m in masks):
                raise ValueError("Evaluator.add: every mask must be an [H, W] = [%d, %d] tensor" % (H, W))
            if len({(m.dtype, m.device) for m in masks}) != 1:
                raise ValueError("Evaluator.add: the masks differ in dtype or device")
            masks = torch.stack(list(masks))
        if tuple(masks.shape) != (n, H, W):
            raise ValueError("Evaluator.add: masks must be [regions, H, W] = [%d, %d, %d], got %s" % (n, H, W, tuple(masks.shape)))
        if masks.dtype != torch.float32:
            raise TypeError("Evaluator.add: masks must be float32 weights in [0, 1], got %s" % masks.dtype)
        if masks.device != self.device:
            raise RuntimeError("Evaluator.add: masks are on %s, the Evaluator on %s" % (masks.device, self.device))
        return masks.detach().contiguous()

    def add(self, image, gt, masks=None, u8=None):
        """One view: image, gt [C, H, W] float32 on the Evaluator's device (C = 1 or 3; unclipped), masks: `regions` weights in [0, 1]
        as one [regions, H, W] float32 tensor or a sequence of [H, W] ones, u8: None, "round" or "truncate".
        Returns (index of the view, the [H, W, C] uint8 image or None)."""
        if u8 not in U8_MODES:
            raise ValueError("Evaluator.add: u8 must be None, 'round' or 'truncate'")
        if not torch.is_tensor(image) or not torch.is_tensor(gt):
            raise TypeError("Evaluator.add: image and gt must be tensors")
        if image.dim() != 3 or image.shape[0] not in (1, 3) or image.shape[1] < 1 or image.shape[2] < 1:
            raise ValueError("Evaluator.add: image must be [C, H, W] with C = 1 or 3, got %s" % (tuple(image.shape),))
        if gt.shape != image.shape:
            raise ValueError("Evaluator.add: gt %s does not have the image's shape %s" % (tuple(gt.shape), tuple(image.shape)))
        if image.dtype != torch.float32 or gt.dtype != torch.float32:
            raise TypeError("Evaluator.add: image and gt must be float32, got %s and %s" % (image.dtype, gt.dtype))
        if image.device != self.device or gt.device != self.device:
            raise RuntimeError("Evaluator.add: image on %s and gt on %s, the Evaluator on %s; there is no CPU path" % (image.device, gt.device, self.device))
        C, H, W = image.shape
        m = self._masks(masks, H, W)
        index = len(self.channels)
        if index >= self.capacity:
            raise RuntimeError("Evaluator.add: capacity of %d views exceeded" % self.capacity)
        img, ref = image.detach().contiguous(), gt.detach().contiguous()
        out = torch.empty(H, W, C, dtype=torch.uint8, device=self.device) if u8 else None
        desc = _desc(C, H, W, self.regions, self.quantize, U8_MODES[u8])
        _lib.call("adgs_metrics_accumulate", self.device, ctypes.byref(desc), img.data_ptr(), ref.data_ptr(), None if m is None else m.data_ptr(),
                  self.work.data_ptr(), self.table.data_ptr(), index, None if out is None else out.data_ptr())
        self.channels.append(C)
        return index, out

    def results(self):
        """One device-to-host copy of the table -> a list over the regions (0: the whole image, r: mask r - 1) of
        {"l1", "mse", "psnr", "psnr_channel_mean", "ssim": float64 arrays over the views, "weight": the views' sums of weights,
         "count": how many views the region has weight in, "mean": {metric: mean over those views}}.
        mse == 0 gives psnr = inf, as the reference; a view in which a region has no weight is NaN there and left out of the region's means."""
        n = len(self.channels)
        rows = self.table[:n].cpu().numpy()                       # [n, 1 + regions, ROW]
        ch = np.asarray(self.channels, dtype=np.float64)
        out = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for r in range(1 + self.regions):
                row = rows[:, r]
                weight = row[:, 5]
                live = weight > 0
                elements = np.where(live, ch * weight, np.nan)    # NaN, not a division by zero, where the region is empty
                sq = row[:, 1:4]
                mse = sq.sum(1) / elements
                per_channel = 10.0 * np.log10(np.where(live, weight, np.nan)[:, None] / sq)      # [n, 3]; a one-channel view uses column 0
                used = np.arange(3)[None, :] < ch[:, None]
                reg = {"l1": row[:, 0] / elements, "mse": mse, "psnr": 10.0 * np.log10(1.0 / mse),
                       "psnr_channel_mean": np.where(used, per_channel, 0.0).sum(1) / ch, "ssim": row[:, 4] / elements,
                       "weight": weight.copy(), "count": int(live.sum())}
                reg["mean"] = {k: (float(reg[k][live].mean()) if live.any() else float("nan")) for k in METRICS}
                out.append(reg)
        return out


def mse(img1, img2):
    """utils/image_utils.py:14-15: the mean squared difference per entry of dim 0, [N, 1] -- per channel for [C, H, W], per image for
    [B, C, H, W].  No clipping: the callers clip (render.py:54-56, train.py:229-230)."""
    return ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)


def psnr(img1, img2):
    """utils/image_utils.py:17-19, with mse()'s shapes: psnr(a[None], b[None]) is the whole-image PSNR of render.py:59, psnr(a, b).mean() the
    channel mean of train.py:258.  A loop over views wants Evaluator instead: this is the reference's formula on torch tensors."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))


def to8b(image, mode="round"):
    """The 8-bit conversion alone: [C, H, W] float32 on a HIP device -> [H, W, C] uint8, mode "round" (save_image) or "truncate" (to8b).
    The library has one entry point, so this is Evaluator.add of the image against itself with the sums thrown away: the bytes are
    those of add(..., u8=mode) by construction, at the cost of the whole pass (window arithmetic included) plus two small zero fills for
    a one-view Evaluator of its own -- about as much as the five torch passes it replaces.  A loop that also wants the metrics takes the
    bytes from its own add(), where they are free."""
    if mode not in ("round", "truncate"):
        raise ValueError("to8b: mode must be 'round' or 'truncate'")
    if not torch.is_tensor(image) or not image.is_cuda:
        raise RuntimeError("to8b: needs a tensor on a HIP device; there is no CPU path")
    return Evaluator(1, device=image.device).add(image, image, u8=mode)[1]
