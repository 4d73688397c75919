"""Bilateral-grid appearance compensation on the HIP path (include/adgs_bilagrid.h): per training image a grid of 3x4 affine
colour transforms, sliced at (pixel x, pixel y, luma) and applied to the rendered image before the losses, so that exposure and
white balance that differ between the cameras of a rig -- and drift along a drive -- are explained by the grid of that image and
not by floaters.  Opt-in: it sits between `render_pkg["render"]` and the losses,

    image = grid(render_pkg["render"], viewpoint_cam.uid)

and nothing else changes.  Evaluation views have no grid and are rendered without one.

`slice` is what `F.grid_sample(grids[index][None], coords, mode="bilinear", padding_mode="border", align_corners=True)` at
coords (x, y, gray) * 2 - 1 followed by the 3x4 affine map computes; `total_variation` is the usual smoothness regulariser.
There is no CPU fallback.
"""
import torch
from torch import nn

from . import _lib
from .loss import _work
from .optim import FusedAdam

TV_WORK_DOUBLES = 256          # ADGS_BILAGRID_TV_WORK_DOUBLES


def identity_grids(num_images, grid_x=16, grid_y=16, grid_w=8, device="cuda"):
    """[N, 12, L, Hg, Wg] with every cell the identity transform: channel 4 i + j is 1 where i == j."""
    g = torch.zeros(num_images, 12, grid_w, grid_y, grid_x, dtype=torch.float32, device=device)
    g[:, [0, 5, 10]] = 1.0
    return g


def _check_grids(grids, who):
    if not grids.is_cuda:
        raise RuntimeError("%s: grids must be on a HIP device; there is no CPU path" % who)
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError("%s: grids must be [N, 12, L, Hg, Wg], got %s" % (who, tuple(grids.shape)))


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, image, index):
        _check_grids(grids, "bilagrid.slice")
        if not image.is_cuda:
            raise RuntimeError("bilagrid.slice: image must be on a HIP device; there is no CPU path")
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError("bilagrid.slice: image must be [3, H, W], got %s" % (tuple(image.shape),))
        if image.device != grids.device:
            raise ValueError("bilagrid.slice: grids live on %s, the image on %s" % (grids.device, image.device))
        N = grids.shape[0]
        if not 0 <= index < N:
            raise IndexError("bilagrid.slice: image index %d, the model holds %d grids" % (index, N))
        g, img = grids.contiguous().float(), image.contiguous().float()
        L, Hg, Wg = g.shape[2:]
        H, W = img.shape[1:]
        out = torch.empty_like(img)
        _lib.call("adgs_bilagrid_slice_forward", g.device, L, Hg, Wg, g[index].data_ptr(), H, W, img.data_ptr(), out.data_ptr())
        ctx.save_for_backward(g, img)
        ctx.index = index
        return out

    @staticmethod
    def backward(ctx, g_out):
        g, img = ctx.saved_tensors
        L, Hg, Wg = g.shape[2:]
        H, W = img.shape[1:]
        go = g_out.contiguous().float()
        d_grids = torch.zeros_like(g) if ctx.needs_input_grad[0] else None          # dense, zero outside `index`
        d_image = torch.empty_like(img) if ctx.needs_input_grad[1] else None
        _lib.call("adgs_bilagrid_slice_backward", g.device, L, Hg, Wg, g[ctx.index].data_ptr(), H, W, img.data_ptr(), go.data_ptr(),
                  d_grids[ctx.index].data_ptr() if d_grids is not None else None, d_image.data_ptr() if d_image is not None else None)
        return d_grids, d_image, None


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        _check_grids(grids, "bilagrid.total_variation")
        g = grids.contiguous().float()
        N, _, L, Hg, Wg = g.shape
        work, tok = _work(g.device, TV_WORK_DOUBLES)
        out = torch.empty(1, dtype=torch.float32, device=g.device)
        _lib.call("adgs_bilagrid_tv_forward", g.device, N, L, Hg, Wg, g.data_ptr(), work.data_ptr(), out.data_ptr())
        tok.done()
        ctx.save_for_backward(g)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        N, _, L, Hg, Wg = g.shape
        gl = g_loss.reshape(1).float().contiguous()
        out = torch.empty_like(g)
        _lib.call("adgs_bilagrid_tv_backward", g.device, N, L, Hg, Wg, g.data_ptr(), gl.data_ptr(), out.data_ptr())
        return out


def slice(grids, image, index):
    """The grid of image `index` (grids [N, 12, L, Hg, Wg]) applied to image [3, H, W]: [3, H, W].  Differentiable in both; the
    gradient of `grids` is dense and zero outside `index`."""
    return _Slice.apply(grids, image, int(index))


def total_variation(grids):
    """(1 / N) sum over the images and the three grid axes of the mean squared difference of adjacent cells (all 12 channels)."""
    return _TotalVariation.apply(grids)


def backward_path(grids, image):
    """"lds" or "global": how the slice kernels run this grid under this image size (adgs_test_bilagrid_path; the choice depends on the
    shapes alone -- a small image under a large grid does not fit the LDS footprint budget)."""
    L, Hg, Wg = grids.shape[-3:]
    H, W = image.shape[-2:]
    return "lds" if _lib.check(_lib.lib().adgs_test_bilagrid_path(L, Hg, Wg, H, W), "adgs_test_bilagrid_path") else "global"


class BilateralGrid:
    def __init__(self, num_images, grid_x=16, grid_y=16, grid_w=8, device="cuda", sparse_adam=False):
        """One [12, grid_w, grid_y, grid_x] grid per training image, initialised to the identity.
        sparse_adam (opt-in): an iteration uses one grid of hundreds; the optimizer's group is marked for the visibility-masked
        step (adgs.optim: one row per image) and step() updates only the grids __call__ was given since the last step -- the others
        keep their parameters and both moments bit for bit instead of decaying towards the moments' fixed point."""
        self.grids = nn.Parameter(identity_grids(num_images, grid_x, grid_y, grid_w, device).requires_grad_(True))
        self.sparse_adam = bool(sparse_adam)
        self._used = torch.zeros(num_images, dtype=torch.uint8, device=self.grids.device) if self.sparse_adam else None
        self.optimizer = None

    def __call__(self, image, index):
        index = int(index)
        out = slice(self.grids, image, index)
        if self._used is not None and torch.is_grad_enabled():
            self._used[index] = 1          # a device fill: no synchronisation
        return out

    def tv_loss(self):
        return total_variation(self.grids)

    def training_setup(self, training_args):
        group = {"params": [self.grids], "lr": getattr(training_args, "bilagrid_lr", 2e-3), "name": "bilagrid"}
        if self.sparse_adam:
            group["visibility_rows"] = "head"
        self.optimizer = FusedAdam([group], lr=0.0, eps=1e-15)

    def step(self, zero_grad=True):
        """The optimizer's step; with sparse_adam only the grids used since the last step."""
        if self.optimizer is None:
            raise RuntimeError("BilateralGrid.step(): call training_setup() first")
        if self._used is None:
            return self.optimizer.step(zero_grad=zero_grad)
        out = self.optimizer.step(zero_grad=zero_grad, visibility=self._used)
        self._used.zero_()
        return out

    def save_weights(self, weights_path):
        torch.save(self.grids, weights_path)

    def load_weights(self, weights_path):
        grids = torch.load(weights_path, map_location=self.grids.device)
        self.grids = nn.Parameter(grids.requires_grad_(True))
