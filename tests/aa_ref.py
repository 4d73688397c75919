"""Float64 torch restatement of the opacity-compensated 2D filter (anti-aliased splatting, include/adgs_rasterizer.h:
adgs_raster_options) -- test infrastructure.

The filter factor of a Gaussian is

    rho = det(Sigma2D) / det(Sigma2D + 0.3 I),   k = sqrt(max(rho, 2.5e-5)),   opacity_eff = opacity * k

with Sigma2D the EWA screen-space covariance before the 0.3 px^2 dilation (preprocess.hip: `cov`, forward.cu:74-113 of the reference,
with the same 1.3 tan-fov frustum clamp of the view-space position).  The rasterizer with the filter on is the rasterizer with the filter
off run on opacity * k, plus the chain through k: the GPU tests compose the existing oracle with this helper.

clamp_quirk=True reproduces what the reference's backward (and preprocess_bwd.hip) differentiates: where the frustum clamp is active the
clamped coordinate is a constant (no gradient to the position through it, backward.cu:199-201 / 228-233).  False: the true derivative
(what torch.autograd.gradcheck checks against finite differences).
"""
import torch

from tests.torch_ref import CLAMP13, LOWPASS, _f, quat_to_R

RHO_MIN = _f(2.5e-5)


def cov3d(scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
    """[P,3,3] world-space covariance: from (scales, un-normalised rotations) as computeCov3D, or the 6 upper-triangle values."""
    if cov3D_precomp is not None:
        c = cov3D_precomp.to(torch.float64)
        return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    R = quat_to_R(rotations.to(torch.float64))
    Mm = R @ torch.diag_embed(_f(scale_modifier) * scales.to(torch.float64))
    return Mm @ Mm.transpose(1, 2)


def cov2d(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0,
          clamp_quirk=False):
    """(a, b, c) = Sigma2D[0][0], Sigma2D[0][1], Sigma2D[1][1] before the dilation, float64, differentiable."""
    dt = torch.float64
    tanfovx, tanfovy = _f(tanfovx), _f(tanfovy)
    V = viewmatrix.to(dt)                  # transposed convention: p_view = p_row @ V
    m = means3D.to(dt)
    p_view = torch.cat([m, torch.ones(m.shape[0], 1, dtype=dt)], 1) @ V
    tx, ty, tz = p_view[:, 0], p_view[:, 1], p_view[:, 2]
    limx, limy = CLAMP13 * tanfovx, CLAMP13 * tanfovy
    txc = torch.clamp(tx / tz, -limx, limx) * tz
    tyc = torch.clamp(ty / tz, -limy, limy) * tz
    if clamp_quirk:
        txc = torch.where((tx / tz).abs() > limx, txc.detach(), txc)
        tyc = torch.where((ty / tz).abs() > limy, tyc.detach(), tyc)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * txc) / (tz * tz), zero, fy / tz, -(fy * tyc) / (tz * tz)], 1).reshape(-1, 2, 3)
    T = J @ V[:3, :3].transpose(0, 1)
    cov = T @ cov3d(scales, rotations, cov3D_precomp, scale_modifier) @ T.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]


def k_from_cov2d(a, b, c):
    """The filter factor of an undilated 2D covariance (a, b, c)."""
    h = LOWPASS
    rho = (a * c - b * b) / ((a + h) * (c + h) - b * b)
    return torch.sqrt(torch.clamp_min(rho, RHO_MIN))


def rho_from_cov2d(a, b, c):
    h = LOWPASS
    return (a * c - b * b) / ((a + h) * (c + h) - b * b)


def filter_factor(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0,
                  clamp_quirk=False):
    """k per Gaussian ([P], float64).  Meaningful for the Gaussians the rasterizer keeps (radii > 0)."""
    return k_from_cov2d(*cov2d(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales, rotations, cov3D_precomp, scale_modifier, clamp_quirk))


def filter_rho(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
    """rho per Gaussian ([P], float64): which side of the 2.5e-5 clamp a Gaussian lies on."""
    return rho_from_cov2d(*cov2d(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales, rotations, cov3D_precomp, scale_modifier))
