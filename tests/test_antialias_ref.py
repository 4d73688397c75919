"""CPU checks of anti-aliased splatting (the opacity-compensated 2D filter): the float64 helper the GPU tests compose with the oracle
(tests/aa_ref.py), the settings tuple that switches it on, and the option block of the C ABI (validated before any device call)."""
import collections
import ctypes
import math

import pytest
import torch

from tests import aa_ref


def _camera(W=320, H=200, focal=250.0):
    tanfovx, tanfovy = W / (2.0 * focal), H / (2.0 * focal)
    view = torch.eye(4, dtype=torch.float64)      # camera at the origin looking down +z (transposed convention: p_view = p_row @ V)
    return view, tanfovx, tanfovy, W, H


def _rand_quat(n, g):
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    return q / q.norm(dim=1, keepdim=True)


def test_isotropic_known_answer():
    """A 2D covariance sigma^2 I gives k = sigma^2 / (sigma^2 + 0.3) -- directly and through the whole projection chain."""
    h = aa_ref.LOWPASS
    for s2 in (1e-3, 0.05, 0.3, 1.0, 7.5, 400.0):
        a = torch.tensor([s2], dtype=torch.float64)
        k = aa_ref.k_from_cov2d(a, torch.zeros_like(a), a)
        want = s2 / (s2 + h)
        if want * want > aa_ref.RHO_MIN:
            assert float(k) == pytest.approx(want, rel=1e-12)
    # on the optical axis, an isotropic 3D Gaussian of scale s at depth z projects to sigma = focal s / z on both axes (equal focals)
    view, tx, ty, W, H = _camera()
    focal = W / (2.0 * aa_ref._f(tx))
    for s, z in ((0.01, 5.0), (0.002, 3.0), (0.05, 40.0)):
        k = aa_ref.filter_factor(torch.tensor([[0.0, 0.0, z]], dtype=torch.float64), view, tx, ty, W, H,
                                 scales=torch.full((1, 3), s, dtype=torch.float64), rotations=torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64))
        s2 = (focal * s / z) ** 2
        assert float(k) == pytest.approx(s2 / (s2 + aa_ref.LOWPASS), rel=1e-6)


def test_degenerate_covariance_is_clamped_with_zero_gradient():
    """det(Sigma2D) = 0 (a needle seen end-on, a rank-1 covariance): k = sqrt(2.5e-5) = 0.005 and no gradient flows."""
    a = torch.tensor([2.0, 1e-9, 3.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([2.0, 0.0, 0.0], dtype=torch.float64, requires_grad=True)
    c = torch.tensor([2.0, 0.0, 1e-12], dtype=torch.float64, requires_grad=True)
    k = aa_ref.k_from_cov2d(a, b, c)
    assert torch.allclose(k, torch.full_like(k, 0.005), rtol=1e-6)
    k.sum().backward()
    for t in (a, b, c):
        assert torch.count_nonzero(t.grad) == 0
    # through the chain: a Gaussian flattened to a line (two zero scales)
    view, tx, ty, W, H = _camera()
    means = torch.tensor([[0.3, -0.2, 6.0]], dtype=torch.float64, requires_grad=True)
    scales = torch.tensor([[0.2, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    rots = torch.tensor([[0.9, 0.1, 0.3, -0.2]], dtype=torch.float64, requires_grad=True)
    k = aa_ref.filter_factor(means, view, tx, ty, W, H, scales=scales, rotations=rots)
    assert float(k.detach()) == pytest.approx(0.005, rel=1e-6)
    k.sum().backward()
    for t in (means, scales, rots):
        assert float(t.grad.abs().max()) == 0.0


def _chain_points(g, n_in=6, n_out=6):
    """Gaussians inside the 1.3 tan-fov clamp and outside it on either axis (none near the clamp's kink)."""
    view, tx, ty, W, H = _camera()
    lim = 1.3
    z = 2.0 + 6.0 * torch.rand(n_in + n_out, generator=g, dtype=torch.float64)
    u = (torch.rand(n_in + n_out, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.8 * lim       # inside: |x/z| <= 0.8 * 1.3 tan
    u[n_in:, 0] = torch.where(torch.arange(n_out) % 2 == 0, 1.6, -1.7) * lim                          # outside on x
    u[n_in + 1::2, 1] = 1.9 * lim                                                                    # ... and some on y too
    means = torch.stack([u[:, 0] * aa_ref._f(tx) * z, u[:, 1] * aa_ref._f(ty) * z, z], 1)
    scales = 0.002 + 0.03 * torch.rand(n_in + n_out, 3, generator=g, dtype=torch.float64)
    rots = _rand_quat(n_in + n_out, g)
    return view, tx, ty, W, H, means, scales, rots


def test_gradcheck_scales_rotations_inside_and_outside_the_clamp():
    g = torch.Generator().manual_seed(3)
    view, tx, ty, W, H, means, scales, rots = _chain_points(g)
    # the filter factor must be above its clamp for a non-trivial check: at these sizes rho spans ~0.01 .. 0.99
    rho = aa_ref.filter_rho(means, view, tx, ty, W, H, scales=scales, rotations=rots)
    assert bool((rho > 10 * aa_ref.RHO_MIN).all())
    f = lambda m, s, q: aa_ref.filter_factor(m, view, tx, ty, W, H, scales=s, rotations=q)
    inputs = tuple(t.clone().requires_grad_(True) for t in (means, scales, rots))
    assert torch.autograd.gradcheck(f, inputs, eps=1e-7, atol=1e-8, rtol=1e-5)


def test_gradcheck_cov3d_precomp_and_scale_modifier():
    g = torch.Generator().manual_seed(4)
    view, tx, ty, W, H, means, scales, rots = _chain_points(g, 4, 4)
    Sg = aa_ref.cov3d(scales, rots)
    cov6 = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1)
    # (one input at a time: the covariance entries are ~1e-4, the positions ~1 -- each gets a step of its own scale)
    fm = lambda m: aa_ref.filter_factor(m, view, tx, ty, W, H, cov3D_precomp=cov6)
    fc = lambda c: aa_ref.filter_factor(means, view, tx, ty, W, H, cov3D_precomp=c)
    assert torch.autograd.gradcheck(fm, (means.clone().requires_grad_(True),), eps=1e-7, atol=1e-8, rtol=1e-5)
    assert torch.autograd.gradcheck(fc, (cov6.clone().requires_grad_(True),), eps=1e-11, atol=1e-6, rtol=1e-5)
    # the same Gaussians through scales / rotations give the same factor; scale_modifier scales the covariance
    k1 = aa_ref.filter_factor(means, view, tx, ty, W, H, cov3D_precomp=cov6)
    k2 = aa_ref.filter_factor(means, view, tx, ty, W, H, scales=scales, rotations=rots)
    assert torch.allclose(k1, k2, rtol=1e-12)
    k3 = aa_ref.filter_factor(means, view, tx, ty, W, H, scales=scales / 0.5, rotations=rots, scale_modifier=0.5)
    assert torch.allclose(k3, k2, rtol=1e-6)
    # a non-trivial view matrix: a rotated, translated camera
    c, s = math.cos(0.3), math.sin(0.3)
    V = torch.tensor([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0.1, -0.2, 0.5, 1]], dtype=torch.float64)
    f = lambda m, sc, q: aa_ref.filter_factor(m, V, tx, ty, W, H, scales=sc, rotations=q)
    assert torch.autograd.gradcheck(f, tuple(t.clone().requires_grad_(True) for t in (means, scales, rots)), eps=1e-7, atol=1e-8, rtol=1e-5)


def test_clamp_quirk_changes_only_the_clamped_gaussians():
    """clamp_quirk=True is what the reference's backward differentiates (the clamped coordinate held constant): the same factor, the same
    gradient inside the clamp, a different one outside it."""
    g = torch.Generator().manual_seed(5)
    view, tx, ty, W, H, means, scales, rots = _chain_points(g)
    grads = []
    for quirk in (False, True):
        m = means.clone().requires_grad_(True)
        k = aa_ref.filter_factor(m, view, tx, ty, W, H, scales=scales, rotations=rots, clamp_quirk=quirk)
        k.sum().backward()
        grads.append((k.detach(), m.grad))
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.allclose(grads[0][1][:6], grads[1][1][:6], rtol=1e-12, atol=0)
    assert not torch.allclose(grads[0][1][6:], grads[1][1][6:])


def test_settings_tuple_takes_13_positional_fields_and_defaults_to_off():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, _antialiasing
    e = torch.zeros(4, 4)
    args = (200, 320, 0.6, 0.4, torch.zeros(3), 1.0, e, e, 3, torch.zeros(3), False, True, False)
    s = GaussianRasterizationSettings(*args)
    assert s.antialiasing is False and len(s) == 14 and s._fields[-1] == "antialiasing"
    assert _antialiasing(s) is False
    s2 = GaussianRasterizationSettings(*args, True)
    assert s2.antialiasing is True and _antialiasing(s2) is True
    assert s._replace(antialiasing=True).antialiasing is True
    # a settings object of the reference's 13 fields (a caller's own tuple) renders without the filter
    Ref = collections.namedtuple("Ref", GaussianRasterizationSettings._fields[:13])
    assert _antialiasing(Ref(*args)) is False


def test_renderer_reads_the_pipeline_flag():
    """gaussian_renderer reads upstream's PipelineParams.antialiasing; a pipe object without it renders without the filter."""
    import gaussian_renderer

    class Pipe:
        inv_depth, debug = True, False

    class Cam:
        image_height, image_width, FoVx, FoVy = 20, 30, 1.0, 0.8
        world_view_transform = torch.eye(4)
        full_proj_transform = torch.eye(4)
        camera_center = torch.zeros(3)

    class PC:
        active_sh_degree = 3

    s = gaussian_renderer._camera_settings(Cam(), PC(), Pipe(), 1.0, torch.device("cpu"))
    assert s.antialiasing is False
    p = Pipe()
    p.antialiasing = True
    assert gaussian_renderer._camera_settings(Cam(), PC(), p, 1.0, torch.device("cpu")).antialiasing is True


def test_raster_options_mirror_and_validation():
    """The ctypes mirror has the C struct's size; a struct_bytes too small for `antialiasing`, or a flag other than 0 / 1, is refused by
    the `_opts` entries before they touch the device."""
    from adgs import _lib
    lib = _lib.lib()
    assert ctypes.sizeof(_lib.RasterOptions) == lib.adgs_test_abi_sizeof(7)
    o = _lib.raster_options(True)
    assert o.struct_bytes == ctypes.sizeof(_lib.RasterOptions) and o.antialiasing == 1
    null_fn = ctypes.cast(None, _lib.ALLOC_FN)
    fwd_args = lambda opts: (null_fn, None, null_fn, None, null_fn, None, 1, 0, 1, 0, None, 16, 16, None, None, None, None, None, None, None,
                             1.0, None, None, None, None, None, 0.5, 0.5, 0, None, None, None, None, None, 0, None, 0, None, opts)
    for bad, what in ((8, "struct_bytes"), (0, "struct_bytes"), (1 << 20, "struct_bytes")):
        b = _lib.raster_options(True)
        b.struct_bytes = bad
        for name in ("adgs_raster_forward_opts", "adgs_raster_render_opts"):
            assert getattr(lib, name)(*fwd_args(ctypes.byref(b))) == -1
            assert what in _lib.last_error()
    b = _lib.raster_options(False)
    b.antialiasing = 2
    assert lib.adgs_raster_forward_opts(*fwd_args(ctypes.byref(b))) == -1 and "0 or 1" in _lib.last_error()
    raw_args = lambda opts: (null_fn, None, null_fn, None, null_fn, None, 1, 0, 1, 0, None, 16, 16, None, None, None, None, None, None, 1.0,
                             None, None, None, None, 0.5, 0.5, None, None, None, None, None, 0, None, 0, None, opts)
    b.antialiasing, b.struct_bytes = 1, 4
    for name in ("adgs_raster_forward_rawsh_opts", "adgs_raster_render_rawsh_opts"):
        assert getattr(lib, name)(*raw_args(ctypes.byref(b))) == -1 and "struct_bytes" in _lib.last_error()
