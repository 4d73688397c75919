"""CPU checks of the absolute screen-space gradient (AbsGS; include/adgs_rasterizer.h: adgs_raster_backward_options).

  * tests/absgrad_ref.py -- the float64 restatement of the hand-written backward's per-pair position terms -- is pinned to something
    already pinned: its SIGNED sums equal the float64 CPU oracle's dL_dmeans2D on the small seeded scenes of tests/test_oracle_raster.py,
    within the tolerance that file applies to that tensor (rtol 1e-7, atol 1e-9 x scale).  Only then do the GPU tests
    (tests/test_gpu_absgrad.py) trust its absolute sums.
  * the Python plumbing that needs no device: the key render() adds, the leaf the model's statistics read, the ctypes mirror of the
    option block, the refusals of the binding.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from adgs import synthetic
from oracle import oracle
from tests import absgrad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_scene(seed):       # tests/test_oracle_raster.py: small_scene
    return synthetic.make_scene(60, 48, 32, 40.0, sh_degree=3, seed=seed, near_frac=0.05, scale_mult=0.03)


def _weights(sc, seed=0):    # tests/test_oracle_raster.py: _weights
    g = synthetic.make_upstream_grads(sc, seed)
    n = float(sc["H"] * sc["W"])
    return {k: (v * n).to(torch.float64) for k, v in g.items()}


def _oracle_mean2d(sc, wts, colors=None, flow=True, sem=True, inv_depth=True, scale_modifier=1.0, degree=None, opacity=True):
    o = oracle.RasterOracle("f64")
    out = o.forward(sc["bg"], sc["means3D"], colors, sc["opacities"], sc["scales"], sc["rotations"], scale_modifier, None, sc["viewmatrix"],
                    sc["projmatrix"], sc["tanfovx"], sc["tanfovy"], sc["H"], sc["W"], sc["shs"] if colors is None else None,
                    sc["flow_points"] if flow else None, sc["semantic"] if sem else None, sc["sh_degree"] if degree is None else degree,
                    sc["campos"], False, inv_depth)
    g = o.backward(wts["color"], wts["depth"], wts["flow"] if flow else None, wts["semantic"] if sem else None,
                   wts["img_opacity"] if opacity else torch.zeros_like(wts["img_opacity"]))
    return out, g


@pytest.mark.parametrize("seed,kw", [(11, {}), (11, dict(flow=False, sem=False)), (11, dict(inv_depth=False)), (21, {}), (0, dict(degree=3)),
                                     (1, dict(inv_depth=False)), (2, dict(degree=1)), (3, dict(degree=0, scale_modifier=0.7)), (4, dict(degree=2))])
def test_signed_sums_equal_the_oracles_dL_dmeans2D(seed, kw):
    sc = small_scene(seed)
    wts = _weights(sc, seed)
    out, g = _oracle_mean2d(sc, wts, **kw)
    r = absgrad_ref.mean2d_pair_sums(sc, wts, **kw)
    np.testing.assert_array_equal(r["radii"], out["radii"])
    assert (out["radii"] > 0).sum() > 10
    ref = np.asarray(g["dL_dmeans2D"], np.float64).reshape(-1, 3)
    scale = max(np.abs(ref).max(), 1e-12)
    np.testing.assert_allclose(r["signed"], ref, rtol=1e-7, atol=1e-9 * scale + 1e-13)
    # ... and what the absolute sums must satisfy whatever the reference: no cancellation, zero exactly where nothing is replayed
    assert (r["abs"] >= np.abs(r["signed"]) - 1e-12 * scale).all()
    assert (r["abs"][r["pairs"] == 0] == 0).all() and (r["abs"][:, 2] == 0).all()
    multi = r["pairs"] > 1
    assert (r["abs"][multi, :2] > np.abs(r["signed"][multi, :2]) * (1 + 1e-9)).mean() > 0.5       # the two statistics really differ
    single = r["pairs"] == 1
    np.testing.assert_allclose(r["abs"][single], np.abs(r["signed"][single]), rtol=1e-12, atol=0)


def test_signed_sums_with_precomputed_colours_and_without_the_opacity_gradient():
    sc = small_scene(11)
    wts = _weights(sc, 3)
    colors = torch.rand(sc["P"], 3, generator=torch.Generator().manual_seed(5))
    for opacity in (True, False):
        out, g = _oracle_mean2d(sc, wts, colors=colors, opacity=opacity)
        w = dict(wts) if opacity else dict(wts, img_opacity=None)
        r = absgrad_ref.mean2d_pair_sums(sc, w, colors=colors)
        ref = np.asarray(g["dL_dmeans2D"], np.float64).reshape(-1, 3)
        np.testing.assert_allclose(r["signed"], ref, rtol=1e-7, atol=1e-9 * np.abs(ref).max() + 1e-13)


def test_negated_upstream_negates_the_signed_and_keeps_the_absolute_sums():
    sc = small_scene(2)
    wts = _weights(sc, 2)
    a = absgrad_ref.mean2d_pair_sums(sc, wts)
    b = absgrad_ref.mean2d_pair_sums(sc, {k: -v for k, v in wts.items()})
    np.testing.assert_allclose(b["signed"], -a["signed"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(b["abs"], a["abs"], rtol=1e-12, atol=0)


# ---------------------------------------------------------------- plumbing without a device
def test_option_block_is_declared_exported_and_mirrored():
    from adgs import _lib
    header = open(os.path.join(ROOT, "include", "adgs_rasterizer.h")).read()
    assert re.search(r"typedef\s+struct\s+adgs_raster_backward_options\s*\{\s*uint64_t\s+struct_bytes;", header)
    for name, old in (("adgs_raster_backward_opts", "adgs_raster_backward"), ("adgs_raster_backward_rawsh_opts", "adgs_raster_backward_rawsh")):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + 1          # the old entries keep their signatures
    lib = _lib.lib()                                                                       # resolves every declared symbol
    assert ctypes.sizeof(_lib.RasterBackwardOptions) == lib.adgs_test_abi_sizeof(9) == 16
    assert ctypes.sizeof(_lib.RasterOptions) == lib.adgs_test_abi_sizeof(7)                # the forward's block is untouched
    o = _lib.raster_backward_options(0x1000)
    assert o.struct_bytes == 16 and o.dL_dmean2D_abs == 0x1000
    assert _lib.raster_backward_options().dL_dmean2D_abs is None


def test_native_backward_refuses_a_malformed_option_block_before_anything_else():
    """P > 0 and no state buffers: the options are read first, so a malformed block is what the error names (nothing can be launched)."""
    from adgs import _lib
    lib = _lib.lib()
    n_args = len(_lib.SIGNATURES["adgs_raster_backward_opts"][1])
    ints = {0: 10, 1: 3, 2: 16, 3: 0, 4: 1, 6: 32, 7: 32}
    floats = (14, 20, 21)

    def call(opts):
        args = [None] * n_args
        for i, v in ints.items():
            args[i] = v
        for i in floats:
            args[i] = 1.0
        args[-4], args[-3], args[-1] = 1, 0, opts
        return lib.adgs_raster_backward_opts(*args)
    for bad in (0, 8, 15, 5000):
        o = _lib.raster_backward_options(0x1000)
        o.struct_bytes = bad
        assert call(ctypes.byref(o)) < 0
        assert "adgs_raster_backward_options.struct_bytes" in _lib.last_error()
    # a well-formed block gets as far as the missing state buffers
    assert call(ctypes.byref(_lib.raster_backward_options(0x1000))) < 0
    assert "state buffers" in _lib.last_error()
    assert call(None) < 0 and "state buffers" in _lib.last_error()


def test_rasterizer_refuses_a_means2D_abs_that_cannot_receive_a_gradient():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    assert len(GaussianRasterizationSettings._fields) == 14                                  # the switch is an input, not a setting
    for fn in (GaussianRasterizer.forward, GaussianRasterizer.forward_rawsh):
        assert inspect.signature(fn).parameters["means2D_abs"].default is None
    for fn in (_C.rasterize_gaussians_backward, _C.rasterize_gaussians_backward_rawsh):
        assert inspect.signature(fn).parameters["absgrad"].default is False
    z = torch.zeros(3)
    s = GaussianRasterizationSettings(8, 8, 1.0, 1.0, z, 1.0, torch.eye(4), torch.eye(4), 0, z, False, True, False)
    rast = GaussianRasterizer(s)
    m3 = torch.zeros(5, 3, requires_grad=True)
    kw = dict(means3D=m3, means2D=torch.zeros(5, 3, requires_grad=True), opacities=torch.ones(5, 1), colors_precomp=torch.ones(5, 3),
              scales=torch.ones(5, 3), rotations=torch.ones(5, 4))
    with pytest.raises(RuntimeError, match="require grad"):
        rast(means2D_abs=torch.zeros(5, 3), **kw)
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        rast(means2D_abs=torch.zeros(4, 3, requires_grad=True), **kw)
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        rast(means2D_abs=torch.zeros(5, 3, dtype=torch.float64, requires_grad=True), **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="gradients switched off"):
        rast(means2D_abs=torch.zeros(5, 3, requires_grad=True), **kw)
    with pytest.raises(RuntimeError, match="no CPU rasterizer|HIP device"):                  # valid request, CPU tensors: the native path says no
        rast(means2D_abs=torch.zeros(5, 3, requires_grad=True), **kw)


class _FakeRasterizer:
    """Stands in for GaussianRasterizer in gaussian_renderer.render(): records what it is handed, returns images that depend on means2D(_abs)."""
    calls = []

    def __init__(self, raster_settings):
        self.s = raster_settings

    def __call__(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, flow_points=None, semantic=None,
                 **kw):
        _FakeRasterizer.calls.append(dict(kw, means2D=means2D))
        H, W, P = self.s.image_height, self.s.image_width, means3D.shape[0]
        x = means2D.sum() + (2.0 * kw["means2D_abs"].sum() if "means2D_abs" in kw else 0.0)
        img = lambda c: torch.zeros(c, H, W) + x
        return img(3), torch.ones(P, dtype=torch.int32), img(1), img(1), img(3), img(1)


class _Model:
    active_sh_degree = 0

    def __init__(self, n=7):
        self.get_xyz = torch.zeros(n, 3)
        self.get_scaling = torch.ones(n, 3)

    def get_deformed_pkg(self, t):
        n = self.get_xyz.shape[0]
        return dict(xyz=self.get_xyz, rotation=torch.ones(n, 4), opacity=torch.ones(n, 1), shs=torch.zeros(n, 1, 3))


def _pipe(**kw):
    class Pipe:
        inv_depth, debug = True, False
    for k, v in kw.items():
        setattr(Pipe, k, v)
    return Pipe()


def test_render_adds_the_second_leaf_only_when_asked(monkeypatch):
    import gaussian_renderer
    monkeypatch.setattr(gaussian_renderer, "GaussianRasterizer", _FakeRasterizer)
    cam = synthetic.camera_object(synthetic.make_camera(32, 16, 20.0), time=0.5)
    for pipe, want in ((_pipe(), False), (_pipe(absgrad=False), False), (_pipe(absgrad=True), True), (_pipe(absgrad=True, antialiasing=True), True)):
        _FakeRasterizer.calls.clear()
        out = gaussian_renderer.render(cam, _Model(), None, pipe)
        assert ("viewspace_points_abs" in out) is want
        assert ("means2D_abs" in _FakeRasterizer.calls[0]) is want          # without the request the rasterizer is called as it always was
        out["render"].sum().backward()
        assert out["viewspace_points"].grad is not None
        if want:
            leaf = out["viewspace_points_abs"]
            assert leaf is _FakeRasterizer.calls[0]["means2D_abs"] and leaf is not out["viewspace_points"]
            assert leaf.is_leaf and leaf.requires_grad and tuple(leaf.shape) == (7, 3) and float(leaf.detach().abs().max()) == 0.0
            assert torch.equal(leaf.grad, 2.0 * out["viewspace_points"].grad)          # its own gradient, not the signed leaf's
    with torch.no_grad():                                                   # evaluation: no backward can deliver it
        assert "viewspace_points_abs" not in gaussian_renderer.render(cam, _Model(), None, _pipe(absgrad=True))


def test_model_statistics_read_the_absolute_leaf_when_present(monkeypatch):
    from adgs import optim
    from adgs.model import SyntheticGaussianModel
    seen = []
    monkeypatch.setattr(optim, "add_densification_stats", lambda accum, denom, max_radii, grad, radii: seen.append(grad))
    m = SyntheticGaussianModel.__new__(SyntheticGaussianModel)
    m.xyz_gradient_accum = m.denom = m.max_radii2D = None
    signed, absol = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, 3, requires_grad=True)
    signed.grad, absol.grad = torch.full((4, 3), 1.0), torch.full((4, 3), 5.0)
    m.add_densification_stats(dict(viewspace_points=signed, radii=None))
    m.add_densification_stats(dict(viewspace_points=signed, viewspace_points_abs=absol, radii=None))
    assert seen[0] is signed.grad and seen[1] is absol.grad
