"""GPU tests of anti-aliased splatting (the opacity-compensated 2D filter, include/adgs_rasterizer.h: adgs_raster_options).

The filter only rescales the opacity, opacity_eff = opacity * k with k a function of the Gaussian's geometry (tests/aa_ref.py).  So the
rasterizer with the filter is checked BY COMPOSITION against the existing oracle: the oracle run on opacity * k gives the images and
dL/d(opacity_eff); the chain through k (torch autograd of the float64 helper) gives the rest -- dL/dopacity = k dL/d(opacity_eff), and
dL/d(opacity_eff) * opacity * dk/d(geometry) added to the oracle's geometry gradients.  The comparison is that of tests/test_gpu_raster.py:
images under the oracle's gate-flip pixel mask, gradients in the strict pass (upstream zeroed at the flagged pixels).  A Gaussian whose
rho lies within float32 rounding of the 2.5e-5 clamp may be clamped on one side only: such rows are treated like gate flips (exempt) and
their number is asserted to be small.
"""
import numpy as np
import pytest
import torch

from adgs import _lib, synthetic
from tests import aa_ref, torch_ref
from tests.parity import assert_close, assert_masked_coverage, assert_rows_conditioned
from tests.test_gpu_raster import GRAD_PAIRS, conditioning_draws, run_oracle

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.cuda()


def settings(sc, aa, scale_modifier=1.0, inv_depth=True, degree=None, bg=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], dev(sc["bg"] if bg is None else bg), scale_modifier,
                                         dev(sc["viewmatrix"]), dev(sc["projmatrix"]), sc["sh_degree"] if degree is None else degree,
                                         dev(sc["campos"]), False, inv_depth, False, aa)


def run_hip(sc, aa=True, colors=None, cov3D=None, flow=True, sem=True, inv_depth=True, scale_modifier=1.0, degree=None, bg=None, grads=None,
            strict_mask=None):
    """tests/test_gpu_raster.py: run_hip with the filter switch."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rast = GaussianRasterizer(settings(sc, aa, scale_modifier, inv_depth, degree, bg))
    leaf = lambda t: None if t is None else t.cuda().clone().requires_grad_(True)
    L = dict(means3D=leaf(sc["means3D"]), means2D=torch.zeros(sc["P"], 3, device="cuda", requires_grad=True), opacities=leaf(sc["opacities"]),
             shs=leaf(sc["shs"]) if colors is None else None, colors=leaf(colors), scales=leaf(sc["scales"]) if cov3D is None else None,
             rotations=leaf(sc["rotations"]) if cov3D is None else None, cov3D=leaf(cov3D), flow=leaf(sc["flow_points"]) if flow else None,
             sem=leaf(sc["semantic"]) if sem else None)
    out = rast(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], shs=L["shs"], colors_precomp=L["colors"], scales=L["scales"],
               rotations=L["rotations"], cov3D_precomp=L["cov3D"], flow_points=L["flow"], semantic=L["sem"])
    color, radii, depth, img_opacity, img_flow, img_sem = out
    res = dict(color=color, radii=radii, depth=depth, img_opacity=img_opacity, img_flow=img_flow, img_semantic=img_sem,
               num_rendered=_lib.frame_stats()["num_rendered"])
    if grads is not None:
        def total(g):
            loss = (color * dev(g["color"])).sum() + (depth * dev(g["depth"])).sum() + (img_opacity * dev(g["img_opacity"])).sum()
            if flow:
                loss = loss + (img_flow * dev(g["flow"])).sum()
            if sem:
                loss = loss + (img_sem * dev(g["semantic"])).sum()
            return loss
        total(grads).backward(retain_graph=strict_mask is not None)
        res["grads"] = {k: (v.grad if v is not None else None) for k, v in L.items()}
        if strict_mask is not None:
            from tests.parity import mask_upstream
            for v in L.values():
                if v is not None:
                    v.grad = None
            total(mask_upstream(grads, strict_mask)).backward()
            res["grads_strict"] = {k: (v.grad if v is not None else None) for k, v in L.items()}
    torch.cuda.synchronize()
    return res


class FilterChain:
    """k of every Gaussian in front of the near plane (float64, with the reference backward's clamp quirk), and the chain through it."""

    def __init__(self, sc, cov3D=None, scale_modifier=1.0):
        m = sc["means3D"].double()
        V = sc["viewmatrix"].double()
        self.near = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64)], 1) @ V)[:, 2] > 0.2
        n = self.near
        self.leaves = dict(means3D=m[n].clone().requires_grad_(True))
        if cov3D is None:
            self.leaves["scales"] = sc["scales"].double()[n].clone().requires_grad_(True)
            self.leaves["rotations"] = sc["rotations"].double()[n].clone().requires_grad_(True)
        else:
            self.leaves["cov3D"] = cov3D.double()[n].clone().requires_grad_(True)
        L = self.leaves
        args = (L["means3D"], V, sc["tanfovx"], sc["tanfovy"], sc["W"], sc["H"])
        self.k_near = aa_ref.filter_factor(*args, scales=L.get("scales"), rotations=L.get("rotations"), cov3D_precomp=L.get("cov3D"),
                                           scale_modifier=scale_modifier, clamp_quirk=True)
        with torch.no_grad():
            rho = aa_ref.filter_rho(*args, scales=L.get("scales"), rotations=L.get("rotations"), cov3D_precomp=L.get("cov3D"), scale_modifier=scale_modifier)
        self.k = torch.ones(m.shape[0], dtype=torch.float64)
        self.k[n] = self.k_near.detach()
        self.rho = torch.full((m.shape[0],), 1.0, dtype=torch.float64)
        self.rho[n] = rho
        self.opacity = sc["opacities"].double()[:, 0]
        self.scale_modifier = scale_modifier

    def scene(self, sc):
        """The scene with the effective opacities (what the oracle without the filter is run on)."""
        out = dict(sc)
        out["opacities"] = (sc["opacities"].double() * self.k[:, None]).float().contiguous()
        return out

    def near_clamp(self, radii, rel=2e-2):
        """Visible Gaussians whose rho lies within float32 rounding of the clamp (relative: det0 is a difference of products)."""
        return (torch.as_tensor(np.asarray(radii)) > 0) & ((self.rho / float(aa_ref.RHO_MIN) - 1.0).abs() < rel)

    def grads(self, og):
        """The filter's gradients from the oracle's gradients on the effective opacities."""
        g_eff = torch.as_tensor(np.asarray(og["dL_dopacity"]), dtype=torch.float64).reshape(-1)
        out = {"dL_dopacity": (g_eff * self.k).numpy().reshape(-1, 1)}
        w = (g_eff * self.opacity)[self.near]
        chain = torch.autograd.grad(self.k_near, list(self.leaves.values()), grad_outputs=w, retain_graph=True)
        names = dict(means3D="dL_dmeans3D", scales="dL_dscales", rotations="dL_drotations", cov3D="dL_dcov3D")
        for (name, leaf), c in zip(self.leaves.items(), chain):
            if name == "scales":      # the reference's scale gradient is taken against scale_modifier * scale (backward.cu:278-341, as the oracle's)
                c = c / self.scale_modifier
            base = torch.as_tensor(np.asarray(og[names[name]]), dtype=torch.float64).reshape(-1, leaf.shape[1]).clone()
            base[self.near] += c
            out[names[name]] = base.numpy()
        return {k: (out[k] if k in out else v) for k, v in og.items()}


def compare_aa(sc, coverage=None, **kw):
    """HIP with the filter against the oracle on opacity * k, composed with the chain through k."""
    grads = kw.get("grads")
    fc = FilterChain(sc, kw.get("cov3D"), kw.get("scale_modifier", 1.0))
    okw = {k: v for k, v in kw.items() if k != "grads"}
    o = run_oracle(fc.scene(sc), grads=grads, strict=True, **okw)
    ex = o["explained"]
    assert_masked_coverage(ex, **({} if coverage is None else dict(limit=coverage)))
    h = run_hip(sc, aa=True, strict_mask=ex["pixel"], **kw)
    np.testing.assert_array_equal(h["radii"].cpu().numpy(), o["radii"])
    edge = fc.near_clamp(o["radii"])
    assert int(edge.sum()) <= max(2, sc["P"] // 10000), "%d Gaussians within rounding of the filter's clamp" % int(edge.sum())
    for k in ("color", "depth", "img_opacity", "img_flow", "img_semantic"):
        assert_close(k, h[k].detach().cpu().numpy(), o[k], explained=ex["pixel"])
    want = fc.grads(o["grads_strict"])
    exempt = lambda hk, a, b: (b.__setitem__(edge.numpy(), a[edge.numpy()]) if edge.any() and hk in ("means3D", "opacities", "scales", "rotations", "cov3D")
                               else None)      # like a gate flip: the two sides may clamp differently
    n, failed = 0, []
    for hk, ok in GRAD_PAIRS:
        got = h["grads_strict"].get(hk)
        if got is None:
            continue
        a = got.cpu().numpy().astype(np.float64)
        b = np.asarray(want[ok], np.float64).reshape(a.shape).copy()
        exempt(hk, a, b)
        try:
            assert_close("aa grad_" + hk, a, b, strict=True)
        except AssertionError as exc:
            failed.append((hk, ok, a, str(exc).splitlines()[0]))
        n += 1
    assert n >= 4
    if failed:
        # tests/test_gpu_raster.py: compare_strict_grads -- a failing tensor is re-examined row by row against the float64 oracle (composed with
        # the same chain), the float32 oracle's own deviation from it being the yardstick (ill-conditioned rotation rows of nearly isotropic Gaussians)
        okw2 = {k: v for k, v in okw.items()}
        exact, pert = conditioning_draws(fc.scene(sc), grads, ex["pixel"], **okw2)
        assert np.array_equal(np.asarray(exact["radii"]), np.asarray(o["radii"])), failed[0][3]
        ex_g = fc.grads(exact["grads_strict"])
        draws = [want] + ([fc.grads(pert["grads_strict"])] if pert is not None and np.array_equal(np.asarray(pert["radii"]), np.asarray(o["radii"])) else [])
        for hk, ok, a, msg in failed:
            f32 = []
            for d in draws:
                b = np.asarray(d[ok], np.float64).reshape(a.shape).copy()
                exempt(hk, a, b)
                f32.append(b)
            e = np.asarray(ex_g[ok], np.float64).reshape(a.shape).copy()
            exempt(hk, a, e)
            assert_rows_conditioned("aa grad_" + hk, a, f32, e, context=msg)
    return h, o, fc


@pytest.mark.parametrize("seed,degree,inv_depth", [(0, 3, True), (1, 2, False), (2, 1, True), (3, 0, True)])
def test_aa_matches_oracle_composition_small(seed, degree, inv_depth):
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=seed, n_objects=2)
    h, o, fc = compare_aa(sc, degree=degree, inv_depth=inv_depth, grads=synthetic.make_upstream_grads(sc, seed))
    vis = h["radii"].cpu() > 0
    assert float(fc.k[vis].min()) < 0.9            # the filter does something on these scenes


def test_aa_colors_precomp_scale_modifier_no_flow_sem():
    sc = synthetic.make_scene(2500, 160, 120, 120.0, seed=9)
    colors = torch.rand(sc["P"], 3, generator=torch.Generator().manual_seed(1))
    compare_aa(sc, colors=colors, scale_modifier=0.7, bg=torch.tensor([0.2, 0.5, 0.9]), grads=synthetic.make_upstream_grads(sc, 9))
    compare_aa(sc, flow=False, sem=False, grads=synthetic.make_upstream_grads(sc, 10))


def test_aa_cov3d_precomp():
    sc = synthetic.make_scene(2000, 160, 120, 120.0, seed=10)
    Sg = aa_ref.cov3d(sc["scales"], sc["rotations"])
    cov3D = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float().contiguous()
    compare_aa(sc, cov3D=cov3D, grads=synthetic.make_upstream_grads(sc, 10))


def test_aa_c2_full_size():
    sc = synthetic.make_config_scene("C2")
    compare_aa(sc, grads=synthetic.make_upstream_grads(sc, 0))


def test_aa_against_dense_float64_reference():
    """Independent of the oracle: tests/torch_ref.render_dense on opacity * k, k in the autograd graph, on tiny scenes with no Gaussian
    outside the frustum clamp and grad_img_opacity = 0 (the conditions under which the reference's backward is the true derivative)."""
    for seed in (0, 1, 2):
        sc = synthetic.make_scene(60, 48, 32, 40.0, sh_degree=3, seed=seed, near_frac=0.05, scale_mult=0.03)
        p, z = sc["means3D"], sc["means3D"][:, 2]
        vis = z > 0.2
        assert bool(((p[:, 0].abs() / z)[vis] < 1.3 * sc["tanfovx"]).all() and ((p[:, 1].abs() / z)[vis] < 1.3 * sc["tanfovy"]).all())
        up = synthetic.make_upstream_grads(sc, seed)
        up["img_opacity"] = torch.zeros_like(up["img_opacity"])
        L = {k: sc[k].double().clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations", "flow_points", "semantic")}
        k = torch.ones(sc["P"], dtype=torch.float64)
        k_vis = aa_ref.filter_factor(L["means3D"][vis], sc["viewmatrix"], sc["tanfovx"], sc["tanfovy"], sc["W"], sc["H"], scales=L["scales"][vis],
                                     rotations=L["rotations"][vis])
        k = k.masked_scatter(vis, k_vis)
        color, radii, depth, op, fl, sem = torch_ref.render_dense(
            L["means3D"], None, L["opacities"] * k[:, None], L["shs"], None, L["scales"], L["rotations"], None, L["flow_points"], L["semantic"],
            sc["bg"], sc["viewmatrix"], sc["projmatrix"], sc["campos"], sc["tanfovx"], sc["tanfovy"], sc["H"], sc["W"], 3, 1.0, True)
        loss = (color * up["color"]).sum() + (depth * up["depth"]).sum() + (fl * up["flow"]).sum() + (sem * up["semantic"]).sum()
        loss.backward()
        h = run_hip(sc, aa=True, grads=up)
        np.testing.assert_array_equal(h["radii"].cpu().numpy(), radii.numpy())
        for name, a, b in (("color", h["color"], color), ("depth", h["depth"], depth), ("img_opacity", h["img_opacity"], op), ("img_flow", h["img_flow"], fl)):
            b = b.detach().numpy()
            np.testing.assert_allclose(a.detach().cpu().numpy(), b, rtol=1e-4, atol=1e-4 * np.abs(b).max(), err_msg=name)
        for hk, lk in (("means3D", "means3D"), ("opacities", "opacities"), ("scales", "scales"), ("rotations", "rotations"), ("shs", "shs")):
            a, b = h["grads"][hk].cpu().numpy(), L[lk].grad.numpy().reshape(h["grads"][hk].shape)
            np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-3 * np.abs(b).max(), err_msg="grad " + hk)


def _model_render(P, W, H, focal, raw_sh, raw_scene, aa, seed=17):
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    sc = synthetic.make_scene(P, W, H, focal, sh_degree=3, seed=seed, n_objects=3)
    camd = synthetic.make_camera(W, H, focal, cam_seed=5)
    model = SyntheticGaussianModel.from_scene(sc, device="cuda", seed=2)
    model.raw_sh, model.raw_scene = raw_sh, raw_scene

    class Pipe:
        inv_depth, debug, antialiasing = True, False, aa
    cam = synthetic.camera_object(camd, time=0.61)
    out = render(cam, model, None, Pipe(), flow_pkg=(0.66, None, None, None, None, None), render_objmask=True)
    up = synthetic.make_upstream_grads(sc, 9)
    d = lambda k: up[k].cuda()
    torch.autograd.backward([out["render"], out["depth"], out["img_opacity"], out["img_flow"]],
                            [d("color"), d("depth")[0], d("img_opacity")[0], d("flow")])
    torch.cuda.synchronize()
    from tests import chain_ref
    grads = {}
    for name in chain_ref.RAW_NAMES:
        p = getattr(model, chain_ref.attr_of(name))
        if p.grad is not None:
            grads[name] = p.grad.detach().cpu().numpy()
    return out, grads


def test_aa_raw_sh_and_raw_scene_render_match_the_plain_entry():
    """gaussian_renderer.render() with pipe.antialiasing: the raw-SH and raw-scene paths (activations inside the preprocess) give what the
    plain entry gives -- images, radii and the gradients of every raw parameter."""
    args = (40000, 640, 400, 620.0)
    ref_out, ref_g = _model_render(*args, raw_sh=False, raw_scene=False, aa=True)
    off_out, _ = _model_render(*args, raw_sh=False, raw_scene=False, aa=False)
    assert torch.equal(ref_out["radii"], off_out["radii"])
    assert not torch.allclose(ref_out["render"], off_out["render"])          # the pipe flag reaches the rasterizer
    for raw_scene in (False, True):
        out, g = _model_render(*args, raw_sh=True, raw_scene=raw_scene, aa=True)
        assert torch.equal(out["radii"], ref_out["radii"])
        for key in ("render", "depth", "img_opacity", "img_flow"):
            assert_close("raw_scene=%s %s" % (raw_scene, key), out[key].detach().cpu().numpy(), ref_out[key].detach().cpu().numpy(), tol=2e-5,
                         max_frac=1e-4, rel_l2=2e-5)
        assert set(g) == set(ref_g)
        for name in g:
            # two HIP runs on different paths: the float atomics' order and the activations' rounding differ
            assert_close("raw_scene=%s grad %s" % (raw_scene, name), g[name], ref_g[name], tol=5e-5, max_frac=1e-4, rel_l2=5e-5)


def _plain_args(sc):
    e = torch.Tensor([])
    return (dev(sc["bg"]), dev(sc["means3D"]), e, dev(sc["opacities"]), dev(sc["scales"]), dev(sc["rotations"]), 1.0, e, dev(sc["viewmatrix"]),
            dev(sc["projmatrix"]), sc["tanfovx"], sc["tanfovy"], sc["H"], sc["W"], dev(sc["shs"]), dev(sc["flow_points"]), dev(sc["semantic"]), 3,
            dev(sc["campos"]), False, True, False)


def test_aa_forward_only_equals_training_forward_and_graph_replay():
    """With the filter the forward-only render gives the training forward's images and radii bit for bit -- plain and raw-SH entries --
    and one HIP-graph replay of the forward-only render equals the eager call."""
    from adgs import graph
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    sc = synthetic.make_scene(30000, 480, 320, 400.0, seed=93, n_objects=2)
    a = _plain_args(sc)
    tr = _C.rasterize_gaussians(*a, antialiasing=True)
    ev = _C.rasterize_gaussians(*a, training=False, antialiasing=True)
    for i in (1, 2, 3, 4, 8, 9):
        assert torch.equal(tr[i], ev[i]), i
    # raw-SH entries through render(): under no_grad the forward-only entry is taken
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    model = SyntheticGaussianModel.from_scene(sc, device="cuda", seed=2)
    model.raw_sh = True
    cam = synthetic.camera_object(synthetic.make_camera(sc["W"], sc["H"], 400.0, cam_seed=3), time=0.4)

    class Pipe:
        inv_depth, debug, antialiasing = True, False, True
    train = render(cam, model, None, Pipe(), render_objmask=True)
    with torch.no_grad():
        evr = render(cam, model, None, Pipe(), render_objmask=True)
    for key in ("render", "depth", "img_opacity", "radii"):
        assert evr[key].grad_fn is None and torch.equal(evr[key], train[key].detach()), key
    # graph replay
    rast = GaussianRasterizer(settings(sc, True))
    t = {k: sc[k].cuda() for k in ("means3D", "opacities", "shs", "scales", "rotations", "flow_points", "semantic")}
    m2 = torch.zeros(sc["P"], 3, device="cuda")

    def fn():
        with torch.no_grad():
            return rast(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                        flow_points=t["flow_points"], semantic=t["semantic"])
    want = [o.clone() for o in fn()]
    assert torch.equal(want[0], ev[1])
    step = graph.GraphedStep(fn)
    got = step()
    torch.cuda.synchronize()
    assert step.validate(repair=False)
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_aa_radii_num_rendered_and_null_options_entries():
    """The filter leaves radii alone and can only drop (cell, Gaussian) pairs; the `_opts` entries with NULL options are the old entries."""
    import ctypes
    from diff_gaussian_rasterization import _C
    sc = synthetic.make_scene(20000, 400, 260, 330.0, seed=41, n_objects=2)
    a = _plain_args(sc)
    on, off = _C.rasterize_gaussians(*a, antialiasing=True), _C.rasterize_gaussians(*a, antialiasing=False)
    assert torch.equal(on[4], off[4])
    assert 0 < on[0] < off[0]
    assert not torch.equal(on[1], off[1])
    # NULL options: bit for bit the old entry -- the binding's own marshalling, with its `_opts` call routed to each in turn
    lib = _lib.lib()
    for old, new in (("adgs_raster_forward", "adgs_raster_forward_opts"), ("adgs_raster_render", "adgs_raster_render_opts")):
        f_old, f_new = getattr(lib, old), getattr(lib, new)
        outs = []
        try:
            for route in (lambda *args: f_new(*(args[:-1] + (None,))), lambda *args: f_old(*args[:-1])):
                setattr(lib, new, route)
                outs.append(_C.rasterize_gaussians(*a, training=(old == "adgs_raster_forward")))
        finally:
            setattr(lib, new, f_new)
        for i in (0, 1, 2, 3, 4, 8, 9):
            x, y = outs[0][i], outs[1][i]
            assert (x == y) if isinstance(x, int) else torch.equal(x, y), (old, i)


def _backward(sc, g, r, geom, binning, img):
    from diff_gaussian_rasterization import _C
    e = torch.Tensor([])
    return _C.rasterize_gaussians_backward(dev(sc["bg"]), dev(sc["means3D"]), r[4], e, dev(sc["scales"]), dev(sc["rotations"]), 1.0, e, dev(sc["viewmatrix"]),
                                           dev(sc["projmatrix"]), sc["tanfovx"], sc["tanfovy"], dev(g["color"]), dev(g["depth"]), dev(g["flow"]), dev(g["semantic"]),
                                           dev(sc["semantic"]), dev(sc["flow_points"]), dev(sc["shs"]), 3, dev(sc["campos"]), geom, r[0], binning, img, r[3],
                                           dev(g["img_opacity"]), True, False)


def test_aa_backward_over_cloned_state_and_classic_agrees_with_v2_at_c3(monkeypatch):
    """A backward over COPIES of the state buffers reads the forward's mode from the image state's header (the frame table does not know
    the copies), for both pipelines; at C3 size the classic pipeline (blend atomics, opacity gradient rescaled in place) and v2 agree."""
    from diff_gaussian_rasterization import _C
    sc = synthetic.make_config_scene("C3")
    g = synthetic.make_upstream_grads(sc, 2)
    a = _plain_args(sc)
    res = {}
    for mode in ("classic", "v2"):
        monkeypatch.setenv("ADGS_RASTER_MODE", mode)
        r = _C.rasterize_gaussians(*a, antialiasing=True)
        monkeypatch.delenv("ADGS_RASTER_MODE")
        want = _backward(sc, g, r, r[5], r[6], r[7])
        got = _backward(sc, g, r, r[5].clone(), r[6].clone(), r[7].clone())
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert_close("cloned state " + mode, x.cpu().numpy(), y.cpu().numpy(), tol=2e-5, max_frac=1e-4, rel_l2=2e-5)
        res[mode] = (r, want)
        # the mode really travels: the same state's backward without the filter would differ in the opacity gradient
        off = _C.rasterize_gaussians(*a, antialiasing=False)
        assert not torch.allclose(_backward(sc, g, off, off[5], off[6], off[7])[2], want[2])
    (rc, gc), (rv, gv) = res["classic"], res["v2"]
    assert torch.equal(rc[4], rv[4])
    for name, i in (("color", 1), ("depth", 2), ("img_opacity", 3), ("img_flow", 8), ("img_semantic", 9)):
        assert_close("classic vs v2 " + name, rc[i].cpu().numpy(), rv[i].cpu().numpy(), max_frac=5e-6)
    for i, name in enumerate(("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "flow", "semantic")):
        if name in ("colors", "cov3D"):          # intermediates the classic pipeline fills and v2 does not hand out
            continue
        assert_close("classic vs v2 grad " + name, gc[i].cpu().numpy(), gv[i].cpu().numpy(), max_frac=2e-4)
