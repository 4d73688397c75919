"""GPU tests of the absolute screen-space gradient (AbsGS; include/adgs_rasterizer.h: adgs_raster_backward_options.dL_dmean2D_abs,
GaussianRasterizer.forward(means2D_abs=...), gaussian_renderer.render() with pipe.absgrad).

The reference for the new tensor is tests/absgrad_ref.py (a float64 restatement of the hand-written backward's per-pair position terms,
pinned on the CPU to the oracle's signed dL_dmeans2D: tests/test_absgrad_ref.py).  It is compared in the project's strict manner
(tests/parity.py): the oracle's gate-flip pixel mask zeroes the upstream gradients on both sides, its coverage is asserted, and then EVERY
element is held to assert_close(strict=True) -- the rules the signed dL_dmeans2D gets, no tolerance of its own.  The other tests need no
reference: identities that hold for any correct implementation (one pair per Gaussian, the triangle inequality, invariance under a sign
flip of the upstream gradients).
"""
import numpy as np
import pytest
import torch

from adgs import _lib, synthetic
from tests import absgrad_ref
from tests.parity import assert_close, assert_masked_coverage, mask_upstream
from tests.test_gpu_antialias import FilterChain
from tests.test_gpu_raster import compare_strict_grads, conditioning_draws, run_oracle

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.cuda()


def _settings(sc, aa=False, inv_depth=True):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], dev(sc["bg"]), 1.0, dev(sc["viewmatrix"]), dev(sc["projmatrix"]),
                                         sc["sh_degree"], dev(sc["campos"]), False, inv_depth, False, aa)


class Frame:
    """One forward of a scene through the plain or the raw-SH entry, with the second screen-space leaf; backward(grads) runs a backward over
    it (retain_graph: several per forward) and returns (dL_dmeans2D, absolute sums, all leaf gradients)."""

    def __init__(self, sc, aa=False, inv_depth=True, rawsh=False, absgrad=True, semantic=None, flow=True, sem=True):
        from diff_gaussian_rasterization import GaussianRasterizer, RawSH
        from adgs.deform import make_func_eval
        leaf = lambda t: None if t is None else t.cuda().contiguous().clone().requires_grad_(True)
        self.sc, self.flow, self.sem = sc, flow, sem
        self.L = L = dict(means3D=leaf(sc["means3D"]), means2D=torch.zeros(sc["P"], 3, device="cuda", requires_grad=True), opacities=leaf(sc["opacities"]),
                          scales=leaf(sc["scales"]), rotations=leaf(sc["rotations"]), flow=leaf(sc["flow_points"]) if flow else None,
                          sem=leaf(sc["semantic"] if semantic is None else semantic) if sem else None)
        self.abs_leaf = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True) if absgrad else None
        kw = dict(means2D_abs=self.abs_leaf) if absgrad else {}
        rast = GaussianRasterizer(_settings(sc, aa, inv_depth))
        if rawsh:
            Ns, shs = (2 * sc["P"]) // 3, sc["shs"]
            raw = RawSH(leaf(shs[:Ns, :1]), leaf(shs[Ns:, :1]), leaf(shs[:Ns, 1:]), leaf(shs[Ns:, 1:]), torch.zeros(Ns, 3, 0, device="cuda"),
                        torch.zeros(sc["P"] - Ns, 3, 0, device="cuda"), make_func_eval(0.3, [0] * 6, 0))
            out = rast.forward_rawsh(L["means3D"], L["means2D"], L["opacities"], raw, L["scales"], L["rotations"], flow_points=L["flow"], semantic=L["sem"], **kw)
        else:
            L["shs"] = leaf(sc["shs"])
            out = rast(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], shs=L["shs"], scales=L["scales"], rotations=L["rotations"],
                       flow_points=L["flow"], semantic=L["sem"], **kw)
        self.color, self.radii, self.depth, self.img_opacity, self.img_flow, self.img_sem = out

    def backward(self, g):
        for v in list(self.L.values()) + [self.abs_leaf]:
            if v is not None:
                v.grad = None
        loss = (self.color * dev(g["color"])).sum() + (self.depth * dev(g["depth"])).sum() + (self.img_opacity * dev(g["img_opacity"])).sum()
        if self.flow:
            loss = loss + (self.img_flow * dev(g["flow"])).sum()
        if self.sem:
            loss = loss + (self.img_sem * dev(g["semantic"])).sum()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        grads = {k: (v.grad.clone() if v is not None and v.grad is not None else None) for k, v in self.L.items()}
        return grads["means2D"].cpu().numpy().astype(np.float64), (None if self.abs_leaf is None else self.abs_leaf.grad.cpu().numpy().astype(np.float64)), grads


def _scene(name):
    if name == "C1":
        return synthetic.make_config_scene("C1")
    return synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=int(name), n_objects=2)      # tests/test_gpu_raster.py: test_forward_backward_small


@pytest.mark.parametrize("name,aa,inv_depth,rawsh", [("C1", False, True, False), ("C1", True, False, False), ("0", True, True, False), ("1", False, False, False),
                                                      ("2", False, True, True), ("3", True, False, True)])
def test_absolute_sums_match_the_float64_restatement_strictly(name, aa, inv_depth, rawsh):
    sc = _scene(name)
    seed = 0 if name == "C1" else int(name)
    up = synthetic.make_upstream_grads(sc, seed)
    fc = FilterChain(sc) if aa else None
    osc = fc.scene(sc) if aa else sc                  # anti-aliasing: the oracle (gate-flip mask) sees the filtered opacities
    o = run_oracle(osc, inv_depth=inv_depth, grads=up, strict=True)
    ex = o["explained"]
    assert_masked_coverage(ex)
    f = Frame(sc, aa=aa, inv_depth=inv_depth, rawsh=rawsh)
    np.testing.assert_array_equal(f.radii.cpu().numpy(), o["radii"])
    masked = mask_upstream(up, ex["pixel"])
    signed, absol, _ = f.backward(masked)
    ref = absgrad_ref.mean2d_pair_sums(sc, masked, inv_depth=inv_depth, opacity_factor=None if fc is None else fc.k)
    np.testing.assert_array_equal(ref["radii"], o["radii"])
    vis = o["radii"] > 0
    assert vis.sum() > 500 and (ref["pairs"][vis] > 1).mean() > 0.5
    for label, got, want in (("signed dL_dmeans2D vs restatement", signed, ref["signed"]), ("absgrad", absol, ref["abs"])):
        st = assert_close(label, got, want, strict=True)
        print("%s %s aa=%s inv_depth=%s rawsh=%s: rel_l2=%.3g max_err=%.3g scale=%.3g row_p99=%.3g" % (
            label, name, aa, inv_depth, rawsh, st["rel_l2"], st["max_err"], st["scale"], st.get("row_rel_p99", 0.0)))
    # the restatement's signed sums are the oracle's (the CPU pin, once more at this size and in float32)
    assert_close("restatement vs oracle", ref["signed"], np.asarray(o["grads_strict"]["dL_dmeans2D"], np.float64).reshape(-1, 3), strict=True)
    assert (absol[~vis] == 0).all() and (absol[:, 2] == 0).all()


def test_one_hot_upstream_gradient_gives_the_absolute_value_of_the_signed_gradient():
    """A single pixel carries a gradient: every Gaussian has at most one pair, so absgrad == |dL_dmeans2D| to rounding.  No reference."""
    sc = _scene("0")
    for aa, rawsh, rank in ((False, False, 0), (True, True, 7), (False, True, 40)):
        f = Frame(sc, aa=aa, rawsh=rawsh)
        up = synthetic.make_upstream_grads(sc, 5)
        # one of the most opaque pixels of the frame: several Gaussians are blended there
        y, x = divmod(int(torch.argsort(f.img_opacity.detach().reshape(-1), descending=True)[rank]), sc["W"])
        hot = np.zeros((sc["H"], sc["W"]), bool)
        hot[y, x] = True
        signed, absol, _ = f.backward(mask_upstream(up, ~hot))
        assert (np.abs(signed).sum(1) > 0).sum() >= 2                 # the pixel blends several Gaussians
        scale = np.abs(signed).max()
        # one term each, formed in two different orders (dx S0 and L dy combined per Gaussian / A dx + B dy combined per pair): ~8 float32 roundings
        # (u = 6e-8), amplified where A dx and B dy nearly cancel -- relative 1e-5, or 1e-6 of the largest element
        np.testing.assert_allclose(absol, np.abs(signed), rtol=1e-5, atol=1e-6 * scale)


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_triangle_inequality_and_zero_rows_at_full_size(cfg):
    sc = synthetic.make_config_scene(cfg)
    up = synthetic.make_upstream_grads(sc, 0)
    f = Frame(sc)
    signed, absol, _ = f.backward(up)
    vis = f.radii.cpu().numpy() > 0
    assert (absol[~vis] == 0).all() and (absol[:, 2] == 0).all() and (absol >= 0).all() and np.isfinite(absol).all()
    # sums of up to thousands of float32 terms through float atomics, in two different orders: |sum t| <= sum |t| up to the rounding of the
    # sums, which is relative to sum |t| itself (n u with n terms, u = 6e-8; 1e-4 covers 1600 terms at worst-case growth)
    assert (absol[:, :2] >= np.abs(signed[:, :2]) - 1e-4 * absol[:, :2] - 1e-30).all()
    # Strictly greater wherever a Gaussian has two pairs whose terms differ in sign.  A visible Gaussian no pixel blends (behind saturated
    # pixels, or below 1/255 everywhere: most of C3's) has both statistics exactly 0, so the share is taken over the Gaussians that
    # receive a gradient at all; with random upstream gradients two terms agree in sign on both axes with probability 1/4, and a
    # Gaussian that is blended covers several pixels: more than a quarter of them must show the gap (the share of ALL visible ones is reported).
    touched = vis & (absol[:, :2].sum(1) > 0)
    strictly = (absol[:, :2] > 1.01 * np.abs(signed[:, :2])).any(1)
    share, share_vis = float(strictly[touched].mean()), float(strictly[vis].mean())
    ratio = np.linalg.norm(absol[touched, :2], axis=1) / np.maximum(np.linalg.norm(signed[touched, :2], axis=1), 1e-30)
    print("%s: %d visible, %d receive a gradient; absgrad exceeds |dL_dmeans2D| by more than 1 %% on %.1f %% of those (%.1f %% of the visible); median norm ratio %.2f" % (
        cfg, int(vis.sum()), int(touched.sum()), 100 * share, 100 * share_vis, float(np.median(ratio))))
    assert touched.sum() > 10000 and share > 0.25 and share_vis > 0


def test_negated_upstream_gradients_leave_the_absolute_sums_unchanged():
    sc = _scene("1")
    up = synthetic.make_upstream_grads(sc, 1)
    for rawsh in (False, True):
        f = Frame(sc, aa=True, rawsh=rawsh)
        s1, a1, _ = f.backward(up)
        s2, a2, _ = f.backward({k: -v for k, v in up.items()})
        # the same terms with the other sign: only the order of the float atomics differs between two runs
        assert_close("signed", s2, -s1, tol=2e-5, max_frac=1e-4, rel_l2=2e-5)
        assert_close("absgrad", a2, a1, tol=2e-5, max_frac=1e-4, rel_l2=2e-5)
        assert np.abs(a1).max() > 0


def test_signed_gradients_are_unchanged_and_a_second_backward_gives_the_same_sums():
    """A backward that also computes absgrad passes the oracle comparison its signed gradients pass without it; a second backward over the
    same forward (the accumulator lines are zeroed again) repeats the sums."""
    sc = _scene("0")
    up = synthetic.make_upstream_grads(sc, 0)
    o = run_oracle(sc, grads=up, strict=True)
    ex = o["explained"]
    assert_masked_coverage(ex)
    f = Frame(sc)
    masked = mask_upstream(up, ex["pixel"])
    _, a1, g1 = f.backward(masked)
    h = dict(grads_strict={("colors" if k == "colors" else k): v for k, v in g1.items()})
    n = compare_strict_grads(h, o, label="with absgrad ", draws=lambda: conditioning_draws(sc, up, ex["pixel"]))
    assert n >= 8
    _, a2, g2 = f.backward(masked)
    assert_close("absgrad, second backward", a2, a1, tol=2e-5, max_frac=1e-4, rel_l2=2e-5)
    assert_close("dL_dmeans3D, second backward", g2["means3D"].cpu().numpy(), g1["means3D"].cpu().numpy(), tol=2e-5, max_frac=1e-4, rel_l2=2e-5)
    # ... and without the request the same frame gives the same signed gradients (another kernel instantiation, the same sums)
    f0 = Frame(sc, absgrad=False)
    s0, none, g0 = f0.backward(masked)
    assert none is None
    for k in ("means2D", "means3D", "opacities", "shs", "scales", "rotations"):
        assert_close("off vs on " + k, g1[k].cpu().numpy(), g0[k].cpu().numpy(), tol=2e-5, max_frac=1e-4, rel_l2=2e-5)


def test_accumulates_in_the_leafs_grad_over_renders():
    sc = _scene("2")
    up = synthetic.make_upstream_grads(sc, 2)
    f = Frame(sc)
    _, a1, _ = f.backward(up)
    loss = (f.color * dev(up["color"])).sum()
    loss.backward(retain_graph=True)                       # a second backward WITHOUT clearing the leaf: .grad accumulates
    (f.color * dev(up["color"])).sum().backward(retain_graph=True)
    torch.cuda.synchronize()
    f2 = Frame(sc)
    f2.abs_leaf.grad = None
    (f2.color * dev(up["color"])).sum().backward()
    only = f2.abs_leaf.grad.cpu().numpy().astype(np.float64)
    assert_close("accumulated", f.abs_leaf.grad.cpu().numpy().astype(np.float64), a1 + 2 * only, tol=2e-5, max_frac=1e-4, rel_l2=2e-5)


def test_unsupported_requests_raise_and_launch_nothing(monkeypatch):
    sc = synthetic.make_scene(2000, 160, 96, 120.0, sh_degree=3, seed=4, n_objects=2)
    up = synthetic.make_upstream_grads(sc, 4, D_S=3)
    sem3 = torch.rand(sc["P"], 3, generator=torch.Generator().manual_seed(3))
    # D_S > 1 with a semantic gradient: refused by name, and the leaves stay without gradients
    f = Frame(sc, semantic=sem3)
    with pytest.raises(RuntimeError, match="D_S > 1 semantic channels"):
        f.backward(up)
    assert f.abs_leaf.grad is None and f.L["means3D"].grad is None
    # ... the same frame without the semantic gradient is served
    f.sem = False
    _, a, _ = f.backward(up)
    assert np.abs(a).max() > 0
    # the classic pipeline does not form the sums: refused, never zeros
    monkeypatch.setenv("ADGS_RASTER_MODE", "classic")
    fcl = Frame(sc)
    monkeypatch.delenv("ADGS_RASTER_MODE")
    with pytest.raises(RuntimeError, match="classic pipeline"):
        fcl.backward(synthetic.make_upstream_grads(sc, 4))
    assert fcl.abs_leaf.grad is None
    # a leaf that cannot receive the result
    from diff_gaussian_rasterization import GaussianRasterizer
    with pytest.raises(RuntimeError, match="require grad"):
        GaussianRasterizer(_settings(sc))(means3D=dev(sc["means3D"]).requires_grad_(True), means2D=torch.zeros(sc["P"], 3, device="cuda"), opacities=dev(sc["opacities"]),
                                          shs=dev(sc["shs"]), scales=dev(sc["scales"]), rotations=dev(sc["rotations"]), means2D_abs=torch.zeros(sc["P"], 3, device="cuda"))
    assert _lib.lib().adgs_device_check() == 0


def test_graph_replay_delivers_the_absolute_sums():
    """A captured training frame (adgs.graph.GraphedStep) carries the request like any other kernel argument."""
    from adgs import graph
    sc = _scene("3")
    up = synthetic.make_upstream_grads(sc, 3)
    f = Frame(sc)
    _, want, _ = f.backward(up)
    from diff_gaussian_rasterization import GaussianRasterizer
    rast = GaussianRasterizer(_settings(sc))
    t = {k: dev(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    gc, gd, go = dev(up["color"]), dev(up["depth"]), dev(up["img_opacity"])
    gf, gs = dev(up["flow"]), dev(up["semantic"])
    fl, se = dev(sc["flow_points"]), dev(sc["semantic"])

    def fn():
        m2, m2a = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True), torch.zeros(sc["P"], 3, device="cuda", requires_grad=True)
        c, r, d, o, ifl, ise = rast(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                                    flow_points=fl, semantic=se, means2D_abs=m2a)
        ga, = torch.autograd.grad((c * gc).sum() + (d * gd).sum() + (o * go).sum() + (ifl * gf).sum() + (ise * gs).sum(), [m2a])
        return ga
    eager = fn().clone()
    step = graph.GraphedStep(fn)
    got = step()
    torch.cuda.synchronize()
    assert step.validate(repair=False)
    for name, x in (("eager", eager), ("replayed", got)):
        assert_close("absgrad " + name, x.cpu().numpy().astype(np.float64), want, tol=2e-5, max_frac=1e-4, rel_l2=2e-5)


def test_render_to_densification_statistics_end_to_end():
    """render(pipe.absgrad) -> loss -> backward -> model.add_densification_stats: the accumulator receives the norm of
    viewspace_points_abs.grad[:, :2] at the visible Gaussians, and that differs from the signed statistic."""
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    P, W, H, focal = 40000, 640, 400, 620.0
    sc = synthetic.make_scene(P, W, H, focal, sh_degree=3, seed=17, n_objects=3)
    up = synthetic.make_upstream_grads(sc, 9)
    cam = synthetic.camera_object(synthetic.make_camera(W, H, focal, cam_seed=5), time=0.61)
    res = {}
    for raw_sh, raw_scene in ((False, False), (True, False), (True, True)):
        for absgrad in (True, False):
            model = SyntheticGaussianModel.from_scene(sc, device="cuda", seed=2)
            model.raw_sh, model.raw_scene = raw_sh, raw_scene
            model.training_setup()

            class Pipe:
                inv_depth, debug, antialiasing = True, False, False
            Pipe.absgrad = absgrad
            out = render(cam, model, None, Pipe(), flow_pkg=(0.66, None, None, None, None, None), render_objmask=True)
            assert ("viewspace_points_abs" in out) is absgrad
            torch.autograd.backward([out["render"], out["depth"], out["img_opacity"], out["img_flow"]],
                                    [dev(up["color"]), dev(up["depth"])[0], dev(up["img_opacity"])[0], dev(up["flow"])])
            before = model.xyz_gradient_accum.clone()
            assert float(before.abs().max()) == 0.0
            model.add_densification_stats(out)
            torch.cuda.synchronize()
            leaf = out["viewspace_points_abs" if absgrad else "viewspace_points"]
            vis = out["radii"] > 0
            want = torch.where(vis, leaf.grad[:, :2].norm(dim=1), torch.zeros_like(vis, dtype=torch.float32))
            got = model.xyz_gradient_accum.reshape(-1)
            assert_close("xyz_gradient_accum", got.cpu().numpy(), want.cpu().numpy(), tol=1e-6, max_frac=0, rel_l2=1e-6)
            assert torch.equal(model.denom.reshape(-1) > 0, vis)
            if absgrad:
                assert out["viewspace_points"].grad is not None          # the signed leaf still gets its gradient
                a, s = leaf.grad, out["viewspace_points"].grad
                assert bool((a[:, :2] >= s[:, :2].abs() * (1 - 1e-4)).all())
            res[(raw_sh, raw_scene, absgrad)] = got.cpu().numpy().astype(np.float64)
        on, off = res[(raw_sh, raw_scene, True)], res[(raw_sh, raw_scene, False)]
        assert (on >= off * (1 - 1e-4)).all() and (on > 1.01 * off).mean() > 0.25, (raw_sh, raw_scene)
    # the three entries of render() agree on the statistic (two HIP runs on different paths: atomics' order, activations' rounding)
    for key in ((True, False, True), (True, True, True)):
        assert_close("statistic %s" % (key,), res[key], res[(False, False, True)], tol=5e-5, max_frac=1e-4, rel_l2=5e-5)
