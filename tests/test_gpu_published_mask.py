"""GPU tests of the forward's "published" mask (a byte per Gaussian) and of the preprocess backward that reads nothing of a Gaussian whose byte is 0
(api.hip: GeomStateV2::published; render_v2.hip: flush_chunk; preprocess_bwd.hip: load_preb_in; switch: ADGS_PUBLISHED_MASK=0).

A Gaussian whose byte is 0 had an all-zero accumulator line, so each of its outputs was +-0 with the mask off and is +0 with it on, and a
published Gaussian is computed by unchanged code: EVERY gradient tensor of a frame must compare equal element for element under `==`
between ADGS_PUBLISHED_MASK unset and =0.  No tolerance; -0 == +0; a NaN on either side fails.

How the two sides see the same sums.  The blend backward adds a Gaussian's per-tile sums with float atomics, which commute but do not
associate: two runs of it differ in the last bits wherever a Gaussian covers more than two tiles (tests/test_gpu_optim.py), with or
without this mask.  `==` is a statement about the PREPROCESS backward, so both sides are given the same accumulator lines: frame A (switch
unset) runs forward and backward as usual; frame B (switch =0) runs its own forward, then its geometry state is overwritten with A's state as
A's backward left it (same scene, same layout) and B's backward is called without the binning state (R = 0), which skips the blend backward and
leaves the lines as they are (the first backward over a forward does not zero them).  B is therefore the mask-off preprocess backward over
exactly the lines A's mask-on preprocess backward read.  Channels >= 1 of dL_dsemantic come from the extra replays of the blend backward,
which B skips: with D_S = 2 channel 0 (the preprocess backward's) is compared.

Every geometry state is filled with 0xFF bytes when it is allocated: a mask that only works on fresh zero pages fails here.  `poison`
runs: the lines of the unpublished Gaussians are overwritten with NaN before a replayed backward -- with the mask on nothing changes (the
lines are not read), with the switch at 0 the NaNs come out (the switch really switches the mask off).
"""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from adgs import _lib, synthetic
from tests.parity import assert_close

pytestmark = pytest.mark.gpu

ENV = "ADGS_PUBLISHED_MASK"


def dev(t):
    return None if t is None else t.cuda()


class Tap:
    """Wraps the native backward bindings: records the geometry state a backward ran over; mode 'replay' first overwrites the state with a
    kept one and drops the binning state (module docstring).  Also fills every state buffer with 0xFF at allocation."""

    def __init__(self, monkeypatch):
        from diff_gaussian_rasterization import _C
        self.mode, self.kept, self.last, self.poison = "plain", None, None, None
        for name in ("rasterize_gaussians_backward", "rasterize_gaussians_backward_rawsh"):
            monkeypatch.setattr(_C, name, self._wrap(getattr(_C, name)))

        def alloc(user, nbytes):
            t = _C._Buffer._tls.slots[user]
            t.resize_(int(nbytes))
            t.fill_(0xFF)
            return t.data_ptr()
        self._cb = _lib.ALLOC_FN(alloc)
        monkeypatch.setattr(_C, "_ALLOC_CB", self._cb)

    def _wrap(self, orig):
        sig = inspect.signature(orig)

        def wrapped(*a, **kw):
            b = sig.bind(*a, **kw)
            ar = b.arguments
            geom = ar["geomBuffer"]
            if self.mode == "replay":
                assert geom.shape == self.kept.shape and geom.data_ptr() != self.kept.data_ptr()
                geom.data.copy_(self.kept)
                if self.poison is not None:
                    P = ar["means3D"].size(0)
                    lines = geom.data[self.poison[0]:self.poison[0] + 64 * P].view(torch.float32).view(P, 16)
                    lines[self.poison[1]] = float("nan")
                ar["R"] = 0
                ar["binningBuffer"] = torch.empty(0, dtype=torch.uint8, device=geom.device)
            res = orig(*b.args, **b.kwargs)
            self.last = dict(geom=geom, P=ar["means3D"].size(0), radii=ar["radii"])
            return res
        wrapped.__signature__ = sig
        return wrapped


@pytest.fixture
def tap(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    return Tap(monkeypatch)


def read_state(last):
    """(published [P] bool, lines [P,16] float32, the mask's bytes) of a geometry state, through the test hook."""
    lib, P = _lib.lib(), last["P"]
    raw, lines = np.full(P, 7, np.uint8), np.zeros((P, 16), np.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.adgs_test_v2_published_mask(last["geom"].data_ptr(), P, raw.ctypes.data, lines.ctypes.data, st) == P
    assert (raw <= 1).all(), "every byte of the mask is 0 (zeroed by the forward's preprocess) or 1 (set by the blend)"
    return raw == 1, lines, raw


def offsets(P):
    out = (ctypes.c_longlong * 2)()
    assert _lib.lib().adgs_test_v2_geom_offsets(P, out) == 0
    return int(out[0]), int(out[1])


def check_superset(bits, lines, radii):
    vis = radii.cpu().numpy() > 0
    touched = vis & (lines != 0).any(1)      # (the line of a culled Gaussian is never zeroed, added to or read: whatever the allocation held)
    assert not (touched & ~bits).any(), "a Gaussian with a non-zero accumulator word is not published"
    assert not (bits & ~vis).any(), "a published Gaussian is not visible"
    return vis


def assert_equal_grads(ga, gb, what):
    assert ga.keys() == gb.keys()
    n = 0
    for k in ga:
        a, b = ga[k], gb[k]
        assert (a is None) == (b is None), (what, k)
        if a is None:
            continue
        assert a.shape == b.shape, (what, k)
        same = (a == b)
        assert bool(same.all()), "%s: %s differs between mask on and off in %d of %d elements (NaNs: %d / %d)" % (
            what, k, int((~same).sum()), a.numel(), int(torch.isnan(a).sum()), int(torch.isnan(b).sum()))
        n += 1
    assert n >= 4, (what, n)


def zero_rows_are_zero(g, bits, keys):
    """With the mask on the rows of an unpublished Gaussian are +0 (the zero-row branch), bit for bit."""
    clear = torch.from_numpy(~bits).cuda()
    for k in keys:
        if g.get(k) is not None and g[k].shape[0] == clear.shape[0]:
            rows = g[k][clear]
            assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any()), k


# ---------------------------------------------------------------- static scenes through the two rasterizer entries
class Static:
    """A static scene through GaussianRasterizer.forward (materialised [P,M,3] SH) or forward_rawsh (raw SH split at Ns, no deformation)."""

    def __init__(self, sc, rawsh=False, degree=None, aa=False, absgrad=False, sem=None, Ns=None):
        self.sc, self.rawsh, self.aa, self.absgrad, self.sem, self.Ns = sc, rawsh, aa, absgrad, sem, Ns
        self.degree = sc["sh_degree"] if degree is None else degree

    def forward(self):
        from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, RawSH
        from adgs.deform import make_func_eval
        sc = self.sc
        leaf = lambda t: t.cuda().contiguous().clone().requires_grad_(True)
        s = GaussianRasterizationSettings(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], dev(sc["bg"]), 1.0, dev(sc["viewmatrix"]), dev(sc["projmatrix"]),
                                          self.degree, dev(sc["campos"]), False, True, False, self.aa)
        L = dict(means3D=leaf(sc["means3D"]), means2D=torch.zeros(sc["P"], 3, device="cuda", requires_grad=True), opacities=leaf(sc["opacities"]),
                 scales=leaf(sc["scales"]), rotations=leaf(sc["rotations"]), flow=leaf(sc["flow_points"]),
                 sem=leaf(sc["semantic"] if self.sem is None else self.sem))
        kw = {}
        if self.absgrad:
            L["means2D_abs"] = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True)
            kw = dict(means2D_abs=L["means2D_abs"])
        rast = GaussianRasterizer(s)
        if self.rawsh:
            Ns, shs = (2 * sc["P"]) // 3 if self.Ns is None else self.Ns, sc["shs"]
            for n, t in (("scene_dc", shs[:Ns, :1]), ("obj_dc", shs[Ns:, :1]), ("scene_rest", shs[:Ns, 1:]), ("obj_rest", shs[Ns:, 1:])):
                L[n] = leaf(t)
            raw = RawSH(L["scene_dc"], L["obj_dc"], L["scene_rest"], L["obj_rest"], torch.zeros(Ns, 3, 0, device="cuda"),
                        torch.zeros(sc["P"] - Ns, 3, 0, device="cuda"), make_func_eval(0.3, [0] * 6, 0))
            out = rast.forward_rawsh(L["means3D"], L["means2D"], L["opacities"], raw, L["scales"], L["rotations"], flow_points=L["flow"], semantic=L["sem"], **kw)
        else:
            L["shs"] = leaf(sc["shs"])
            out = rast(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], shs=L["shs"], scales=L["scales"], rotations=L["rotations"],
                       flow_points=L["flow"], semantic=L["sem"], **kw)
        self.L, self.out = L, out
        return out

    def backward(self, up, retain=False):
        for v in self.L.values():
            v.grad = None
        color, radii, depth, op, fl, se = self.out
        torch.autograd.backward([color, depth, op, fl, se], [dev(up["color"]), dev(up["depth"]), dev(up["img_opacity"]), dev(up["flow"]), dev(up["semantic"])],
                                retain_graph=retain)
        torch.cuda.synchronize()
        g = {k: (None if v.grad is None else v.grad.clone()) for k, v in self.L.items()}
        if g["sem"] is not None and g["sem"].shape[1] > 1:
            g["sem"] = g["sem"][:, :1].clone()      # channels >= 1: the blend backward's own replays (module docstring)
        return g


def run_pair(tap, monkeypatch, make, up, env=None, poison=False):
    """Frame A: switch unset, forward + backward.  Frame B: switch = 0, forward, then the preprocess backward alone over A's state.
    Returns (A's gradients, B's, bits, lines, radii, A's frame).  poison: two more replays over NaN-filled unpublished lines."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(ENV, raising=False)
    tap.mode, tap.poison = "record", None
    fa = make()
    fa.forward()
    ga = fa.backward(up)
    rec = tap.last
    bits, lines, _ = read_state(rec)
    vis = check_superset(bits, lines, rec["radii"])

    def replay(switch, poisoned):
        if switch is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, switch)
        f = make()
        f.forward()
        tap.mode, tap.kept = "replay", rec["geom"]
        tap.poison = (offsets(rec["P"])[1], torch.from_numpy(~bits).cuda()) if poisoned else None
        try:
            return f.backward(up)
        finally:
            tap.mode, tap.poison = "record", None
    gb = replay("0", False)
    if poison and (vis & ~bits).any():
        assert_equal_grads(ga, replay(None, True), "NaN in the unpublished lines, mask on")      # ... which the masked backward never reads
        gp = replay("0", True)
        assert any(v is not None and bool(torch.isnan(v).any()) for v in gp.values()), "ADGS_PUBLISHED_MASK=0 did not switch the mask off"
    monkeypatch.delenv(ENV, raising=False)
    for k in (env or {}):
        monkeypatch.delenv(k)
    tap.mode = "plain"
    return ga, gb, bits, lines, rec["radii"], fa


def occluded_scene(P=8192, W=96, H=64, focal=80.0, seed=5):
    """Three layers of 8 x 8 large, nearly opaque Gaussians in front of everything else (ids 0 .. 191: three waves, all published), one wave of
    tiny Gaussians straight behind the centres of the front ones (ids 192 .. 255: visible, never blended) and a random cloud behind."""
    sc = synthetic.make_scene(P, W, H, focal, sh_degree=3, seed=seed, n_objects=0, near_frac=0.0)
    g = torch.Generator().manual_seed(seed)
    cx = (torch.arange(8).float() + 0.5) / 8 * 2 - 1
    gy, gx = torch.meshgrid(cx, cx, indexing="ij")
    for layer in range(3):
        z = 2.0 + 0.5 * layer
        i = slice(64 * layer, 64 * layer + 64)
        sc["means3D"][i] = torch.stack([gx.reshape(-1) * z * sc["tanfovx"], gy.reshape(-1) * z * sc["tanfovy"], torch.full((64,), z)], 1)
        sc["scales"][i] = 6.0 * z / focal
        sc["opacities"][i] = 0.99
    z = 20.0
    sc["means3D"][192:256] = torch.stack([gx.reshape(-1) * z * sc["tanfovx"], gy.reshape(-1) * z * sc["tanfovy"], torch.full((64,), z)], 1)
    sc["scales"][192:256] = 0.3 * z / focal
    sc["rotations"][:256] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc["means3D"][256:, 2] = torch.rand(P - 256, generator=g) * 60.0 + 10.0
    sc["flow_points"] = (sc["means3D"] + 0.05 * torch.randn(P, 3, generator=g)).contiguous()
    return sc


def wave_classes(bits, vis):
    n = len(bits) // 64 * 64
    b, v = bits[:n].reshape(-1, 64), vis[:n].reshape(-1, 64)
    full_vis = v.all(1)
    return int((b.all(1)).sum()), int((full_vis & ~b.any(1)).sum()), int((b.any(1) & ~b.all(1)).sum())


# ---------------------------------------------------------------- the tests
class ModelFrame:
    """T3 through gaussian_renderer.render() on the raw-SH / raw-scene model: deformation, flow, object mask, the ddir path."""

    def __init__(self, sc, seed=3):
        self.sc, self.seed = sc, seed

    def forward(self):
        from adgs.model import SyntheticGaussianModel
        from gaussian_renderer import render
        self.model = SyntheticGaussianModel.from_scene(self.sc, device="cuda", seed=self.seed)
        self.model.raw_sh = self.model.raw_scene = True
        cam = synthetic.camera_object(self.sc, time=0.37)
        pipe = types.SimpleNamespace(inv_depth=True, debug=False)
        self.out = render(cam, self.model, None, pipe, flow_pkg=(0.66, None, None, None, None, None), render_objmask=True)
        return self.out

    def backward(self, up, retain=False):
        o = self.out
        torch.autograd.backward([o["render"], o["depth"], o["img_opacity"], o["img_flow"], o["img_semantic"]],
                                [dev(up["color"]), dev(up["depth"])[0], dev(up["img_opacity"])[0], dev(up["flow"]), dev(up["semantic"])], retain_graph=retain)
        torch.cuda.synchronize()
        from adgs.model import _RAW
        g = {n: (None if p.grad is None else p.grad.clone()) for n, p in zip(_RAW, self.model.parameters())}
        g["means2D"] = o["viewspace_points"].grad.clone()
        return g


def test_t3_rawsh_frame_mask_on_equals_mask_off(tap, monkeypatch):
    sc = synthetic.make_config_scene("T3")
    up = synthetic.make_upstream_grads(sc, 7)
    ga, gb, bits, lines, radii, fa = run_pair(tap, monkeypatch, lambda: ModelFrame(sc), up, poison=True)
    vis = radii.cpu().numpy() > 0
    share = float((bits & vis).sum()) / float(vis.sum())
    print("T3: %d visible, %d published (%.1f %%), %d with a non-zero line" % (vis.sum(), bits.sum(), 100 * share, (vis & (lines != 0).any(1)).sum()))
    assert vis.sum() > 10000 and 0.10 <= share <= 0.90, "the frame must exercise both classes"
    assert_equal_grads(ga, gb, "T3 rawsh")
    assert float(ga["means2D"].abs().max()) > 0 and float(ga["_scene_shs_rest"].abs().max()) > 0
    zero_rows_are_zero(ga, bits, ("means2D",))


@pytest.mark.parametrize("rawsh", [False, True])
def test_occluded_scene_most_visible_gaussians_are_unpublished(tap, monkeypatch, rawsh):
    sc = occluded_scene()
    up = synthetic.make_upstream_grads(sc, 5)
    ga, gb, bits, lines, radii, _ = run_pair(tap, monkeypatch, lambda: Static(sc, rawsh=rawsh), up, poison=True)
    vis = radii.cpu().numpy() > 0
    all_set, all_clear, mixed = wave_classes(bits, vis)
    print("occluded: %d visible, %d published; waves all set / all clear (and visible) / mixed: %d / %d / %d" % (vis.sum(), bits.sum(), all_set, all_clear, mixed))
    assert vis.sum() > 4000 and (vis & ~bits).sum() > 0.5 * vis.sum()
    assert all_set >= 1 and all_clear >= 1 and mixed >= 1
    assert_equal_grads(ga, gb, "occluded rawsh=%s" % rawsh)
    zero_rows_are_zero(ga, bits, ("means3D", "means2D", "opacities", "scales", "rotations", "flow", "shs"))


def _edge_scene(kind):
    if kind == "P=1061":                       # no multiple of 32 or 64; raw path: Ns = 707, the scene / object boundary falls inside a wave
        return synthetic.make_scene(1061, 96, 64, 80.0, sh_degree=3, seed=11, n_objects=2), None
    if kind == "P=20":
        return synthetic.make_scene(20, 48, 32, 40.0, sh_degree=3, seed=12, n_objects=0, near_frac=0.0, scale_mult=0.02), None
    if kind == "nothing published":            # everything behind the camera
        sc = synthetic.make_scene(777, 96, 64, 80.0, sh_degree=3, seed=13, n_objects=0)
        sc["means3D"][:, 2] = -sc["means3D"][:, 2].abs() - 1.0
        return sc, "none"
    sc = synthetic.make_scene(300, 96, 64, 80.0, sh_degree=3, seed=14, n_objects=0, near_frac=0.0, scale_mult=0.03)      # sparse, translucent, on screen
    sc["opacities"][:] = 0.25
    sc["means3D"][:, :2] *= 0.7
    sc["flow_points"][:, :2] *= 0.7
    return sc, "all"


@pytest.mark.parametrize("kind", ["P=1061", "P=20", "nothing published", "every visible one published"])
@pytest.mark.parametrize("rawsh", [False, True])
def test_edges_of_the_gating(tap, monkeypatch, kind, rawsh):
    sc, expect = _edge_scene(kind)
    up = synthetic.make_upstream_grads(sc, 1)
    Ns = 13 if (rawsh and sc["P"] == 20) else None
    ga, gb, bits, lines, radii, _ = run_pair(tap, monkeypatch, lambda: Static(sc, rawsh=rawsh, Ns=Ns), up, poison=True)
    vis = radii.cpu().numpy() > 0
    print("%s rawsh=%s: P=%d visible=%d published=%d" % (kind, rawsh, sc["P"], vis.sum(), bits.sum()))
    if expect == "none":
        assert vis.sum() == 0 and bits.sum() == 0
        assert all(v is None or float(v.abs().max()) == 0 for v in ga.values())
    elif expect == "all":
        assert vis.sum() > 100 and (bits == vis).all()
    else:
        assert bits.sum() > 0
    assert_equal_grads(ga, gb, kind)


@pytest.mark.parametrize("name,kw", [
    ("materialised [P,16,3] SH", dict()),
    ("sh_degree 0, one coefficient (non-staged kernel)", dict(sh0=True)),
    ("raw SH below degree 3 (no ddir: the rest rows are staged)", dict(rawsh=True, degree=2)),
    ("absolute gradient", dict(absgrad=True)),
    ("absolute gradient, raw SH", dict(absgrad=True, rawsh=True)),
    ("D_S = 2", dict(D_S=2)),
    ("anti-aliasing", dict(aa=True)),
    ("anti-aliasing, raw SH", dict(aa=True, rawsh=True)),
    ("staging off (non-staged raw kernel)", dict(rawsh=True, env=dict(ADGS_NO_SH_STAGING="1"))),
])
def test_other_paths(tap, monkeypatch, name, kw):
    kw = dict(kw)
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=0 if kw.pop("sh0", False) else 3, seed=2, n_objects=2)
    D_S, env = kw.pop("D_S", 1), kw.pop("env", None)
    up = synthetic.make_upstream_grads(sc, 2, D_S=D_S)
    if D_S > 1:
        kw["sem"] = torch.cat([sc["semantic"], torch.rand(sc["P"], D_S - 1, generator=torch.Generator().manual_seed(3))], 1)
    ga, gb, bits, lines, radii, _ = run_pair(tap, monkeypatch, lambda: Static(sc, **kw), up, env=env, poison=True)
    vis = radii.cpu().numpy() > 0
    print("%s: visible=%d published=%d" % (name, vis.sum(), bits.sum()))
    assert (vis & ~bits).sum() > 50 and bits.sum() > 500
    assert_equal_grads(ga, gb, name)
    if kw.get("absgrad"):
        assert float(ga["means2D_abs"].abs().max()) > 0
        zero_rows_are_zero(ga, bits, ("means2D_abs",))


# Two runs of the blend backward: the order of its float atomics differs (tests/test_gpu_raster.py compares such pairs the same way)
TWO_RUNS = dict(tol=2e-5, max_frac=1e-4, rel_l2=2e-5)


def test_classic_pipeline_ignores_the_switch(monkeypatch):
    """The classic pipeline has no mask: its backward reads every Gaussian whatever the switch says, and agrees with the default
    pipeline's (masked) gradients as two independent implementations do."""
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=2, n_objects=2)
    up = synthetic.make_upstream_grads(sc, 2)
    res = {}
    for mode, switch in (("classic", None), ("classic", "0"), ("v2", None)):
        monkeypatch.setenv("ADGS_RASTER_MODE", mode)
        monkeypatch.delenv(ENV, raising=False)
        if switch is not None:
            monkeypatch.setenv(ENV, switch)
        f = Static(sc)
        f.forward()
        res[(mode, switch)] = f.backward(up)
    for k, a in res[("classic", None)].items():
        if a is not None:
            assert_close("classic, switch " + k, res[("classic", "0")][k].cpu().numpy(), a.cpu().numpy(), **TWO_RUNS)
            assert_close("classic vs masked v2 " + k, res[("v2", None)][k].cpu().numpy(), a.cpu().numpy(), tol=2e-5, max_frac=2e-4, rel_l2=2e-5)


@pytest.mark.parametrize("rawsh", [False, True])
def test_second_backward_and_backward_over_cloned_state(tap, monkeypatch, rawsh):
    """retain_graph: the second backward zeroes the lines and replays the same chunks -- the mask of the forward still holds.  Cloned state
    buffers: the mask travels inside the geometry state and the header word says that it is there."""
    from diff_gaussian_rasterization import _C
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=6, n_objects=2)
    up = synthetic.make_upstream_grads(sc, 6)
    tap.mode = "record"
    f = Static(sc, rawsh=rawsh)
    f.forward()
    g1 = f.backward(up, retain=True)
    bits1, _, words1 = read_state(tap.last)
    g2 = f.backward(up, retain=True)
    bits2, lines2, words2 = read_state(tap.last)
    assert (words1 == words2).all() and (~bits1).sum() > 50
    check_superset(bits2, lines2, tap.last["radii"])
    # the third backward runs over COPIES of the three state buffers
    for name in ("rasterize_gaussians_backward", "rasterize_gaussians_backward_rawsh"):
        inner = getattr(_C, name)
        sig = inspect.signature(inner)

        def cloned(*a, _inner=inner, _sig=sig, **kw):
            b = _sig.bind(*a, **kw)
            for k in ("geomBuffer", "binningBuffer", "imageBuffer"):
                b.arguments[k] = b.arguments[k].clone()
            b.arguments.pop("plan", None)
            return _inner(*b.args, **b.kwargs)
        monkeypatch.setattr(_C, name, cloned)
    g3 = f.backward(up)
    bits3, lines3, _ = read_state(tap.last)
    assert (bits3 == bits1).all()
    check_superset(bits3, lines3, tap.last["radii"])
    for k, a in g1.items():
        if a is not None:
            assert_close("second backward " + k, g2[k].cpu().numpy(), a.cpu().numpy(), **TWO_RUNS)
            assert_close("cloned state " + k, g3[k].cpu().numpy(), a.cpu().numpy(), **TWO_RUNS)
    zero_rows_are_zero(g2, bits1, ("means3D", "means2D", "scales", "rotations"))
    zero_rows_are_zero(g3, bits1, ("means3D", "means2D", "scales", "rotations"))


def test_adam_in_the_backward_with_the_mask_equals_the_separate_step_without_it(monkeypatch):
    """FusedAdam(in_backward=True) on masked frames against the two-kernel step on frames with ADGS_PUBLISHED_MASK=0: parameters and both
    moments of every group bit-identical after every iteration (32 x 4 frames have two tiles: the blend backward itself repeats bit for
    bit there, tests/test_gpu_optim.py).  A `rest` row whose Gaussian is not published has a zero gradient row, not no row: its moments decay."""
    from tests.test_gpu_optim import _render_model, _one_iteration
    d = torch.device("cuda", 0)
    P, n_objects, seed, W, H = 4099, 3, 4, 32, 4
    monkeypatch.delenv(ENV, raising=False)
    a, cams = _render_model(P, n_objects, seed, d, True, W, H)
    b, _ = _render_model(P, n_objects, seed, d, False, W, H)
    g = torch.Generator().manual_seed(seed)
    decayed = 0
    for it in range(6):
        cam = cams[it % len(cams)]
        weights = [torch.randn(3, H, W, generator=g).to(d), torch.randn(H, W, generator=g).to(d) * 0.1, torch.randn(H, W, generator=g).to(d) * 0.1]
        m_before = a.optimizer.state[a._scene_shs_rest]["exp_avg"].clone() if it else None
        monkeypatch.delenv(ENV, raising=False)
        fa = _one_iteration(a, cam, weights, True)
        monkeypatch.setenv(ENV, "0")
        _one_iteration(b, cam, weights, False)
        assert fa["scene_shs_rest"] and fa["obj_shs_rest"]
        torch.cuda.synchronize()
        for ga_, gb_ in zip(a.optimizer.param_groups, b.optimizer.param_groups):
            pa, pb = ga_["params"][0], gb_["params"][0]
            if pa.numel() == 0 or pa not in a.optimizer.state:
                continue
            sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
            assert torch.equal(pa.detach(), pb.detach()), (it, ga_["name"])
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (it, ga_["name"])
        if it:
            m_after = a.optimizer.state[a._scene_shs_rest]["exp_avg"]
            beta1 = [grp for grp in a.optimizer.param_groups if grp["params"][0] is a._scene_shs_rest][0]["betas"][0]
            # a zero gradient row: m <- beta1 m (to the rounding of the update's own form); any other row moves by (1 - beta1) g as well
            rows = (m_before.flatten(1) != 0).any(1) & ((m_after - m_before * beta1).abs() <= 1e-6 * m_before.abs()).flatten(1).all(1)
            decayed += int(rows.sum())
    assert decayed > 0, "no row with a zero gradient and non-zero moments: the frames should leave such Gaussians"


def test_forward_only_frame_writes_no_mask_and_the_same_images(tap):
    """torch.no_grad(): the PUBLISH = false blend; the mask keeps the fill it was allocated with."""
    from diff_gaussian_rasterization import _C
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=9, n_objects=2)
    e = torch.Tensor([])
    args = (dev(sc["bg"]), dev(sc["means3D"]), e, dev(sc["opacities"]), dev(sc["scales"]), dev(sc["rotations"]), 1.0, e, dev(sc["viewmatrix"]),
            dev(sc["projmatrix"]), sc["tanfovx"], sc["tanfovy"], sc["H"], sc["W"], dev(sc["shs"]), dev(sc["flow_points"]), dev(sc["semantic"]), 3,
            dev(sc["campos"]), False, True, False)
    train = _C.rasterize_gaussians(*args)
    only = _C.rasterize_gaussians(*args, training=False)
    torch.cuda.synchronize()
    for i in (1, 2, 3, 4, 8, 9):
        assert torch.equal(train[i], only[i]), i
    P = sc["P"]
    bits, _, _ = read_state(dict(geom=train[5], P=P, radii=train[4]))
    assert 0 < bits.sum() < (train[4] > 0).sum()
    off = offsets(P)[0]
    raw = only[5][off:off + P].cpu().numpy()
    assert (raw == 0xFF).all(), "the forward-only frame touched the published mask"
