"""GPU tests of the gradient prefill (grad_prefill.h; switch: ADGS_GRAD_PREFILL=0, read by the frame's forward): the zero rows of the sparse
groups of 256 Gaussians are stored by fill workgroups inside the blend backward's grid (or by a launch of their own when a backward has no
blend backward), and the preprocess backward and the SH-deformation row kernel then store the published rows only.

What is asserted, for every case: with every float32 destination the bindings allocate PRE-FILLED WITH NaN (a row nobody writes shows),
  - no NaN is left in any gradient tensor of the frame;
  - every gradient tensor compares equal under `==`, element for element, to the ADGS_GRAD_PREFILL=0 path over the same accumulator lines;
  - the rows of unpublished Gaussians are all zero.
"The same accumulator lines" as in tests/test_gpu_published_mask.py (whose shapes and helpers are used here): frame A runs forward and
backward with the switch unset (the fill rides in the blend backward); frame B (switch = 0) and frame C (switch unset) run their own forward,
get A's geometry state copied over theirs, and run their backward without the binning state -- no blend backward, so C runs the stand-alone
fill kernel.  A == B and C == B.
"""
import numpy as np
import pytest
import torch

from adgs import synthetic
from tests import test_gpu_published_mask as pm
from tests.parity import assert_close
from tests.test_gpu_published_mask import tap  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ENV = "ADGS_GRAD_PREFILL"


class _NaNTorch:
    """Stands in for the `torch` global of the bindings: every float32 tensor they allocate uninitialised comes back filled with NaN and,
    with `offset`, 4 bytes past a 16-byte boundary (a slice of a gradient arena need not be aligned)."""

    def __init__(self, offset):
        self.offset = offset

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        if kw.get("dtype", torch.float32) != torch.float32:
            return torch.empty(*shape, **kw)
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        n = int(np.prod(shape)) if len(shape) else 1
        flat = torch.full((n + 4,), float("nan"), **kw)
        assert flat.data_ptr() % 16 == 0
        o = 1 if self.offset else 0
        return flat[o:o + n].view(shape)

    def empty_like(self, t, **kw):
        if t.dtype != torch.float32:
            return torch.empty_like(t, **kw)
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


@pytest.fixture
def nan_dst(monkeypatch):
    from diff_gaussian_rasterization import _C

    def install(offset=False):
        monkeypatch.setattr(_C, "torch", _NaNTorch(offset))
    install()
    return install


class Static(pm.Static):
    """pm.Static; `nosem`: no semantic input at all (D_S = 0)."""

    def __init__(self, sc, nosem=False, **kw):
        super().__init__(sc, **kw)
        self.nosem = nosem

    def forward(self):
        if not self.nosem:
            return super().forward()
        from diff_gaussian_rasterization import GaussianRasterizer
        # the same call with semantic=None: the rasterizer is asked through a class whose calls drop the argument
        real_fwd, real_raw = GaussianRasterizer.forward, GaussianRasterizer.forward_rawsh
        GaussianRasterizer.forward = lambda r, **kw: real_fwd(r, **dict(kw, semantic=None))
        GaussianRasterizer.forward_rawsh = lambda r, *a, **kw: real_raw(r, *a, **dict(kw, semantic=None))
        try:
            return super().forward()
        finally:
            GaussianRasterizer.forward, GaussianRasterizer.forward_rawsh = real_fwd, real_raw

    def backward(self, up, retain=False):
        for v in self.L.values():
            v.grad = None
        color, radii, depth, op, fl, se = self.out
        pairs = [(color, up["color"]), (depth, up["depth"]), (op, up["img_opacity"]), (fl, up["flow"]), (se, up["semantic"])]
        pairs = [(o, pm.dev(g)) for o, g in pairs if o.requires_grad]      # D_S = 0: no semantic image
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs], retain_graph=retain)
        torch.cuda.synchronize()
        g = {k: (None if v.grad is None else v.grad.clone()) for k, v in self.L.items()}
        if g["sem"] is not None and g["sem"].shape[1] > 1:
            self.sem_rest = g["sem"][:, 1:].clone()
            g["sem"] = g["sem"][:, :1].clone()      # channels >= 1: the blend backward's own replays
        return g


def run_triple(tap, monkeypatch, make, up, env=None):
    """(A's gradients, bits, radii, A's frame) after A == B and C == B have been asserted (module docstring)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(ENV, raising=False)
    tap.mode, tap.poison = "record", None
    for _ in range(2):      # the library sizes a frame's state from what its thread's earlier frames measured: let that settle, the three frames below share a layout
        make().forward()
    torch.cuda.synchronize()
    fa = make()
    fa.forward()
    ga = fa.backward(up)
    rec = tap.last
    bits, lines, _ = pm.read_state(rec)
    pm.check_superset(bits, lines, rec["radii"])

    def replay(switch):
        if switch is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, switch)
        f = make()
        f.forward()
        tap.mode, tap.kept = "replay", rec["geom"]
        try:
            return f.backward(up)
        finally:
            tap.mode = "record"
    gb = replay("0")
    gc = replay(None)
    monkeypatch.delenv(ENV, raising=False)
    for k in (env or {}):
        monkeypatch.delenv(k)
    tap.mode = "plain"
    for what, g in (("in-grid fill", ga), ("switch off", gb), ("stand-alone fill", gc)):
        for k, v in g.items():
            assert v is None or not bool(torch.isnan(v).any()), "%s: %s has %d NaN of %d: rows nobody wrote" % (what, k, int(torch.isnan(v).sum()), v.numel())
    pm.assert_equal_grads(ga, gb, "in-grid fill vs switch off")
    pm.assert_equal_grads(gc, gb, "stand-alone fill vs switch off")
    return ga, bits, rec["radii"], fa


ROWS = ("means3D", "means2D", "means2D_abs", "opacities", "scales", "rotations", "flow", "sem", "shs")


def unpublished_rows_are_zero(g, bits, Ns=None):
    clear = torch.from_numpy(~bits).cuda()
    for k in ROWS:
        if g.get(k) is not None:
            assert bool((g[k][clear] == 0).all()), k
    if Ns is not None:
        for k, c in (("scene_dc", clear[:Ns]), ("scene_rest", clear[:Ns]), ("obj_dc", clear[Ns:]), ("obj_rest", clear[Ns:])):
            if g.get(k) is not None and g[k].shape[0] == c.shape[0]:
                assert bool((g[k][c] == 0).all()), k


def thin(sc, lo, hi, keep_every=4):
    """Puts Gaussians [lo, hi) behind the camera but for every keep_every-th one (0: all of them): their groups come out sparse whatever the
    scene -- with no published row at all, or with a few rows of their own between the zero rows."""
    sc = dict(sc, means3D=sc["means3D"].clone())
    idx = torch.arange(lo, hi)
    gone = idx if keep_every == 0 else idx[idx % keep_every != 0]
    sc["means3D"][gone, 2] = -5.0
    return sc


def groups(bits):
    """(sparse, dense) groups of 256 by the rule of grad_prefill.h: sparse = fewer than half of the group's Gaussians published."""
    n = [(int(bits[i:i + 256].sum()), len(bits[i:i + 256])) for i in range(0, len(bits), 256)]
    return sum(1 for c, m in n if 2 * c < m), sum(1 for c, m in n if 2 * c >= m)


# ---------------------------------------------------------------- edges of the grouping
@pytest.mark.parametrize("kind,rawsh,Ns", [
    ("P=20", False, None), ("P=20", True, 13),
    ("P=20 thinned", False, None), ("P=20 thinned", True, 13),      # 5 of 20 in front of the camera: one sparse group, less than a wave
    ("P=1061", False, None), ("P=1061", True, None),      # raw: Ns = 707, the scene / object boundary inside a wave and inside a group
    ("P=1061", True, 1061),                               # No = 0
    ("P=1061 thinned", False, None), ("P=1061 thinned", True, None), ("P=1061 thinned", True, 1061),      # ... inside a SPARSE group
    ("nothing published", False, None), ("nothing published", True, None),
    ("every visible one published", False, None), ("every visible one published", True, None),
])
def test_edges_of_the_grouping(tap, nan_dst, monkeypatch, kind, rawsh, Ns):
    sc, expect = pm._edge_scene(kind.replace(" thinned", ""))
    if kind == "P=20 thinned":
        sc = thin(sc, 0, 20)
    elif kind == "P=1061 thinned":
        sc = thin(thin(sc, 300, 900), 900, 1061, keep_every=0)      # groups 1 .. 3 sparse with rows of their own, the last one empty
    up = synthetic.make_upstream_grads(sc, 1)
    ga, bits, radii, _ = run_triple(tap, monkeypatch, lambda: Static(sc, rawsh=rawsh, Ns=Ns), up)
    vis = radii.cpu().numpy() > 0
    sparse, dense = groups(bits)
    if "thinned" in kind:
        assert sparse >= (1 if sc["P"] == 20 else 3) and (sc["P"] == 20 or bits[300:900].sum() > 20)
    print("%s rawsh=%s: P=%d visible=%d published=%d groups sparse/dense=%d/%d" % (kind, rawsh, sc["P"], vis.sum(), bits.sum(), sparse, dense))
    if expect == "none":
        assert bits.sum() == 0 and dense == 0
        assert all(v is None or float(v.abs().max()) == 0 for v in ga.values())      # the fill wrote everything
    elif expect == "all":
        assert vis.sum() > 100 and (bits == vis).all() and sparse == 0               # every group dense: the fill writes nothing
    unpublished_rows_are_zero(ga, bits, Ns if Ns is not None else ((2 * sc["P"]) // 3 if rawsh else None))


@pytest.mark.parametrize("rawsh", [False, True])
def test_occluded_scene_has_waves_all_clear_all_set_and_mixed(tap, nan_dst, monkeypatch, rawsh):
    sc = pm.occluded_scene()
    up = synthetic.make_upstream_grads(sc, 5)
    ga, bits, radii, _ = run_triple(tap, monkeypatch, lambda: Static(sc, rawsh=rawsh), up)
    vis = radii.cpu().numpy() > 0
    all_set, all_clear, mixed = pm.wave_classes(bits, vis)
    sparse, dense = groups(bits)
    print("occluded rawsh=%s: published %d of %d; waves set/clear/mixed %d/%d/%d; groups sparse/dense %d/%d" % (rawsh, bits.sum(), vis.sum(), all_set, all_clear, mixed, sparse, dense))
    assert all_set >= 1 and all_clear >= 1 and mixed >= 1 and sparse >= 1 and dense >= 1
    assert float(ga["means2D"].abs().max()) > 0
    unpublished_rows_are_zero(ga, bits, (2 * sc["P"]) // 3 if rawsh else None)


@pytest.mark.parametrize("H,wtiles", [(1016, 2032), (1024, 2048)])
def test_below_and_at_the_tile_order_threshold(tap, nan_dst, monkeypatch, H, wtiles):
    """256 x H with two pixels per lane: 16 x ceil(H / 8) work tiles -- the longest-first tile order (and with it the fill's place behind
    the tile workgroups of an ORDERED grid) switches on at 2048."""
    sc = synthetic.make_scene(3000, 256, H, 300.0, sh_degree=3, seed=21, n_objects=2)
    sc = thin(thin(sc, 512, 1536, keep_every=0), 1536, 2304)      # four groups with nothing published, three with at most a quarter
    assert (256 // 16) * ((H + 7) // 8) == wtiles
    up = synthetic.make_upstream_grads(sc, 21)
    ga, bits, radii, _ = run_triple(tap, monkeypatch, lambda: Static(sc, rawsh=True), up, env=dict(ADGS_V2_PPL="2"))
    sparse, dense = groups(bits)
    print("H=%d: published %d, groups sparse/dense %d/%d" % (H, bits.sum(), sparse, dense))
    assert bits.sum() > 100 and sparse >= 7 and dense >= 1 and bits[1536:2304].sum() > 20
    unpublished_rows_are_zero(ga, bits, (2 * sc["P"]) // 3)


@pytest.mark.parametrize("name,kw", [
    ("destinations 4 bytes past a 16-byte boundary", dict(offset=True)),
    ("destinations 4 bytes past a 16-byte boundary, raw SH", dict(offset=True, rawsh=True)),
    ("sh_degree 0, one coefficient (non-staged kernel)", dict(sh0=True)),
    ("raw SH below degree 3 (the rest rows are staged)", dict(rawsh=True, degree=2)),
    ("absolute gradient", dict(absgrad=True)),
    ("absolute gradient, raw SH", dict(absgrad=True, rawsh=True)),
    ("anti-aliasing", dict(aa=True)),
    ("anti-aliasing, raw SH", dict(aa=True, rawsh=True)),
    ("D_S = 0", dict(D_S=0)),
    ("D_S = 0, raw SH", dict(D_S=0, rawsh=True)),
    ("D_S = 2", dict(D_S=2)),
    ("D_S = 2, raw SH", dict(D_S=2, rawsh=True)),
    ("staging off (non-staged raw kernel)", dict(rawsh=True, env=dict(ADGS_NO_SH_STAGING="1"))),
])
def test_other_paths(tap, nan_dst, monkeypatch, name, kw):
    kw = dict(kw)
    nan_dst(kw.pop("offset", False))
    sc = synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=0 if kw.pop("sh0", False) else 3, seed=2, n_objects=2)
    sc = thin(thin(sc, 512, 1536, keep_every=0), 1536, 2304)      # Ns = 2000 lies inside a sparse group
    D_S, env = kw.pop("D_S", 1), kw.pop("env", None)
    up = synthetic.make_upstream_grads(sc, 2, D_S=D_S)
    if D_S == 2:
        kw["sem"] = torch.cat([sc["semantic"], torch.rand(sc["P"], 1, generator=torch.Generator().manual_seed(3))], 1)
    kw["nosem"] = D_S == 0
    ga, bits, radii, fa = run_triple(tap, monkeypatch, lambda: Static(sc, **kw), up, env=env)
    sparse, dense = groups(bits)
    print("%s: published=%d groups sparse/dense=%d/%d" % (name, bits.sum(), sparse, dense))
    assert sparse >= 7 and dense >= 1 and bits.sum() > 500 and bits[1536:2304].sum() > 20
    unpublished_rows_are_zero(ga, bits, 2000 if kw.get("rawsh") else None)
    if kw.get("absgrad"):
        assert float(ga["means2D_abs"].abs().max()) > 0
    if D_S == 2:
        # channels >= 1 keep their memset and the extra replay's sums: written in frame A (the two replays have no blend backward)
        assert not bool(torch.isnan(fa.sem_rest).any()) and float(fa.sem_rest.abs().max()) > 0
        assert bool((fa.sem_rest[torch.from_numpy(~bits).cuda()] == 0).all())


def test_t3_model_frame_with_deformation_rows(tap, nan_dst, monkeypatch):
    """gaussian_renderer.render() on the raw-SH / raw-scene model: the raw scene rows, the object side, and the SH-deformation rows of the
    row kernel (sparse groups: published rows only)."""
    sc = synthetic.make_config_scene("T3")
    up = synthetic.make_upstream_grads(sc, 7)
    ga, bits, radii, _ = run_triple(tap, monkeypatch, lambda: pm.ModelFrame(sc), up)
    sparse, dense = groups(bits)
    print("T3: published %d of %d, groups sparse/dense %d/%d" % (bits.sum(), len(bits), sparse, dense))
    assert sparse >= 1 and float(ga["means2D"].abs().max()) > 0 and float(ga["_scene_shs_rest"].abs().max()) > 0
    sp = [k for k in ga if k.startswith("shs_deform_param") and ga[k] is not None and ga[k].numel() > 0]
    assert sp, "the model frame carries SH-deformation rows"
    assert any(float(ga[k].abs().max()) > 0 for k in sp)
    unpublished_rows_are_zero(ga, bits)


@pytest.mark.parametrize("rawsh", [False, True])
def test_second_backward_over_one_forward(tap, nan_dst, monkeypatch, rawsh):
    """retain_graph: the second backward fills, blends and stores again into fresh (NaN) destinations."""
    sc = thin(synthetic.make_scene(3000, 200, 136, 150.0, sh_degree=3, seed=6, n_objects=2), 1024, 2304)
    up = synthetic.make_upstream_grads(sc, 6)
    monkeypatch.delenv(ENV, raising=False)
    tap.mode = "record"
    f = Static(sc, rawsh=rawsh)
    f.forward()
    g1 = f.backward(up, retain=True)
    bits, _, _ = pm.read_state(tap.last)
    g2 = f.backward(up)
    for k, a in g1.items():
        if a is not None:
            assert not bool(torch.isnan(g2[k]).any()), k
            assert_close("second backward " + k, g2[k].cpu().numpy(), a.cpu().numpy(), **pm.TWO_RUNS)
    assert groups(bits)[0] >= 1
    unpublished_rows_are_zero(g1, bits, 2000 if rawsh else None)
    unpublished_rows_are_zero(g2, bits, 2000 if rawsh else None)


def test_captured_frame_replays_the_fill(nan_dst, monkeypatch):
    """adgs.graph: the fill workgroups are part of the captured blend backward launch.  32 x 4 pixels are two tiles: the blend backward's
    float atomics add at most two terms per word, so the eager switch-off frame is the reference bit for bit (tests/test_gpu_optim.py)."""
    from adgs import graph
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sc = synthetic.make_scene(2500, 32, 4, 30.0, sh_degree=3, seed=8, n_objects=0)
    up = synthetic.make_upstream_grads(sc, 8)
    s = GaussianRasterizationSettings(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], pm.dev(sc["bg"]), 1.0, pm.dev(sc["viewmatrix"]), pm.dev(sc["projmatrix"]),
                                      3, pm.dev(sc["campos"]), False, True, False, False)
    rast = GaussianRasterizer(s)
    t = {k: pm.dev(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    fl, se = pm.dev(sc["flow_points"]), pm.dev(sc["semantic"])
    ups = [pm.dev(up[k]) for k in ("color", "depth", "img_opacity", "flow", "semantic")]

    def fn():
        m2 = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True)
        c, r, d, o, ifl, ise = rast(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                                    flow_points=fl, semantic=se)
        loss = sum((x * g).sum() for x, g in zip((c, d, o, ifl, ise), ups))
        return torch.autograd.grad(loss, [m2] + [t[k] for k in sorted(t)])
    monkeypatch.setenv(ENV, "0")
    want = [x.clone() for x in fn()]
    monkeypatch.delenv(ENV, raising=False)
    eager = [x.clone() for x in fn()]
    step = graph.GraphedStep(fn)
    for _ in range(2):
        got = step()
    torch.cuda.synchronize()
    assert step.validate(repair=False)
    assert float(want[0].abs().max()) > 0 and int((want[0] == 0).all(1).sum()) > 256      # more than a group of zero rows
    for i, w in enumerate(want):
        assert not bool(torch.isnan(got[i]).any()), i
        assert bool((eager[i] == w).all()) and bool((got[i] == w).all()), i


def test_adam_in_the_backward_with_the_fill_equals_the_separate_step_without_it(monkeypatch):
    """FusedAdam(in_backward=True) on prefilled frames against the two-kernel step on frames with ADGS_GRAD_PREFILL=0: parameters and both
    moments of every group bit-identical after every iteration (tests/test_gpu_optim.py; 32 x 4 frames, as there).  The tensors whose Adam
    slot is on have no gradient store and stay dense; every other gradient of these frames goes through the fill."""
    from tests.test_gpu_optim import _render_model, _one_iteration
    d = torch.device("cuda", 0)
    P, n_objects, seed, W, H = 4099, 3, 4, 32, 4
    monkeypatch.delenv(ENV, raising=False)
    a, cams = _render_model(P, n_objects, seed, d, True, W, H)
    b, _ = _render_model(P, n_objects, seed, d, False, W, H)
    g = torch.Generator().manual_seed(seed)
    for it in range(4):
        cam = cams[it % len(cams)]
        weights = [torch.randn(3, H, W, generator=g).to(d), torch.randn(H, W, generator=g).to(d) * 0.1, torch.randn(H, W, generator=g).to(d) * 0.1]
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
