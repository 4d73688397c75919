"""The 3D smoothing filter on the GPU (adgs.filter3d over include/adgs_filter3d.h) against the float64 reference of
tests/filter3d_ref.py.

accumulate: P in {1, 63, 64, 257, 1000} x camera counts {1, 3, 65, 300}.  The kernel has NO camera-table chunk (the table is read
record by record through the scalar cache, any count is one loop), so the counts beside 1 and 3 are the issue's 65 and 300.  A thread
takes four consecutive Gaussians: 63 / 257 / 1000 leave single-row threads behind the aligned middle, 257 and 1000 span more than one
workgroup of 256 threads only in rows -- 1000 rows are 250 group threads --, so the sub-range case (row0 = 37: three head rows in
front of the first aligned group) and P = 1 / 63 exercise the single-row threads.
Every row must satisfy rate_lo (1 - tol) <= got <= rate_hi (1 + tol); rate_lo / rate_hi: the reference's rate over the firmly / firmly
or marginally seeing cameras (a gate within 1e-5 x its summed term magnitudes of its threshold is marginal).  ACC_TABLE: per case the
seed (the first for which the reference alone has at most 1 % of its rows with rate_lo != rate_hi), that count, and the largest
relative error of the float32 torch-CPU evaluation of the rate against float64 over the firm rows; tol = 4 x that, never above 1e-4.

apply: tolerance per element = 4 x (the largest relative error of the float32 torch-CPU evaluation of the same formulas against
float64, per tensor: APPLY_TABLE) x |ref|, floored at one float32 ulp of the reference value and capped by tests/parity.py's rule
1e-4 |ref| + 1e-4 max |ref|.

End to end, gradients.  The rasterizer's backward sums a Gaussian's per-tile contributions with float atomics (arrival order: the suite's
other tests compare two backward runs of one frame with a tolerance, e.g. tests/test_gpu_loss.py, tests/test_gpu_absgrad.py), so two
separate backward runs are not bit-reproducible whatever feeds them.  What this feature computes IS held bit for bit: render()'s
apply outputs equal the hand call's, and the gradients of every parameter that is reached only through apply (scales, opacities, time
sigma) equal, bit for bit, the hand chain apply -> deformation backward fed with the SAME upstream gradients render()'s rasterizer
delivered.  Against the hand call's own rasterizer backward every parameter gradient is held to tests/parity.py's element rule."""
import functools
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import filter3d_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

P_LIST = (1, 63, 64, 257, 1000)
C_LIST = (1, 3, 65, 300)

# (P, cameras): (seed, rows with rate_lo != rate_hi, max relative |float32 CPU rate - float64| over the firm rows)
ACC_TABLE = {
    (1, 1): (1, 0, 0.000e+00),
    (1, 3): (1, 0, 0.000e+00),
    (1, 65): (1, 0, 1.206e-08),
    (1, 300): (1, 0, 9.101e-08),
    (63, 1): (1, 0, 9.424e-08),
    (63, 3): (1, 0, 9.865e-08),
    (63, 65): (1, 0, 1.829e-07),
    (63, 300): (1, 0, 5.285e-07),
    (64, 1): (1, 0, 9.424e-08),
    (64, 3): (1, 0, 9.865e-08),
    (64, 65): (1, 0, 1.829e-07),
    (64, 300): (1, 0, 5.285e-07),
    (257, 1): (1, 0, 1.056e-07),
    (257, 3): (1, 0, 1.647e-07),
    (257, 65): (1, 0, 2.361e-07),
    (257, 300): (1, 0, 5.285e-07),
    (1000, 1): (1, 0, 1.056e-07),
    (1000, 3): (1, 0, 1.647e-07),
    (1000, 65): (1, 0, 2.877e-07),
    (1000, 300): (1, 0, 5.285e-07),
}
# P: (seed, max relative |float32 CPU - float64| of S, O, dL/ds, dL/do)
APPLY_TABLE = {
    1: (1, 2.728e-08, 6.218e-08, 4.543e-08, 6.799e-08),
    63: (1, 8.443e-08, 1.744e-07, 5.485e-06, 1.720e-07),
    64: (1, 8.785e-08, 1.601e-07, 2.720e-07, 1.554e-07),
    257: (1, 9.236e-08, 2.339e-07, 9.539e-07, 2.497e-07),
    1000: (1, 1.034e-07, 2.067e-07, 1.211e-05, 1.951e-07),
}


@functools.lru_cache(maxsize=None)
def _acc_case(P, C, seed=None):
    """inputs (float32, CPU) and the float64 reference of one case: computed once, shared, never modified"""
    seed = ACC_TABLE[(P, C)][0] if seed is None else seed
    recs = ref.random_cameras(C, seed)
    xyz = ref.random_points(P, seed, recs)
    r = ref.rates(xyz, recs)
    return dict(recs=recs, xyz=xyz, lo=r["rate_lo"], hi=r["rate_hi"], outcomes=r["outcomes"], unsure=int((r["rate_lo"] != r["rate_hi"]).sum()),
                err32=ref.float32_rate_error(xyz, recs, r))


def _check_rates(got, c, tol, what):
    got = got.double().cpu().reshape(-1)
    below, above = got < c["lo"] * (1 - tol), got > c["hi"] * (1 + tol)
    worst = float(torch.maximum((c["lo"] - got) / c["lo"].clamp(min=1e-30), (got - c["hi"]) / c["hi"].clamp(min=1e-30)).max())
    print("%s: worst excursion %.3e relative, tolerance %.3e, %d rows with rate_lo != rate_hi, %d rows seen" % (
        what, max(worst, 0.0), tol, c["unsure"], int((c["lo"] > 0).sum())))
    assert not below.any() and not above.any(), (what, int(below.sum()), int(above.sum()))


def _accumulate(xyz, recs, rate=None, row0=0, rows=None, init=True):
    from adgs import filter3d
    rate = torch.empty(xyz.shape[0], device="cuda") if rate is None else rate
    return filter3d.accumulate(xyz, recs, rate, row0=row0, rows=rows, init=init)


def test_tables_describe_the_cases_and_every_gate_has_both_outcomes():
    assert sorted(ACC_TABLE) == sorted((P, C) for P in P_LIST for C in C_LIST) and sorted(APPLY_TABLE) == sorted(P_LIST)
    total = {}
    for (P, C), (seed, unsure, err32) in ACC_TABLE.items():
        c = _acc_case(P, C)
        assert c["unsure"] == unsure <= P // 100, (P, C)
        # err32 is a measurement on one CPU (ACC_TABLE); the float32 evaluation of the machine that runs the test must meet the tolerance
        assert c["err32"] <= max(4 * err32, 2.0 ** -23) and 4 * err32 <= 1e-4, (P, C, c["err32"])
        for k, (yes, no) in c["outcomes"].items():
            total[k] = (total.get(k, (0, 0))[0] + yes, total.get(k, (0, 0))[1] + no)
    for k, (yes, no) in total.items():
        assert yes > 0 and no > 0, k
    big = _acc_case(1000, 300)["outcomes"]
    assert all(yes > 0 and no > 0 for yes, no in big.values())


@pytest.mark.parametrize("C", C_LIST)
@pytest.mark.parametrize("P", P_LIST)
def test_accumulate(P, C):
    c = _acc_case(P, C)
    got = _accumulate(c["xyz"].cuda(), c["recs"].cuda())
    _check_rates(got, c, 4 * ACC_TABLE[(P, C)][2], "accumulate P=%d C=%d" % (P, C))


def test_accumulate_sub_range_leaves_the_other_rows_alone():
    c = _acc_case(257, 65)
    xyz, recs = c["xyz"].cuda(), c["recs"].cuda()
    sentinel = torch.arange(257, dtype=torch.float32, device="cuda") * -1.5 - 7.0
    for init in (True, False):
        rate = sentinel.clone()
        _accumulate(xyz, recs, rate, row0=37, rows=100, init=init)
        keep = torch.ones(257, dtype=torch.bool, device="cuda")
        keep[37:137] = False
        assert torch.equal(rate[keep], sentinel[keep])
        sub = dict(c, lo=c["lo"][37:137], hi=c["hi"][37:137])
        _check_rates(rate[37:137], sub, 4 * ACC_TABLE[(257, 65)][2], "sub-range init=%d" % init)      # negative old values lose to 0 and to any rate
    # an unaligned rate / position base runs the single-row threads for every row: the same bits
    full = _accumulate(xyz, recs)
    pad_xyz, pad_rate = torch.zeros(257 * 3 + 1, device="cuda"), torch.zeros(258, device="cuda")
    pad_xyz[1:] = xyz.reshape(-1)
    _accumulate(pad_xyz[1:].view(257, 3), recs, pad_rate[1:])
    assert torch.equal(pad_rate[1:], full)


def test_accumulate_split_camera_sets_equal_the_union_bit_for_bit():
    c = _acc_case(1000, 300)
    xyz, recs = c["xyz"].cuda(), c["recs"].cuda()
    union = _accumulate(xyz, recs)
    for cut in (1, 117, 299):
        rate = _accumulate(xyz, recs[:cut].contiguous())
        _accumulate(xyz, recs[cut:], rate, init=False)
        assert torch.equal(rate, union), cut
        other = _accumulate(xyz, recs[cut:])
        _accumulate(xyz, recs[:cut].contiguous(), other, init=False)
        assert torch.equal(other, union), cut


def _rates_by_hand():
    g = torch.Generator().manual_seed(9)
    seen_all = torch.rand(300, generator=g) * 50 + 0.5
    some = seen_all.clone()
    some[torch.rand(300, generator=g) < 0.4] = 0.0
    last = torch.rand(1000, generator=g) * 50 + 2.0
    last[997] = 0.75          # the minimum in the last, partial wave (1000 = 15 x 64 + 40)
    last[::7] = 0.0
    return {"all seen": seen_all, "some unseen": some, "all unseen": torch.zeros(129), "single row": torch.tensor([3.25]),
            "single unseen row": torch.zeros(1), "minimum in the last partial wave": last}


@pytest.mark.parametrize("name", sorted(_rates_by_hand()))
def test_finalize(name):
    from adgs import filter3d
    rate = _rates_by_hand()[name]
    want = ref.filter_from_rate(rate.double())
    got = filter3d.finalize(rate.cuda())
    again = filter3d.finalize(rate.cuda())
    torch.cuda.synchronize()
    assert got.shape == (rate.numel(), 1) and torch.equal(got, again)
    got = got.cpu().reshape(-1)
    assert ((got.double() - want).abs() <= 1e-6 * want).all()
    seen = rate > 0
    if not seen.any():
        assert not got.any()
    else:
        assert torch.equal(got[~seen], got[seen].max().expand_as(got[~seen]))
        assert got[seen].max() == got[seen][rate[seen].argmin()]
    # in place on the rates
    buf = rate.cuda()
    assert torch.equal(filter3d.finalize(buf, out=buf).reshape(-1).cpu(), got)


@functools.lru_cache(maxsize=None)
def _apply_case(P):
    s, o, f, gS, gO = ref.make_apply_case(P, APPLY_TABLE[P][0])
    d = [t.double() for t in (s, o, f, gS, gO)]
    want = ref.apply_forward(*d[:3]) + ref.apply_backward(*d)
    f32 = ref.apply_forward(s, o, f) + ref.apply_backward(s, o, f, gS, gO)
    err32 = tuple(float(((a.double() - b).abs() / b.abs().clamp(min=1e-300)).max()) for a, b in zip(f32, want))
    return dict(inputs=(s, o, f, gS, gO), want=want, err32=err32)


def _ulp32(x64):
    x = x64.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _apply_on_gpu(s, o, f, gS, gO):
    from adgs import filter3d
    ss, oo = s.cuda().requires_grad_(True), o.cuda().requires_grad_(True)
    S, O = filter3d.apply(ss, oo, f.cuda())
    torch.autograd.backward([S, O], [gS.cuda(), gO.cuda()])
    torch.cuda.synchronize()
    return S.detach().cpu(), O.detach().cpu(), ss.grad.cpu(), oo.grad.cpu()


def test_apply_table_bounds_the_float32_cpu_evaluation():
    """APPLY_TABLE is a measurement (float32 torch on one CPU); torch's float32 kernels differ in the last bit between CPUs, so the
    table is not re-derived here: the float32 CPU evaluation of the machine that runs the test must itself meet the tolerance."""
    for P, (seed, *errs) in APPLY_TABLE.items():
        for a, b in zip(_apply_case(P)["err32"], errs):
            assert a <= max(4 * b, 2.0 ** -23), (P, a, b)


@pytest.mark.parametrize("P", P_LIST)
def test_apply_forward_and_backward(P):
    c = _apply_case(P)
    got = _apply_on_gpu(*c["inputs"])
    for name, g, w, e32 in zip(("S", "O", "dL/ds", "dL/do"), got, c["want"], APPLY_TABLE[P][1:]):
        assert g.shape == w.shape and g.dtype == torch.float32
        tol = torch.minimum(torch.maximum(4 * e32 * w.abs(), _ulp32(w)), 1e-4 * w.abs() + 1e-4 * w.abs().max())
        err = (g.double() - w).abs()
        print("apply P=%d %s: max err / tolerance %.3f (float32 CPU relative error %.2e)" % (P, name, float((err / tol).max()), e32))
        assert (err <= tol).all(), (name, int((err > tol).sum()))


def test_apply_unaligned_pointers_take_the_single_row_threads():
    from adgs import filter3d
    s, o, f, gS, gO = _apply_case(257)["inputs"]
    want = _apply_on_gpu(s, o, f, gS, gO)
    pad = lambda t: torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()[1:].view(t.shape)      # 4 bytes past a 16-byte boundary
    ss, oo = pad(s).requires_grad_(True), pad(o).requires_grad_(True)
    assert ss.data_ptr() % 16 == 4
    S, O = filter3d.apply(ss, oo, pad(f))
    torch.autograd.backward([S, O], [pad(gS), pad(gO)])
    for a, b in zip((S.detach(), O.detach(), ss.grad, oo.grad), want):
        assert torch.equal(a.cpu(), b)


def test_apply_zero_filter_rows_are_the_identity():
    s, o, f, gS, gO = _apply_case(1000)["inputs"]
    S, O, gs, go = _apply_on_gpu(s, o, f, gS, gO)
    zero = (f == 0).reshape(-1)
    assert 200 < int(zero.sum()) < 500
    assert ((S[zero].double() - s[zero].double()).abs() <= _ulp32(s[zero].double())).all()
    assert ((O[zero].double() - o[zero].double()).abs() <= 2 * _ulp32(o[zero].double())).all()
    assert ((go[zero].double() - gO[zero].double()).abs() <= 2 * _ulp32(gO[zero].double())).all()


def test_apply_nan_upstream_gradient_stays_in_its_row():
    s, o, f, gS, gO = _apply_case(257)["inputs"]
    clean = _apply_on_gpu(s, o, f, gS, gO)
    gS2, gO2 = gS.clone(), gO.clone()
    rows = [5, 130, 256]                                   # inside groups of four, and the single-row tail
    gS2[5, 1] = float("nan")
    gO2[130, 0] = float("nan")
    gS2[256, 0] = gO2[256, 0] = float("nan")
    dirty = _apply_on_gpu(s, o, f, gS2, gO2)
    keep = torch.ones(257, dtype=torch.bool)
    keep[rows] = False
    for a, b in zip(dirty, clean):
        assert torch.equal(a[keep], b[keep]) and not torch.isnan(a[keep]).any()
    assert torch.isnan(dirty[2][5, 1]) and torch.isnan(dirty[3][130, 0]) and torch.isnan(dirty[2][256, 0])
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1])


# ---------------------------------------------------------------- end to end: model, renderer, graph
W, H, FOCAL = 64, 48, 60.0


class Pipe:
    inv_depth, debug = True, False


def _pipe(**kw):
    p = Pipe()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _scene():
    from adgs import synthetic
    sc = synthetic.make_scene(300, W, H, FOCAL, sh_degree=3, seed=21, n_objects=2)
    cams = [synthetic.camera_object(synthetic.make_camera(W, H, FOCAL, cam_seed=k), time=t) for t in (0.2, 0.7) for k in (1, 2)]
    return sc, cams


def _model(raw_sh=False, raw_scene=False, filtered=True):
    from adgs.model import SyntheticGaussianModel
    sc, cams = _scene()
    m = SyntheticGaussianModel.from_scene(sc, device="cuda", seed=2)
    m.raw_sh, m.raw_scene = raw_sh, raw_scene
    if filtered:
        m.compute_3d_filter(cams)
    return m


def _reference_rates(model, cams):
    """The reference composition of compute_3d_filter: per time stamp the float64 rates of get_deformed_xyz(t) under that stamp's cameras."""
    from adgs import filter3d
    lo = hi = None
    err32 = 0.0
    for t in sorted({c.time for c in cams}):
        with torch.no_grad():
            xyz = model.get_deformed_xyz(t).cpu()
        recs = filter3d.camera_records([c for c in cams if c.time == t], "cpu")
        r = ref.rates(xyz, recs)
        err32 = max(err32, ref.float32_rate_error(xyz, recs, r))
        lo = r["rate_lo"] if lo is None else torch.maximum(lo, r["rate_lo"])
        hi = r["rate_hi"] if hi is None else torch.maximum(hi, r["rate_hi"])
    return lo, hi, err32


def test_compute_3d_filter_equals_the_reference_composition():
    sc, cams = _scene()
    m = _model()
    lo, hi, err32 = _reference_rates(m, cams)
    assert m.filter_3D.shape == (300, 1) and not m.filter_3D.requires_grad
    seen = lo > 0
    assert int((lo != hi).sum()) <= 3 and 30 < int(seen.sum())
    tol = min(4 * err32, 1e-4)
    got = m.filter_3D.double().cpu().reshape(-1)
    f_hi, f_lo = ref.filter_from_rate(lo), ref.filter_from_rate(hi)          # a smaller rate is a larger filter
    print("compute_3d_filter: %d of 300 rows seen, float32 CPU rate error %.2e, tolerance %.2e" % (int(seen.sum()), err32, tol))
    assert ((got >= f_lo * (1 - tol) * (1 - 1e-6)) & (got <= f_hi * (1 + tol) * (1 + 1e-6))).all()
    from adgs import deform, filter3d
    pkg = deform.get_deformed_pkg(m, 0.0, want=("opacity", "scales"))
    S, O = filter3d.apply(pkg["scales"], pkg["opacity"], m.filter_3D)
    assert torch.equal(m.get_scaling_with_3D_filter, S) and torch.equal(m.get_opacity_with_3D_filter(0.0), O)


def _hand_render(model, cam, pipe, grads=True):
    """The rasterizer entry render() takes for this model, called by hand with apply(...) outputs."""
    import gaussian_renderer as gr
    from adgs import filter3d
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = model._scene_xyz.device
    n = model.get_pts_num
    means2D = gr.screenspace_points(n, dev)
    absgrad = bool(getattr(pipe, "absgrad", False)) and torch.is_grad_enabled()
    kw = dict(means2D_abs=gr.screenspace_points(n, dev)) if absgrad else {}
    rast = GaussianRasterizer(raster_settings=gr._camera_settings(cam, model, pipe, 1.0, dev))
    pkg = model.get_deformed_pkg(cam.time, full_rows=True)
    S, O = filter3d.apply(pkg["scales"], pkg["opacity"], model.filter_3D)
    if torch.is_tensor(pkg["shs"]):
        out = rast(means3D=pkg["xyz"], means2D=means2D, opacities=O, shs=pkg["shs"], colors_precomp=None, scales=S, rotations=pkg["rotation"],
                   flow_points=None, semantic=None, **kw)
    else:
        out = rast.forward_rawsh(pkg["xyz"], means2D, O, pkg["shs"], S, pkg["rotation"], flow_points=None, semantic=None, factor_sink=None, bg_image=None, **kw)
    return dict(render=out[0], radii=out[1], depth=out[2].squeeze(0), img_opacity=out[3].squeeze(0), opacity=pkg["opacity"], viewspace_points=means2D,
                **({"viewspace_points_abs": kw["means2D_abs"]} if absgrad else {}))


def _upstream():
    g = torch.Generator().manual_seed(77)
    return [(torch.randn(3, H, W, generator=g) / (H * W)).cuda(), (torch.randn(H, W, generator=g) / (H * W)).cuda(),
            (torch.randn(H, W, generator=g) / (H * W)).cuda()]


def _backward(out, model):
    model.zero_grad()
    torch.autograd.backward([out["render"], out["depth"], out["img_opacity"]], _upstream())
    torch.cuda.synchronize()
    # background_deform_param is not listed: its one row is summed over all Gaussians with float atomics and is 1e-5 of the others
    grads = {n: getattr(model, n).grad.clone() for n in
             ("_scene_xyz", "_obj_xyz", "_scene_scaling", "_obj_scaling", "_scene_opacity", "_obj_opacity", "_scene_rotation", "_obj_rotation",
              "_scene_shs_dc", "_obj_shs_dc", "_scene_shs_rest", "_obj_shs_rest", "xyz_deform_param", "rotation_deform_param", "gs_time_sigma")
             if getattr(model, n).grad is not None}
    for k in ("viewspace_points", "viewspace_points_abs"):
        if k in out:
            grads[k] = out[k].grad.clone()
    return grads


def _render_spying(cam, model, pipe):
    """render() with adgs.filter3d.apply wrapped: (result, the calls' outputs with their gradients retained)."""
    from adgs import filter3d
    from gaussian_renderer import render
    calls, real = [], filter3d.apply

    def spy(s, o, f):
        S, O = real(s, o, f)
        if S.requires_grad:
            S.retain_grad()
            O.retain_grad()
        calls.append((S, O))
        return S, O
    filter3d.apply = spy
    try:
        return render(cam, model, None, pipe), calls
    finally:
        filter3d.apply = real


def _assert_parity(name, got, want):
    err = (got.double() - want.double()).abs()
    assert (err <= 1e-4 * want.double().abs() + 1e-4 * float(want.abs().max())).all(), (name, float(err.max()), float(want.abs().max()))


THROUGH_APPLY = ("_scene_scaling", "_obj_scaling", "_scene_opacity", "_obj_opacity", "gs_time_sigma")


@pytest.mark.parametrize("raw_sh,raw_scene", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("extra", [{}, {"antialiasing": True, "absgrad": True}])
def test_render_is_the_hand_call_with_apply_outputs(raw_sh, raw_scene, extra):
    from adgs import filter3d
    from gaussian_renderer import render
    sc, cams = _scene()
    cam = cams[2]
    m = _model(raw_sh, raw_scene)
    pipe = _pipe(filter_3d=True, **extra)
    out, calls = _render_spying(cam, m, pipe)
    assert len(calls) == 1
    g_render = _backward(out, m)
    hand = _hand_render(m, cam, pipe)
    g_hand = _backward(hand, m)
    for k in ("render", "radii", "depth", "img_opacity"):
        assert torch.equal(out[k], hand[k]), k
    assert int((out["radii"] > 0).sum()) > 50
    assert torch.equal(out["opacity"], hand["opacity"])      # the result's opacity stays the unfiltered one
    assert sorted(g_render) == sorted(g_hand) and len(g_render) >= 15 + (1 if extra else 0)
    for k in g_render:
        _assert_parity(k, g_render[k], g_hand[k])
    # the feature's own chain, bit for bit: the same apply outputs, and from the upstream gradients render()'s rasterizer delivered the
    # same gradients of everything that is reached through apply alone
    m.zero_grad()
    pkg = m.get_deformed_pkg(cam.time, full_rows=True)
    S, O = filter3d.apply(pkg["scales"], pkg["opacity"], m.filter_3D)
    assert torch.equal(S, calls[0][0]) and torch.equal(O, calls[0][1])
    torch.autograd.backward([S, O], [calls[0][0].grad, calls[0][1].grad])
    for k in THROUGH_APPLY:
        assert torch.equal(getattr(m, k).grad, g_render[k]), k
        assert float(g_render[k].abs().max()) > 0, k
    # the filter does something: the unfiltered frame differs
    plain = render(cam, m, None, _pipe(**extra))
    assert not torch.equal(plain["render"], out["render"])
    with torch.no_grad():
        ev, ev_hand = render(cam, m, None, pipe), _hand_render(m, cam, pipe)
    for k in ("render", "radii", "depth", "img_opacity"):
        assert ev[k].grad_fn is None and torch.equal(ev[k], ev_hand[k]) and torch.equal(ev[k], out[k].detach()), k


def test_render_raises_without_a_filter_and_after_densification():
    from gaussian_renderer import render
    sc, cams = _scene()
    m = _model(filtered=False)
    assert m.filter_3D is None
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        render(cams[0], m, None, _pipe(filter_3d=True))
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        m.get_scaling_with_3D_filter
    m.compute_3d_filter(cams)
    render(cams[0], m, None, _pipe(filter_3d=True))
    stale = m.filter_3D
    m.training_setup()
    m.xyz_gradient_accum += 1.0
    m.denom += 1.0
    m.densify_and_prune(0.5, 0.5, 0.005, False)
    assert m.filter_3D is None and m.get_pts_num != 300
    m.filter_3D = stale                                     # a filter of the wrong length
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        render(cams[0], m, None, _pipe(filter_3d=True))
    m.compute_3d_filter(cams)
    assert m.filter_3D.shape[0] == m.get_pts_num
    render(cams[0], m, None, _pipe(filter_3d=True))


def test_pipe_without_the_attribute_is_the_flag_off():
    """Neither frame reaches apply or asks the deformation pass for more rows: today's code path, the same forward bits (the two
    backward runs agree as two runs of one frame do: float atomics)."""
    sc, cams = _scene()
    m = _model(True, True)
    a, calls_a = _render_spying(cams[1], m, _pipe())
    ga = _backward(a, m)
    b, calls_b = _render_spying(cams[1], m, _pipe(filter_3d=False))
    gb = _backward(b, m)
    assert not calls_a and not calls_b
    assert type(a) is type(b) and sorted(a.keys()) == sorted(b.keys())
    for k in ("render", "radii", "depth", "img_opacity"):
        assert torch.equal(a[k], b[k]), k
    assert sorted(ga) == sorted(gb)
    for k in ga:
        _assert_parity(k, ga[k], gb[k])


def test_all_unseen_warns_once_and_gives_zeros():
    from adgs import filter3d, synthetic
    sc, cams = _scene()
    m = _model(filtered=False)
    away = synthetic.make_camera(W, H, FOCAL, cam_seed=1)
    away["viewmatrix"] = away["viewmatrix"].clone()
    away["viewmatrix"][3, 2] -= 1000.0                     # everything far behind the camera
    filter3d._warned_unseen = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m.compute_3d_filter([synthetic.camera_object(away, time=0.5)])
        m.compute_3d_filter([synthetic.camera_object(away, time=0.5)])
    assert len([w for w in rec if "no camera sees" in str(w.message)]) == 1
    assert m.filter_3D.shape == (300, 1) and not m.filter_3D.any()


def test_graph_replay_of_a_filtered_frame():
    from adgs import graph
    from gaussian_renderer import render
    sc, cams = _scene()
    m = _model(True, True)
    pipe = _pipe(filter_3d=True)

    def fn():
        with torch.no_grad():
            out = render(cams[3], m, None, pipe)
        return out["render"], out["depth"], out["img_opacity"]
    eager = [t.clone() for t in fn()]
    step = graph.GraphedStep(fn)
    got = step()
    torch.cuda.synchronize()
    assert step.validate(repair=False)
    for a, b in zip(got, eager):
        assert torch.equal(a, b)


def test_ply_round_trip_on_the_device(tmp_path):
    sc, cams = _scene()
    m = _model()
    path = os.path.join(str(tmp_path), "point_cloud.ply")
    m.save_ply(path)
    n = _model(filtered=False)
    n.load_ply(path)
    assert torch.equal(n.filter_3D, m.filter_3D) and n.filter_3D.is_cuda
    m.filter_3D = None
    m.save_ply(path)
    n.load_ply(path)
    assert n.filter_3D is None
