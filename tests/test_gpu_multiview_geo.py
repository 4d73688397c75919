"""The multi-view geometric consistency loss on the GPU (adgs.multiview over include/adgs_multiview_geo.h, csrc/multiview_geo.hip)
against tests/multiview_geo_ref.py (float64 torch-CPU, autograd) on the cases of tests/multiview_geo_cases.py.

The cases: a 48 x 64 reference against a 40 x 72 neighbour with its own field of view, both inv_depth settings, with and without a
weight; 45 x 61 (no multiple of the 32 x 8 tile); 272 x 512 (544 workgroups on the 256 slot rows); 24 x 32 against 160 x 288 (a tile's
footprint in the neighbour exceeds the 2048-pixel LDS window: the direct-atomic path; every other case takes the window); 96 x 128
against 12 x 16 (~64 reference pixels add into each neighbour pixel); one case whose max_pixel_error is the median of its errors.  A
weighted case's weight is zero within 1e-3 of every gate and the unweighted cases have no such pixel (the margin rule of the case
generator), so the kernel and the reference decide alike wherever it counts: L within rtol 1e-5; err_out within 1e-5 px, weight_out
within 1e-5 and validity equal outside the near-gate pixels; every gradient element within 1e-4 max|ref| of its tensor and exactly zero
where the reference's gradient is.  A reference is computed once per case and shared.

The float32 restatement of the reference misses these tolerances (tests/test_multiview_geo_ref.py: at 1280 x 1920 err is off by up to
5.2e-4 px and the gradients by 1.7 max|ref|), which is why the kernel carries the chain in double."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import multiview_geo_cases as cases
from tests import multiview_geo_ref as ref
from tests.multiview_cases import TAN, TAN_N

pytestmark = pytest.mark.gpu
NAMES = ("depth", "opacity", "nbr_depth", "nbr_opacity")


def run_gpu(inp, c, pose=None, upstream=1.0, need=(True, True, True, True), prepare=None, **over):
    """-> (L, [gD, gO, gDn, gOn] as float64 numpy or None, err [H, W], geo_weight [H, W]) of adgs.multiview on a case's inputs."""
    from adgs import multiview
    maps = [t.cuda().requires_grad_(n) for t, n in zip((inp.D, inp.O, inp.Dn, inp.On), need)]
    weight = None if inp.weight is None else inp.weight.cuda()
    given = list(maps)
    if prepare is not None:
        given, weight = prepare(given, weight)
    kw = dict(weight=weight, inv_depth=c.inv_depth, max_pixel_error=inp.max_pixel_error)
    kw.update(over)
    args = (given[0], given[1], TAN, given[2], given[3], TAN_N, inp.pose if pose is None else pose)
    L = multiview.geometric_consistency_loss(*args, **kw)
    if any(need):
        (L * upstream).backward()
    grads = [None if t.grad is None else t.grad.cpu().double().numpy() for t in maps]
    err, gw = multiview.reprojection_errors(*args, **kw)
    assert err.dtype == gw.dtype == torch.float32 and err.shape == gw.shape == inp.D.shape[-2:]
    return L.item(), grads, err.cpu(), gw.cpu()


def reference_of(inp, c, pose=None, **over):
    kw = dict(weight=inp.weight, inv_depth=c.inv_depth, max_pixel_error=inp.max_pixel_error)
    kw.update(over)
    return ref.with_grads(inp.D, inp.O, TAN, inp.Dn, inp.On, TAN_N, inp.pose if pose is None else pose, **kw)


def compare(got, want, what, upstream=1.0, need=(True, True, True, True)):
    L, grads, err, gw = got
    res, rg = want
    rL = float(res.L)
    far = ~ref.near_gate(res.margins)
    print("%s: L = %.9g (ref %.9g), %d of %d pixels valid, %d near a gate" % (what, L, rL, int(res.valid.sum()), res.valid.numel(), int((~far).sum())))
    assert abs(L - rL) <= 1e-5 * abs(rL), (what, L, rL)
    e_err, e_gw = float((err.double() - res.err)[far].abs().max()), float((gw.double() - res.gw)[far].abs().max())
    print("    err_out: max error %.2e px; weight_out: max error %.2e" % (e_err, e_gw))
    assert e_err <= 1e-5 and e_gw <= 1e-5, what
    assert torch.equal((gw > 0)[far], res.valid[far]), what
    for name, g, r, wanted in zip(NAMES, grads, rg, need):
        assert (g is not None) == wanted, (what, name)
        if not wanted:
            continue
        r = r.numpy()
        assert g.shape == r.shape and np.isfinite(g).all(), (what, name)
        e, scale = np.abs(g - upstream * r).max(), np.abs(r).max() * abs(upstream)
        print("    dL/d%s: max error %.2e of max|ref| %.2e" % (name, e / scale if scale else e, scale))
        assert e <= 1e-4 * scale, (what, name, e, scale)
        assert not g[r == 0].any(), (what, name)                   # exactly zero wherever the reference is


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_values_and_gradients(name):
    c, inp = cases.BY_NAME[name], cases.inputs(name)
    compare(run_gpu(inp, c), cases.reference(name), name)


def test_an_upstream_factor():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    compare(run_gpu(inp, c, upstream=-1.3), cases.reference(cases.BASE), "upstream -1.3", upstream=-1.3)


def test_each_subset_of_requires_grad():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    for need in itertools.product((False, True), repeat=4):
        compare(run_gpu(inp, c, need=need), cases.reference(cases.BASE), "requires_grad %s" % (need,), need=need)


def test_reference_gradients_do_not_depend_on_the_neighbour_gradients():
    """The neighbour rendered under no_grad: no fill and no atomic, and the reference view's gradients are the same bits."""
    for name in (cases.BASE, "big_nbr"):
        c, inp = cases.BY_NAME[name], cases.inputs(name)
        with_n, without = run_gpu(inp, c)[1], run_gpu(inp, c, need=(True, True, False, False))[1]
        assert without[2] is None and without[3] is None
        assert np.array_equal(with_n[0], without[0]) and np.array_equal(with_n[1], without[1]) and with_n[0].any()


def test_all_pixels_invalid():
    """Nothing opaque enough, or nothing weighted: L == 0 and the gradients are exactly zero, decided on the device."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    dim = inp._replace(O=torch.full_like(inp.O, 0.3))
    dim_n = inp._replace(On=torch.full_like(inp.On, 0.3))
    unweighted = inp._replace(weight=torch.zeros_like(inp.O))
    for what, variant in (("opacity 0.3", dim), ("neighbour's opacity 0.3", dim_n), ("weight 0", unweighted)):
        L, grads, err, gw = run_gpu(variant, c, upstream=2.0)
        res, rg = reference_of(variant, c)
        assert float(res.L) == 0.0 and not any(g.any() for g in rg)
        assert L == 0.0 and all(g is not None and not g.any() for g in grads), what
        far = ~ref.near_gate(res.margins)
        assert torch.equal((gw > 0)[far], res.valid[far]) and float((err.double() - res.err)[far].abs().max()) <= 1e-5
    for variant in (dim, dim_n):
        L, grads, err, gw = run_gpu(variant, c)
        assert not gw.any() and not err.any()


def test_a_neighbour_behind_the_reference_camera():
    """The neighbour looks the other way: every Y.z <= 0, which is an invalid pixel and not a fault; nothing of the neighbour is read."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    pose = torch.tensor([[-1.0, 0, 0, 0.1], [0, 1.0, 0, 0], [0, 0, -1.0, -0.5]], dtype=torch.float64)
    res, rg = reference_of(inp, c, pose=pose)
    assert not res.geo.any() and float(res.margins[..., 1][torch.isfinite(res.margins[..., 1])].max()) < -0.5
    L, grads, err, gw = run_gpu(inp, c, pose=pose)
    assert L == 0.0 and not gw.any() and not err.any() and all(not g.any() for g in grads)


def test_non_contiguous_and_batched_inputs():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)

    def prepare(maps, weight):
        def strided(t):                                            # the same values behind a column stride of two
            wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device)
            wide[..., ::2] = t.detach()
            return wide[..., ::2]
        weight = strided(weight)[None]
        D, O, Dn, On = maps
        given = [D[None], O.t().contiguous().t()[None], Dn.t().contiguous().t(), On[None]]
        assert not weight.is_contiguous() and not given[1].is_contiguous() and not given[2].is_contiguous() and given[0].dim() == 3
        return given, weight

    compare(run_gpu(inp, c, prepare=prepare), cases.reference(cases.BASE), "non-contiguous, [1, H, W]")


def test_two_calls_on_one_work_buffer_are_identical():
    """The finish kernel leaves the slot rows zero: a second call on the same buffer gives the same bits (12 workgroups: one add per
    slot row, so the sums themselves are deterministic), and so does the reference view's half of the backward, which stores once per
    pixel.  The neighbour's half is a sum of float atomics in arrival order: within the tolerance only."""
    from adgs import _lib, multiview
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    dev = torch.device("cuda", torch.cuda.current_device())
    D, O, Dn, On, w = (t.to(dev).contiguous() for t in (inp.D, inp.O, inp.Dn, inp.On, inp.weight))
    assert ((c.H + 7) // 8) * ((c.W + 31) // 32) <= multiview.SLOTS
    R, t = ref.pose12(inp.pose)
    desc = multiview.make_geo_desc(c.H, c.W, c.Hn, c.Wn, c.inv_depth, TAN, TAN_N, 0.5, inp.max_pixel_error, R.reshape(-1).tolist() + t.tolist())
    work = torch.zeros(multiview.MULTIVIEW_GEO_WORK_DOUBLES, dtype=torch.float64, device=dev)
    g_loss = torch.ones(1, device=dev)
    outs = []
    for _ in range(2):
        loss, err, gw = torch.empty(1, device=dev), torch.full_like(D, float("nan")), torch.full_like(D, float("nan"))
        gD, gO, gDn, gOn = (torch.full_like(x, float("nan")) for x in (D, O, Dn, On))       # the call writes or zero-fills every element
        _lib.call("adgs_multiview_geo_forward", dev, ctypes.byref(desc), D.data_ptr(), O.data_ptr(), Dn.data_ptr(), On.data_ptr(), w.data_ptr(),
                  work.data_ptr(), loss.data_ptr(), err.data_ptr(), gw.data_ptr())
        _lib.call("adgs_multiview_geo_backward", dev, ctypes.byref(desc), D.data_ptr(), O.data_ptr(), Dn.data_ptr(), On.data_ptr(), w.data_ptr(),
                  work.data_ptr(), g_loss.data_ptr(), gD.data_ptr(), gO.data_ptr(), gDn.data_ptr(), gOn.data_ptr())
        outs.append([x.cpu() for x in (loss, err, gw, gD, gO, work, gDn, gOn)])
    a, b = outs
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    rows = multiview.SLOTS * 2
    assert not a[5][:rows].any() and float(a[5][rows + 1]) > 0       # the rows are zero again; sum w v is behind them
    res, rg = cases.reference(cases.BASE)
    assert abs(float(a[0]) - float(res.L)) <= 1e-5 * float(res.L) and abs(float(a[5][rows + 2]) - float(res.L)) <= 1e-9
    for out in (a, b):
        for g, r in zip((out[3], out[4], out[6], out[7]), rg):
            assert torch.isfinite(g).all() and float((g.double() - r).abs().max()) <= 1e-4 * float(r.abs().max())
