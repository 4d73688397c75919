"""The multi-view photometric consistency loss on the GPU (adgs.multiview over include/adgs_multiview.h, csrc/multiview.hip) against
tests/multiview_ref.py (float64 torch-CPU, autograd) on the cases of tests/multiview_cases.py.

The cases: a 48 x 64 reference against a 40 x 72 neighbour with its own field of view, 1024 unique samples, radius 1, 2, 3 (9, 25, 49 of
the wave's 64 lanes), both inv_depth settings, with and without a weight; S = 1, 3, 257 (one wave, one partial workgroup, one past 64
workgroups); 96 x 96 with S = 9000 at radius 1 (2250 groups of four samples on the 2048 workgroups the grid is capped at: waves stride to a second sample, eight adds per slot row); one
case whose max_error lies inside the distribution of e.  Every case's samples keep 1e-3 away from every gate (the margin rule of the
case generator), so the kernel and the reference decide every validity alike and every sample is compared: L within rtol 1e-5, every
gradient element within 1e-4 max|ref| of its tensor, exactly zero where the reference's gradient is (every unsampled pixel), e within
1e-5 and `valid` equal.  A reference is computed once per case and shared.

The float32 restatement of the reference misses these tolerances (tests/test_multiview_ref.py: up to 2.2e-3 max|ref| in the gradients at
radius 1), which is why the kernel carries the per-tap chain and the sums in double."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import multiview_cases as cases
from tests import multiview_ref as ref

pytestmark = pytest.mark.gpu


def run_gpu(inp, c, samples=None, pose=None, upstream=1.0, need=(True, True, True), prepare=None, **over):
    """-> (L, [gN, gD, gO] as float64 numpy or None, e [S], valid [S]) of adgs.multiview on a case's inputs."""
    from adgs import multiview
    N, D, O = inp.N.cuda().requires_grad_(need[0]), inp.D.cuda().requires_grad_(need[1]), inp.O.cuda().requires_grad_(need[2])
    consts = dict(ref=inp.ref_gray.cuda(), nbr=inp.nbr_gray.cuda(), weight=None if inp.weight is None else inp.weight.cuda())
    maps = dict(N=N, D=D, O=O)
    if prepare is not None:
        maps, consts = prepare(maps, consts)
    s = (inp.samples if samples is None else samples).cuda()
    kw = dict(weight=consts["weight"], radius=c.radius, inv_depth=c.inv_depth, max_error=c.max_error)
    kw.update(over)
    args = (maps["N"], maps["D"], maps["O"], cases.TAN, consts["ref"], consts["nbr"], cases.TAN_N, inp.pose if pose is None else pose, s)
    L = multiview.photometric_consistency_loss(*args, **kw)
    if any(need):
        (L * upstream).backward()
    grads = [None if t.grad is None else t.grad.cpu().double().numpy() for t in (N, D, O)]
    e, valid = multiview.patch_errors(*args, **kw)
    return L.item(), grads, e.cpu(), valid.cpu()


def reference_of(inp, c, samples=None, pose=None, **over):
    kw = dict(weight=inp.weight, radius=c.radius, inv_depth=c.inv_depth, max_error=c.max_error)
    kw.update(over)
    res, grads = ref.with_grads(inp.N, inp.D, inp.O, cases.TAN, inp.ref_gray, inp.nbr_gray, cases.TAN_N, inp.pose if pose is None else pose,
                                inp.samples if samples is None else samples, **kw)
    assert not ref.near_gate(res.margins).any()                    # the kernel and the reference decide every validity alike
    return res, grads


def compare(got, want, what, upstream=1.0, need=(True, True, True)):
    L, grads, e, valid = got
    res, rg = want
    rL = float(res.L)
    print("%s: L = %.9g (ref %.9g), %d of %d samples valid" % (what, L, rL, int(valid.sum()), valid.numel()))
    assert abs(L - rL) <= 1e-5 * abs(rL), (what, L, rL)
    assert torch.equal(valid, res.valid), what
    assert float((e.double() - res.e).abs().max()) <= 1e-5 if e.numel() else True, what
    for name, g, r, wanted in zip(("normal", "depth", "opacity"), grads, rg, need):
        assert (g is not None) == wanted, (what, name)
        if not wanted:
            continue
        r = r.numpy()
        assert g.shape == r.shape and np.isfinite(g).all(), (what, name)
        err, scale = np.abs(g - upstream * r).max(), np.abs(r).max() * abs(upstream)
        print("    dL/d%s: max error %.2e of max|ref| %.2e" % (name, err / scale if scale else err, scale))
        assert err <= 1e-4 * scale, (what, name, err, scale)
        assert not g[r == 0].any(), (what, name)                   # exactly zero wherever the reference is: every unsampled pixel


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_values_and_gradients(name):
    c, inp = cases.BY_NAME[name], cases.inputs(name)
    compare(run_gpu(inp, c), cases.reference(name), name)


def test_an_upstream_factor():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    compare(run_gpu(inp, c, upstream=-1.3), cases.reference(cases.BASE), "upstream -1.3", upstream=-1.3)


def test_each_subset_of_requires_grad():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    for need in itertools.product((False, True), repeat=3):
        compare(run_gpu(inp, c, need=need), cases.reference(cases.BASE), "requires_grad %s" % (need,), need=need)


def test_all_samples_invalid():
    """Nothing opaque enough, or nothing weighted: L == 0 and the gradients are exactly zero, decided on the device."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    dim = inp._replace(O=torch.full_like(inp.O, 0.3))
    unweighted = inp._replace(weight=torch.zeros_like(inp.O))
    for what, variant in (("opacity 0.3", dim), ("weight 0", unweighted)):
        L, grads, e, valid = run_gpu(variant, c, upstream=2.0)
        res, rg = reference_of(variant, c)
        assert float(res.L) == 0.0 and not any(g.any() for g in rg)
        assert L == 0.0 and all(g is not None and not g.any() for g in grads), what
        assert torch.equal(valid, res.valid) and float((e.double() - res.e).abs().max()) <= 1e-5
    assert not run_gpu(dim, c)[3].any()


def test_a_neighbour_behind_the_reference_camera():
    """The neighbour looks the other way: every tap has m.z <= 0, which is an invalid sample and not a fault."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    pose = torch.tensor([[-1.0, 0, 0, 0.1], [0, 1.0, 0, 0], [0, 0, -1.0, -0.5]], dtype=torch.float64)
    res, rg = reference_of(inp, c, pose=pose)
    assert not res.valid.any() and float(res.margins[:, 3].min()) < -0.5
    L, grads, e, valid = run_gpu(inp, c, pose=pose)
    assert L == 0.0 and not valid.any() and not e.any() and all(not g.any() for g in grads)


def test_border_pixels_and_indices_outside_the_image():
    """Border pixels and indices outside [0, H W) are invalid samples: never dereferenced, no gradient, and the rest is unchanged."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    HW, W, r = c.H * c.W, c.W, c.radius
    odd = [0, W - 1, HW - 1, HW - W, (r - 1) * W + 20, 20 * W + r - 1, 20 * W + W - r, (c.H - r) * W + 20,
           -1, -5, -HW, HW, HW + 7, 3 * HW + 11, 2 ** 31 - 1, -2 ** 31, 2 ** 30]
    s = torch.cat([inp.samples[:200], torch.tensor(odd, dtype=torch.int32), inp.samples[200:400]])
    want = reference_of(inp, c, samples=s)
    assert not want[0].valid[200:200 + len(odd)].any() and int(want[0].valid.sum()) > 100
    got = run_gpu(inp, c, samples=s)
    compare(got, want, "border and out-of-range indices")
    assert not got[2][200:200 + len(odd)].any()


def test_duplicate_indices_receive_the_sum():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    s = torch.cat([inp.samples[:300], inp.samples[:300], inp.samples[100:200], inp.samples[300:350]])
    want = reference_of(inp, c, samples=s)
    compare(run_gpu(inp, c, samples=s), want, "duplicates")


def test_non_contiguous_and_batched_inputs():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)

    def prepare(maps, consts):
        def strided(t):                                            # the same values behind a column stride of two
            wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device)
            wide[..., ::2] = t.detach()
            return wide[..., ::2]
        for k in ("ref", "nbr", "weight"):
            consts[k] = strided(consts[k])
            assert not consts[k].is_contiguous()
        consts["weight"] = consts["weight"][None]
        maps = dict(N=maps["N"].permute(1, 2, 0).contiguous().permute(2, 0, 1), D=maps["D"][None], O=maps["O"].t().contiguous().t()[None])
        assert not maps["N"].is_contiguous() and not maps["O"].is_contiguous() and maps["D"].dim() == 3
        return maps, consts

    compare(run_gpu(inp, c, prepare=prepare), cases.reference(cases.BASE), "non-contiguous, [1, H, W]")


def test_two_calls_on_one_work_buffer_are_identical():
    """The finish kernel leaves the slot rows zero: a second call on the same buffer gives the same bits (1024 samples are at most 256
    workgroups: one add per slot row, so the sums themselves are deterministic), and so does the backward, which adds once per pixel."""
    from adgs import _lib, multiview
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    dev = torch.device("cuda", torch.cuda.current_device())
    N, D, O, Ir, In, w, s = (t.to(dev).contiguous() for t in (inp.N, inp.D, inp.O, inp.ref_gray, inp.nbr_gray, inp.weight, inp.samples))
    S = s.numel()
    assert S <= 1024 and torch.unique(s).numel() == S
    R, t = ref.pose12(inp.pose)
    desc = multiview.make_desc(c.H, c.W, c.Hn, c.Wn, c.radius, c.inv_depth, cases.TAN, cases.TAN_N, 0.5, 0.1, c.max_error, multiview.EPS,
                               R.reshape(-1).tolist() + t.tolist())
    work = torch.zeros(multiview.MULTIVIEW_WORK_DOUBLES, dtype=torch.float64, device=dev)
    g_loss = torch.ones(1, device=dev)
    outs = []
    for _ in range(2):
        loss, e, valid = torch.empty(1, device=dev), torch.empty(S, device=dev), torch.empty(S, dtype=torch.uint8, device=dev)
        gN, gD, gO = torch.full_like(N, float("nan")), torch.full_like(D, float("nan")), torch.full_like(O, float("nan"))     # the call zero-fills
        _lib.call("adgs_multiview_ncc_forward", dev, ctypes.byref(desc), N.data_ptr(), D.data_ptr(), O.data_ptr(), Ir.data_ptr(), In.data_ptr(), w.data_ptr(),
                  s.data_ptr(), S, work.data_ptr(), loss.data_ptr(), e.data_ptr(), valid.data_ptr())
        _lib.call("adgs_multiview_ncc_backward", dev, ctypes.byref(desc), N.data_ptr(), D.data_ptr(), O.data_ptr(), Ir.data_ptr(), In.data_ptr(), w.data_ptr(),
                  s.data_ptr(), S, work.data_ptr(), g_loss.data_ptr(), gN.data_ptr(), gD.data_ptr(), gO.data_ptr())
        outs.append([x.cpu() for x in (loss, e, valid, gN, gD, gO, work)])
    a, b = outs
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rows = multiview.SLOTS * 2
    assert not a[6][:rows].any() and float(a[6][rows + 1]) > 0       # the rows are zero again; sum w v is behind them
    res, rg = cases.reference(cases.BASE)
    assert abs(float(a[0]) - float(res.L)) <= 1e-5 * float(res.L) and abs(float(a[6][rows + 2]) - float(res.L)) <= 1e-9
    for g, r in zip(a[3:6], rg):
        assert torch.isfinite(g).all() and float((g.double() - r).abs().max()) <= 1e-4 * float(r.abs().max())
