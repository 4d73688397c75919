"""The weighted image losses (adgs.loss with `weight=`) and the sparse metric depth term on the GPU against tests/masked_loss_ref.py
(float64 torch-CPU): values at rtol 1e-5, gradients at atol = 1e-4 max|ref| (the tolerances of tests/test_gpu_loss.py for this kernel
family), no element exempt.  Shapes are the smallest at which the 32x16 tile kernels can go wrong."""
import functools

import numpy as np
import pytest
import torch

from tests import masked_loss_ref as ref

pytestmark = pytest.mark.gpu

# [..., C, H, W]: below one tile and below the window; exactly one tile; one-pixel partial tiles on both axes (four workgroups); several
# tiles with partial ones; 3 x 7 x 16 = 336 workgroups (more than the 256 slot rows: the slot wrap); the weight's broadcast over a batch
SHAPES = [(C, H, W) for H, W in ((1, 1), (3, 5), (16, 32), (17, 33), (37, 121)) for C in (1, 3)] + [(3, 97, 481), (2, 3, 17, 33)]
WEIGHTS = ("ones", "zeros", "zero_rows", "binary", "fractional", "corner_pixel")
UPSTREAM = ((1.0, 0.0), (0.0, 1.0), (0.7, -1.3))               # the L1 part, the SSIM part, both


def make_weight(kind, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "ones":
        return torch.ones(H, W)
    if kind == "zeros":
        return torch.zeros(H, W)
    if kind == "zero_rows":                                    # the ego vehicle: whole tile rows at the bottom (half the rows below one tile)
        cut = 16 * (((H + 15) // 16) // 2) or H // 2
        w = torch.ones(H, W)
        w[cut:] = 0
        return w
    if kind == "binary":
        return (torch.rand(H, W, generator=g) > 0.5).float()
    if kind == "fractional":
        return torch.rand(H, W, generator=g)
    if kind == "corner_pixel":
        w = torch.zeros(H, W)
        w[H - 1, W - 1] = 0.75
        return w
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def images(shape):
    g = torch.Generator().manual_seed(sum(shape) * 7 + len(shape))
    gt = torch.rand(*shape, generator=g)
    img = (gt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return img, gt


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """(weight, L1_w, SSIM_w, dL1_w, dSSIM_w) in float64 on the CPU, computed once per case and shared"""
    img, gt = images(shape)
    w = make_weight(kind, *shape[-2:])
    return (w,) + ref.l1_ssim_grads(img, gt, w)


def assert_grad(got, want, what):
    want = want.numpy() if torch.is_tensor(want) else want
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), want, rtol=0, atol=1e-4 * np.abs(want).max(), err_msg=str(what))


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weighted_l1_ssim_values_and_gradients(shape, kind):
    from adgs import loss
    img, gt = images(shape)
    w, r_l1, r_s, rg_l1, rg_s = reference(shape, kind)
    x = img.cuda().requires_grad_(True)
    wd = w.cuda()
    l1, s = loss.l1_ssim(x, gt.cuda(), weight=wd if shape[-1] % 2 else wd[None])         # both accepted layouts
    v_l1, v_s = float(l1.detach()), float(s.detach())
    print("%s %s: L1 %.9g (ref %.9g)  SSIM %.9g (ref %.9g)" % (shape, kind, v_l1, r_l1, v_s, r_s))
    np.testing.assert_allclose(v_l1, r_l1, rtol=1e-5, atol=0)
    np.testing.assert_allclose(v_s, r_s, rtol=1e-5, atol=0)
    for a, b in UPSTREAM:
        (g,) = torch.autograd.grad((l1, s), x, (torch.tensor(a).cuda(), torch.tensor(b).cuda()), retain_graph=True)
        want = a * rg_l1 + b * rg_s
        print("  upstream (%g, %g): max|err| %.3g of max|ref| %.3g" % (a, b, float((g.cpu().double() - want).abs().max()), float(want.abs().max())))
        assert g.shape == x.shape and bool(torch.isfinite(g).all())
        assert_grad(g, want, (shape, kind, a, b))
        if b == 0.0:                                           # the L1 gradient is exactly zero where nothing is supervised
            assert not g[..., wd == 0].any()
    if kind == "zeros":
        assert v_l1 == 0.0 and v_s == 0.0
        (g,) = torch.autograd.grad(l1 + s, x)
        assert bool(torch.isfinite(g).all()) and not g.any()


def test_named_wrappers_take_the_weight():
    from adgs import loss
    shape = (3, 17, 33)
    img, gt = images(shape)
    w, r_l1, r_s, rg_l1, rg_s = reference(shape, "fractional")
    x, y, wd = img.cuda().requires_grad_(True), gt.cuda(), w.cuda()
    np.testing.assert_allclose(float(loss.l1_loss(x, y, weight=wd)), r_l1, rtol=1e-5)
    np.testing.assert_allclose(float(loss.ssim(x, y, weight=wd)), r_s, rtol=1e-5)
    lam = 0.2
    total, l1, dssim = loss.photometric_loss(x, y, lam, weight=wd)
    np.testing.assert_allclose([float(l1), float(dssim)], [r_l1, 1 - r_s], rtol=1e-5)
    total.backward()
    assert_grad(x.grad, (1 - lam) * rg_l1 - lam * rg_s, "photometric_loss")


def test_slot_rows_are_left_zero_and_each_backward_uses_its_own_sum_of_weights():
    """Two calls in a row on one stream return the same values (the forward leaves its slot rows zero, whichever arena slice the second
    call gets); a forward, a second forward with another weight, then both backwards: sum w stays on the device, per call."""
    from adgs import loss
    shape = (3, 97, 481)
    img, gt = images(shape)
    y = gt.cuda()
    wa, wb = make_weight("fractional", 97, 481).cuda(), make_weight("zero_rows", 97, 481).cuda()

    def alone(w):
        x = img.cuda().requires_grad_(True)
        l1, s = loss.l1_ssim(x, y, weight=w)
        (g,) = torch.autograd.grad(0.7 * l1 - 1.3 * s, x)
        return l1.detach(), s.detach(), g
    first, again = alone(wa), alone(wa)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    arena = loss._ARENAS[(wa.device, loss._lib.stream_ptr(wa.device).value, loss.L1_SSIM_WEIGHTED_WORK_DOUBLES)]
    assert float(arena.buf[:, :3 * loss.SLOTS].abs().max()) == 0.0
    only_b = alone(wb)
    xa, xb = img.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
    ta, tb = loss.l1_ssim(xa, y, weight=wa), loss.l1_ssim(xb, y, weight=wb)
    (0.7 * ta[0] - 1.3 * ta[1]).backward()
    (0.7 * tb[0] - 1.3 * tb[1]).backward()
    assert torch.equal(ta[0], first[0]) and torch.equal(tb[1], only_b[1])
    assert torch.equal(xa.grad, first[2]) and torch.equal(xb.grad, only_b[2])
    assert float(wa.sum()) != float(wb.sum())


def test_no_weight_is_bitwise_the_call_without_the_argument():
    from adgs import loss
    img, gt = images((3, 37, 121))
    y = gt.cuda()

    def run(**kw):
        x = img.cuda().requires_grad_(True)
        l1, s = loss.l1_ssim(x, y, **kw)
        (g,) = torch.autograd.grad(0.7 * l1 - 1.3 * s, x)
        return l1.detach(), s.detach(), g
    for a, b in zip(run(), run(weight=None)):
        assert torch.equal(a, b)
    g = torch.Generator().manual_seed(4)
    pred, tgt = (torch.rand(37, 121, generator=g) * 0.9 + 0.05).cuda(), (torch.rand(37, 121, generator=g) > 0.5).float().cuda()
    for fn in (loss.sky_loss, lambda p, t, **kw: loss.obj_loss(p[None], t, **kw), loss.bce_clip_loss):
        pa, pb = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
        a, b = fn(pa, tgt), fn(pb, tgt, weight=None)
        a.backward(); b.backward()
        assert torch.equal(a, b) and torch.equal(pa.grad, pb.grad)


@pytest.mark.parametrize("shape", [(1, 3, 5), (3, 17, 33), (3, 37, 121), (2, 3, 17, 33), (3, 97, 481)], ids=lambda s: "x".join(map(str, s)))
def test_weight_of_ones_against_the_unweighted_path(shape):
    """3x97x481: 336 workgroups, the slot wrap of the unweighted kernel (the weighted one meets its reference there, above)"""
    from adgs import loss
    img, gt = images(shape)
    y = gt.cuda()
    res = []
    for kw in ({}, {"weight": torch.ones(shape[-2:], device="cuda")}):
        x = img.cuda().requires_grad_(True)
        l1, s = loss.l1_ssim(x, y, **kw)
        (g,) = torch.autograd.grad(0.7 * l1 - 1.3 * s, x)
        res.append((float(l1), float(s), g.cpu().numpy()))
    (l1_u, s_u, g_u), (l1_w, s_w, g_w) = res
    np.testing.assert_allclose([l1_w, s_w], [l1_u, s_u], rtol=1e-6, atol=0)
    np.testing.assert_allclose(g_w, g_u, rtol=0, atol=1e-6 * np.abs(g_u).max())


@pytest.mark.parametrize("C", [1, 3])
def test_training_loss_over_a_region_is_the_evaluators_metric_over_it(C):
    """images in [0, 1] (the Evaluator clips): L1_w and SSIM_w are region 1 of an Evaluator fed the same weight"""
    from adgs import loss, metrics
    img, gt = images((C, 37, 121))
    for kind in ("zero_rows", "fractional"):
        w = make_weight(kind, 37, 121).cuda()
        x, y = img.cuda(), gt.cuda()
        ev = metrics.Evaluator(1, regions=1)
        ev.add(x, y, masks=[w])
        region = ev.results()[1]
        l1, s = loss.l1_ssim(x, y, weight=w)
        np.testing.assert_allclose(float(l1), region["l1"][0], rtol=1e-5)
        np.testing.assert_allclose(float(s), region["ssim"][0], rtol=1e-5)


# the ids of the 37 x 121 cases are "term-kind", as they were before the second shape
BCE_CASES = [pytest.param(term, kind, H, W, id="-".join((term, kind) + (("%dx%d" % (H, W),) if (H, W) != (37, 121) else ())))
             for H, W in ((37, 121), (130, 127)) for kind in WEIGHTS for term in ("obj", "sky")]


@pytest.mark.parametrize("term,kind,H,W", BCE_CASES)
def test_weighted_bce_terms(term, kind, H, W):
    """both parameter sets, predictions drawn away from the clip bounds; the tolerances of tests/test_gpu_loss.py:136-139.
    37 x 121: 18 workgroups, one add per slot row; 130 x 127 = 16 510 elements: 65 workgroups of four waves, 260 adds into the 256 rows
    (rows 0 - 3 take two each: a + b onto +0.0 in either order is the same double, so the result is still the same from every call)."""
    from adgs import loss
    g = torch.Generator().manual_seed(21)
    pred = torch.rand(H, W, generator=g) * 0.9 + 0.05
    tgt = (torch.rand(H, W, generator=g) > 0.6).float() * (3.0 if term == "obj" else 1.0)      # gt_semantic holds object ids: (> 0) is the target
    w = make_weight(kind, H, W, seed=1)
    params = loss.OBJ_BCE if term == "obj" else loss.SKY_BCE
    want, want_g = ref.value_and_grad(lambda p: ref.bce_clip(p, tgt, *params, weight=w), pred)
    p = pred.cuda().requires_grad_(True)
    val = loss.obj_loss(p[None], tgt.cuda(), weight=w.cuda()) if term == "obj" else loss.sky_loss(p, tgt.cuda(), weight=w.cuda()[None])
    (2.5 * val).backward()
    print("%s %s: %.9g (ref %.9g)" % (term, kind, float(val), want))
    np.testing.assert_allclose(float(val), want, rtol=1e-5)
    np.testing.assert_allclose(p.grad.cpu().numpy() / 2.5, want_g.numpy(), rtol=1e-4, atol=1e-8)
    assert not p.grad[w.cuda() == 0].any()
    direct = loss.bce_clip_loss(pred.cuda(), tgt.cuda(), *params, weight=w.cuda())
    assert torch.equal(direct, val.detach())
    if kind == "ones":                                         # the kernel without a weight, against the same reference
        np.testing.assert_allclose(float(loss.bce_clip_loss(pred.cuda(), tgt.cuda(), *params)), want, rtol=1e-5)


@pytest.mark.parametrize("H,W,D_S", [(17, 33, 1), (37, 121, 2)])
def test_image_losses_node_with_a_weight_equals_the_six_functions(H, W, D_S):
    """The comparison of tests/test_gpu_loss.py::test_image_losses_node_equals_the_six_functions with weight= on both sides: the same kernels,
    so the same values bit for bit; the gradient of every input equal (img_opacity receives the flow term and the weighted sky term).
    And without a weight the node is what it was."""
    from adgs import loss
    g = torch.Generator().manual_seed(H * 1000 + W)
    dev = "cuda"
    r = lambda *s: torch.rand(*s, generator=g)
    gt_img, gt_depth, gt_sem, gt_sky = r(3, H, W).to(dev), (r(H, W) * 0.5 + 0.01).to(dev), (r(H, W) > 0.8).float().to(dev), (r(H, W) > 0.7).float().to(dev)
    K = torch.tensor([[90.0, 0.0, W / 2.0], [0.0, 90.0, H / 2.0], [0.0, 0.0, 1.0]])
    R, T = torch.eye(3), torch.tensor([0.05, -0.02, 0.1])
    flow_pkg = (0.4, K, R, T, torch.stack([r(H, W) * (W - 1), r(H, W) * (H - 1)]).to(dev), (r(H, W) > 0.3).float().to(dev))
    base = dict(image=r(3, H, W), depth=r(H, W) * 0.4 + 0.05, img_flow=torch.cat([r(2, H, W) * 4 - 2, r(1, H, W) * 5 + 1]), img_opacity=r(H, W) * 0.98 + 0.01,
                img_semantic=r(D_S, H, W))
    mix = torch.tensor([0.8, 0.2, 0.1, 0.1, 0.1, 0.05], device=dev)
    weight = make_weight("fractional", H, W, seed=2)
    weight[H // 2:] = 0
    weight = weight.to(dev)

    def run(fused, w):
        kw = {} if w is None else {"weight": w}
        x = {k: v.clone().to(dev).requires_grad_(True) for k, v in base.items()}
        if fused:
            terms = loss.image_losses(x["image"], gt_img, x["depth"], gt_depth, x["img_flow"], flow_pkg, x["img_opacity"], x["img_semantic"], gt_sem, gt_sky, dist=0.02, **kw)
        else:
            l1, s = loss.l1_ssim(x["image"], gt_img, **kw)
            terms = (l1, s, loss.get_depth_loss(x["depth"], gt_depth, mask=w), loss.get_flow_loss(x["img_flow"], flow_pkg, x["img_opacity"], dist=0.02),
                     loss.obj_loss(x["img_semantic"], gt_sem, **kw), loss.sky_loss(x["img_opacity"], gt_sky, **kw))
        total = (torch.stack([t.reshape(()) for t in terms]) * mix).sum()
        total.backward()
        return [t.detach().clone() for t in terms], {k: v.grad.detach().clone() for k, v in x.items()}

    for w in (weight, None):
        ta, ga = run(False, w)
        tb, gb = run(True, w)
        assert len(tb) == 6
        for a, b in zip(ta, tb):
            assert torch.equal(a, b), (a, b)
        for k in ga:
            assert gb[k].shape == ga[k].shape, k
            assert torch.allclose(gb[k], ga[k], rtol=1e-6, atol=1e-9 + 1e-6 * float(ga[k].abs().max())), k
    # the weight did something: every weighted term differs from its unweighted value, the flow term (selected by flow_vis) does not
    tw, tn = run(True, weight)[0], run(True, None)[0]
    assert all(not torch.equal(tw[i], tn[i]) for i in (0, 1, 2, 4, 5)) and torch.equal(tw[3], tn[3])


def lidar_case(H, W, valid_fraction=0.02, seed=0):
    g = torch.Generator().manual_seed(300 + seed + H)
    depth = torch.rand(H, W, generator=g) * 60 + 1
    lidar = (depth + torch.randn(H, W, generator=g)).clamp_min(0.5)
    mask = torch.rand(H, W, generator=g) < valid_fraction
    mask[0, 0] = True                                                   # at least one valid pixel
    mask[H - 1, W - 1] = True
    lidar[H - 1, W - 1] = 0                                             # masked, but no return: not valid, and 1 / 0 must not appear
    return depth, lidar, mask


@pytest.mark.parametrize("mask_dtype", ["bool", "float"])
@pytest.mark.parametrize("inv_depth", [False, True])
@pytest.mark.parametrize("H,W", [(3, 5), (37, 121), (130, 127)])
def test_lidar_depth_loss(H, W, inv_depth, mask_dtype):
    """130 x 127: 65 workgroups, more waves than slot rows"""
    from adgs import loss
    depth, lidar, mask = lidar_case(H, W)
    if inv_depth:
        depth = 1 / depth                                               # what the rasterizer renders under pipe.inv_depth
    m = mask if mask_dtype == "bool" else mask.float() * 0.5            # a fractional confidence is a weight
    want, want_g = ref.value_and_grad(lambda d: ref.lidar_depth(d, lidar, m, inv_depth), depth)
    d = depth.cuda().requires_grad_(True)
    val = loss.lidar_depth_loss(d, lidar.cuda(), m.cuda(), inv_depth=inv_depth)
    (1.7 * val).backward()
    print("lidar %dx%d inv=%s: %.9g (ref %.9g), %d valid" % (H, W, inv_depth, float(val), want, int((mask & (lidar > 0)).sum())))
    assert bool(torch.isfinite(val)) and bool(torch.isfinite(d.grad).all())
    np.testing.assert_allclose(float(val), want, rtol=1e-5)
    assert_grad(d.grad / 1.7, want_g, "lidar")
    assert not d.grad[~(mask & (lidar > 0)).cuda()].any()


def test_lidar_depth_loss_with_nothing_valid():
    from adgs import loss
    depth, lidar, mask = lidar_case(37, 121)
    for l, m in ((lidar, torch.zeros_like(mask)), (torch.zeros_like(lidar), mask), (lidar * (~mask), mask)):
        d = depth.cuda().requires_grad_(True)
        val = loss.lidar_depth_loss(d, l.cuda(), m.cuda(), inv_depth=True)
        val.backward()
        assert float(val) == 0.0 and bool(torch.isfinite(d.grad).all()) and not d.grad.any()
