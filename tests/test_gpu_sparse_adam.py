"""The visibility-masked ("sparse") fused Adam: FusedAdam.step(visibility=...) / adgs_adam_step_rows (include/adgs_optim.h).

The contract is bitwise, so every comparison here is torch.equal on the parameter and both moments:
  * a visible row takes exactly the update of the dense kernel -- with every row visible the masked step IS the dense step;
  * in general the result is "dense step on a copy, then torch.where(row_visible, stepped, old)" for p, exp_avg, exp_avg_sq;
  * an invisible row keeps its bits whatever its gradient holds, and is still zero-filled when a fill is asked for.
One independent anchor besides that composition: the visible rows of a first step against torch.optim.Adam on the CPU in float64,
with the bound of tests/test_gpu_optim.py::test_fused_adam_matches_torch_adam (max(3e-6, 4 * the float32 CPU error))."""
import os
import types

import numpy as np
import pytest
import torch

from tests.test_gpu_optim import _groups

pytestmark = pytest.mark.gpu

EXTRA_SHAPES = [((4099, 15, 3), 1.25e-4), ((700, 3, 18), 1.6e-4), ((257, 2), 1e-3), ((1, 3, 6), 1e-3), ((0, 3), 1e-2)]
SEED_BASE = int(os.environ.get("ADGS_TEST_SEED_BASE", "0"))
SEEDS = range(SEED_BASE, SEED_BASE + int(os.environ.get("ADGS_TEST_SPARSE_ADAM_SEEDS", "8")))
DENSITIES = [0.0, 0.03, 0.5, 0.97, 1.0]


def _shapes_and_lrs():
    base = [(tuple(g["params"][0].shape), g["lr"]) for g in _groups(0, torch.float32, "cpu")]
    return base + EXTRA_SHAPES


def _leaf(values, dev, misaligned):
    """A leaf parameter on the device; misaligned: a view one float into its buffer (4-byte but not 16-byte aligned: the kernel's
    scalar path)."""
    if not misaligned:
        return values.to(dev).clone().requires_grad_(True)
    buf = torch.zeros(values.numel() + 4, device=dev)
    v = buf[1:1 + values.numel()].view(values.shape)
    v.copy_(values.to(dev))
    p = v.detach().requires_grad_(True)
    assert p.data_ptr() % 16 == 4 or p.numel() == 0
    return p


def _grad_like(p, values):
    """A gradient with the alignment of its parameter (the kernel takes the vector path only if all four pointers are aligned)."""
    if p.numel() and p.data_ptr() % 16:
        buf = torch.zeros(p.numel() + 4, device=p.device)
        g = buf[1:1 + p.numel()].view(p.shape)
        g.copy_(values.to(p.device))
        return g
    return values.to(p.device).clone()


def _build(seed, dev, misaligned=False, marks=None, **kw):
    """Two optimizers over bit-identical parameters.  marks: per group "head" / "tail" / None for the first optimizer."""
    from adgs.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    spec = _shapes_and_lrs()
    values = [torch.randn(*s, generator=g) for s, _ in spec]
    opts = []
    for which in range(2):
        ps = [_leaf(v, dev, misaligned) for v in values]
        opts.append(FusedAdam([{"params": [p], "lr": lr, "name": "g%d" % i} for i, (p, (_, lr)) in enumerate(zip(ps, spec))], lr=0.0, eps=1e-15, **kw))
    if marks is None:
        marks = ["head" if i % 2 == 0 else "tail" for i in range(len(spec))]
    for grp, m in zip(opts[0].param_groups, marks):
        grp["visibility_rows"] = m
    return opts[0], opts[1], marks


def _n_gaussians(opt, slack=13):
    return max(int(grp["params"][0].shape[0]) for grp in opt.param_groups) + slack


def _row_mask(vis, where, R):
    on = vis > 0 if vis.dtype == torch.int32 else vis != 0
    return on[:R] if where == "head" else on[on.numel() - R:]


def _pmv(opt, p):
    st = opt.state.get(p, {})
    return (p.detach(), st.get("exp_avg", torch.zeros_like(p)), st.get("exp_avg_sq", torch.zeros_like(p)))


def _snapshot(opt):
    return [tuple(t.clone() for t in _pmv(opt, grp["params"][0])) + (float(opt.state.get(grp["params"][0], {}).get("step", 0.0)),)
            for grp in opt.param_groups]


def _composed_reference_step(ref, marks, vis, **kw):
    """Contract item 1: the dense step on `ref`, then row by row the stepped or the old bits."""
    old = _snapshot(ref)
    had_grad = [grp["params"][0].grad is not None for grp in ref.param_groups]
    ref.step(**kw)
    for grp, where, (p0, m0, v0, _), had in zip(ref.param_groups, marks, old, had_grad):
        p = grp["params"][0]
        if where is None or not had or p.numel() == 0:
            continue
        on = _row_mask(vis, where, p.shape[0]).view([-1] + [1] * (p.dim() - 1))
        st = ref.state[p]
        with torch.no_grad():
            p.copy_(torch.where(on, p.detach(), p0))
            st["exp_avg"].copy_(torch.where(on, st["exp_avg"], m0))
            st["exp_avg_sq"].copy_(torch.where(on, st["exp_avg_sq"], v0))


def _assert_same(a, b, what):
    for ga, gb in zip(a.param_groups, b.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert (pa in a.state) == (pb in b.state), (what, ga["name"])
        for x, y, k in zip(_pmv(a, pa), _pmv(b, pb), ("p", "exp_avg", "exp_avg_sq")):
            assert x.shape == y.shape and torch.equal(x, y), (what, ga["name"], tuple(pa.shape), k, int((x != y).sum()))
        if pa in a.state:
            assert float(a.state[pa]["step"]) == float(b.state[pb]["step"]), (what, ga["name"])


def _set_grads(a, b, gen, it, skip_group=3, poison=None, vis=None, marks=None):
    for gi, (ga, gb) in enumerate(zip(a.param_groups, b.param_groups)):
        pa, pb = ga["params"][0], gb["params"][0]
        if gi == skip_group and it % 2 == 1:
            pa.grad = pb.grad = None
            continue
        g = torch.randn(*pa.shape, generator=gen) * (10.0 ** (gi % 4 - 2))
        if poison is not None and marks[gi] is not None and pa.numel():
            off = ~_row_mask(vis.cpu(), marks[gi], pa.shape[0])
            bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38])[torch.arange(pa.shape[0]) % 4]
            g = torch.where(off.view([-1] + [1] * (pa.dim() - 1)), bad.view([-1] + [1] * (pa.dim() - 1)).expand_as(g), g)
        pa.grad, pb.grad = _grad_like(pa, g), _grad_like(pb, g)


@pytest.mark.parametrize("misaligned", [False, True])
def test_all_rows_visible_is_the_dense_step_bit_for_bit(misaligned):
    dev = torch.device("cuda", 0)
    a, b, marks = _build(1, dev, misaligned)
    N = _n_gaussians(a, slack=0)
    gen = torch.Generator().manual_seed(99)
    for it in range(5):
        _set_grads(a, b, gen, it)
        a.param_groups[4]["lr"] = b.param_groups[4]["lr"] = 5e-3 * (0.9 ** it)
        vis = torch.full((N,), 1 + it, dtype=torch.int32, device=dev)
        a.step(visibility=vis)
        b.step()
        _assert_same(a, b, ("all visible", it))


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_masks_equal_dense_step_then_where(seed, density):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7000 + seed)
    n_spec = len(_shapes_and_lrs())
    marks = [None if i == 5 else ("head", "tail")[int(rng.integers(0, 2))] for i in range(n_spec)]     # one group dense in the same launch
    a, ref, marks = _build(100 + seed, dev, misaligned=bool(seed % 2), marks=marks)
    N = _n_gaussians(a)
    gen = torch.Generator().manual_seed(500 + seed)
    for it in range(6):
        vis_cpu = (torch.rand(N, generator=gen) < density).to(torch.int32) * torch.randint(1, 200, (N,), generator=gen, dtype=torch.int32)
        vis = vis_cpu.to(dev)
        for ga, gb in zip(a.param_groups, ref.param_groups):
            ga["lr"] = gb["lr"] = float(rng.choice([0.0, 1e-4, 1e-2, 0.3]))
        _set_grads(a, ref, gen, it)
        if it == 0:
            start = [(grp["params"][0].detach().cpu(), None if grp["params"][0].grad is None else grp["params"][0].grad.cpu(), grp["lr"]) for grp in a.param_groups]
        a.step(visibility=vis)
        _composed_reference_step(ref, marks, vis)
        _assert_same(a, ref, ("seed %d density %g" % (seed, density), it))
        if it == 0:
            _float64_anchor(a, start, marks, vis_cpu)


def _float64_anchor(a, start, marks, vis_cpu):
    """Visible rows of the first step against torch.optim.Adam on the CPU in float64; bound of test_fused_adam_matches_torch_adam."""
    for grp, (p0, g0, lr), where in zip(a.param_groups, start, marks):
        if g0 is None or p0.numel() == 0:
            continue
        on = torch.ones(p0.shape[0], dtype=torch.bool) if where is None else _row_mask(vis_cpu, where, p0.shape[0])
        if not bool(on.any()):
            continue
        res = {}
        for dt in (torch.float64, torch.float32):
            q = p0.to(dt).clone().requires_grad_(True)
            o = torch.optim.Adam([{"params": [q], "lr": lr}], lr=0.0, eps=1e-15)
            q.grad = g0.to(dt)
            o.step()
            res[dt] = q.detach().double().numpy()[on.numpy()]
        x = grp["params"][0].detach().cpu().double().numpy()[on.numpy()]
        scale = max(np.abs(res[torch.float64]).max(), 1e-30)
        err, err32 = np.abs(x - res[torch.float64]).max() / scale, np.abs(res[torch.float32] - res[torch.float64]).max() / scale
        assert err <= max(3e-6, 4 * err32), (grp["name"], err, err32)


@pytest.mark.parametrize("density", [0.0, 0.5, 0.97])
def test_invisible_rows_ignore_their_gradient_whatever_it_holds(density):
    """NaN / Inf / huge gradients on the invisible rows: their p, m, v keep their bits; the visible rows are finite and as composed."""
    dev = torch.device("cuda", 0)
    a, ref, marks = _build(11, dev)
    N = _n_gaussians(a)
    gen = torch.Generator().manual_seed(77)
    for it in range(3):
        vis = ((torch.rand(N, generator=gen) < density).to(torch.int32) * 5).to(dev)
        before = _snapshot(a)
        _set_grads(a, ref, gen, it, poison=True, vis=vis, marks=marks)
        a.step(visibility=vis)
        _composed_reference_step(ref, marks, vis)
        _assert_same(a, ref, ("poisoned", it))
        for grp, where, (p0, m0, v0, _) in zip(a.param_groups, marks, before):
            p = grp["params"][0]
            if p.numel() == 0 or p.grad is None:
                continue
            off = ~_row_mask(vis, where, p.shape[0])
            for x, x0 in zip(_pmv(a, p), (p0, m0, v0)):
                assert torch.equal(x[off], x0[off]), (it, grp["name"])
                assert bool(torch.isfinite(x).all()), (it, grp["name"])
            if bool(off.any()):
                assert not bool(torch.isfinite(p.grad[off]).all())           # the poison was really there


def test_zero_grad_modes_cover_invisible_rows():
    dev = torch.device("cuda", 0)
    for mode in (False, True, "zeros"):
        a, ref, marks = _build(21, dev, misaligned=(mode == "zeros"))
        N = _n_gaussians(a)
        gen = torch.Generator().manual_seed(5)
        vis = ((torch.rand(N, generator=gen) < 0.4).to(torch.int32)).to(dev)
        vis[:300] = 0                                                        # whole tiles without a visible row as well
        _set_grads(a, ref, gen, 0)
        grads = [None if grp["params"][0].grad is None else grp["params"][0].grad for grp in a.param_groups]
        kept = [None if g is None else g.clone() for g in grads]
        a.step(zero_grad=mode, visibility=vis)
        _composed_reference_step(ref, marks, vis, zero_grad=mode)
        _assert_same(a, ref, ("zero_grad", mode))
        for grp, g, g0 in zip(a.param_groups, grads, kept):
            p = grp["params"][0]
            if p.numel() == 0:
                continue                                                     # an empty tensor is not part of any launch, dense or masked
            if mode is True:
                assert p.grad is None
            elif mode is False:
                assert p.grad is g and torch.equal(g, g0)
            else:
                assert p.grad is g and (g.numel() == 0 or float(g.abs().max()) == 0.0), grp["name"]


def test_int32_bool_and_uint8_visibilities_give_the_same_bits():
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(8)
    results = []
    pattern = None
    for kind in ("int32", "bool", "uint8"):
        a, _, marks = _build(31, dev)
        N = _n_gaussians(a)
        if pattern is None:
            pattern = torch.randint(-3, 4, (N,), generator=gen, dtype=torch.int32)          # zeros and negative radii: not visible
            assert bool((pattern < 0).any()) and bool((pattern == 0).any()) and bool((pattern > 0).any())
        on = pattern > 0
        vis = {"int32": pattern, "bool": on, "uint8": on.to(torch.uint8) * 200}[kind].to(dev)
        g2 = torch.Generator().manual_seed(9)
        for it in range(2):
            _set_grads(a, a, g2, it)
            a.step(visibility=vis)
        results.append(a)
    _assert_same(results[0], results[1], "int32 vs bool")
    _assert_same(results[0], results[2], "int32 vs uint8")


def _camera(W, H, focal, time):
    from adgs import synthetic
    return synthetic.camera_object(synthetic.make_camera(W, H, focal), time=time)


def test_head_and_tail_groups_on_the_model_through_a_densification():
    """training_setup(sparse_adam=True): scene groups read the head of the radii, object groups the tail; deform_xyz / time_sigma stay
    dense; the marks and the offsets survive densify_and_prune (new tensors, new Ns and No)."""
    from adgs import synthetic
    from adgs.model import SyntheticGaussianModel
    from adgs.optim import FusedAdam
    from gaussian_renderer import render
    dev = torch.device("cuda", 0)
    sc = synthetic.make_scene(5000, 208, 130, 150.0, sh_degree=3, seed=4, n_objects=2)
    model = SyntheticGaussianModel.from_scene(sc, dev, seed=2)
    model.raw_sh = True
    opt = model.training_setup(percent_dense=0.01, scene_extent=20.0, object_extent=4.0, near_num=8, sparse_adam=True)
    marks = {g["name"]: g.get("visibility_rows") for g in opt.param_groups}
    assert marks["scene_xyz"] == marks["scene_shs_rest"] == marks["deform_shs_scene"] == "head"
    assert marks["obj_xyz"] == marks["obj_shs_rest"] == marks["deform_shs_obj"] == marks["deform_rotation"] == "tail"
    assert marks["deform_xyz"] is None and marks["time_sigma"] is None and marks["deform_background"] is None
    cam = _camera(120, 130, 150.0, 0.4)                    # narrower than the scene was laid out for: part of it is outside the frustum
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)

    def iteration():
        pkg = render(cam, model, None, pipe, flow_pkg=(0.45,) + (None,) * 5, render_objmask=True)
        radii = pkg["radii"]
        N, Ns = model.get_pts_num, model.get_scene_pts_num
        n_vis = int((radii > 0).sum())
        assert radii.numel() == N and 0 < n_vis < N, (n_vis, N)
        assert 0 < int((radii[:Ns] > 0).sum()) < Ns and 0 < int((radii[Ns:] > 0).sum()) < N - Ns
        # regularisers that reach every row of the dense groups and of a masked one (whose invisible rows must ignore it)
        loss = pkg["render"].mean() + pkg["depth"].mean() * 0.1 + (model.xyz_deform_param ** 2).sum() * 1e-3 + (model.gs_time_sigma ** 2).sum() * 1e-3 \
            + (model._scene_scaling ** 2).sum() * 1e-4 + (model._obj_opacity ** 2).sum() * 1e-4
        loss.backward()
        model.add_densification_stats(pkg)
        before, dense_ref = {}, {}
        for g in opt.param_groups:
            p = g["params"][0]
            st = opt.state.get(p, {})
            before[g["name"]] = tuple(t.clone() for t in (p.detach(), st.get("exp_avg", torch.zeros_like(p)), st.get("exp_avg_sq", torch.zeros_like(p))))
            if g["name"] in ("deform_xyz", "time_sigma") and p.grad is not None:
                q = torch.nn.Parameter(p.detach().clone())
                o = FusedAdam([{"params": [q], "lr": g["lr"]}], lr=0.0, eps=1e-15)
                o.state[q] = {"step": torch.tensor(float(st.get("step", 0.0))), "exp_avg": before[g["name"]][1].clone(), "exp_avg_sq": before[g["name"]][2].clone()}
                q.grad = p.grad.clone()
                o.step()
                dense_ref[g["name"]] = (q.detach(), o.state[q]["exp_avg"], o.state[q]["exp_avg_sq"])
        had_grad = {g["name"]: g["params"][0].grad is not None for g in opt.param_groups}
        opt.step(zero_grad=True, visibility=radii)
        assert set(dense_ref) == {"deform_xyz", "time_sigma"}
        moved = 0
        for g in opt.param_groups:
            name, p = g["name"], g["params"][0]
            assert p.grad is None
            now = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) if p in opt.state else before[name]
            if name in dense_ref:
                for x, y in zip(now, dense_ref[name]):
                    assert torch.equal(x, y), name
            elif g.get("visibility_rows") is not None and had_grad[name]:
                R = p.shape[0]
                rows = radii[:R] if g["visibility_rows"] == "head" else radii[N - R:]
                assert R == (Ns if g["visibility_rows"] == "head" else N - Ns), name
                off = rows <= 0
                for x, x0 in zip(now, before[name]):
                    assert torch.equal(x[off], x0[off]), name
                moved += int((now[1][~off] != before[name][1][~off]).sum())
        assert moved > 0
        # the regularised masked groups: a dense step would have moved their invisible rows
        assert bool((model._scene_scaling.detach()[radii[:Ns] <= 0] == before["scene_scaling"][0][radii[:Ns] <= 0]).all())

    iteration()
    n0 = model.get_pts_num
    thr = float((model.xyz_gradient_accum / model.denom.clamp_min(1)).quantile(0.9))
    torch.manual_seed(0)
    model.densify_and_prune(thr, thr, 0.005, True)
    assert model.get_pts_num != n0
    assert {g["name"]: g.get("visibility_rows") for g in opt.param_groups} == marks
    iteration()


def test_refusals_leave_everything_as_it_was():
    from adgs.optim import FusedAdam
    dev = torch.device("cuda", 0)

    def fresh(**kw):
        p = torch.randn(100, 3, device=dev, requires_grad=True)
        q = torch.randn(40, 5, device=dev, requires_grad=True)
        o = FusedAdam([{"params": [p], "lr": 1e-2, "name": "p", "visibility_rows": "head"}, {"params": [q], "lr": 1e-2, "name": "q", "visibility_rows": "tail"}],
                      lr=0.0, eps=1e-15, **kw)
        p.grad, q.grad = torch.randn_like(p), torch.randn_like(q)
        o.step()
        p.grad, q.grad = torch.randn_like(p), torch.randn_like(q)
        return o

    good = torch.ones(140, dtype=torch.int32, device=dev)
    bad = {
        "too short for a group": torch.ones(99, dtype=torch.int32, device=dev),
        "not the head rows + the tail rows (stale radii)": torch.ones(150, dtype=torch.int32, device=dev),
        "cpu": torch.ones(140, dtype=torch.int32),
        "float": torch.ones(140, device=dev),
        "2-D": torch.ones(140, 1, dtype=torch.int32, device=dev),
        "non-contiguous": torch.ones(280, dtype=torch.int32, device=dev)[::2],
    }
    for what, vis in bad.items():
        o = fresh()
        snap = _snapshot(o)
        with pytest.raises(ValueError):
            o.step(visibility=vis)
        for s0, s1 in zip(snap, _snapshot(o)):
            assert all(torch.equal(x, y) for x, y in zip(s0[:3], s1[:3])) and s0[3] == s1[3], what
    o = fresh()
    o.param_groups[0]["visibility_rows"] = "middle"
    with pytest.raises(ValueError):
        o.step(visibility=good)
    # the dormant-tile map and the row visibility
    o = fresh(skip_dormant_tiles=True)
    snap = _snapshot(o)
    with pytest.raises(ValueError, match="skip_dormant_tiles"):
        o.step(visibility=good)
    for s0, s1 in zip(snap, _snapshot(o)):
        assert all(torch.equal(x, y) for x, y in zip(s0[:3], s1[:3])) and s0[3] == s1[3]
    o.step()                                                   # without a visibility it is the optimizer it was
    # the C entry refuses the same combination, and the shapes that do not add up (before any launch)
    import ctypes
    from adgs import _lib
    from adgs.optim import AdamGroup, AdamRows
    p = torch.zeros(12, device=dev); g = torch.ones(12, device=dev); m = torch.zeros(12, device=dev); v = torch.zeros(12, device=dev)
    tiles = torch.ones(1, dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    for grp, rows in ((AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 12, 1e-2, 1, tiles.data_ptr(), 0, 0), AdamRows(good.data_ptr(), 4, 3, 1)),
                      (AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 12, 1e-2, 1, None, 0, 0), AdamRows(good.data_ptr(), 5, 3, 1)),
                      (AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 12, 1e-2, 1, None, 0, 0), AdamRows(good.data_ptr(), 12, 0, 1)),
                      (AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 12, 1e-2, 1, None, 0, 0), AdamRows(good.data_ptr(), 4, 3, 7))):
        code = lib.adgs_adam_step_rows(ctypes.byref(grp), ctypes.byref(rows), 1, 0.9, 0.999, 1e-15, 0, _lib.stream_ptr(dev))
        assert code < 0 and _lib.last_error()
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(m.abs().max()) == 0.0


def test_in_backward_claim_and_visibility_are_refused():
    from tests.test_gpu_optim import _render_model
    from gaussian_renderer import render
    dev = torch.device("cuda", 0)
    m, cams = _render_model(900, 1, 8, dev, True)
    from adgs.optim import mark_visibility_groups
    mark_visibility_groups(m.optimizer)
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    m.optimizer.arm_backward()
    pkg = render(cams[0], m, None, pipe)
    pkg["render"].sum().backward()
    assert m.optimizer.backward_epilogue.claimed
    snap = _snapshot(m.optimizer)
    with pytest.raises(RuntimeError, match="cannot be mixed"):
        m.optimizer.step(zero_grad=True, visibility=pkg["radii"])
    for s0, s1 in zip(snap, _snapshot(m.optimizer)):
        assert all(torch.equal(x, y) for x, y in zip(s0[:3], s1[:3])) and s0[3] == s1[3]
    m.optimizer.step(zero_grad=True)                           # the dense step finishes the iteration
    # an unarmed iteration of the same optimizer may be masked
    pkg = render(cams[1], m, None, pipe)
    pkg["render"].sum().backward()
    m.optimizer.step(zero_grad=True, visibility=pkg["radii"])


def test_merge_visibility_is_the_elementwise_maximum():
    from adgs.optim import merge_visibility
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(2)
    rs = [torch.randint(-2, 50, (1000,), generator=gen, dtype=torch.int32).to(dev) for _ in range(3)]
    keep = [r.clone() for r in rs]
    acc = None
    for r in rs:
        acc = merge_visibility(acc, r)
    assert torch.equal(acc, torch.maximum(torch.maximum(rs[0], rs[1]), rs[2]))
    assert all(torch.equal(a, b) for a, b in zip(rs, keep))                  # the cameras' own radii are left alone
    bs = [r > 0 for r in rs]
    assert torch.equal(merge_visibility(merge_visibility(None, bs[0]), bs[1]), bs[0] | bs[1])


def test_masked_step_captured_in_a_graph_replays_to_the_eager_bits():
    dev = torch.device("cuda", 0)
    a, b, marks = _build(41, dev)
    N = _n_gaussians(a)
    gen = torch.Generator().manual_seed(3)
    vis = ((torch.rand(N, generator=gen) < 0.5).to(torch.int32) * 7).to(dev)
    _set_grads(a, b, gen, 0)
    for grp, where in zip(b.param_groups, marks):
        grp["visibility_rows"] = where
        b._init_state(grp["params"][0])                        # the moments exist before the capture
    a.step(visibility=vis)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.step(visibility=vis)                                 # host code runs once (step counters -> 1), the launch is recorded
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(a, b, "graph replay")


def test_closure_and_visibility_mask_the_gradients_the_closure_produces():
    """step(closure, visibility=...): the gradients appear inside the closure (every .grad is None on entry, as after zero_grad=True);
    the masked groups must be masked all the same, and the checks against the visibility still come before anything is stepped."""
    dev = torch.device("cuda", 0)
    a, ref, marks = _build(51, dev)
    N = _n_gaussians(a)
    gen = torch.Generator().manual_seed(12)
    for it in range(3):
        vis = ((torch.rand(N, generator=gen) < 0.5).to(torch.int32) * 3).to(dev)
        grads = [torch.randn(*grp["params"][0].shape, generator=gen).to(dev) for grp in a.param_groups]
        for grp in list(a.param_groups) + list(ref.param_groups):
            grp["params"][0].grad = None

        def closure():
            for grp, g in zip(a.param_groups, grads):
                grp["params"][0].grad = g.clone()
            return torch.tensor(float(it))
        assert float(a.step(closure, zero_grad=True, visibility=vis)) == float(it)
        for grp, g in zip(ref.param_groups, grads):
            grp["params"][0].grad = g.clone()
        _composed_reference_step(ref, marks, vis, zero_grad=True)
        _assert_same(a, ref, ("closure", it))
    # a visibility that does not fit the gradients the closure produced: refused, nothing stepped
    snap = _snapshot(a)
    with pytest.raises(ValueError):
        a.step(closure, visibility=torch.ones(5, dtype=torch.int32, device=dev))
    for s0, s1 in zip(snap, _snapshot(a)):
        assert all(torch.equal(x, y) for x, y in zip(s0[:3], s1[:3])) and s0[3] == s1[3]
