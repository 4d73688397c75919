"""The normal-map prior on the GPU (adgs.normals over include/adgs_normals.h, csrc/normals.hip) against tests/normals_ref.py (float64
torch-CPU, autograd), and pipe.render_normals of gaussian_renderer.render().

Gaussian normals: N in {0, 1, 63, 64, 65, 257, 1000} (one thread per Gaussian, 256-thread blocks: a partial wave, a full wave, one past it,
one past a block, four blocks) x (stride, c0, mask) in {(3, 0, no), (4, 1, yes), (7, 2, no), (32, 29, yes)} through the C ABI, the two
layouts of the Python surface through autograd as well.  The inputs keep the float64 reference's decisions away from their switches (the
smallest scale at most 0.8 x the next except in exact-tie rows; |n_c . p_c| >= 1e-3 |p_c|, rows redrawn on the CPU until they do), so
every row is compared: values within 1e-5, dL/drotations within 1e-4 max|ref|.

Consistency loss: the shapes put the 32 x 16 tiles and their halos (1 forward, 2 backward) where they can go wrong -- no interior pixel,
one interior pixel, one tile exactly, one-pixel partial tiles, two-pixel partial tiles (the backward halo crosses), several partial tiles --
times both inv_depth settings, seven weight kinds, five opacity patterns and two depth fields; 161 x 1025 has 363 workgroups for 256 slot
rows.  L within rtol 1e-5, every gradient element within 1e-4 max|ref|, exactly zero where the reference's gradient is; a reference is
computed once per case and shared by both upstream gradients.

The float32 torch restatement of the reference on the 161 x 1025 inputs (tests/normals_cases.float32_errors) is off by up to 4.0e-5 in the
normals and 6.3e-5 max|ref| in the gradients at tanfov (2.0, 0.35), more than a quarter of the tolerance, and a wider field of view makes it
worse ((4.0, 0.7): 7.1e-5 / 7.2e-5; (8.0, 1.4): 1.1e-4 / 1.3e-4: the cross product cancels terms that grow with the ray's slope).  The
kernels therefore form z and everything behind it in double from the float inputs; the large case stays at (2.0, 0.35) and at 1e-4."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import normals_cases as cases
from tests import normals_ref as ref

pytestmark = pytest.mark.gpu

N_LIST = (0, 1, 63, 64, 65, 257, 1000)
LAYOUTS = ((3, 0, False), (4, 1, True), (7, 2, False), (32, 29, True))          # (stride, c0, mask)
SMALL = [(1, 1), (2, 5), (3, 3), (3, 40), (16, 32), (17, 33), (18, 66), (37, 121)]
UPSTREAM = (1.0, -1.3)


# ---------------------------------------------------------------------------------------------- Gaussian normals
def random_view(g):
    """The transposed 4x4 view matrix of a random rotation plus translation."""
    A = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    if torch.linalg.det(A) < 0:
        A[:, 0] = -A[:, 0]
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = A
    view[3, :3] = torch.tensor([0.4, -0.3, 6.0], dtype=torch.float64)
    return view.float()


@functools.lru_cache(maxsize=None)
def gaussian_inputs(N):
    g = torch.Generator().manual_seed(500 + N)
    view = random_view(g)
    q = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1) * (0.3 + 2.7 * torch.rand(N, 1, generator=g))
    scales = 0.5 + torch.rand(N, 3, generator=g)
    rows = torch.arange(N)
    k = rows % 3
    small = 0.8 * scales.min(dim=1).values * (0.3 + 0.7 * torch.rand(N, generator=g))
    scales[rows, k] = small                                        # every axis is the shortest in a third of the rows
    ties = rows[rows % 7 == 3]                                     # exact ties: all three equal, or the two smallest equal
    for n, i in enumerate(ties.tolist()):
        if n % 3 == 0:
            scales[i] = scales[i, 0]
        elif n % 3 == 1:
            scales[i, 0] = scales[i, 1] = 0.25
            scales[i, 2] = 0.75
        else:
            scales[i, 1] = scales[i, 2] = 0.25
            scales[i, 0] = 0.75
    means = torch.randn(N, 3, generator=g) * 3
    for _ in range(100):                                           # the flip must not hang on rounding
        n_c, p_c, _k = ref.gaussian_normals_parts(scales, q, means, view)
        close = (n_c * p_c).sum(-1).abs() < 1e-3 * p_c.norm(dim=-1)
        if not close.any():
            break
        means[close] = torch.randn(int(close.sum()), 3, generator=g) * 3
    else:
        raise AssertionError("could not draw means away from the flip")
    mask = (torch.rand(N, generator=g) > 0.5).float()
    return scales, q, means, view, mask


@functools.lru_cache(maxsize=None)
def gaussian_reference(N):
    scales, q, means, view, _ = gaussian_inputs(N)
    n_c, p_c, k = ref.gaussian_normals_parts(scales, q, means, view)
    if N >= 63:
        assert sorted(k.unique().tolist()) == [0, 1, 2]
        assert int(((scales[:, 0] == scales[:, 1]) & (scales[:, 1] == scales[:, 2])).sum()) >= 1
        flip = (n_c * p_c).sum(-1) > 0
        assert 0 < int(flip.sum()) < N
    ln = q.norm(dim=1)
    assert N == 0 or (float(ln.min()) >= 0.3 - 1e-6 and float(ln.max()) <= 3 + 1e-6)
    return ref.gaussian_normals(scales, q, means, view)


def gaussian_reference_grad(N, G):
    scales, q, means, view, _ = gaussian_inputs(N)
    qg = q.double().requires_grad_(True)
    (ref.gaussian_normals(scales, qg, means, view) * G.double()).sum().backward()
    return qg.grad


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "stride%d_c%d_%s" % (l[0], l[1], "mask" if l[2] else "nomask"))
@pytest.mark.parametrize("N", N_LIST)
def test_gaussian_normals_through_the_abi(N, layout):
    from adgs import _lib
    stride, c0, use_mask = layout
    scales, q, means, view, mask = gaussian_inputs(N)
    want = gaussian_reference(N)
    dev = torch.device("cuda", torch.cuda.current_device())
    s, r, p, v, m = (t.to(dev).contiguous() for t in (scales, q, means, view, mask))
    g = torch.Generator().manual_seed(900 + N + stride)
    before = torch.randn(max(N, 1), stride, generator=g)[:N].contiguous()
    out = before.to(dev)
    dummy = torch.zeros(4, device=dev)
    ptr = lambda t: t.data_ptr() or dummy.data_ptr()             # an empty tensor has no storage; a required pointer must not be NULL
    _lib.call("adgs_gaussian_normals_forward", dev, N, ptr(s), ptr(r), ptr(p), v.data_ptr(), ptr(m) if use_mask else None, stride, c0, ptr(out))
    got = out.cpu()
    assert got[:, c0:c0 + 3].shape[0] == N                         # every row is compared
    if N:
        err = (got[:, c0:c0 + 3].double() - want).abs().max()
        assert float(err) <= 1e-5, float(err)
    untouched = [c for c in range(stride) if not (c0 <= c < c0 + 3) and not (use_mask and c == 0)]
    if untouched:
        assert torch.equal(got[:, untouched].contiguous().view(torch.int32), before[:, untouched].contiguous().view(torch.int32))      # bit-unchanged
    if use_mask:
        assert torch.equal(got[:, 0], mask)
    G = torch.randn(max(N, 1), stride, generator=g)[:N].contiguous()
    want_g = gaussian_reference_grad(N, G[:, c0:c0 + 3])
    for up in UPSTREAM:
        g_rot = torch.full((N, 4), float("nan"), device=dev)
        gu = (G * up).to(dev)
        _lib.call("adgs_gaussian_normals_backward", dev, N, ptr(s), ptr(r), ptr(p), v.data_ptr(), ptr(gu), stride, c0, ptr(g_rot))
        got_g = g_rot.cpu().double()
        assert got_g.shape == (N, 4)
        if N:
            assert torch.isfinite(got_g).all()                     # every element was written
            scale = float(want_g.abs().max()) * abs(up)
            assert float((got_g - up * want_g).abs().max()) <= 1e-4 * scale, (float((got_g - up * want_g).abs().max()), scale)


@pytest.mark.parametrize("use_mask", (False, True))
@pytest.mark.parametrize("N", N_LIST)
def test_gaussian_normals_through_autograd(N, use_mask):
    from adgs import normals
    scales, q, means, view, mask = gaussian_inputs(N)
    want = gaussian_reference(N)
    c0 = 1 if use_mask else 0
    G = torch.randn(max(N, 1), c0 + 3, generator=torch.Generator().manual_seed(77 + N))[:N]
    want_g = gaussian_reference_grad(N, G[:, c0:])
    for up in UPSTREAM:
        leaves = [t.cuda().requires_grad_(True) for t in (scales, q, means)]
        out = normals.gaussian_normals(leaves[0], leaves[1], leaves[2], view.cuda(), mask=mask.cuda()[:, None] if use_mask else None)
        assert out.shape == (N, c0 + 3)
        (out * (G * up).cuda()).sum().backward()
        assert leaves[0].grad is None and leaves[2].grad is None  # the axis and the flip are piecewise constant
        got, got_g = out.detach().cpu(), leaves[1].grad.cpu().double()
        if use_mask:
            assert torch.equal(got[:, 0], mask)
        if N:
            assert float((got[:, c0:].double() - want).abs().max()) <= 1e-5
            assert float((got_g - up * want_g).abs().max()) <= 1e-4 * float(want_g.abs().max()) * abs(up)
        else:
            assert got_g.shape == (0, 4)


# ---------------------------------------------------------------------------------------------- depth normals and the consistency loss
def run_gpu(N, D, O, w, tan, inv, upstream=1.0, need=(True, True, True), batched=False):
    from adgs import normals
    n, d, o = N.cuda().requires_grad_(need[0]), (D[None] if batched else D).cuda().requires_grad_(need[1]), (O[None] if batched else O).cuda().requires_grad_(need[2])
    L = normals.normal_consistency_loss(n, d, o, tan, weight=None if w is None else w.cuda(), inv_depth=inv)
    if any(need):
        (L * upstream).backward()
    grads = [None if t.grad is None else t.grad.cpu().double().reshape(t.shape[-3:] if k == 0 else t.shape[-2:]).numpy() for k, t in enumerate((n, d, o))]
    return L.item(), grads


@functools.lru_cache(maxsize=None)
def reference(H, W, tan, dk, ok, wk, inv):
    N, D, O = cases.maps(H, W, dk, ok, inv)
    L, gN, gD, gO = ref.normal_consistency_with_grads(N, D, O, *tan, weight=cases.make_weight(wk, H, W), inv_depth=inv)
    return float(L), [g.numpy() for g in (gN, gD, gO)]


def check_case(H, W, tan, dk, ok, wk, inv, upstreams=UPSTREAM):
    N, D, O = cases.maps(H, W, dk, ok, inv)
    w = cases.make_weight(wk, H, W)
    rL, rg = reference(H, W, tan, dk, ok, wk, inv)
    what = dict(shape=(H, W), depth=dk, opacity=ok, weight=wk, inv_depth=inv)
    structurally_zero = ok == "below" or H < 3 or W < 3 or wk in ("zeros", "corner_pixel")
    if structurally_zero:
        assert rL == 0.0 and not any(g.any() for g in rg), what
    for up in upstreams:
        L, grads = run_gpu(N, D, O, w, tan, inv, up)
        assert abs(L - rL) <= 1e-5 * abs(rL), (what, L, rL)
        for name, g, r in zip(("normal", "depth", "opacity"), grads, rg):
            assert g.shape == r.shape and np.isfinite(g).all(), (what, name)
            np.testing.assert_allclose(g, up * r, rtol=0, atol=1e-4 * np.abs(r).max() * abs(up), err_msg=str((what, name, up)))
            assert not g[r == 0].any(), (what, name)              # exactly zero wherever no valid term reaches
        if structurally_zero:
            assert L == 0.0 and not any(g.any() for g in grads), what


def check_depth_to_normal(H, W, tan, dk, ok, inv):
    from adgs import normals
    _, D, O = cases.maps(H, W, dk, ok, inv)
    want, m = ref.depth_normals(D.double(), O.double(), *tan, inv_depth=inv)
    got = normals.depth_to_normal(D.cuda(), O.cuda()[None], *tan, inv_depth=inv).cpu()
    assert got.shape == (3, H, W)
    assert float((got.double() - want).abs().max()) <= 1e-4 if H * W else True
    assert not got[:, ~m].any()                                    # zero where invalid


@pytest.mark.parametrize("inv", (True, False), ids=("inv_depth", "depth"))
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_values_and_gradients(shape, inv):
    for dk, ok in itertools.product(cases.DEPTHS, cases.OPACITIES):
        check_depth_to_normal(*shape, cases.TAN, dk, ok, inv)
        for wk in cases.WEIGHTS:
            check_case(*shape, cases.TAN, dk, ok, wk, inv)


def test_more_workgroups_than_slot_rows():
    """161 x 1025: 11 x 33 = 363 workgroups of 32 x 16 pixels"""
    for dk, ok, wk, inv in cases.LARGE_CASES:
        check_case(*cases.LARGE, cases.LARGE_TAN, dk, ok, wk, inv, upstreams=(-1.3,))
        check_depth_to_normal(*cases.LARGE, cases.LARGE_TAN, dk, ok, inv)


def test_each_subset_of_requires_grad():
    H, W, inv = 18, 66, True
    N, D, O = cases.maps(H, W, "noisy", "mixed", inv)
    w = cases.make_weight("fractional", H, W)
    rL, rg = reference(H, W, cases.TAN, "noisy", "mixed", "fractional", inv)
    for need in itertools.product((False, True), repeat=3):
        L, grads = run_gpu(N, D, O, w, cases.TAN, inv, need=need, batched=need[0])
        assert abs(L - rL) <= 1e-5 * abs(rL), need
        for want, g, r in zip(need, grads, rg):
            assert (g is not None) == want, need
            if want:
                np.testing.assert_allclose(g, r, rtol=0, atol=1e-4 * np.abs(r).max(), err_msg=str(need))


def test_plane_on_the_device():
    """n . P = d rendered with a constant opacity: the depth normal is the plane's at every interior pixel and N = O n_d costs nothing;
    float32 inputs, within 5e-6 (tests/test_normals_ref.py holds the float64 evaluation of the same inputs to that bound)."""
    from adgs import normals
    from tests.test_normals_ref import plane_inputs
    H, W = 17, 33
    for inv in (True, False):
        for n, d in (((0.3, -0.2, 1.0), 7.0), ((-0.5, 0.4, 1.0), 12.0), ((0.0, 0.0, 1.0), 4.0)):
            D, O, facing = plane_inputs(H, W, n, d, inv_depth=inv)
            nd = normals.depth_to_normal(D.cuda(), O.cuda(), *cases.TAN, inv_depth=inv)
            err = float((nd.cpu().double()[:, 1:-1, 1:-1] - facing[:, None, None]).abs().max())
            print("plane %s inv_depth=%s: max |n_d - n| = %.2e" % (n, inv, err))
            assert err <= 5e-6
            border = torch.ones(H, W, dtype=torch.bool)
            border[1:-1, 1:-1] = False
            assert not nd.cpu()[:, border].any()
            L = normals.normal_consistency_loss(O.cuda()[None] * nd, D.cuda(), O.cuda(), cases.TAN, inv_depth=inv)
            assert abs(L.item()) <= 5e-6


# ---------------------------------------------------------------------------------------------- render()
RW, RH, FOCAL = 64, 48, 60.0
PATHS = [(False, False), (True, False), (True, True)]              # (raw_sh, raw_scene)
PARAMS = ("_scene_xyz", "_obj_xyz", "_scene_scaling", "_obj_scaling", "_scene_opacity", "_obj_opacity", "_scene_rotation", "_obj_rotation",
          "_scene_shs_dc", "_obj_shs_dc", "_scene_shs_rest", "_obj_shs_rest", "xyz_deform_param", "rotation_deform_param", "gs_time_sigma")
# what carries the rotations of this model: with the default orders a quaternion spline replaces _obj_rotation (its gradient is exactly zero)
ROTATION_PARAMS = ("_scene_rotation", "rotation_deform_param")


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
    sc = synthetic.make_scene(2000, RW, RH, FOCAL, sh_degree=3, seed=31, n_objects=2)
    cam = synthetic.camera_object(synthetic.make_camera(RW, RH, FOCAL, cam_seed=3), time=0.4)
    return sc, cam


def _model(raw_sh, raw_scene):
    from adgs.model import SyntheticGaussianModel
    m = SyntheticGaussianModel.from_scene(_scene()[0], device="cuda", seed=4)
    m.raw_sh, m.raw_scene = raw_sh, raw_scene
    return m


def torch_gaussian_normals(scales, rotations, means3D, view):
    """The float32 torch composition the kernel replaces: quaternion to matrix, gather of the shortest axis, view rotation, flip."""
    q = rotations / rotations.norm(dim=1, keepdim=True)
    R = ref.rotation_matrix(q)
    k = scales.detach().argmin(dim=1)
    n_w = R.gather(2, k[:, None, None].expand(-1, 3, 1)).squeeze(2)
    n_c = n_w @ view[:3, :3]
    p_c = means3D.detach() @ view[:3, :3] + view[3, :3]
    flip = (n_c.detach() * p_c).sum(-1, keepdim=True) > 0
    return torch.where(flip, -n_c, n_c)


def _hand_render(model, cam, pipe, objmask):
    """The rasterizer entry render() takes for this model, with the normals of the torch composition handed in as `semantic`."""
    import gaussian_renderer as gr
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = model._scene_xyz.device
    means2D = gr.screenspace_points(model.get_pts_num, dev)
    rast = GaussianRasterizer(raster_settings=gr._camera_settings(cam, model, pipe, 1.0, dev))
    pkg = model.get_deformed_pkg(cam.time, full_rows=True)
    normal = torch_gaussian_normals(pkg["scales"], pkg["rotation"], pkg["xyz"], rast.raster_settings.viewmatrix)
    semantic = torch.cat([model.obj_mask_float, normal], dim=1) if objmask else normal
    if torch.is_tensor(pkg["shs"]):
        out = rast(means3D=pkg["xyz"], means2D=means2D, opacities=pkg["opacity"], shs=pkg["shs"], colors_precomp=None, scales=pkg["scales"],
                   rotations=pkg["rotation"], flow_points=None, semantic=semantic)
    else:
        out = rast.forward_rawsh(pkg["xyz"], means2D, pkg["opacity"], pkg["shs"], pkg["scales"], pkg["rotation"], flow_points=None, semantic=semantic,
                                 factor_sink=None, bg_image=None)
    c0 = semantic.shape[1] - 3
    return dict(render=out[0], radii=out[1], depth=out[2].squeeze(0), img_opacity=out[3].squeeze(0), img_normal=out[5][c0:],
                img_semantic=out[5][:1] if objmask else None)


def _grads(model, img_normal, upstream):
    model.zero_grad()
    img_normal.backward(upstream)
    torch.cuda.synchronize()
    return {n: getattr(model, n).grad.clone() for n in PARAMS if getattr(model, n).grad is not None}


@pytest.mark.parametrize("objmask", (False, True), ids=("nomask", "objmask"))
@pytest.mark.parametrize("raw_sh,raw_scene", PATHS, ids=("plain", "raw_sh", "raw_scene"))
def test_render_normals(raw_sh, raw_scene, objmask):
    from gaussian_renderer import render
    sc, cam = _scene()
    m = _model(raw_sh, raw_scene)
    # the float64 reference's decisions are not within float32 rounding of a switch for any Gaussian of this scene
    with torch.no_grad():
        pkg = m.get_deformed_pkg(cam.time, full_rows=True)
    n_c, p_c, _ = ref.gaussian_normals_parts(pkg["scales"], pkg["rotation"], pkg["xyz"], cam.world_view_transform)
    assert float(((n_c * p_c).sum(-1).abs() / p_c.norm(dim=-1)).min()) > 1e-5
    s2 = pkg["scales"].cpu().sort(dim=1).values
    assert float((s2[:, 1] / s2[:, 0]).min()) > 1 + 1e-5
    on, off = _pipe(render_normals=True), _pipe()
    got = render(cam, m, None, on, render_objmask=objmask)
    plain = render(cam, m, None, off, render_objmask=objmask)
    assert "img_normal" not in plain and tuple(got["img_normal"].shape) == (3, RH, RW)
    assert int((got["radii"] > 0).sum()) > 300
    identical = True
    assert torch.equal(got["radii"], plain["radii"])
    for k in ("render", "depth", "img_opacity", "img_flow", "img_semantic"):
        if plain[k] is None:
            assert got[k] is None, k
            continue
        assert got[k].shape == plain[k].shape, k
        assert float((got[k].detach() - plain[k].detach()).abs().max()) <= 1e-6, k
        identical = identical and torch.equal(got[k], plain[k])
    print("render_normals on/off, %s: the pre-existing entries are %sbit-identical" % ((raw_sh, raw_scene, objmask), "" if identical else "NOT "))
    hand = _hand_render(m, cam, on, objmask)
    assert float((got["img_normal"].detach() - hand["img_normal"].detach()).abs().max()) <= 1e-5
    assert float(got["img_normal"].detach().abs().max()) > 0.3
    if objmask:
        assert float((got["img_semantic"].detach() - hand["img_semantic"].detach()).abs().max()) <= 1e-6 and tuple(got["img_semantic"].shape) == (1, RH, RW)
    g = torch.Generator().manual_seed(5)
    for upstream in (torch.ones(3, RH, RW), torch.randn(3, RH, RW, generator=g)):
        up = upstream.cuda()
        a = _grads(m, render(cam, m, None, on, render_objmask=objmask)["img_normal"], up)
        b = _grads(m, _hand_render(m, cam, on, objmask)["img_normal"], up)
        assert sorted(a) == sorted(b) and all(k in a for k in ROTATION_PARAMS)
        for k in a:
            scale = float(b[k].abs().max())
            assert float((a[k] - b[k]).abs().max()) <= 1e-4 * scale, (k, float((a[k] - b[k]).abs().max()), scale)
        for k in ROTATION_PARAMS:
            assert float(a[k].abs().max()) > 0, k
    with pytest.raises(RuntimeError, match="render_normals"):
        render(cam, m, None, _pipe(render_normals=True, absgrad=True), render_objmask=objmask)
    with torch.no_grad():
        ev = render(cam, m, None, on, render_objmask=objmask)
        ev_abs = render(cam, m, None, _pipe(render_normals=True, absgrad=True), render_objmask=objmask)
    for e in (ev, ev_abs):
        assert e["img_normal"].grad_fn is None and float((e["img_normal"] - got["img_normal"].detach()).abs().max()) <= 1e-6
        assert (e["img_semantic"] is None) == (not objmask)
