"""Bilateral-grid appearance compensation on the GPU (adgs.bilagrid over include/adgs_bilagrid.h) against the float64
reference of tests/bilagrid_ref.py.

Shapes: every grid of ref.GRIDS under every image of ref.IMAGES.  (28, 110) is not in the issue's list: under the (8, 16, 16) grid
it is a multi-workgroup image with partial tiles whose tile footprint (11 x 4 grid columns, 45 padded, x 96 channel-levels = 4320
floats) exceeds the 4096-float LDS budget, i.e. the global-memory path away from the single-workgroup images; (37, 121) under the
same grid is the LDS path just under the budget (3936 floats).  Tiles are 64 x 4 pixels: (37, 121) and (48, 200) have partial
tiles in x and y and tiles that span several grid columns.

Forward tolerance: 4 x the largest error of the float32 torch-CPU evaluation of the grid_sample form against float64 on the same
inputs, measured per case on the CPU (FWD_TABLE: seed, that error, max |ref|, knot pixels of the seed), and never looser than
1e-4 max(1, max |ref|).  The seeds are the first for which the reference alone has its knot pixels inside the cap (none under
500 pixels, 0.2 % above) and no unplanted pixel within 1e-4 of gray (L - 1) = 0 or L - 1."""
import ctypes
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import bilagrid_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# (grid, image): (seed, max |float32 CPU grid_sample form - float64|, max |ref|, knot pixels)
FWD_TABLE = {
    ((2, 2, 2), (1, 1)): (1, 4.16e-08, 1.042, 0),
    ((2, 2, 2), (3, 5)): (1, 3.11e-07, 2.926, 0),
    ((2, 2, 2), (16, 64)): (1, 3.18e-07, 2.485, 0),
    ((2, 2, 2), (37, 121)): (1, 3.35e-07, 2.564, 0),
    ((2, 2, 2), (48, 200)): (1, 5.48e-07, 3.301, 0),
    ((2, 2, 2), (28, 110)): (2, 4.28e-07, 2.721, 0),
    ((3, 5, 7), (1, 1)): (1, 1.02e-07, 0.848, 0),
    ((3, 5, 7), (3, 5)): (1, 3.06e-07, 4.648, 0),
    ((3, 5, 7), (16, 64)): (1, 2.93e-07, 2.294, 0),
    ((3, 5, 7), (37, 121)): (1, 7.15e-07, 2.705, 0),
    ((3, 5, 7), (48, 200)): (1, 7.35e-07, 3.433, 2),
    ((3, 5, 7), (28, 110)): (2, 5.44e-07, 2.653, 0),
    ((8, 4, 4), (1, 1)): (1, 4.64e-08, 0.697, 0),
    ((8, 4, 4), (3, 5)): (1, 3.44e-07, 2.296, 0),
    ((8, 4, 4), (16, 64)): (1, 7.45e-07, 2.619, 0),
    ((8, 4, 4), (37, 121)): (1, 9.13e-07, 2.450, 0),
    ((8, 4, 4), (48, 200)): (1, 1.35e-06, 3.003, 3),
    ((8, 4, 4), (28, 110)): (1, 9.12e-07, 3.135, 1),
    ((8, 16, 16), (1, 1)): (1, 2.29e-08, 0.950, 0),
    ((8, 16, 16), (3, 5)): (1, 2.73e-07, 3.329, 0),
    ((8, 16, 16), (16, 64)): (1, 7.52e-07, 2.894, 0),
    ((8, 16, 16), (37, 121)): (1, 1.97e-06, 2.779, 0),
    ((8, 16, 16), (48, 200)): (1, 1.67e-06, 3.143, 3),
    ((8, 16, 16), (28, 110)): (1, 2.06e-06, 2.714, 1),
}
# the shapes whose tile footprint does not fit the LDS budget: columns along x = min(Wg, floor((min(64, W) - 1) / W (Wg - 1)) + 3),
# the same along y with 4-pixel tiles, 12 L (columns | 1) floats against 4096
GLOBAL_PATH = {((8, 16, 16), (3, 5)), ((8, 16, 16), (16, 64)), ((8, 16, 16), (28, 110))}
CASES = sorted(FWD_TABLE)
INDEX = 1


def _grad_tol(t):
    return 1e-4 * max(1.0, t.abs().max().item())


@functools.lru_cache(maxsize=None)
def _case(grid, image):
    """inputs (float32, CPU) and the float64 reference of one case: computed once, shared, never modified"""
    grids, img, d_out, planted = ref.make_case(*grid, *image, FWD_TABLE[(grid, image)][0])
    g64, i64, d64 = grids[INDEX].double(), img.double(), d_out.double()
    out = ref.slice_forward(g64, i64)
    d_grid, d_image = ref.slice_backward(g64, i64, d64)
    return dict(grids=grids, image=img, d_out=d_out, planted=planted, out=out, d_grid=d_grid, d_image=d_image, knots=ref.knot_mask(img, grid[0]))


@functools.lru_cache(maxsize=None)
def _gpu_backward(grid, image):
    """(d grids [N, ...], d image, path) of one case through adgs.bilagrid.slice and autograd"""
    from adgs import bilagrid
    c = _case(grid, image)
    grids = c["grids"].cuda().requires_grad_(True)
    img = c["image"].cuda().requires_grad_(True)
    out = bilagrid.slice(grids, img, INDEX)
    out.backward(c["d_out"].cuda())
    torch.cuda.synchronize()
    return grids.grad.cpu(), img.grad.cpu(), out.detach().cpu(), bilagrid.backward_path(grids, img)


def _raw_backward(c, grid, image, want_grid=True, want_image=True):
    from adgs import _lib
    L, Hg, Wg = grid
    H, W = image
    g = c["grids"][INDEX].cuda().contiguous()
    img, d_out = c["image"].cuda(), c["d_out"].cuda()
    d_grid = torch.zeros_like(g) if want_grid else None
    d_image = torch.full_like(img, float("nan")) if want_image else None
    _lib.check(_lib.lib().adgs_bilagrid_slice_backward(L, Hg, Wg, g.data_ptr(), H, W, img.data_ptr(), d_out.data_ptr(),
                                                       d_grid.data_ptr() if want_grid else None, d_image.data_ptr() if want_image else None,
                                                       _lib.stream_ptr(g.device)), "adgs_bilagrid_slice_backward")
    torch.cuda.synchronize()
    return (d_grid.cpu() if want_grid else None), (d_image.cpu() if want_image else None)


def test_cases_cover_both_paths_and_the_reference_respects_the_knot_cap():
    assert GLOBAL_PATH and GLOBAL_PATH < set(CASES)
    for grid, image in CASES:
        c = _case(grid, image)
        n = image[0] * image[1]
        knots = int(c["knots"].sum())
        assert knots == FWD_TABLE[(grid, image)][3]
        assert knots <= (0 if n < 500 else int(0.002 * n))
        v = ref.gray_of(c["image"].double()) * (grid[0] - 1)
        assert not ((v - (grid[0] - 1)).abs() <= 1e-4).any()
        near0 = (v.abs() <= 1e-4).reshape(-1)
        if c["planted"]:
            flat = v.reshape(-1)
            assert flat[c["planted"][0]] == 0 and abs(flat[c["planted"][1]] - 2.0 * (grid[0] - 1)) < 1e-9 and flat[c["planted"][2]] < 0
            assert not c["knots"].reshape(-1)[c["planted"]].any()
            near0[c["planted"][0]] = False
        assert not near0.any()


@pytest.mark.parametrize("grid,image", CASES)
def test_forward(grid, image):
    from adgs import bilagrid
    c = _case(grid, image)
    _, err32, max_ref, _ = FWD_TABLE[(grid, image)]
    assert abs(c["out"].abs().max().item() - max_ref) < 1e-3
    with torch.no_grad():
        out = bilagrid.slice(c["grids"].cuda(), c["image"].cuda(), INDEX).cpu()
    err = (out.double() - c["out"]).abs().max().item()
    tol = min(4 * err32, 1e-4 * max(1.0, max_ref))
    print("forward %s %s: max err %.3e, tolerance %.3e (float32 CPU error %.2e)" % (grid, image, err, tol, err32))
    assert err <= tol


@pytest.mark.parametrize("grid,image", CASES)
def test_backward_grid(grid, image):
    c = _case(grid, image)
    d_grids, _, _, path = _gpu_backward(grid, image)
    assert path == ("global" if (grid, image) in GLOBAL_PATH else "lds")
    assert d_grids.shape == c["grids"].shape
    assert not d_grids[0].any() and not d_grids[2].any()
    err = (d_grids[INDEX].double() - c["d_grid"]).abs().max().item()
    print("dL/dG %s %s (%s): max err %.3e, tolerance %.3e" % (grid, image, path, err, _grad_tol(c["d_grid"])))
    assert err <= _grad_tol(c["d_grid"])
    # the bias channels 4 i + 3 receive d_out[i] with weights that sum to one
    for i in range(3):
        want = c["d_out"][i].double().sum().item()
        got = d_grids[INDEX, 4 * i + 3].double().sum().item()
        assert abs(got - want) <= 1e-4 * abs(want)


@pytest.mark.parametrize("grid,image", CASES)
def test_backward_image(grid, image):
    c = _case(grid, image)
    _, d_image, _, _ = _gpu_backward(grid, image)
    n = image[0] * image[1]
    exempt = c["knots"]
    assert int(exempt.sum()) <= (0 if n < 500 else int(0.002 * n))
    err = (d_image.double() - c["d_image"]).abs().amax(dim=0)
    tol = _grad_tol(c["d_image"])
    print("dL/dI %s %s: max err %.3e outside %d knot pixels, tolerance %.3e" % (grid, image, err[~exempt].max().item(), int(exempt.sum()), tol))
    assert err[~exempt].max().item() <= tol
    if c["planted"]:
        assert (err.reshape(-1)[c["planted"]] <= tol).all()


@pytest.mark.parametrize("grid,image", [((8, 16, 16), (48, 200)), ((8, 16, 16), (28, 110)), ((2, 2, 2), (37, 121))])
def test_backward_null_outputs_and_repeat(grid, image):
    c = _case(grid, image)
    both_g, both_i = _raw_backward(c, grid, image)
    only_g, none_i = _raw_backward(c, grid, image, want_image=False)
    none_g, only_i = _raw_backward(c, grid, image, want_grid=False)
    assert none_i is None and none_g is None
    assert torch.equal(only_i, both_i)                     # per-pixel arithmetic: no accumulation order involved
    tol = _grad_tol(c["d_grid"])
    assert (only_g.double() - c["d_grid"]).abs().max().item() <= tol
    assert (both_g.double() - c["d_grid"]).abs().max().item() <= tol
    assert (both_g - only_g).abs().max().item() <= tol     # a second backward into fresh zeros
    assert not torch.isnan(both_i).any()                   # dL_dimage is fully written


def test_backward_smooth_image_merges_neighbours():
    """A smooth image: neighbouring pixels share their luma level, the case the LDS accumulation sums across lanes before it adds."""
    from adgs import bilagrid
    grid, (H, W) = (8, 16, 16), (48, 200)
    gen = torch.Generator().manual_seed(5)
    grids = ref.identity_grid(*grid, torch.float32)[None] + 0.3 * torch.randn(3, 12, *grid, generator=gen)
    x = (torch.arange(W, dtype=torch.float32) + 0.5) / W
    y = (torch.arange(H, dtype=torch.float32) + 0.5) / H
    img = torch.stack([0.1 + 0.8 * x[None, :] * y[:, None], 0.3 + 0.4 * y[:, None].expand(H, W), 0.9 - 0.7 * x[None, :].expand(H, W)])
    img = (img + 0.004 * torch.rand(3, H, W, generator=gen)).contiguous()
    d_out = torch.randn(3, H, W, generator=gen)
    want_g, want_i = ref.slice_backward(grids[INDEX].double(), img.double(), d_out.double())
    gg, ii = grids.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
    assert bilagrid.backward_path(gg, ii) == "lds"
    bilagrid.slice(gg, ii, INDEX).backward(d_out.cuda())
    assert (gg.grad[INDEX].cpu().double() - want_g).abs().max().item() <= _grad_tol(want_g)
    knots = ref.knot_mask(img, grid[0])
    assert int(knots.sum()) <= int(0.002 * H * W)
    assert (ii.grad.cpu().double() - want_i).abs().amax(dim=0)[~knots].max().item() <= _grad_tol(want_i)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("grid", [(2, 2, 2), (8, 16, 16)])
def test_total_variation(N, grid):
    from adgs import bilagrid
    gen = torch.Generator().manual_seed(17)
    grids = ref.identity_grid(*grid, torch.float32)[None] + 0.3 * torch.randn(N, 12, *grid, generator=gen)
    g64 = grids.double().requires_grad_(True)
    want = ref.total_variation(g64)
    want.backward()
    gg = grids.cuda().requires_grad_(True)
    tv = bilagrid.total_variation(gg)
    (tv * 1.5).backward()
    assert abs(tv.item() - want.item()) <= 1e-6 * abs(want.item())
    scale = (1.5 * g64.grad).abs().max().item()
    assert (gg.grad.cpu().double() - 1.5 * g64.grad).abs().max().item() <= 1e-6 * scale
    # the work buffer is left zero: a second call gives the same loss
    assert bilagrid.total_variation(gg.detach()).item() == tv.item()


def test_refusals_launch_nothing():
    from adgs import _lib
    lib = _lib.lib()
    L, Hg, Wg, H, W, N = 3, 4, 5, 6, 70, 2
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    grids = torch.randn(N, 12, L, Hg, Wg, device=dev)
    img, d_out = torch.rand(3, H, W, device=dev), torch.randn(3, H, W, device=dev)
    out = torch.full((3, H, W), 7.0, device=dev)
    d_grid, d_image = torch.full((12, L, Hg, Wg), 7.0, device=dev), torch.full((3, H, W), 7.0, device=dev)
    d_grids = torch.full_like(grids, 7.0)
    work = torch.zeros(256, dtype=torch.float64, device=dev)
    loss, g_loss = torch.full((1,), 7.0, device=dev), torch.ones(1, device=dev)
    p = lambda t: t.data_ptr()
    fwd = lambda L=L, Hg=Hg, Wg=Wg, g=p(grids), H=H, W=W, i=p(img), o=p(out): lib.adgs_bilagrid_slice_forward(L, Hg, Wg, g, H, W, i, o, st)
    bwd = lambda L=L, Hg=Hg, Wg=Wg, g=p(grids), H=H, W=W, i=p(img), d=p(d_out): lib.adgs_bilagrid_slice_backward(L, Hg, Wg, g, H, W, i, d, p(d_grid), p(d_image), st)
    tvf = lambda N=N, L=L, Hg=Hg, Wg=Wg, g=p(grids), w=p(work), l=p(loss): lib.adgs_bilagrid_tv_forward(N, L, Hg, Wg, g, w, l, st)
    tvb = lambda N=N, L=L, Hg=Hg, Wg=Wg, g=p(grids), gl=p(g_loss), d=p(d_grids): lib.adgs_bilagrid_tv_backward(N, L, Hg, Wg, g, gl, d, st)
    calls = []
    for f in (fwd, bwd):
        calls += [lambda f=f: f(L=1), lambda f=f: f(Hg=1), lambda f=f: f(Wg=1), lambda f=f: f(H=0), lambda f=f: f(W=0), lambda f=f: f(g=None), lambda f=f: f(i=None)]
    calls += [lambda: fwd(o=None), lambda: bwd(d=None)]
    for f in (tvf, tvb):
        calls += [lambda f=f: f(N=0), lambda f=f: f(L=1), lambda f=f: f(Hg=1), lambda f=f: f(Wg=1), lambda f=f: f(g=None)]
    calls += [lambda: tvf(w=None), lambda: tvf(l=None), lambda: tvb(gl=None), lambda: tvb(d=None)]
    for k, call in enumerate(calls):
        assert call() < 0, "refusal %d was accepted" % k
        assert _lib.last_error().startswith("adgs_bilagrid_"), _lib.last_error()
    torch.cuda.synchronize()
    for t in (out, d_grid, d_image, d_grids, loss):
        assert (t == 7.0).all()
    assert not work.any()
    assert lib.adgs_test_bilagrid_path(1, 2, 2, 4, 4) < 0
    # and the Python surface refuses CPU tensors
    from adgs import bilagrid
    with pytest.raises(RuntimeError):
        bilagrid.slice(grids.cpu(), img, 0)
    with pytest.raises(RuntimeError):
        bilagrid.slice(grids, img.cpu(), 0)
    with pytest.raises(RuntimeError):
        bilagrid.total_variation(grids.cpu())


def test_graph_capture():
    from adgs import bilagrid
    grid, image = (8, 16, 16), (16, 64)
    c = _case(grid, image)
    grids = c["grids"].cuda().requires_grad_(True)
    img = c["image"].cuda().requires_grad_(True)
    d_out = c["d_out"].cuda()

    def run():
        return torch.autograd.grad(bilagrid.slice(grids, img, INDEX), (grids, img), d_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_grids, g_img = run()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    e_grids, e_img = run()
    assert (g_grids - e_grids).abs().max().item() <= _grad_tol(c["d_grid"])
    assert (g_grids[INDEX].cpu().double() - c["d_grid"]).abs().max().item() <= _grad_tol(c["d_grid"])
    assert torch.equal(g_img, e_img)


# |float32 - float64| of the CPU reference loop's loss at each of the ten steps (losses 1.07e-2 ... 5.5e-3), measured on the CPU
MODULE_LOOP_F32_ERR = (1.83e-09, 6.93e-09, 3.38e-09, 4.18e-09, 2.84e-09, 3.89e-09, 3.08e-09, 2.78e-09, 2.96e-09, 2.80e-09)


def _tinted(dtype):
    gen = torch.Generator().manual_seed(11)
    img = torch.rand(3, 16, 64, generator=gen, dtype=torch.float32).to(dtype)
    return img, img * torch.tensor([1.2, 0.9, 0.8], dtype=dtype)[:, None, None] + 0.05


def _cpu_loop(dtype):
    img, target = _tinted(dtype)
    grids = ref.identity_grid(8, 4, 4, dtype)[None].repeat(2, 1, 1, 1, 1).requires_grad_(True)
    opt = torch.optim.Adam([grids], lr=2e-3, eps=1e-15)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = ((ref.grid_sample_form(grids[1], img) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def test_module_fits_a_tint_like_the_cpu_loop(tmp_path):
    from adgs import bilagrid
    want = _cpu_loop(torch.float64)
    img, target = (t.cuda() for t in _tinted(torch.float32))
    model = bilagrid.BilateralGrid(2, grid_x=4, grid_y=4, grid_w=8)
    assert torch.equal(model.grids.detach().cpu(), ref.identity_grid(8, 4, 4, torch.float32)[None].repeat(2, 1, 1, 1, 1))
    model.training_setup(object())
    assert model.optimizer.param_groups[0]["name"] == "bilagrid" and model.optimizer.param_groups[0]["lr"] == 2e-3
    got = []
    for _ in range(10):
        loss = ((model(img, 1) - target) ** 2).mean()
        loss.backward()
        model.step()
        got.append(loss.item())
    for k in range(10):
        print("step %d: loss %.9e, reference %.9e, diff %.2e, tolerance %.2e" % (k, got[k], want[k], abs(got[k] - want[k]), 4 * MODULE_LOOP_F32_ERR[k]))
    for k in range(10):
        assert abs(got[k] - want[k]) <= 4 * MODULE_LOOP_F32_ERR[k]
    assert got[-1] < 0.6 * got[0]
    path = str(tmp_path / "bilagrid.pth")
    model.save_weights(path)
    other = bilagrid.BilateralGrid(2, grid_x=4, grid_y=4, grid_w=8)
    other.load_weights(path)
    assert torch.equal(other.grids.detach(), model.grids.detach()) and other.grids.requires_grad
    assert model.tv_loss().item() > 0


def test_sparse_adam_leaves_unused_grids_alone():
    from adgs import bilagrid
    gen = torch.Generator().manual_seed(23)
    img = torch.rand(3, 16, 64, generator=gen).cuda()
    target = (img * 1.1 + 0.02).contiguous()
    sparse = bilagrid.BilateralGrid(5, grid_x=4, grid_y=4, grid_w=8, sparse_adam=True)
    dense = bilagrid.BilateralGrid(5, grid_x=4, grid_y=4, grid_w=8)
    for m in (sparse, dense):
        m.training_setup(object())
    assert sparse.optimizer.param_groups[0]["visibility_rows"] == "head"

    def iteration(used):
        # the slice backward accumulates with float atomics: both models step on the SAME gradient tensor values
        loss = sum(((sparse(img, k) - target) ** 2).mean() for k in used)
        loss.backward()
        dense.grids.grad = sparse.grids.grad.clone()
        sparse.step()
        dense.step()

    iteration(range(5))                                     # every grid used: moments everywhere, the two models agree
    assert torch.equal(sparse.grids.detach(), dense.grids.detach())
    state = lambda m: (m.grids.detach().clone(), m.optimizer.state[m.grids]["exp_avg"].clone(), m.optimizer.state[m.grids]["exp_avg_sq"].clone())
    before = state(sparse)
    iteration((1, 3))
    after, after_dense = state(sparse), state(dense)
    for b, a, d in zip(before, after, after_dense):
        for k in (0, 2, 4):
            assert torch.equal(a[k], b[k])                  # unused: parameters and both moments bit for bit
        for k in (1, 3):
            assert torch.equal(a[k], d[k]) and not torch.equal(a[k], b[k])
    assert not torch.equal(after_dense[0][0], before[0][0])  # the dense step does move an unused grid (decaying moments)
    assert not sparse._used.any()
