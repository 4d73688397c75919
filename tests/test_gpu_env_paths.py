"""Environment-map kernels (csrc/envmap.hip) at every channel count, on both backward paths, in every pair-merge case, with the
tile marks and the accumulate contract of the raw ABI -- each against the float64 NumPy oracle, with the path a launch takes
asserted on the oracle (tests/env_cases.py mirrors TEXCAP and the 64 x 4 workgroup and checks them against the source).

Pixels within env_cases.EPS of the azimuth seam or the pole (oracle.env_oracle.unstable_pixels) carry zero upstream weight and
are left out of the forward comparison; there are at most max(H, W) of them per image.  Everywhere else NO outlier is allowed.
Tolerance per case: 8 * d32 + 2e-6 * scale, d32 = the float32 oracle's own deviation from the float64 one, scale = 1 for the
background and max |gradient| for the gradient, and never above the 3e-5 + 4e-6 * max(Hm, Wm) of tests/test_gpu_env.py.

Measured on an MI355X (largest error / d32 over the cases of each test; largest error / tolerance in brackets).  The device allows
163 840 B of LDS per workgroup, so the 65 552 B of C = 8 launch as they are.

    test                                      background     gradient
    every_channel_count   generic             0.91 (0.10)    1.57 (0.18)
                          neg_x               0.96 (0.11)    1.32 (0.15)
                          neg_x_wide_map      0.63 (0.08)    1.33 (0.17)
    lds_and_direct_atomics_paths              0.83 (0.10)    1.17 (0.15)
    pair_merge            same                1.28 (0.06)    1.91 (0.16)
                          adjacent            0.99 (0.12)    2.26 (0.23)
                          neither             1.19 (0.15)    1.27 (0.16)
    backward_accumulates  x1, x2                             0.65 (0.08)
    tile_marks            lds / fallback                     0.79 (0.09) / 0.34 (0.04)
    expanded_upstream     (gradient of ones)                 0.97 (0.09)
    non_contiguous_map_view                   0.83 (0.09)    0.92 (0.10)

The kernels deviate from the float64 oracle about as much as the float32 oracle does (at most 2.3 x), so the factor 8 stands
with no outlier anywhere.  Each of four deliberately wrong builds -- `v1 += p0` dropped from the adjacent-column merge, the
channel stride of s_acc halved, the mark index without `c * plane`, the direct-atomics row stride a.Hm for a.Wm -- failed
32, 6, 12 and 22 of the 53 tests.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import env_oracle
from tests import env_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lds_limit():
    """Decided before the first launch: envmap_bwd_kernel asks for C * TEXCAP * 4 B of dynamic LDS on top of the 16 B of its static
    s_box, 65 552 B at C = 8.  A workgroup of this device must be allowed that much (host-side property query, no launch)."""
    ec.assert_mirrors_kernel()
    limit = torch.cuda.get_device_properties(torch.cuda.current_device()).shared_memory_per_block
    need = ec.MAXC * ec.TEXCAP * 4 + 16
    print("LDS per workgroup: device allows %d B, envmap_bwd_kernel needs %d B at C = %d" % (limit, need, ec.MAXC))
    assert limit >= need, "device allows %d B of LDS per workgroup, envmap_bwd_kernel needs %d B at C = %d" % (limit, need, ec.MAXC)
    return limit


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rarr(R):
    return (ctypes.c_float * 9)(*[float(v) for v in np.asarray(R).reshape(-1)])


def _premise_few_unstable(ref, H, W):
    n = int((~ref.stable).sum())
    assert n <= max(H, W), "%d unstable pixels: more than one line of the %d x %d image" % (n, H, W)
    return n


def _close(what, got, want, d32, scale, Hm, Wm, mask=None, extra=0.0):
    """No outliers: every element within the tolerance.  Prints the figures first."""
    tol = min(ec.tolerance(d32, scale), ec.ceiling(Hm, Wm, scale))
    err = np.abs(np.asarray(got, np.float64) - want)
    if mask is not None:
        err = err * mask
    worst = float(err.max()) if err.size else 0.0
    print("%s: err %.3g  d32 %.3g  err/d32 %.2f  tol %.3g  err/tol %.3f" % (what, worst, d32, worst / d32 if d32 > 0 else float("inf"), tol, worst / tol))
    assert np.all(err <= tol + extra), (what, worst, tol, int((err > tol + extra).sum()))
    return worst


def _wrapper_run(ref, H, W, focal, R, batched=True):
    """adgs.env.image_background forward and backward with the case's upstream weights."""
    from adgs import env
    gm = torch.tensor(ref.gm)
    gm = (gm[None] if batched else gm).cuda().requires_grad_(True)
    bg = env.image_background(gm, H, W, focal, np.asarray(R).tolist())
    (bg * torch.tensor(ref.w).cuda()).sum().backward()
    return bg.detach().cpu().numpy(), gm.grad.cpu().numpy()


def _check_wrapper(what, Hm, Wm, H, W, focal, R, C, batched=True, seed=0):
    ref = ec.reference(C, Hm, Wm, H, W, focal, R, seed)
    _premise_few_unstable(ref, H, W)
    bg, g = _wrapper_run(ref, H, W, focal, R, batched)
    assert bg.shape == (C, H, W) and g.shape == ((1, C, Hm, Wm) if batched else (C, Hm, Wm))
    _close(what + " background", bg, ref.bg, ref.bg_d32, 1.0, Hm, Wm, mask=ref.stable)
    _close(what + " gradient", g.reshape(C, Hm, Wm), ref.grad, ref.grad_d32, ref.grad_scale, Hm, Wm)
    return ref


def _paths(Hm, Wm, H, W, focal, R):
    """(number of workgroups on the direct-atomics path, on the LDS path) -- by the float64 oracle, with the blocks whose class an
    unstable pixel could change required to be none."""
    bb = env_oracle.block_boxes(H, W, focal, R, Hm, Wm, bw=ec.BLOCK_W, bh=ec.BLOCK_H)
    stable = ~env_oracle.unstable_pixels(H, W, focal, R, ec.EPS)
    bs = env_oracle.block_boxes(H, W, focal, R, Hm, Wm, bw=ec.BLOCK_W, bh=ec.BLOCK_H, pixel_mask=stable)
    assert np.array_equal(bb.area > ec.TEXCAP, bs.area > ec.TEXCAP), "an unstable pixel decides a workgroup's path: move the camera"
    return int((bb.area > ec.TEXCAP).sum()), int(((bb.area <= ec.TEXCAP) & ~bb.empty).sum())


# ---- channel counts

CHANNEL_CASES = {            # name -> (Hm, Wm, H, W, focal, camera)
    "generic": (33, 64, 37, 121, 80.0, ec.CAM_GENERIC),
    "neg_x": (33, 64, 37, 121, 80.0, ec.CAM_NEG_X),                 # the seam blocks' boxes span the map's width and still fit the LDS image
    "neg_x_wide_map": (2, 4096, 37, 121, 80.0, ec.CAM_NEG_X),       # here they do not: direct atomics at every channel count
}


@pytest.mark.parametrize("case", sorted(CHANNEL_CASES))
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 7, 8])
def test_every_channel_count_forward_and_gradient(C, case):
    Hm, Wm, H, W, focal, R = CHANNEL_CASES[case]
    fallback, lds = _paths(Hm, Wm, H, W, focal, R)
    if case == "neg_x_wide_map":
        assert fallback > 0 and lds > 0, "TEXCAP = %d, %d x %d workgroups: the seam blocks must exceed the LDS image, the others fit" % (ec.TEXCAP, ec.BLOCK_W, ec.BLOCK_H)
    else:
        assert fallback == 0 and lds > 0, "TEXCAP = %d: a 33 x 64 map fits the LDS image whatever the box" % ec.TEXCAP
    if case == "neg_x":
        bb = env_oracle.block_boxes(H, W, focal, R, Hm, Wm, bw=ec.BLOCK_W, bh=ec.BLOCK_H)
        assert ((bb.box[..., 0] == 0) & (bb.box[..., 2] == Wm - 1)).any()       # a box from the map's first to its last column
    _check_wrapper("C=%d %s [1,C,Hm,Wm]" % (C, case), Hm, Wm, H, W, focal, R, C, batched=True)
    _check_wrapper("C=%d %s [C,Hm,Wm]" % (C, case), Hm, Wm, H, W, focal, R, C, batched=False)


# ---- both backward paths in one launch

PATH_CAMERAS = {"neg_x": (8, 192, 100.0, ec.CAM_NEG_X), "pole": (16, 256, 100.0, ec.CAM_POLE)}       # name -> (H, W, focal, camera)


@pytest.mark.parametrize("cam", sorted(PATH_CAMERAS))
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("Hm,Wm", [(8, 2048), (2, 4096)])
def test_lds_and_direct_atomics_paths_in_one_launch(Hm, Wm, C, cam):
    H, W, focal, R = PATH_CAMERAS[cam]
    fallback, lds = _paths(Hm, Wm, H, W, focal, R)
    assert fallback > 0, "no workgroup's box exceeds TEXCAP = %d texels (%d x %d-pixel workgroups): the direct-atomics path is not run" % (ec.TEXCAP, ec.BLOCK_W, ec.BLOCK_H)
    assert lds > 0, "every workgroup's box exceeds TEXCAP = %d texels (%d x %d-pixel workgroups): the LDS path is not run" % (ec.TEXCAP, ec.BLOCK_W, ec.BLOCK_H)
    ref = _check_wrapper("%dx%d C=%d %s" % (Hm, Wm, C, cam), Hm, Wm, H, W, focal, R, C)
    n = int((~ref.stable).sum())
    if cam == "pole":
        assert n == 1 and not ref.stable[H // 2, W // 2]          # the principal point, and nothing else
    else:
        assert n == H and not ref.stable[:, W // 2].any()         # exactly the centre column


# ---- pair merge

@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("config", sorted(ec.PAIR_CONFIGS))
def test_pair_merge_classes_and_partly_filled_blocks(config, C):
    Hm, Wm, focal, R, cls = ec.PAIR_CONFIGS[config]
    for W in ec.PAIR_WIDTHS:
        for H in ec.PAIR_HEIGHTS:
            pc = env_oracle.pair_classes(H, W, focal, R, Hm, Wm)
            assert int((pc == env_oracle.PARTNER_INVALID).sum()) == (H if W % 2 else 0)
            if W > 1:
                share = float((pc == cls).sum()) / (H * (W // 2))
                assert share >= 0.25, "%s: only %.0f %% of the pairs of the %d x %d image are of the class" % (config, 100 * share, H, W)
            fallback, lds = _paths(Hm, Wm, H, W, focal, R)
            assert fallback == 0 and lds > 0, "TEXCAP = %d: the pair merge runs on the LDS path only" % ec.TEXCAP
            _check_wrapper("%s C=%d %dx%d" % (config, C, H, W), Hm, Wm, H, W, focal, R, C, seed=W * 8 + H)


# ---- the raw ABI: accumulation and tile marks

def _raw_forward(ref, Hm, Wm, H, W, focal, R):
    from adgs import _lib
    C = ref.gm.shape[0]
    gm, bg = torch.tensor(ref.gm).cuda(), torch.empty(C, H, W, device="cuda")
    assert _lib.call("adgs_envmap_forward", _dev(), C, Hm, Wm, gm.data_ptr(), H, W, focal, _rarr(R), bg.data_ptr()) == 0
    return bg


def test_backward_accumulates_into_its_destination():
    """A destination that holds g0 comes back as g0 + g, and as g0 + 2 g after a second call -- on the LDS path and on the
    direct-atomics path (both are in this launch).  The second comparison applies the same tolerance to the reference 2 g."""
    from adgs import _lib
    Hm, Wm, H, W, focal, R = CHANNEL_CASES["neg_x_wide_map"]
    C = 3
    fallback, lds = _paths(Hm, Wm, H, W, focal, R)
    assert fallback > 0 and lds > 0, "TEXCAP = %d: both paths must be in the launch" % ec.TEXCAP
    ref = ec.reference(C, Hm, Wm, H, W, focal, R)
    bg, w = _raw_forward(ref, Hm, Wm, H, W, focal, R), torch.tensor(ref.w).cuda()
    g0 = torch.randn(C, Hm, Wm, generator=torch.Generator().manual_seed(11)).cuda()
    dst = g0.clone()
    for k in (1, 2):
        assert _lib.call("adgs_envmap_backward", _dev(), C, Hm, Wm, H, W, focal, _rarr(R), bg.data_ptr(), w.data_ptr(), dst.data_ptr()) == 0
        got = dst.cpu().numpy().astype(np.float64)
        ulp = np.spacing(np.abs(dst.cpu().numpy())).astype(np.float64) * k                       # one rounding of g0 + ... per call
        _close("accumulate x%d" % k, got - g0.cpu().numpy().astype(np.float64), k * ref.grad, k * ref.grad_d32, k * ref.grad_scale, Hm, Wm, extra=ulp)
    untouched = ~np.broadcast_to(env_oracle.tap_footprint(H, W, focal, R, Hm, Wm, slack=8 * ref.coord_d32 + 1e-4), (C, Hm, Wm))
    assert np.array_equal(dst.cpu().numpy()[untouched], g0.cpu().numpy()[untouched])            # and nothing else is written


MARK_LAUNCHES = {"lds": CHANNEL_CASES["generic"], "fallback": CHANNEL_CASES["neg_x_wide_map"]}
GUARD = 64


@pytest.mark.parametrize("launch", sorted(MARK_LAUNCHES))
@pytest.mark.parametrize("tile_elems", [256, 7])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_tile_marks_cover_the_gradient_and_stay_inside_the_footprint(C, tile_elems, launch):
    from adgs import _lib
    Hm, Wm, H, W, focal, R = MARK_LAUNCHES[launch]
    fallback, lds = _paths(Hm, Wm, H, W, focal, R)
    assert (fallback > 0) == (launch == "fallback") and lds > 0, "TEXCAP = %d: the launch must%s hold direct-atomics workgroups" % (ec.TEXCAP, "" if launch == "fallback" else " not")
    assert Wm % 7 and (Hm * Wm) % 7                                         # 7 divides neither a row nor a plane
    ref = ec.reference(C, Hm, Wm, H, W, focal, R)
    assert ref.stable.all()
    bg, w = _raw_forward(ref, Hm, Wm, H, W, focal, R), torch.tensor(ref.w).cuda()
    n_tiles = (C * Hm * Wm + tile_elems - 1) // tile_elems
    buf = torch.full((GUARD + n_tiles + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + n_tiles] = 0
    g, g_plain = torch.zeros(C, Hm, Wm, device="cuda"), torch.zeros(C, Hm, Wm, device="cuda")
    assert _lib.call("adgs_envmap_backward_marked", _dev(), C, Hm, Wm, H, W, focal, _rarr(R), bg.data_ptr(), w.data_ptr(), g.data_ptr(),
                     buf.data_ptr() + GUARD, tile_elems) == 0
    assert _lib.call("adgs_envmap_backward", _dev(), C, Hm, Wm, H, W, focal, _rarr(R), bg.data_ptr(), w.data_ptr(), g_plain.data_ptr()) == 0
    buf, g, g_plain = buf.cpu().numpy(), g.cpu().numpy(), g_plain.cpu().numpy()
    assert (buf[:GUARD] == 0xAB).all() and (buf[GUARD + n_tiles:] == 0xAB).all()          # nothing outside ceil(C Hm Wm / tile_elems)
    marks = buf[GUARD:GUARD + n_tiles]
    assert set(np.unique(marks)) <= {0, 1}

    def by_tile(flat):
        return np.concatenate([flat, np.zeros(n_tiles * tile_elems - flat.size, bool)]).reshape(n_tiles, tile_elems).any(1)

    holds_gradient = by_tile(g.reshape(-1) != 0)
    assert holds_gradient.any() and marks[holds_gradient].all()                            # every tile with a gradient is marked
    footprint = env_oracle.tap_footprint(H, W, focal, R, Hm, Wm, slack=8 * ref.coord_d32 + 1e-4)
    reachable = by_tile(np.broadcast_to(footprint, (C, Hm, Wm)).reshape(-1))
    assert not marks[~reachable].any(), "%d marked tiles hold no texel any tap reaches" % int(marks[~reachable].sum())
    assert not reachable.all()                                                              # (or that says nothing)
    _close("marked C=%d tile=%d %s" % (C, tile_elems, launch), g, ref.grad, ref.grad_d32, ref.grad_scale, Hm, Wm)
    _close("unmarked C=%d tile=%d %s" % (C, tile_elems, launch), g_plain, ref.grad, ref.grad_d32, ref.grad_scale, Hm, Wm)


# ---- autograd plumbing of adgs.env

def test_expanded_upstream_gradient_conserves_mass_per_channel():
    """bg.sum().backward() hands the backward a stride-0 expanded tensor of ones.  The four bilinear weights of a pixel whose taps
    are all in the map sum to 1, so each channel's gradient sums to its sum of b (1 - b) over those pixels; the camera is chosen
    so that they are all the pixels.  Bound: 8 x the float32 oracle's deviation of that mass + 2e-6 of it."""
    from adgs import env
    Hm, Wm, H, W, focal, R = CHANNEL_CASES["generic"]
    C = 5
    ref = ec.reference(C, Hm, Wm, H, W, focal, R)
    ix, iy = env_oracle.sample_coords(H, W, focal, R, Hm, Wm)
    inside = (np.floor(ix) >= 0) & (np.floor(ix) + 1 < Wm) & (np.floor(iy) >= 0) & (np.floor(iy) + 1 < Hm)
    assert inside.all() and ref.stable.all()
    gm = torch.tensor(ref.gm)[None].cuda().requires_grad_(True)
    bg = env.image_background(gm, H, W, focal, R.tolist())
    bg.sum().backward()
    mass = (ref.bg * (1 - ref.bg) * inside).sum((1, 2))
    bg32 = env_oracle.background(ref.gm, H, W, focal, R, np.float32)
    mass32 = (bg32 * (1 - bg32) * inside).sum((1, 2), dtype=np.float32)
    got = gm.grad.double().sum((0, 2, 3)).cpu().numpy()
    for c in range(C):
        d32 = abs(float(mass32[c]) - mass[c])
        print("mass c=%d: %.6f vs %.6f  err %.3g  d32 %.3g" % (c, got[c], mass[c], abs(got[c] - mass[c]), d32))
        assert abs(got[c] - mass[c]) <= ec.tolerance(d32, mass[c])
    ones = env_oracle.background_grad(ref.gm, H, W, focal, R, np.ones((C, H, W)))
    ones32 = env_oracle.background_grad(ref.gm, H, W, focal, R, np.ones((C, H, W)), np.float32)
    _close("ones gradient", gm.grad.cpu().numpy()[0], ones, float(np.abs(ones - ones32).max()), float(np.abs(ones).max()), Hm, Wm)


def test_non_contiguous_map_view_equals_its_contiguous_copy():
    from adgs import env
    Hm, Wm, H, W, focal, R = CHANNEL_CASES["generic"]
    C = 3
    ref = ec.reference(C, Hm, Wm, H, W, focal, R)
    w = torch.tensor(ref.w).cuda()
    base = torch.tensor(ref.gm)[None].transpose(-1, -2).contiguous().cuda().requires_grad_(True)      # [1, C, Wm, Hm]
    view = base.transpose(-1, -2)
    assert view.shape == (1, C, Hm, Wm) and not view.is_contiguous()
    bg_v = env.image_background(view, H, W, focal, R.tolist())
    (bg_v * w).sum().backward()
    copy = view.detach().contiguous().requires_grad_(True)
    bg_c = env.image_background(copy, H, W, focal, R.tolist())
    (bg_c * w).sum().backward()
    assert torch.equal(bg_v, bg_c)
    assert base.grad.shape == base.shape and copy.grad.shape == (1, C, Hm, Wm)
    _close("view background", bg_v.detach().cpu().numpy(), ref.bg, ref.bg_d32, 1.0, Hm, Wm, mask=ref.stable)
    _close("view gradient", base.grad.transpose(-1, -2).cpu().numpy()[0], ref.grad, ref.grad_d32, ref.grad_scale, Hm, Wm)
    _close("copy gradient", copy.grad.cpu().numpy()[0], ref.grad, ref.grad_d32, ref.grad_scale, Hm, Wm)


# ---- rejected arguments launch nothing

GOOD = dict(C=3, Hm=8, Wm=8, H=5, W=7, focal=6.0, tile_elems=16)
BAD_ARGUMENTS = [("C", 0), ("C", 9), ("Hm", 1), ("Wm", 1), ("focal", 0.0), ("focal", -1.0), ("focal", float("nan"))]
SENTINEL = -123.5


def _buffers():
    """Large enough for 9 channels of the GOOD shapes: a call that wrongly launched would still stay in bounds."""
    t = lambda *s: torch.full(s, SENTINEL, device="cuda")
    return dict(grid=t(9, 8, 8), bg=t(9, 5, 7), g_bg=t(9, 5, 7), g_grid=t(9, 8, 8), marks=torch.full((9 * 64,), 0xAB, dtype=torch.uint8, device="cuda"))


def _call(entry, a, b):
    from adgs import _lib
    R = _rarr(ec.CAM_GENERIC)
    if entry == "adgs_envmap_forward":
        return _lib.call(entry, _dev(), a["C"], a["Hm"], a["Wm"], b["grid"].data_ptr(), a["H"], a["W"], a["focal"], R, b["bg"].data_ptr())
    args = (a["C"], a["Hm"], a["Wm"], a["H"], a["W"], a["focal"], R, b["bg"].data_ptr(), b["g_bg"].data_ptr(), b["g_grid"].data_ptr())
    if entry == "adgs_envmap_backward_marked":
        args += (b["marks"].data_ptr(), a["tile_elems"])
    return _lib.call(entry, _dev(), *args)


def _unchanged(b):
    torch.cuda.synchronize()
    return all(bool((v == (0xAB if k == "marks" else SENTINEL)).all()) for k, v in b.items())


@pytest.mark.parametrize("entry", ["adgs_envmap_forward", "adgs_envmap_backward", "adgs_envmap_backward_marked"])
def test_rejected_arguments_raise_and_write_nothing(entry):
    b = _buffers()
    for name, value in BAD_ARGUMENTS:
        with pytest.raises(RuntimeError) as err:
            _call(entry, dict(GOOD, **{name: value}), b)
        assert str(err.value).startswith(entry + " failed:") and "bad arguments (1..8 channels, map >= 2x2, focal > 0" in str(err.value), (name, value, str(err.value))
        assert _unchanged(b), (name, value)
    if entry == "adgs_envmap_backward_marked":
        with pytest.raises(RuntimeError) as err:
            _call(entry, dict(GOOD, tile_elems=0), b)
        assert str(err.value) == entry + " failed: adgs_envmap_backward_marked: tile_elems must be positive"
        assert _unchanged(b)
    for name in ("H", "W"):                                   # an empty image is no error and no launch
        assert _call(entry, dict(GOOD, **{name: 0}), b) == 0
        assert _unchanged(b), name
    # and the same buffers are written by the accepted call: the sentinel check above can fail
    assert _call(entry, GOOD, b) == 0
    assert not _unchanged(b)
