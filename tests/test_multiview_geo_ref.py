"""Pins tests/multiview_geo_ref.py, the float64 yardstick of the multi-view geometric consistency loss (include/adgs_multiview_geo.h),
and the conditions of tests/multiview_geo_cases.py; measures what the float32 restatement of the chain holds at 1280 x 1920; tests
adgs.multiview.nearest_cameras (host torch).  No GPU."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests import multiview_geo_cases as cases  # noqa: E402
from tests import multiview_geo_ref as ref  # noqa: E402
from tests.multiview_cases import TAN, TAN_N  # noqa: E402

WALL = (((0.0, 0.0, -1.0), -8.0),)                                 # one fronto-parallel plane 8 m ahead
SHIFT = torch.tensor([[1.0, 0, 0, -0.25], [0, 1.0, 0, 0.0625], [0, 0, 1.0, -0.375]], dtype=torch.float64)     # no rotation, exact in float32: centre (0.25, -0.0625, 0.375)


def wall_views(H=24, W=32, Hn=20, Wn=36, scale_n=1.0):
    """Exact float64 maps of the wall under a pure translation: the neighbour's depth is constant, so its bilinear sample is exact."""
    z, zn = cases.true_depths(H, W, Hn, Wn, SHIFT, WALL)
    O, On = torch.full_like(z, 0.8), torch.full_like(zn, 0.9)
    return O / z, O, On / (zn * scale_n), On


def evaluate64(D, O, Dn, On, **kw):
    """The reference on float64 maps as they are (no rounding to float32: the exactness tests need the exact depths)."""
    leaves = [t.clone().requires_grad_(True) for t in (D, O, Dn, On)]
    return ref.evaluate(leaves[0], leaves[1], TAN, leaves[2], leaves[3], TAN_N, SHIFT, **kw), leaves


def test_exact_depths_close_the_round_trip():
    for inv in (True, False):
        D, O, Dn, On = wall_views()
        if not inv:
            D, Dn = O * O / D, On * On / Dn                        # D = O z
        r, _ = evaluate64(D, O, Dn, On, inv_depth=inv)
        assert float(r.geo.float().mean()) > 0.5 and bool((r.valid == r.geo).all())
        assert float(r.err.detach().max()) < 1e-9 and abs(float(r.L.detach())) < 1e-9
        assert bool((r.gw[r.valid] > 1 - 1e-9).all()) and not r.gw[~r.valid].any()


def test_a_scaled_neighbour_depth_moves_the_point_along_the_parallax():
    """Dn scaled so that zh = (1 + eps) z_n:  Y' = (1 + eps) Y, X' = X + eps (X - C) with C = -R^T t the neighbour's centre: the landing
    pixel moves along the epipolar line, by kx eps (X.x C.z - C.x X.z) / X.z^2 to first order."""
    H, W = 24, 32
    eps = 1e-3
    D, O, Dn, On = wall_views(H, W, scale_n=1 + eps)
    r, _ = evaluate64(D, O, Dn, On, max_pixel_error=100.0)
    C = -SHIFT[:, :3].T @ SHIFT[:, 3]
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    rx, ry = ref.ray_xy(x, y, H, W, (ref.f32(TAN[0]), ref.f32(TAN[1])))
    X = torch.stack([8.0 * rx, 8.0 * ry, torch.full_like(rx, 8.0)], dim=-1)
    Xp = X + eps * (X - C)
    tan = (ref.f32(TAN[0]), ref.f32(TAN[1]))
    xp, yp = ref.pixel_of(Xp[..., 0], Xp[..., 1], Xp[..., 2], H, W, tan)
    dx, dy = xp - x, yp - y
    want = (dx * dx + dy * dy).sqrt()
    assert bool(r.geo.any()) and float((r.err.detach() - want)[r.geo].abs().max()) < 1e-9
    first = eps * torch.stack([(X[..., 0] * C[2] - C[0] * X[..., 2]) / 64.0 / tan[0] * (W / 2), (X[..., 1] * C[2] - C[1] * X[..., 2]) / 64.0 / tan[1] * (H / 2)], dim=-1)
    assert float((torch.stack([dx, dy], dim=-1) - first).abs().max()) < 5 * eps * float(first.abs().max())      # second order in eps
    assert float(want[r.geo].max()) > 1e-3


@pytest.mark.parametrize("inv", (True, False))
def test_autograd_agrees_with_finite_differences(inv):
    """Directional derivatives of L with validity and exp(-err) frozen (what autograd differentiates), for all four maps."""
    c = cases.BY_NAME["inv_w" if inv else "lin_w"]
    inp = cases.inputs(c.name)
    maps = [t.double() for t in (inp.D, inp.O, inp.Dn, inp.On)]
    kw = dict(weight=inp.weight, inv_depth=c.inv_depth, max_pixel_error=inp.max_pixel_error)
    leaves = [t.clone().requires_grad_(True) for t in maps]
    base = ref.evaluate(leaves[0], leaves[1], TAN, leaves[2], leaves[3], TAN_N, inp.pose, **kw)
    base.L.backward()
    g = torch.Generator().manual_seed(5)
    h = 1e-6
    for i, name in enumerate(("depth", "opacity", "nbr_depth", "nbr_opacity")):
        d = torch.randn(maps[i].shape, generator=g, dtype=torch.float64) * maps[i]
        L = []
        for s in (+1, -1):
            moved = [m + s * h * d if j == i else m for j, m in enumerate(maps)]
            moved = [m.clone().requires_grad_(True) for m in moved]
            L.append(float(ref.evaluate(moved[0], moved[1], TAN, moved[2], moved[3], TAN_N, inp.pose, frozen=base, **kw).L.detach()))
        fd, an = (L[0] - L[1]) / (2 * h), float((leaves[i].grad * d).sum())
        print("%s: finite difference %.9g, autograd %.9g" % (name, fd, an))
        assert abs(an) > 1e-4 and abs(fd - an) <= 1e-5 * abs(an), name


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_case_conditions(name):
    c, inp = cases.BY_NAME[name], cases.inputs(name)
    r, grads = cases.reference(name)
    near, valid = float(inp.near.float().mean()), float(r.valid.float().mean())
    q = [float(r.err[r.geo].quantile(p)) for p in (0.1, 0.5, 0.9, 0.99)]
    print("%s: %.1f %% valid, %.2f %% near a gate, err quantiles 10/50/90/99 %% = %.3f / %.3f / %.3f / %.3f px" % (name, 100 * valid, 100 * near, *q))
    assert near <= 0.02 and valid >= 0.25
    assert bool((ref.near_gate(r.margins) == inp.near).all())
    if c.weighted:
        assert not inp.weight[inp.near].any() and bool((inp.weight[~inp.near] > 0).any())
    else:
        assert not inp.near.any()                                   # the seed and the threshold of cases.find_gap
    assert float(r.L) > 0 and all(bool(t.any()) and bool(torch.isfinite(t).all()) for t in grads)
    if name == "tight":
        assert 0.4 < float(r.valid.sum()) / float(r.geo.sum()) < 0.6
    if name in ("many_blocks", "dense", "inv_now"):
        assert bool((r.geo & ~r.valid).any())                       # the last gate decides somewhere


def test_the_unweighted_cases_sit_in_a_gap():
    for name in ("inv_now", "lin_now"):
        c = cases.BY_NAME[name]
        seed, threshold, half = cases.find_gap(c)
        assert (seed, threshold) == (c.seed, c.max_pixel_error) and half > 1e-2


def test_float32_restatement_at_full_resolution():
    """What decides float against double in the kernel: the same chain in float32 against float64 at 1280 x 1920 (0.3 % depth noise, the
    errors of a settled geometry).  Measured: err off by up to 5.2e-4 px, L by 2.3e-5 relative, 25 validities differ, and the gradients by
    up to 1.7 max|ref| of their tensor -- the direction (dx, dy) / err of an error far below a pixel is rounding noise in float32, where
    one ulp of a pixel coordinate of 1900 is 1.2e-4.  The GPU test's tolerances are 1e-5 px and 1e-4 max|ref|: the chain is double."""
    c = cases.Case("full", 1280, 1920, 1280, 1920, True, False, 11, 0.003, 1.0)
    D, O, Dn, On, _, pose = cases.raw_inputs(c)
    r64, g64 = ref.with_grads(D, O, TAN, Dn, On, TAN, pose)
    r32, g32 = ref.with_grads(D, O, TAN, Dn, On, TAN, pose, dtype=torch.float32)
    both = r64.geo & r32.geo
    e_err = float((r32.err.double() - r64.err)[both].abs().max())
    e_L = abs(float(r32.L) - float(r64.L)) / float(r64.L)
    e_g = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(g32, g64)]
    print("float32 against float64 at 1280 x 1920: err off by %.2e px, L by %.2e relative, %d validities differ, gradients by %s of max|ref|"
          % (e_err, e_L, int((r64.valid != r32.valid).sum()), ", ".join("%.2e" % e for e in e_g)))
    assert float(r64.valid.float().mean()) > 0.25
    assert e_err > 1e-5 and max(e_g) > 1e-4                         # float32 cannot meet the tolerances of tests/test_gpu_multiview_geo.py


def test_nearest_cameras():
    from adgs import multiview

    class Cam:
        pass

    def camera(centre, yaw):
        """world_view_transform of a camera at `centre` looking along (sin yaw, 0, cos yaw)."""
        c, s = math.cos(yaw), math.sin(yaw)
        R = torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], dtype=torch.float64)
        A = torch.eye(4, dtype=torch.float64)
        A[:3, :3], A[:3, 3] = R, -R @ torch.tensor(centre, dtype=torch.float64)
        cam = Cam()
        cam.world_view_transform = A.T.contiguous().float()
        return cam

    # a straight track along the viewing direction, 0.5 m apart: every angle is 0, the distance ranks
    straight = [camera((0.0, 0.0, 0.5 * i), 0.0) for i in range(6)]
    assert multiview.nearest_cameras(straight) == [[1], [0], [1], [2], [3], [4]]            # ties go to the lower index
    assert multiview.nearest_cameras(straight, k=3) == [[1, 2, 3], [0, 2, 3], [1, 3, 0], [2, 4, 1], [3, 5, 2], [4, 3, 2]]
    assert multiview.nearest_cameras(straight, k=3, max_distance=0.75) == [[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]
    assert multiview.nearest_cameras(straight, k=2, min_distance=0.75, max_distance=1.0) == [[2], [3], [0, 4], [1, 5], [2], [3]]
    assert multiview.nearest_cameras(straight, k=0) == [[]] * 6 and multiview.nearest_cameras([]) == []
    # a turning track: 20 degrees per camera, so only the adjacent cameras (and, at 40 degrees, nobody else) pass max_angle = 30 degrees
    turning = [camera((0.3 * i * (1 + 0.1 * i), 0.0, 0.3 * i * (1 + 0.1 * i)), math.radians(20.0 * i)) for i in range(4)]      # growing steps: no ties
    assert multiview.nearest_cameras(turning, k=3) == [[1], [0, 2], [1, 3], [2]]
    assert multiview.nearest_cameras(turning, k=3, max_angle=math.radians(45.0)) == [[1, 2], [0, 2, 3], [1, 3, 0], [2, 1]]
    assert multiview.nearest_cameras(turning, k=3, max_angle=math.radians(10.0)) == [[], [], [], []]
    # a stationary pair has no baseline: min_distance = 0 excludes it (the interval is open at its lower end)
    still = [camera((1.0, 0.0, 2.0), 0.1), camera((1.0, 0.0, 2.0), 0.1), camera((1.0, 0.0, 2.4), 0.1)]
    assert multiview.nearest_cameras(still, k=2) == [[2], [2], [0, 1]]
    # matrices are accepted as relative_pose accepts them; anything else is refused
    assert multiview.nearest_cameras([c.world_view_transform for c in straight]) == multiview.nearest_cameras(straight)
    with pytest.raises(ValueError, match="nearest_cameras"):
        multiview.nearest_cameras([torch.eye(3)])
    with pytest.raises(ValueError, match="nearest_cameras"):
        multiview.nearest_cameras(straight, k=-1)
    with pytest.raises(ValueError, match="nearest_cameras"):
        multiview.nearest_cameras(straight, min_distance=2.0, max_distance=1.0)
