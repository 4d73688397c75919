"""Pins tests/multiview_ref.py, the float64 yardstick of the multi-view photometric consistency loss (include/adgs_multiview.h), and the
case generator tests/multiview_cases.py, without a GPU.

The float32 restatement of the reference (dtype=torch.float32: the same chain, every tensor float32) on the generated cases, recorded
here and not asserted: radius 1 (r1_inv_now): L off by 9.7e-5 relative, the gradients by up to 2.2e-3 of their tensor's largest entry;
radius 3 (r3_inv_now): 4.0e-6 and 9.5e-5.  The project's tolerances are 1e-5 and 1e-4: sum a^2 - Sa^2 / T cancels on low-texture patches,
so the kernel carries the per-tap chain and the five sums in double."""
import math

import pytest
import torch

from tests import multiview_cases as cases
from tests import multiview_ref as ref

OBLIQUE = (((0.3 / math.sqrt(1.34), -0.5 / math.sqrt(1.34), -1.0 / math.sqrt(1.34)), -6.0),)      # one plane that every ray of both views hits


def exact_scene(H, W, Hn, Wn, inv_depth, seed=1, radius=3, S=1024):
    pose = cases.neighbour_pose()
    Ir, In, z, n = cases.render_views(H, W, Hn, Wn, cases.TAN, cases.TAN_N, pose, OBLIQUE)
    g = torch.Generator().manual_seed(seed)
    N, D, O = cases.rendered_maps(z, n, inv_depth, g, exact=True)
    return pose, Ir.float(), In.float(), N, D, O, cases.unique_samples(H, W, radius, S, g)


@pytest.mark.parametrize("inv", (True, False), ids=("inv_depth", "depth"))
def test_exact_geometry_is_photometrically_consistent(inv):
    """The true depth and normal of a textured plane: every valid sample has e < 1e-3 (measured: at most 6.2e-4, median 3.5e-6; what
    is left is eps = 1e-8 against Va Vb on the low-texture patches and the bilinear interpolation of the neighbour), which confirms
    the sign convention of the homography; the same maps with the depth off by a factor 1.2 are an order of magnitude worse."""
    pose, Ir, In, N, D, O, s = exact_scene(96, 128, 160, 288, inv)
    res = ref.evaluate(N, D, O, cases.TAN, Ir, In, cases.TAN_N, pose, s, radius=3, inv_depth=inv)
    assert int(res.valid.sum()) >= 0.25 * s.numel()
    e = res.e[res.valid]
    print("exact geometry: %d valid, e median %.2e max %.2e" % (e.numel(), float(e.median()), float(e.max())))
    assert float(e.max()) < 1e-3
    off = ref.evaluate(N, D / 1.2 if inv else D * 1.2, O, cases.TAN, Ir, In, cases.TAN_N, pose, s, radius=3, inv_depth=inv)
    assert float(off.e[off.geo].median()) > 1e-3 > 10 * float(e.median())


def test_tap_positions_are_ray_plane_intersections():
    """(u, v) of every tap = intersect the tap's ray with the plane Nh . X = z c0, move the point to the neighbour's frame, project."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    res, _ = cases.reference(cases.BASE)
    k = res.geo.nonzero().reshape(-1)
    idx = inp.samples.long()[k]
    y0, x0 = idx // c.W, idx % c.W
    R, t = ref.pose12(inp.pose)
    tan, tan_n = tuple(map(ref.f32, cases.TAN)), tuple(map(ref.f32, cases.TAN_N))
    Ns, Ds, Os = inp.N.double().reshape(3, -1)[:, idx].T, inp.D.double().reshape(-1)[idx], inp.O.double().reshape(-1)[idx]
    g = ref.warp(Ns, Ds, Os, x0, y0, (c.H, c.W, c.Hn, c.Wn, tan, tan_n, R, t), c.radius, c.inv_depth)
    assert g["u"].shape == (k.numel(), (2 * c.radius + 1) ** 2) and k.numel() > 500
    z = Os / Ds
    Nh = Ns / Ns.norm(dim=1, keepdim=True)
    r0 = torch.stack([*ref.ray_xy(x0, y0, c.H, c.W, tan), torch.ones(k.numel(), dtype=torch.float64)], dim=1)
    P0 = z[:, None] * r0                                           # the surface point of the centre pixel lies on the plane
    rq = torch.stack([g["rqx"], g["rqy"], torch.ones_like(g["rqx"])], dim=-1)
    lam = (Nh * P0).sum(-1)[:, None] / (rq * Nh[:, None]).sum(-1)
    X = lam[..., None] * rq
    assert float(((X * Nh[:, None]).sum(-1) - (Nh * P0).sum(-1)[:, None]).abs().max()) < 1e-9
    Xn = X @ R.T + t
    u = (Xn[..., 0] / Xn[..., 2]) / tan_n[0] * c.Wn / 2 + (c.Wn - 1) / 2
    v = (Xn[..., 1] / Xn[..., 2]) / tan_n[1] * c.Hn / 2 + (c.Hn - 1) / 2
    assert float((u - g["u"]).abs().max()) < 1e-9 and float((v - g["v"]).abs().max()) < 1e-9
    # row-major over (dy, dx): the middle tap is the sampled pixel itself
    centre = g["u"].shape[1] // 2
    assert torch.equal(g["qx"][:, centre], x0) and torch.equal(g["qy"][:, centre], y0)


def test_autograd_agrees_with_central_differences():
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    res, _ = cases.reference(cases.BASE)
    pick = inp.samples[res.valid][:20].contiguous()
    assert pick.numel() == 20
    args = (cases.TAN, inp.ref_gray, inp.nbr_gray, cases.TAN_N, inp.pose, pick)
    kw = dict(weight=inp.weight, radius=c.radius, inv_depth=c.inv_depth)
    r0, grads = ref.with_grads(inp.N, inp.D, inp.O, *args, **kw)
    assert int(r0.valid.sum()) == 20 and float(ref.near_gate(r0.margins).sum()) == 0
    base = [inp.N.double(), inp.D.double(), inp.O.double()]
    worst = 0.0
    for which, (t, g) in enumerate(zip(base, grads)):
        flat_g = g.reshape(-1)
        scale = float(flat_g.abs().max())
        assert scale > 0
        for p in pick.long().tolist():
            for ch in range(3 if which == 0 else 1):
                j = ch * c.H * c.W + p
                h = 1e-6 * max(abs(float(t.reshape(-1)[j])), 1e-2)
                L = []
                for sgn in (1.0, -1.0):
                    moved = [b.clone() for b in base]
                    moved[which].reshape(-1)[j] += sgn * h
                    L.append(float(ref.evaluate(*moved, *args, **kw).L))
                fd = (L[0] - L[1]) / (2 * h)
                worst = max(worst, abs(fd - float(flat_g[j])) / scale)
    print("autograd against central differences: worst %.2e of the tensor's largest gradient" % worst)
    assert worst < 1e-5
    # nothing but the sampled pixels receives a gradient
    listed = torch.zeros(c.H * c.W, dtype=torch.bool)
    listed[pick.long()] = True
    for g in grads:
        assert not g.reshape(-1, c.H * c.W)[:, ~listed].any()


def test_identity_pose_has_no_error_and_no_gradient():
    """R = I, t = 0 and I_n = I_r: the warp is the identity whatever the plane (t = 0 removes s_k), so e is rounding and the gradients
    are exactly zero."""
    c, inp = cases.BY_NAME[cases.BASE], cases.inputs(cases.BASE)
    pose = torch.eye(4, dtype=torch.float64)[:3]
    res, grads = ref.with_grads(inp.N, inp.D, inp.O, cases.TAN, inp.ref_gray, inp.ref_gray, cases.TAN, pose, inp.samples, radius=c.radius,
                                inv_depth=c.inv_depth)
    assert int(res.valid.sum()) > 0.5 * inp.samples.numel()
    # C = Va = Vb up to rounding, so what is left of e is eps / (Va^2 + eps)
    idx = inp.samples.long()[res.valid]
    dx, dy = ref.tap_offsets(c.radius)
    a = inp.ref_gray.double()[(idx // c.W)[:, None] + dy[None], (idx % c.W)[:, None] + dx[None]]
    Va = (a * a).sum(-1) - a.sum(-1) ** 2 / a.shape[1]
    eps = ref.f32(1e-8)
    assert float((res.e[res.valid] - eps / (Va * Va + eps)).abs().max()) < 1e-9
    assert float(res.e[res.valid].abs().max()) < 1e-4 and abs(float(res.L)) < 1e-4
    for g in grads:
        assert not g.any()


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_cases_keep_away_from_the_gates(name):
    """At most 2 % of a case's samples are within 1e-3 of a gate (and dropped); at least 25 % of the rest are valid; the thinned
    list has no sample near a gate."""
    c, inp = cases.BY_NAME[name], cases.inputs(name)
    res, grads = cases.reference(name)
    kept = inp.samples.numel()
    assert kept + inp.dropped == c.S and inp.dropped <= 0.02 * c.S
    assert not ref.near_gate(res.margins).any()
    assert int(res.valid.sum()) >= 0.25 * kept and int(res.valid.sum()) >= 1
    assert torch.unique(inp.samples).numel() == kept
    assert float(res.L) > 0 and all(float(g.abs().max()) > 0 for g in grads)
    if c.S >= 257:                                                 # the gates that the generator can reach are reached
        m = res.margins
        assert int((m[:, 0] < 0).sum()) > 0 and int((m[:, 1] < 0).sum()) > 0 and int((m[:, 2] < 0).sum()) > 0
    if c.max_error < 0.5:
        assert int((res.geo & ~res.valid).sum()) >= 20             # the error gate decides


def test_float32_restatement_is_recorded():
    for name in ("r1_inv_now", "r3_inv_now"):
        eL, eg = cases.float32_errors(name)
        print("float32 restatement on %s: L off by %.1e relative, gradients by up to %.1e of max |ref|" % (name, eL, eg))
        assert math.isfinite(eL) and math.isfinite(eg)
