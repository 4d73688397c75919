"""The 3D smoothing filter of Mip-Splatting (include/adgs_filter3d.h) restated in torch, dtype-generic: evaluated in float64 it is the
reference of tests/test_gpu_filter3d.py, in float32 (on the CPU) the yardstick its tolerances are measured with.

Written from the paper (Yu et al., CVPR 2024, section 4.1) and the header's definition.  The seen-gates (z > 0.2, the 15 % image
margin) are hard thresholds on computed values: `rates` classifies every (row, camera) gate decision as firm or MARGINAL -- the
compared quantity lies within MARGIN x (the magnitudes of its terms, summed) of its threshold -- and returns the rate over the
firmly seeing cameras (rate_lo) and over the firm plus marginal ones (rate_hi); a correct float32 evaluation lies between them."""
import math

import torch

SQRT02 = math.sqrt(0.2)
MARGIN = 1e-5
CAMERA_KINDS = ((60.0, 60.0, 64.0, 48.0), (110.0, 100.0, 96.0, 80.0))      # (fx, fy, W, H): two focal lengths, two image sizes


def random_cameras(n, seed, kinds=CAMERA_KINDS):
    """[n, 16] float32 records (R row-major, t, fx, fy, W, H): random rigid poses with the centre in [-3, 3]^3."""
    g = torch.Generator().manual_seed(1000 + int(seed))
    recs = torch.zeros(n, 16, dtype=torch.float64)
    for i in range(n):
        q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        q = q * torch.sign(torch.diagonal(r))[None, :]
        if torch.det(q) < 0:
            q[:, 2] = -q[:, 2]
        centre = torch.rand(3, generator=g, dtype=torch.float64) * 6 - 3
        recs[i, :9] = q.reshape(-1)
        recs[i, 9:12] = -(q @ centre)
        recs[i, 12:] = torch.tensor(kinds[i % len(kinds)], dtype=torch.float64)
    return recs.float()


def random_points(P, seed, recs):
    """[P, 3] float32 in [-8, 8]^3 (about half of them behind any given camera, most of the rest outside its margin), with four
    planted rows (P >= 4) relative to camera 0: behind it, nearer than 0.2, outside the 15 % margin, in the image centre."""
    g = torch.Generator().manual_seed(int(seed))
    xyz = torch.rand(P, 3, generator=g, dtype=torch.float64) * 16 - 8
    if P >= 4:
        c = recs[0].double()
        R, t = c[:9].reshape(3, 3), c[9:12]
        local = torch.tensor([[0.1, 0.1, -2.0], [0.01, 0.0, 0.1], [2.5 * float(c[14]) / float(c[12]), 0.0, 3.0], [0.0, 0.0, 3.0]], dtype=torch.float64)
        xyz[:4] = (local - t) @ R          # R^T (p_cam - t), row-vector form
    return xyz.float()


def camera_space(xyz, recs):
    """x, y, z [P, C] in the header's order of operations, and the summed magnitudes of their terms."""
    R, t = recs[:, :9].reshape(-1, 3, 3), recs[:, 9:12]
    px, py, pz = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    axis = lambda i: ((R[:, i, 0] * px + R[:, i, 1] * py) + R[:, i, 2] * pz) + t[:, i]
    mag = lambda i: (R[:, i, 0] * px).abs() + (R[:, i, 1] * py).abs() + (R[:, i, 2] * pz).abs() + t[:, i].abs()
    return [axis(i) for i in range(3)], [mag(i) for i in range(3)]


def rate(xyz, recs):
    """The definition, literally, in the dtype of its inputs: [P]."""
    if recs.shape[0] == 0:
        return torch.zeros(xyz.shape[0], dtype=xyz.dtype)
    (x, y, z), _ = camera_space(xyz, recs)
    fx, fy, W, H = recs[:, 12], recs[:, 13], recs[:, 14], recs[:, 15]
    zc = z.clamp(min=0.001)
    u, v = x / zc * fx + W / 2, y / zc * fy + H / 2
    seen = (z > 0.2) & (u >= -0.15 * W) & (u <= 1.15 * W) & (v >= -0.15 * H) & (v <= 1.15 * H)
    return torch.where(seen, fx / z, torch.zeros_like(z)).amax(dim=1)


def rates(xyz, recs, margin=MARGIN):
    """float64: dict(rate_lo, rate_hi [P], outcomes = {gate: (pairs that pass, pairs that fail)}, marginal_pairs)."""
    xyz, recs = xyz.double(), recs.double()
    (x, y, z), (mx, my, mz) = camera_space(xyz, recs)
    fx, fy, W, H = recs[:, 12], recs[:, 13], recs[:, 14], recs[:, 15]
    zc = z.clamp(min=0.001)
    passes, marginal, outcomes = [], [], {}

    def gate(name, value, thr, upper, mag):
        ok = value <= thr if upper else value >= thr
        passes.append(ok)
        marginal.append((value - thr).abs() <= margin * (mag + thr.abs()))
        outcomes[name] = (int(ok.sum()), int((~ok).sum()))

    ok_z = z > 0.2
    passes.append(ok_z)
    marginal.append((z - 0.2).abs() <= margin * (mz + 0.2))
    outcomes["behind"] = (int((z > 0).sum()), int((z <= 0).sum()))
    outcomes["near"] = (int(ok_z.sum()), int(((z > 0) & ~ok_z).sum()))
    for name, a, ma, f, n in (("u", x, mx, fx, W), ("v", y, my, fy, H)):
        val = a / zc * f + n / 2
        mag = ma * f / zc + (a * f / zc).abs() * (mz / zc) + n / 2          # the terms of a, and of zc through the quotient
        gate(name + "_lo", val, (-0.15 * n).expand_as(val), False, mag)
        gate(name + "_hi", val, (1.15 * n).expand_as(val), True, mag)
    firm = torch.ones_like(ok_z)
    possible = torch.ones_like(ok_z)
    any_marginal = torch.zeros_like(ok_z)
    for ok, mg in zip(passes, marginal):
        firm &= ok & ~mg
        possible &= ok | mg
        any_marginal |= mg
    r = fx / z
    zero = torch.zeros_like(z)
    return dict(rate_lo=torch.where(firm, r, zero).amax(dim=1), rate_hi=torch.where(possible, r, zero).amax(dim=1), outcomes=outcomes,
                marginal_pairs=int((any_marginal & possible).sum()))


def float32_rate_error(xyz, recs, lo_hi):
    """Largest relative error of the float32 evaluation of `rate` against float64, over the rows whose gates are all firm."""
    r32, r64 = rate(xyz.float(), recs.float()).double(), rate(xyz.double(), recs.double())
    firm = (lo_hi["rate_lo"] == lo_hi["rate_hi"]) & (r64 > 0)
    assert torch.equal(r64[firm], lo_hi["rate_lo"][firm])
    return float(((r32 - r64).abs() / r64)[firm].max()) if bool(firm.any()) else 0.0


def filter_from_rate(r):
    """[P] rates -> [P] filter sizes (any dtype)."""
    seen = r > 0
    if not bool(seen.any()):
        return torch.zeros_like(r)
    return torch.where(seen, SQRT02 / r.clamp(min=1e-300 if r.dtype == torch.float64 else 1e-37), SQRT02 / r[seen].min())


def apply_forward(s, o, f):
    """scales [P,3], opacity [P,1], filter [P,1] -> (S [P,3], O [P,1]), the coefficient as a product of three ratios."""
    f2 = f * f
    q = s * s
    d = q + f2
    ratio = q / d
    return torch.sqrt(d), o * torch.sqrt((ratio[:, 0:1] * ratio[:, 1:2]) * ratio[:, 2:3])


def apply_backward(s, o, f, gS, gO):
    """The header's analytic backward: (dL/ds [P,3], dL/do [P,1])."""
    f2 = f * f
    q = s * s
    d = q + f2
    ratio = q / d
    coef = torch.sqrt((ratio[:, 0:1] * ratio[:, 1:2]) * ratio[:, 2:3])
    return gS * (s / torch.sqrt(d)) + (gO * (o * coef)) * (f2 / (s * d)), gO * coef


def make_apply_case(P, seed):
    """float32 inputs: scales log-uniform in [1e-4, 10], filters from {0, 1e-3, 0.3} mixed per row, opacity in (0, 1), upstream gradients."""
    g = torch.Generator().manual_seed(5000 + int(seed))
    s = torch.exp(torch.rand(P, 3, generator=g, dtype=torch.float64) * (math.log(10.0) - math.log(1e-4)) + math.log(1e-4)).float()
    o = (torch.rand(P, 1, generator=g, dtype=torch.float64) * 0.998 + 0.001).float()
    f = torch.tensor([0.0, 1e-3, 0.3])[torch.randint(0, 3, (P, 1), generator=g)].float()
    if P >= 3:
        f[:3, 0] = torch.tensor([0.0, 1e-3, 0.3])
    gS = torch.randn(P, 3, generator=g, dtype=torch.float64).float()
    gO = torch.randn(P, 1, generator=g, dtype=torch.float64).float()
    return s, o, f, gS, gO
