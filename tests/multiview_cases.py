"""Inputs of tests/test_gpu_multiview.py and tests/test_multiview_ref.py, generated on the CPU with seeded generators.

The scene: textured planes in the reference camera's frame -- a ground plane 1.5 m below the camera and a wall across the road -- whose
grey value is a sum of sinusoids of the 3D point, seen from both cameras by exact ray-plane intersection (nearest hit).  The neighbour is
0.35 m ahead with 0.02 rad of yaw and has its own size and field of view.  The rendered maps are the true depth with 1 % noise, the true
normal with 0.05 noise and a random length, an opacity in [0.55, 1] with 5 % of the pixels at 0.3, and 3 % of the pixels with a random
normal (grazing or back-facing planes: the cosine gate, taps behind the neighbour or outside its image, errors near 1).

The margin rule: a case drops, before use, every sample whose margin to any gate (tests/multiview_ref.py) is below 1e-3, so that the
float64 reference and the kernel cannot disagree on a validity; at most 2 % of a case's samples may be dropped and at least 25 % of what
remains must be valid (asserted for every case by tests/test_multiview_ref.py)."""
import collections
import functools
import math

import torch

from tests import multiview_ref as ref

PLANES = (((0.0, -1.0, 0.0), -1.5), ((0.0, 0.0, -1.0), -8.0))          # (n, d): n . X = d, n facing the camera
TAN, TAN_N = (0.7, 0.5), (0.78, 0.46)
SMALL, SMALL_N = (48, 64), (40, 72)
Case = collections.namedtuple("Case", "name H W Hn Wn S radius inv_depth weighted seed max_error")
Case.__new__.__defaults__ = (0.9,)
CASES = tuple(Case("r%d_%s_%s" % (r, "inv" if inv else "lin", "w" if wt else "now"), *SMALL, *SMALL_N, 1024, r, inv, wt, 10 * r + 2 * inv + wt)
              for r in (1, 2, 3) for inv in (True, False) for wt in (False, True)) + \
    tuple(Case("S%d" % S, *SMALL, *SMALL_N, S, 3, True, False, 100 + S) for S in (1, 3, 257)) + \
    (Case("many_blocks", 96, 96, 96, 96, 9000, 1, True, True, 200),           # 2250 groups of four samples: past the 2048-workgroup cap, eight adds per slot row
     Case("tight_error", *SMALL, *SMALL_N, 1024, 2, True, True, 300, 0.01))    # the last gate decides: e < max_error splits the samples
BY_NAME = {c.name: c for c in CASES}
BASE = "r3_inv_w"


def neighbour_pose(forward=0.35, yaw=0.02):
    """[3, 4] float64 (R | t), X_n = R X_r + t: the neighbour `forward` metres ahead along z, turned by `yaw` about y."""
    c, s = math.cos(yaw), math.sin(yaw)
    R = torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], dtype=torch.float64)
    centre = torch.tensor([0.0, 0.0, forward], dtype=torch.float64)       # the neighbour's centre in the reference frame
    return torch.cat([R, (-R @ centre)[:, None]], dim=1)


def texture(X):
    """The grey value of the 3D points X [..., 3] (reference frame), in (0, 1)."""
    waves = ((1.9, 0.3, 0.7, 0.0), (-0.6, 1.1, 1.7, 1.0), (2.9, -2.3, 0.4, 2.0), (0.5, 3.1, -1.3, 0.5), (4.3, 0.9, 2.6, 4.0))
    amps = (0.16, 0.12, 0.08, 0.07, 0.04)
    out = torch.full(X.shape[:-1], 0.5, dtype=torch.float64)
    for (kx, ky, kz, ph), a in zip(waves, amps):
        out = out + a * torch.sin(kx * X[..., 0] + ky * X[..., 1] + kz * X[..., 2] + ph)
    return out


def pixel_rays(H, W, tan):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    rx, ry = ref.ray_xy(x, y, H, W, tan)
    return torch.stack([rx, ry, torch.ones_like(rx)], dim=-1)


def intersect(origin, dirs, planes=PLANES):
    """Nearest hit of the rays origin + tau dirs [..., 3] with the planes: (X [..., 3], index of the plane [...])."""
    best = torch.full(dirs.shape[:-1], float("inf"), dtype=torch.float64)
    which = torch.zeros(dirs.shape[:-1], dtype=torch.long)
    for i, (n, d) in enumerate(planes):
        n = torch.tensor(n, dtype=torch.float64)
        tau = (d - (n * origin).sum()) / (dirs * n).sum(-1)
        hit = (tau > 0) & (tau < best)
        best = torch.where(hit, tau, best)
        which = torch.where(hit, torch.full_like(which, i), which)
    assert bool(torch.isfinite(best).all())
    return origin + best[..., None] * dirs, which


def render_views(H, W, Hn, Wn, tan, tan_n, pose, planes=PLANES):
    """(I_r [H, W], I_n [Hn, Wn], z [H, W], n [3, H, W]) in float64: both grey images, and the true depth and normal of the reference."""
    R, t = pose[:, :3], pose[:, 3]
    rays = pixel_rays(H, W, tan)
    X, which = intersect(torch.zeros(3, dtype=torch.float64), rays, planes)
    normals = torch.tensor([p[0] for p in planes], dtype=torch.float64)[which].permute(2, 0, 1)
    Xn, _ = intersect(-R.T @ t, pixel_rays(Hn, Wn, tan_n) @ R, planes)      # rows of (rays @ R) are R^T ray
    return texture(X), texture(Xn), X[..., 2], normals


Inputs = collections.namedtuple("Inputs", "N D O ref_gray nbr_gray weight pose samples dropped")


def rendered_maps(z, n, inv_depth, g, exact=False):
    """float32 (N, D, O) as the rasterizer would render the true depth z and normal n."""
    H, W = z.shape
    O = 0.55 + 0.45 * torch.rand(H, W, generator=g, dtype=torch.float64)
    O = torch.where(torch.rand(H, W, generator=g) < 0.05, torch.full_like(O, 0.3), O)
    zr = z if exact else z * (1 + 0.01 * torch.randn(H, W, generator=g, dtype=torch.float64))
    nr = n if exact else n + 0.05 * torch.randn(3, H, W, generator=g, dtype=torch.float64)
    if not exact:
        wild = torch.rand(H, W, generator=g) < 0.03
        nr = torch.where(wild[None], torch.randn(3, H, W, generator=g, dtype=torch.float64), nr)
    N = nr * (0.3 + 1.2 * torch.rand(H, W, generator=g, dtype=torch.float64)) * O
    D = O / zr if inv_depth else O * zr
    return N.float(), D.float(), O.float()


def make_weight(H, W, g):
    """A fractional weight with exact zeros: the ego vehicle's rows at the bottom and a tenth of the pixels."""
    w = torch.rand(H, W, generator=g)
    w[torch.rand(H, W, generator=g) < 0.1] = 0
    w[H - H // 8:] = 0
    return w


def unique_samples(H, W, radius, S, g):
    """S unique int32 indices of pixels at least `radius` from the border."""
    ys, xs = torch.meshgrid(torch.arange(radius, H - radius), torch.arange(radius, W - radius), indexing="ij")
    cand = (ys * W + xs).reshape(-1)
    return cand[torch.randperm(cand.numel(), generator=g)[:S]].to(torch.int32)


def evaluate(inp, case, samples=None, **kw):
    """tests/multiview_ref.evaluate of a case's inputs."""
    return ref.evaluate(inp.N, inp.D, inp.O, TAN, inp.ref_gray, inp.nbr_gray, TAN_N, inp.pose, inp.samples if samples is None else samples,
                        weight=inp.weight, radius=case.radius, inv_depth=case.inv_depth, max_error=case.max_error, **kw)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The float32 inputs of a case, its samples already thinned by the margin rule; `dropped` counts what the rule took."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(7000 + c.seed)
    pose = neighbour_pose()
    Ir, In, z, n = render_views(c.H, c.W, c.Hn, c.Wn, TAN, TAN_N, pose)
    N, D, O = rendered_maps(z, n, c.inv_depth, g)
    weight = make_weight(c.H, c.W, g) if c.weighted else None
    interior = (c.H - 2 * c.radius) * (c.W - 2 * c.radius)
    samples = unique_samples(c.H, c.W, c.radius if interior >= c.S else 0, c.S, g)      # many_blocks: border pixels too (invalid samples)
    inp = Inputs(N, D, O, Ir.float(), In.float(), weight, pose, samples, 0)
    near = ref.near_gate(evaluate(inp, c).margins)
    return inp._replace(samples=samples[~near].contiguous(), dropped=int(near.sum()))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Result, [gN, gD, gO]) of the float64 reference on a case: computed once, shared, never modified."""
    c, inp = BY_NAME[name], inputs(name)
    return ref.with_grads(inp.N, inp.D, inp.O, TAN, inp.ref_gray, inp.nbr_gray, TAN_N, inp.pose, inp.samples, weight=inp.weight, radius=c.radius,
                          inv_depth=c.inv_depth, max_error=c.max_error)


def float32_errors(name):
    """What the float32 restatement holds on a case: (|L32 - L64| / |L64|, the largest of the three gradients' max |g32 - g64| / max |g64|)."""
    c, inp = BY_NAME[name], inputs(name)
    r64, g64 = reference(name)
    r32, g32 = ref.with_grads(inp.N, inp.D, inp.O, TAN, inp.ref_gray, inp.nbr_gray, TAN_N, inp.pose, inp.samples, weight=inp.weight, radius=c.radius,
                              inv_depth=c.inv_depth, max_error=c.max_error, dtype=torch.float32)
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))
    return abs(float(r32.L) - float(r64.L)) / abs(float(r64.L)), max(rel(a, b) for a, b in zip(g32, g64))
