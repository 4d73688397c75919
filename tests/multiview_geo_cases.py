"""Inputs of tests/test_gpu_multiview_geo.py and tests/test_multiview_geo_ref.py, generated on the CPU with seeded generators.

The scene is the one of tests/multiview_cases.py: a ground plane 1.5 m below the reference camera and a wall across the road, seen from
both cameras by exact ray-plane intersection; the neighbour is 0.35 m ahead with 0.02 rad of yaw and has its own size and field of view.
Both views get the rendered maps of that file's `rendered_maps`, without the normal: the true depth with multiplicative noise (10 %, or
3 % at the larger size, so that the reprojection error straddles max_pixel_error), an opacity in [0.55, 1] with 5 % of the pixels at 0.3.

The margin rule: a weighted case's weight is zero at every pixel within 1e-3 of a gate (tests/multiview_geo_ref.py), so the float64
reference and the kernel cannot disagree where it counts; err_out and weight_out are compared outside those pixels only.  The unweighted
cases use a seed and a max_pixel_error placed in a gap of their own error distribution, with which no pixel at all is near a gate.  At
most 2 % of a case's pixels may be near a gate and at least 25 % must be valid (asserted for every case by
tests/test_multiview_geo_ref.py)."""
import collections
import functools

import torch

from tests import multiview_geo_ref as ref
from tests.multiview_cases import PLANES, TAN, TAN_N, intersect, make_weight, neighbour_pose, pixel_rays

Case = collections.namedtuple("Case", "name H W Hn Wn inv_depth weighted seed noise max_pixel_error")
SMALL, SMALL_N = (48, 64), (40, 72)
CASES = (
    Case("inv_w", *SMALL, *SMALL_N, True, True, 1, 0.10, 1.0),
    Case("lin_w", *SMALL, *SMALL_N, False, True, 2, 0.10, 1.0),
    Case("inv_now", *SMALL, *SMALL_N, True, False, 1, 0.10, 0.9529),        # the seed and the threshold: see find_gap()
    Case("lin_now", *SMALL, *SMALL_N, False, False, 1, 0.10, 0.9529),
    Case("odd", 45, 61, *SMALL_N, True, True, 5, 0.10, 1.0),              # not a multiple of the 32 x 8 tile
    Case("many_blocks", 272, 512, *SMALL_N, True, True, 6, 0.03, 1.0),    # 16 x 34 = 544 workgroups on 256 slot rows
    Case("big_nbr", 24, 32, 160, 288, True, True, 7, 0.10, 1.0),          # a tile's footprint exceeds the LDS window: direct atomics
    Case("dense", 96, 128, 12, 16, True, True, 8, 0.10, 1.0),             # ~64 reference pixels add into each neighbour pixel
    Case("tight", *SMALL, *SMALL_N, True, True, 9, 0.10, None),           # max_pixel_error = the median of the error distribution
)
BY_NAME = {c.name: c for c in CASES}
BASE = "inv_w"
Inputs = collections.namedtuple("Inputs", "D O Dn On weight pose max_pixel_error near")


def true_depths(H, W, Hn, Wn, pose, planes=PLANES):
    """(z [H, W], z_n [Hn, Wn]) in float64: the depth of the nearest plane along every pixel ray of the two cameras, each in its own frame."""
    R, t = pose[:, :3], pose[:, 3]
    X, _ = intersect(torch.zeros(3, dtype=torch.float64), pixel_rays(H, W, TAN), planes)
    Xn, _ = intersect(-R.T @ t, pixel_rays(Hn, Wn, TAN_N) @ R, planes)            # points in the reference frame
    return X[..., 2], (Xn @ R.T + t)[..., 2]


def rendered_depth(z, inv_depth, g, noise):
    """float32 (D, O) as the rasterizer would render the true depth z: the opacity distribution of multiview_cases.rendered_maps."""
    H, W = z.shape
    O = 0.55 + 0.45 * torch.rand(H, W, generator=g, dtype=torch.float64)
    O = torch.where(torch.rand(H, W, generator=g) < 0.05, torch.full_like(O, 0.3), O)
    zr = z * (1 + noise * torch.randn(H, W, generator=g, dtype=torch.float64)) if noise else z
    D = O / zr if inv_depth else O * zr
    return D.float(), O.float()


def raw_inputs(c, seed=None):
    g = torch.Generator().manual_seed(9000 + (c.seed if seed is None else seed))
    pose = neighbour_pose()
    z, zn = true_depths(c.H, c.W, c.Hn, c.Wn, pose)
    D, O = rendered_depth(z, c.inv_depth, g, c.noise)
    Dn, On = rendered_depth(zn, c.inv_depth, g, c.noise)
    weight = make_weight(c.H, c.W, g) if c.weighted else None
    return D, O, Dn, On, weight, pose


def evaluate(inp, c, **kw):
    return ref.evaluate(inp.D, inp.O, TAN, inp.Dn, inp.On, TAN_N, inp.pose, weight=inp.weight, inv_depth=c.inv_depth,
                        max_pixel_error=inp.max_pixel_error, **kw)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The float32 inputs of a case; `near` [H, W]: the pixels within 1e-3 of a gate, where a weighted case's weight is zero."""
    c = BY_NAME[name]
    D, O, Dn, On, weight, pose = raw_inputs(c)
    mpe = c.max_pixel_error
    if mpe is None:                                                       # tight: the median error of the pixels that pass every other gate
        r = ref.evaluate(D, O, TAN, Dn, On, TAN_N, pose, inv_depth=c.inv_depth, max_pixel_error=1e6)
        mpe = ref.f32(float(r.err[r.geo].median()))
    near = ref.near_gate(ref.evaluate(D, O, TAN, Dn, On, TAN_N, pose, inv_depth=c.inv_depth, max_pixel_error=mpe).margins)
    if weight is not None:
        weight = torch.where(near, torch.zeros_like(weight), weight)
    return Inputs(D, O, Dn, On, weight, pose, mpe, near)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    """(Result, [gD, gO, gDn, gOn]) of the reference on a case: computed once, shared, never modified."""
    c, inp = BY_NAME[name], inputs(name)
    return ref.with_grads(inp.D, inp.O, TAN, inp.Dn, inp.On, TAN_N, inp.pose, weight=inp.weight, inv_depth=c.inv_depth,
                          max_pixel_error=inp.max_pixel_error, dtype=dtype)


def find_gap(c, seeds=range(1, 200)):
    """How the unweighted cases were chosen: the first seed with no pixel within 1e-3 of any gate but the last, and the threshold in
    the middle of the widest gap of its sorted errors inside [0.8, 1.2] -> (seed, max_pixel_error, half the gap)."""
    for seed in seeds:
        D, O, Dn, On, _, pose = raw_inputs(c, seed)
        r = ref.evaluate(D, O, TAN, Dn, On, TAN_N, pose, inv_depth=c.inv_depth, max_pixel_error=1e6)
        if ref.near_gate(r.margins[..., :5]).any():
            continue
        e = r.err[r.geo].sort().values
        e = e[(e > 0.8) & (e < 1.2)]
        if e.numel() < 2:
            continue
        gaps = e[1:] - e[:-1]
        i = int(gaps.argmax())
        return seed, round(float(e[i] + e[i + 1]) / 2, 4), float(gaps[i]) / 2
    return None
