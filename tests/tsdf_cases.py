"""Inputs of tests/test_gpu_tsdf.py and tests/test_tsdf_ref.py, generated on the CPU with seeded generators.

Integration: the scene of tests/multiview_cases.py (a ground plane 1.5 m below the first camera and a wall at z = 8, exact ray-plane
depths) seen by four cameras -- the identity; two oblique ones beside it; one that stands INSIDE the volume, so that part of the lattice
is behind it -- at 36 x 48 with TAN, fused into a 41 x 17 x 38 lattice at (-4, -1, 2) with 0.2 m voxels and trunc 0.6.  The opacity lies in
[0.55, 1] with 5 % of the pixels at 0.3 (below min_opacity), the weight has exact zeros and zeroed bottom rows.  The variants: both
inv_depth settings, with and without image, with and without weight, max_weight = 1.5 (the clamp acts from the second view on),
max_depth = 6 (the wall is cut).

The condition every case must meet (tests/test_tsdf_ref.py): per view at most 0.5 % of the lattice is flagged as near a gate
(tests/tsdf_ref.py) and at least 15 % is updated.

Extraction: host-made float32 volumes (the analytic sphere and others), which both sides see bit for bit.

End to end: exact depths of the sphere from six cameras around it."""
import collections
import functools
import math

import numpy as np
import torch

from tests import tsdf_ref as ref
from tests.multiview_cases import PLANES, TAN, intersect, make_weight, pixel_rays

DIMS, ORIGIN, VOXEL, TRUNC = (41, 17, 38), (-4.0, -1.0, 2.0), 0.2, 0.6
H, W = 36, 48
Case = collections.namedtuple("Case", "name inv_depth image weighted max_weight max_depth")
CASES = (Case("base", True, True, True, 64.0, math.inf), Case("lin", False, True, True, 64.0, math.inf),
         Case("noimage", True, False, True, 64.0, math.inf), Case("noweight", True, True, False, 64.0, math.inf),
         Case("clamp", True, True, True, 1.5, math.inf), Case("maxdepth", False, False, False, 64.0, 6.0))
BY_NAME = {c.name: c for c in CASES}
BASE = "base"
# (yaw, pitch, centre)
CAMERAS = ((0.0, 0.0, (0.0, 0.0, 0.0)), (0.31, 0.05, (-1.3, 0.1, 0.4)), (-0.27, -0.04, (1.1, -0.2, 0.9)), (0.13, 0.21, (0.4, -0.6, 3.1)))


def camera_pose(yaw, pitch, centre):
    """[3, 4] float64 (R | t), world to camera: a camera at `centre` turned by `yaw` about y, then by `pitch` about its x."""
    c, s = math.cos(yaw), math.sin(yaw)
    Ry = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    c, s = math.cos(pitch), math.sin(pitch)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    R = Rx @ Ry
    return np.concatenate([R, (-R @ np.array(centre, dtype=np.float64))[:, None]], axis=1)


def look_at(centre, target):
    """[3, 4] float64 (R | t) of a camera at `centre` whose z axis points at `target`."""
    centre, target = np.array(centre, np.float64), np.array(target, np.float64)
    f = (target - centre) / np.linalg.norm(target - centre)
    hint = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(hint, f)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(f, x), f])
    return np.concatenate([R, (-R @ centre)[:, None]], axis=1)


View = collections.namedtuple("View", "D O image weight pose")


def plane_depth(pose, h, w, tan):
    """The exact z-depth [h, w] float64 of the planes from a camera."""
    R, t = torch.from_numpy(pose[:, :3]), torch.from_numpy(pose[:, 3])
    X, _ = intersect(-R.T @ t, pixel_rays(h, w, tan) @ R, PLANES)
    return ((X @ R.T) + t)[..., 2].numpy()


def rendered(z, inv_depth, g, hit=None):
    """float32 (D, O) as the rasterizer would render the depth z: O in [0.55, 1] with 5 % of the pixels at 0.3; O = D = 0 where not hit."""
    h, w = z.shape
    O = 0.55 + 0.45 * torch.rand(h, w, generator=g, dtype=torch.float64).numpy()
    O = np.where(torch.rand(h, w, generator=g).numpy() < 0.05, 0.3, O)
    if hit is not None:
        O = np.where(hit, O, 0.0)
        z = np.where(hit, z, 1.0)
    D = O / z if inv_depth else O * z
    return D.astype(np.float32), O.astype(np.float32)


@functools.lru_cache(maxsize=None)
def views(name):
    """The four float32 views of a case."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(9100 + CASES.index(c))
    out = []
    for cam in CAMERAS:
        pose = camera_pose(*cam)
        D, O = rendered(plane_depth(pose, H, W, TAN), c.inv_depth, g)
        image = torch.rand(3, H, W, generator=g).numpy() if c.image else None
        weight = make_weight(H, W, g).numpy() if c.weighted else None
        out.append(View(D, O, image, weight, pose))
    return tuple(out)


def integrate_kwargs(name):
    c = BY_NAME[name]
    return dict(inv_depth=c.inv_depth, min_opacity=0.5, near=0.2, max_depth=c.max_depth)


def new_volume(name, dims=DIMS, origin=ORIGIN):
    return ref.Volume(origin, VOXEL, dims, color=BY_NAME[name].image)


def fuse(name, vol):
    """Applies the case's views to `vol` in sequence -> [(volume after the view, updated, flagged)]."""
    c = BY_NAME[name]
    steps = []
    for v in views(name):
        upd, flagged = ref.integrate(vol, v.D, v.O, TAN, v.pose, image=v.image, weight=v.weight, trunc=TRUNC, max_weight=c.max_weight,
                                     **integrate_kwargs(name))
        steps.append((vol.copy(), upd, flagged))
    return steps


@functools.lru_cache(maxsize=None)
def reference(name, dims=DIMS):
    """The float64 reference of a case from the empty volume: computed once, shared, never modified."""
    return tuple(fuse(name, new_volume(name, dims)))


# ---- extraction volumes ----

SPHERE_DIMS, SPHERE_C, SPHERE_R = (20, 18, 13), (9.37, 8.61, 6.13), 4.7


def sphere_volume(color=False):
    """tsdf = clip((dist - r) / 3, -1, 1) in float32 on a unit lattice at 0, every weight 1."""
    v = ref.Volume((0.0, 0.0, 0.0), 1.0, SPHERE_DIMS, color=color)
    dist = np.linalg.norm(v.points() - np.array(SPHERE_C), axis=-1)
    v.tsdf = np.clip((dist - SPHERE_R) / 3.0, -1.0, 1.0).astype(np.float32)
    v.wsum[:] = 1.0
    if color:
        v.color = np.random.default_rng(5).random(v.color.shape, dtype=np.float32)
    return v


def plane_volume(dims, normal, offset, origin=(0.3, -1.7, 2.1), voxel=0.25, color=False):
    """tsdf = clip(n . (i, j, k) - offset, -1, 1) in lattice units, float32; every weight 1."""
    v = ref.Volume(origin, voxel, dims, color=color)
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v.tsdf = np.clip(normal[0] * i + normal[1] * j + normal[2] * k - offset, -1.0, 1.0).astype(np.float32)
    v.wsum[:] = 1.0
    if color:
        v.color = np.random.default_rng(6).random(v.color.shape, dtype=np.float32)
    return v


@functools.lru_cache(maxsize=None)
def extraction_volume(name):
    """-> (volume, min_weight): the volumes of the extraction tests."""
    if name == "sphere":
        return sphere_volume(), 1.0
    if name == "sphere_color":
        return sphere_volume(color=True), 1.0
    if name == "slanted_300x5x4":                               # cuts every chunk of 256 points: vertex ids across chunks in x, y and z
        return plane_volume((300, 5, 4), (0.013, 0.37, 0.41), 2.05), 1.0
    if name == "half_unseen":                                   # a boundary: the half space i >= 11 was never observed
        v = sphere_volume()
        v.wsum[:, :, 11:] = 0.0
        return v, 1.0
    if name == "min_weight":                                    # min_weight above some of the weights
        v = sphere_volume(color=True)
        v.wsum = (4.0 * np.random.default_rng(7).random(v.wsum.shape)).astype(np.float32)
        return v, 0.8
    if name == "exact_zeros":                                   # a plane through lattice points: tsdf = 0 there, which is outside
        v = plane_volume((9, 8, 7), (0.5, 0.0, 0.25), 2.0, origin=(0.0, 0.0, 0.0), voxel=0.5)
        assert (v.tsdf == 0).sum() > 20
        return v, 1.0
    if name == "all_positive":
        v = sphere_volume()
        v.tsdf = np.abs(v.tsdf) + np.float32(0.01)
        return v, 1.0
    if name == "fused_base":                                    # the reference's fused volume of the base case, with colour
        return reference(BASE)[-1][0], 1.0
    raise KeyError(name)


EXTRACTION = ("sphere", "sphere_color", "slanted_300x5x4", "half_unseen", "min_weight", "exact_zeros", "all_positive", "fused_base")


@functools.lru_cache(maxsize=None)
def extraction_reference(name):
    vol, mw = extraction_volume(name)
    return ref.extract(vol, mw)


# ---- end to end: the sphere from six cameras ----

E2E_HW, E2E_TAN, E2E_TRUNC = (40, 40), (0.5, 0.5), 3.0
E2E_DIRS = ((1.0, 0.13, 0.07), (-1.0, 0.21, -0.11), (0.09, 1.0, 0.17), (-0.15, -1.0, 0.05), (0.12, -0.08, 1.0), (0.19, 0.06, -1.0))


@functools.lru_cache(maxsize=None)
def sphere_views():
    """Six views of the sphere from 13 units away: exact depth where the ray hits it, O = D = 0 elsewhere (inv_depth)."""
    g = torch.Generator().manual_seed(9200)
    c = np.array(SPHERE_C)
    out = []
    for d in E2E_DIRS:
        d = np.array(d) / np.linalg.norm(d)
        pose = look_at(c + 13.0 * d, c)
        R, t = pose[:, :3], pose[:, 3]
        rays = pixel_rays(*E2E_HW, E2E_TAN).numpy() @ R          # world directions, camera z component 1
        oc = -R.T @ t - c
        a, b, cc = (rays * rays).sum(-1), 2 * (rays @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * cc
        hit = disc > 0
        tau = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a)   # the camera-frame z of the first hit
        D, O = rendered(tau, True, g, hit=hit)
        out.append(View(D, O, None, None, pose))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sphere_fused():
    """-> (the reference's fused volume, the union of the views' flags)."""
    vol = ref.Volume((0.0, 0.0, 0.0), 1.0, SPHERE_DIMS, color=False)
    flags = np.zeros(vol.tsdf.shape, bool)
    for v in sphere_views():
        _, f = ref.integrate(vol, v.D, v.O, E2E_TAN, v.pose, trunc=E2E_TRUNC, max_weight=64.0, inv_depth=True, min_opacity=0.5, near=0.2)
        flags |= f
    return vol, flags
