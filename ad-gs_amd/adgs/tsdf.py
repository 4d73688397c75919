"""From the trained model to a surface (include/adgs_tsdf.h): fuse rendered depth maps into a dense TSDF volume on the device
(Curless & Levoy 1996) and extract an indexed, welded triangle mesh from it by marching tetrahedra (Doi & Koide 1991) -- the last step
of PGSR, 2DGS and GOF, which they do with Open3D on the host.

    vol = TSDFVolume.around(model._scene_xyz.detach(), voxel_size=0.04, margin=0.5)  # the static Gaussians' box
    for cam in cameras:                                                            # static regions only, one time stamp per render
        pkg = render(cam, model, None, pipe)
        vol.integrate(pkg["depth"], pkg["img_opacity"], (cam, camera_pose(cam)), image=pkg["render"], weight=static_mask,
                      inv_depth=pipe.inv_depth)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    adgs.io.write_mesh_ply("mesh.ply", vertices, faces, colors)

NOTHING HERE IS DIFFERENTIABLE: the inputs are detached, the volume is updated in place, and no gradient reaches the renders.  Integration
is one launch per view, one thread per lattice point; extraction is count, scan, one read-back of the totals (the outputs must be
allocated), emit.  There is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _check_weight, _ptr
from .normals import _check_map, _min_opacity, _tanfov

CHUNK = 256                                  # ADGS_TSDF_CHUNK
NEAR = 0.2                                   # the rasterizer's near cull


class TsdfVolumeDesc(ctypes.Structure):
    """adgs_tsdf_volume (include/adgs_tsdf.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("nz", ctypes.c_int), ("voxel_size", ctypes.c_float),
                ("origin", ctypes.c_float * 3)]


class TsdfViewDesc(ctypes.Structure):
    """adgs_tsdf_view (include/adgs_tsdf.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("inv_depth", ctypes.c_int), ("tanfovx", ctypes.c_float),
                ("tanfovy", ctypes.c_float), ("min_opacity", ctypes.c_float), ("near", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("trunc", ctypes.c_float), ("max_weight", ctypes.c_float), ("reserved", ctypes.c_int), ("pose", ctypes.c_double * 12)]


def make_volume_desc(dims, voxel_size, origin):
    """An adgs_tsdf_volume; dims = (nx, ny, nz)."""
    return TsdfVolumeDesc(ctypes.sizeof(TsdfVolumeDesc), dims[0], dims[1], dims[2], voxel_size, (ctypes.c_float * 3)(*origin))


def make_view_desc(H, W, inv_depth, tan, min_opacity, near, max_depth, trunc, max_weight, pose):
    """An adgs_tsdf_view; pose: 12 numbers, R row-major then t, world to camera."""
    return TsdfViewDesc(ctypes.sizeof(TsdfViewDesc), H, W, int(bool(inv_depth)), tan[0], tan[1], min_opacity, near, max_depth, trunc, max_weight, 0,
                        (ctypes.c_double * 12)(*pose))


def camera_pose(camera):
    """The [3, 4] float64 HOST tensor (R | t) with X_c = R X_w + t of a camera, from its `world_view_transform` (or that [4, 4] matrix):
    the transposed, row-vector matrix the rasterizer receives, so A = V.T maps world to camera -- the transposition of
    adgs.multiview.relative_pose.  This READS THE MATRIX BACK from the device: call it once per camera, when the cameras are loaded."""
    V = getattr(camera, "world_view_transform", camera)
    if not torch.is_tensor(V) or tuple(V.shape) != (4, 4):
        raise ValueError("camera_pose: camera must be a camera with a [4, 4] world_view_transform (or that matrix)")
    return V.detach().to("cpu", torch.float64).T[:3, :4].contiguous()


def _pose12(pose, who):
    if not torch.is_tensor(pose):
        raise TypeError("%s: pose must be a tensor (camera_pose), got %s" % (who, type(pose).__name__))
    if tuple(pose.shape) != (3, 4) or not pose.dtype.is_floating_point:
        raise ValueError("%s: pose must be a floating-point [3, 4] tensor (R | t), got %s %s" % (who, pose.dtype, tuple(pose.shape)))
    if pose.device.type != "cpu":
        raise RuntimeError("%s: pose must be a host tensor (camera_pose), it is on %s" % (who, pose.device))
    p = pose.detach().to(torch.float64)
    pose12 = p[:, :3].reshape(-1).tolist() + p[:, 3].tolist()
    if not all(abs(x) < float("inf") for x in pose12):
        raise ValueError("%s: pose must be finite" % who)
    return pose12


def _positive(x, name, who):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise TypeError("%s: %s must be a number, got %r" % (who, name, x)) from None
    if not (0.0 < v < float("inf")):
        raise ValueError("%s: %s must be finite and > 0, got %r" % (who, name, x))
    return v


def _view_arguments(who, volume_device, has_color, depth, img_opacity, camera, image, weight, min_opacity, max_depth, near):
    """The checked arguments of an integrating (or allocating) call -> (H, W, tan, pose12, min_opacity, near, max_depth, depth, opacity,
    image, weight), the maps detached and contiguous.  Everything is checked before anything is launched."""
    _check_map(depth, "depth", None, None, None, who)
    H, W = depth.shape[-2:]
    _check_map(img_opacity, "img_opacity", H, W, depth.device, who)
    if isinstance(camera, (tuple, list)) and len(camera) == 2 and torch.is_tensor(camera[1]):
        tan, pose = _tanfov(camera[0], who), _pose12(camera[1], who)
    elif hasattr(camera, "world_view_transform"):
        tan, pose = _tanfov(camera, who), _pose12(camera_pose(camera), who)
    else:
        raise TypeError("%s: camera must be (camera or (tanfovx, tanfovy), pose) or a camera with a world_view_transform, got %r" % (who, camera))
    if (image is None) == has_color:
        raise ValueError("%s: image must be given exactly when the volume has colour" % who)
    if image is not None:
        if not torch.is_tensor(image):
            raise TypeError("%s: image must be a tensor, got %s" % (who, type(image).__name__))
        if tuple(image.shape) != (3, H, W):
            raise ValueError("%s: image must be [3, H, W] = [3, %d, %d], got %s" % (who, H, W, tuple(image.shape)))
        if image.dtype != torch.float32:
            raise TypeError("%s: image must be float32, got %s" % (who, image.dtype))
        if image.device != depth.device:
            raise RuntimeError("%s: image is on %s, depth on %s" % (who, image.device, depth.device))
    mo = _min_opacity(min_opacity, who)
    md, nr = float(max_depth), float(near)
    if not md > 0.0:
        raise ValueError("%s: max_depth must be > 0 (inf: no limit), got %r" % (who, max_depth))
    if not (0.0 <= nr < float("inf")):
        raise ValueError("%s: near must be finite and >= 0, got %r" % (who, near))
    w = None if weight is None else _check_weight(weight, H, W, depth.device, who)
    if not depth.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
    if depth.device != volume_device:
        raise RuntimeError("%s: depth is on %s, the volume on %s" % (who, depth.device, volume_device))
    d, o = depth.detach().contiguous().reshape(H, W), img_opacity.detach().contiguous().reshape(H, W)
    img = None if image is None else image.detach().contiguous()
    return H, W, tan, pose, mo, nr, md, d, o, img, w


class TSDFVolume:
    """A dense truncated-signed-distance volume on a HIP device: a lattice of dims = (nx, ny, nz) points, X(i, j, k) = origin +
    voxel_size (i, j, k) in world coordinates, with float32 tensors `tsdf` [nz, ny, nx] (1 = free or unseen), `wsum` [nz, ny, nx]
    (0 = never observed) and, with color=True, `color` [3, nz, ny, nx].  trunc: the truncation distance, default 4 voxel_size;
    max_weight: the cap of the accumulated weight, so that late views still count.  Memory: 8 (20 with colour) bytes per lattice
    point; nx ny nz must stay below 2^31.  Not differentiable."""

    def __init__(self, origin, voxel_size, dims, trunc=None, max_weight=64.0, color=True, device="cuda"):
        who = "TSDFVolume"
        try:
            origin = tuple(float(o) for o in origin)
        except (TypeError, ValueError):
            raise TypeError("%s: origin must be three numbers, got %r" % (who, origin)) from None
        if len(origin) != 3 or not all(abs(o) < float("inf") for o in origin):
            raise ValueError("%s: origin must be three finite numbers, got %r" % (who, origin))
        self.origin = origin
        self.voxel_size = _positive(voxel_size, "voxel_size", who)
        try:
            dims = tuple(dims)
        except TypeError:
            raise TypeError("%s: dims must be three integers (nx, ny, nz), got %r" % (who, dims)) from None
        if len(dims) != 3 or any(isinstance(d, bool) or not isinstance(d, int) for d in dims):
            raise TypeError("%s: dims must be three integers (nx, ny, nz), got %r" % (who, dims))
        if any(d < 0 for d in dims) or dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError("%s: dims must be >= 0 with nx * ny * nz below 2^31, got %r" % (who, dims))
        self.dims = dims
        self.trunc = _positive(4.0 * self.voxel_size if trunc is None else trunc, "trunc", who)
        mw = float(max_weight)
        if not mw > 0.0:
            raise ValueError("%s: max_weight must be > 0, got %r" % (who, max_weight))
        self.max_weight = mw
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s: the volume must live on a HIP device; there is no CPU path" % who)
        nx, ny, nz = dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.wsum = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self.device = self.tsdf.device

    @classmethod
    def around(cls, points, voxel_size, margin=0.0, **kw):
        """The volume over the bounding box of a [N, 3] point set (for example the static Gaussians' centres), grown by `margin` on
        every side.  Reads the box back from the device, once."""
        who = "TSDFVolume.around"
        if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise ValueError("%s: points must be a non-empty [N, 3] tensor" % who)
        vs = _positive(voxel_size, "voxel_size", who)
        margin = float(margin)
        if not (0.0 <= margin < float("inf")):
            raise ValueError("%s: margin must be finite and >= 0, got %r" % (who, margin))
        p = points.detach()
        lo, hi = p.min(0).values.double().cpu(), p.max(0).values.double().cpu()
        if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
            raise ValueError("%s: points must be finite" % who)
        lo, hi = lo - margin, hi + margin
        dims = tuple(int(math.ceil(float(h - l) / vs)) + 1 for l, h in zip(lo, hi))
        kw.setdefault("device", points.device)
        return cls(tuple(lo.tolist()), vs, dims, **kw)

    def reset(self):
        """Back to the empty volume: tsdf 1, wsum 0, color 0."""
        self.tsdf.fill_(1.0)
        self.wsum.zero_()
        if self.color is not None:
            self.color.zero_()

    def _desc(self):
        return make_volume_desc(self.dims, self.voxel_size, self.origin)

    @torch.no_grad()
    def integrate(self, depth, img_opacity, camera, image=None, weight=None, inv_depth=True, min_opacity=0.5, max_depth=float("inf"), near=NEAR):
        """Fuses one rendered view into the volume, in place.

        depth, img_opacity: float32 [H, W] or [1, H, W], as render() returns them (`inv_depth` = pipe.inv_depth); camera: a pair
        (camera_or_tanfov, pose) of a camera with FoVx / FoVy (or a (tanfovx, tanfovy) pair) and camera_pose(cam), the [3, 4] host
        world-to-camera matrix -- or a camera alone, whose pose is then READ BACK on every call; image: the float32 [3, H, W] render,
        required exactly when the volume has colour; weight: an optional [H, W] supervision weight (see adgs.loss.l1_ssim): zero
        keeps dynamic objects, the sky and the ego vehicle out of the volume.  A lattice point is updated when it lies beyond `near`
        in front of the camera, its nearest pixel has O >= min_opacity, D > 0 and w > 0, the expected depth z_d there is at most
        max_depth, and it is not more than trunc behind the surface (include/adgs_tsdf.h)."""
        H, W, tan, pose, mo, nr, md, d, o, img, w = _view_arguments("TSDFVolume.integrate", self.device, self.color is not None, depth, img_opacity, camera,
                                                                    image, weight, min_opacity, max_depth, near)
        if self.tsdf.numel() and d.numel():
            _lib.call("adgs_tsdf_integrate", self.device, ctypes.byref(self._desc()),
                      ctypes.byref(make_view_desc(H, W, inv_depth, tan, mo, nr, md, self.trunc, self.max_weight, pose)), d.data_ptr(), o.data_ptr(),
                      _ptr(img), _ptr(w), self.tsdf.data_ptr(), self.wsum.data_ptr(), _ptr(self.color))

    @torch.no_grad()
    def extract_mesh(self, min_weight=1.0):
        """The surface tsdf = 0 by marching tetrahedra over the cells whose 8 corners all have wsum >= min_weight -> (vertices [V, 3]
        float32 world coordinates, faces [F, 3] int32, colors [V, 3] float32 or None without colour), on the volume's device.  The mesh
        is indexed and welded (a vertex per cut lattice edge, shared by every triangle around it), has no unused vertex, is watertight
        wherever the valid cells are, and its normals point towards free space.  Vertices ascend by (lattice point, edge slot), faces
        by (cell, tetrahedron).  Synchronises once, to learn V and F."""
        who = "TSDFVolume.extract_mesh"
        mw = float(min_weight)
        if math.isnan(mw):
            raise ValueError("%s: min_weight must be a number, got %r" % (who, min_weight))
        dev = self.device
        desc = self._desc()
        counts = (ctypes.c_longlong * 3)(0, 0, 0)
        temp = owners = None
        if self.tsdf.numel():
            temp = torch.empty(int(_lib.lib().adgs_tsdf_extract_temp_bytes(ctypes.byref(desc))), dtype=torch.uint8, device=dev)
            _lib.call("adgs_tsdf_extract_count", dev, ctypes.byref(desc), self.tsdf.data_ptr(), self.wsum.data_ptr(), mw, temp.data_ptr(), counts)
        V, F, E = int(counts[0]), int(counts[1]), int(counts[2])
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        colors = None if self.color is None else torch.empty((V, 3), dtype=torch.float32, device=dev)
        if V:
            owners = torch.empty(int(_lib.lib().adgs_tsdf_extract_owner_bytes(E)), dtype=torch.uint8, device=dev)
            _lib.call("adgs_tsdf_extract_emit", dev, ctypes.byref(desc), self.tsdf.data_ptr(), self.wsum.data_ptr(), _ptr(self.color), mw, temp.data_ptr(),
                      owners.data_ptr(), counts, _ptr(vertices), _ptr(faces), _ptr(colors))
        return vertices, faces, colors
