"""Looking at the mesh from a camera (include/adgs_zbuffer.h): a z-buffer of an indexed triangle mesh on the device -- per pixel the nearest
face and its camera depth, optionally its normal --, interpolation of vertex attributes into an image, and per-face visibility over a set
of views, which is what culls the faces no training camera saw (the closed back of the truncation band, the far side of half-observed
objects):

    vis = adgs.zbuffer.visible_faces(vertices, faces, [(cam, camera_pose(cam)) for cam in cameras], size=(H, W), max_depth=fusion_max_depth)
    vertices, faces, colors, _ = adgs.mesh.keep_faces(vis.seen(min_views=2), vertices, faces, colors)

    r = adgs.zbuffer.render_mesh(vertices, faces, (cam, pose), size=(H, W), normals=True)     # r.depth, r.face, r.normal
    image = adgs.zbuffer.interpolate(r, vertices, faces, colors)                               # [3, H, W]

The pixel convention is that of adgs.tsdf (pixel centres at the integers), depth is the camera z, 0 where no face was drawn -- what
TSDFVolume.integrate skips.  The result is a function of the inputs alone: equal as bits from run to run and in any face order.
THERE IS NO NEAR-PLANE CLIPPING: a face with a corner nearer than `near` is not drawn at all.  cull="back" drops the faces whose
geometric normal points away from the camera; use it only for meshes oriented towards free space (extract_mesh's are).

NOTHING HERE IS DIFFERENTIABLE (use render() for gradients): everything runs under no_grad on detached inputs.  There is no CPU fallback.
"""
import collections
import ctypes

import torch

from . import _lib
from .loss import _ptr
from .mesh import _check_faces, _check_rows, _need_device
from .normals import _tanfov
from .tsdf import NEAR, _pose12, camera_pose

COUNTS = ("bad_index", "near", "guard_band", "degenerate", "culled")
_CULL = {"none": 0, "back": 1}


class ZbufferViewDesc(ctypes.Structure):
    """adgs_zbuffer_view (include/adgs_zbuffer.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("cull", ctypes.c_int), ("small_max", ctypes.c_int),
                ("stages", ctypes.c_int), ("tanfovx", ctypes.c_double), ("tanfovy", ctypes.c_double), ("near", ctypes.c_double),
                ("max_depth", ctypes.c_float), ("reserved", ctypes.c_int), ("pose", ctypes.c_double * 12)]


def make_view_desc(H, W, tan, pose, near, max_depth, cull=0, small_max=0, stages=0):
    """An adgs_zbuffer_view; pose: 12 numbers, R row-major then t, world to camera."""
    return ZbufferViewDesc(ctypes.sizeof(ZbufferViewDesc), H, W, cull, small_max, stages, tan[0], tan[1], near, max_depth, 0, (ctypes.c_double * 12)(*pose))


MeshRender = collections.namedtuple("MeshRender", "face depth normal counts size view")
MeshRender.__doc__ = """What render_mesh returns, on the device: face [H, W] int32 (-1: nothing), depth [H, W] float32 camera z (0: nothing), normal
[3, H, W] float32 or None, counts [5] int64 (the faces not drawn, by reason: adgs.zbuffer.COUNTS), size = (H, W), and `view`, the view it
was drawn with (interpolate needs it)."""


def _camera(camera, who):
    if isinstance(camera, (tuple, list)) and len(camera) == 2 and torch.is_tensor(camera[1]):
        return _tanfov(camera[0], who), _pose12(camera[1], who)
    if hasattr(camera, "world_view_transform"):
        return _tanfov(camera, who), _pose12(camera_pose(camera), who)
    raise TypeError("%s: camera must be (camera or (tanfovx, tanfovy), pose) or a camera with a world_view_transform, got %r" % (who, camera))


def _size(size, who):
    try:
        H, W = size
    except (TypeError, ValueError):
        raise TypeError("%s: size must be (H, W), got %r" % (who, size)) from None
    if any(isinstance(s, bool) or not isinstance(s, int) for s in (H, W)):
        raise TypeError("%s: size must be two integers (H, W), got %r" % (who, size))
    if H < 0 or W < 0 or H * W >= 2 ** 31:
        raise ValueError("%s: size must be >= 0 with H * W below 2^31, got %r" % (who, size))
    return H, W


def _mesh(vertices, faces, who):
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
        raise ValueError("%s: V and F must be below 2^31" % who)
    return v, f


@torch.no_grad()
def render_mesh(vertices, faces, camera, size, near=NEAR, max_depth=float("inf"), cull="none", normals=False, _small_max=0, _stages=0):
    """The z-buffer of the mesh (vertices [V, 3] float32, faces [F, 3] int32) from one camera -> MeshRender.

    camera: what TSDFVolume.integrate takes -- a pair (camera_or_tanfov, pose) of a camera with FoVx / FoVy (or a (tanfovx, tanfovy) pair)
    and camera_pose(cam), the [3, 4] host world-to-camera matrix, or a camera alone, whose pose is then READ BACK on every call; size =
    (H, W).  A face is drawn when all its corners lie at or beyond `near` and within the guard band of 16384 pixels around the image;
    samples deeper than max_depth are dropped (give the fusion's).  No read-back, no synchronisation: `counts` stays on the device."""
    who = "render_mesh"
    v, f = _mesh(vertices, faces, who)
    tan, pose = _camera(camera, who)
    H, W = _size(size, who)
    nr, md = float(near), float(max_depth)
    if not (0.0 < nr < float("inf")):
        raise ValueError("%s: near must be finite and > 0, got %r" % (who, near))
    if not md > 0.0:
        raise ValueError("%s: max_depth must be > 0 (inf: no limit), got %r" % (who, max_depth))
    if cull not in _CULL:
        raise ValueError("%s: cull must be 'none' or 'back', got %r" % (who, cull))
    _need_device(f, who)
    dev, V, F = f.device, int(v.shape[0]), int(f.shape[0])
    view = make_view_desc(H, W, tan, pose, nr, md, _CULL[cull], _small_max, _stages)
    face = torch.empty((H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((3, H, W), dtype=torch.float32, device=dev) if normals else None
    counts = (torch.empty if H * W else torch.zeros)(5, dtype=torch.int64, device=dev)        # the draw sets them
    if H * W:
        temp = torch.empty(int(_lib.lib().adgs_zbuffer_temp_bytes(H, W, F)), dtype=torch.uint8, device=dev)
        _lib.call("adgs_zbuffer_draw", dev, ctypes.byref(view), V, F, _ptr(v), _ptr(f), temp.data_ptr(), face.data_ptr(), depth.data_ptr(), _ptr(normal),
                  counts.data_ptr())
    return MeshRender(face, depth, normal, counts, (H, W), view)


@torch.no_grad()
def interpolate(render, vertices, faces, attributes, background=0.0):
    """Vertex attributes [V, C] float32 (colours, normals, labels as floats) into an image [C, H, W] for the faces `render` drew of THIS
    mesh: perspective-correct, from the same integer edge functions as the depth; `background` where nothing was drawn."""
    who = "interpolate"
    if not isinstance(render, MeshRender):
        raise TypeError("%s: render must be the MeshRender of render_mesh, got %s" % (who, type(render).__name__))
    v, f = _mesh(vertices, faces, who)
    V, F, dev = int(v.shape[0]), int(f.shape[0]), f.device
    if not torch.is_tensor(attributes):
        raise TypeError("%s: attributes must be a tensor, got %s" % (who, type(attributes).__name__))
    if attributes.dim() != 2 or attributes.shape[0] != V:
        raise ValueError("%s: attributes must be [V, C] = [%d, C], got %s" % (who, V, tuple(attributes.shape)))
    if attributes.dtype != torch.float32:
        raise TypeError("%s: attributes must be float32, got %s" % (who, attributes.dtype))
    if attributes.device != dev or render.face.device != dev:
        raise RuntimeError("%s: attributes are on %s, the render on %s, faces on %s" % (who, attributes.device, render.face.device, dev))
    bg = float(background)
    _need_device(f, who)
    a = attributes.detach().contiguous()
    (H, W), C = render.size, int(a.shape[1])
    out = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    if C and H * W:
        _lib.call("adgs_zbuffer_interpolate", dev, ctypes.byref(render.view), V, F, _ptr(v), _ptr(f), render.face.data_ptr(), C, _ptr(a), bg,
                  out.data_ptr())
    return out


class FaceVisibility:
    """Per-face visibility over views, on the device: views [F] int32, the number of added renders in which the face won at least one
    pixel; pixels [F] int64, the pixels it won in all of them; num_views, the number of renders added.  Integer atomics: exact."""

    def __init__(self, num_faces, device="cuda"):
        who = "FaceVisibility"
        if isinstance(num_faces, bool) or not isinstance(num_faces, int):
            raise TypeError("%s: num_faces must be an integer, got %r" % (who, num_faces))
        if not 0 <= num_faces < 2 ** 31:
            raise ValueError("%s: num_faces must lie in [0, 2^31), got %r" % (who, num_faces))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s: the counts must live on a HIP device; there is no CPU path" % who)
        self.views = torch.zeros(num_faces, dtype=torch.int32, device=self.device)
        self.pixels = torch.zeros(num_faces, dtype=torch.int64, device=self.device)
        self._scratch = torch.zeros(num_faces, dtype=torch.int32, device=self.device)      # zero between calls
        self.device = self.views.device
        self.num_views = 0

    @torch.no_grad()
    def add(self, render):
        """Counts one render of the mesh these faces belong to.  No read-back."""
        who = "FaceVisibility.add"
        if not isinstance(render, MeshRender):
            raise TypeError("%s: render must be the MeshRender of render_mesh, got %s" % (who, type(render).__name__))
        if render.face.device != self.device:
            raise RuntimeError("%s: the render is on %s, the counts on %s" % (who, render.face.device, self.device))
        H, W = render.size
        F = int(self.views.shape[0])
        if F and H * W:
            _lib.call("adgs_zbuffer_count_faces", self.device, H, W, F, render.face.data_ptr(), self._scratch.data_ptr(), self.views.data_ptr(),
                      self.pixels.data_ptr())
        self.num_views += 1
        return self

    def seen(self, min_views=1, min_pixels=1):
        """bool [F]: the faces that won a pixel in at least min_views renders and at least min_pixels pixels in all."""
        return (self.views >= int(min_views)) & (self.pixels >= int(min_pixels))


@torch.no_grad()
def visible_faces(vertices, faces, cameras, size, **kw):
    """FaceVisibility of the mesh over `cameras` (each what render_mesh takes; pass (cam, camera_pose(cam)) pairs to avoid a read-back per
    camera); size and the keywords go to render_mesh.  No read-back inside."""
    who = "visible_faces"
    v, f = _mesh(vertices, faces, who)
    _need_device(f, who)
    vis = FaceVisibility(int(f.shape[0]), f.device)
    for camera in cameras:
        vis.add(render_mesh(v, f, camera, size, **kw))
    return vis
