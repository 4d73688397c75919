"""Mesh clean-up on the device (include/adgs_mesh.h): what comes between TSDFVolume.extract_mesh and the PLY -- connected components,
the removal of small ones (2DGS's post_process_mesh, which it does with Open3D on the host) and area-weighted vertex normals.

    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    vertices, faces, colors = adgs.mesh.remove_small_components(vertices, faces, colors, largest=50, min_faces=50)
    normals = adgs.mesh.vertex_normals(vertices, faces)
    adgs.io.write_mesh_ply("mesh.ply", vertices, faces, colors, normals=normals)

Components are by VERTEX connectivity (two vertices are connected when a face contains both); Open3D's cluster_connected_triangles joins
triangles that share an edge.  On a welded marching-tetrahedra mesh the two differ only at pinch points.  Component numbers, counts, the
kept faces and the normals are reproducible to the integer / bit from run to run; `area` (double atomics) is not.

NOTHING HERE IS DIFFERENTIABLE: everything runs under no_grad on detached inputs.  There is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from .loss import _ptr


def _check_faces(faces, who):
    if not torch.is_tensor(faces):
        raise TypeError("%s: faces must be a tensor, got %s" % (who, type(faces).__name__))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be [F, 3], got %s" % (who, tuple(faces.shape)))
    if faces.dtype != torch.int32:
        raise TypeError("%s: faces must be int32, got %s (use faces.int())" % (who, faces.dtype))
    return faces.detach().contiguous()


def _need_device(faces, who):
    """Last of the checks, as in adgs.tsdf: shapes and dtypes are refused wherever the tensors live."""
    if not faces.is_cuda:
        raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)


def _check_rows(t, name, V, device, who):
    """A float32 [V, 3] tensor on `device` (V None: any)."""
    if not torch.is_tensor(t):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if t.dim() != 2 or t.shape[1] != 3 or (V is not None and t.shape[0] != V):
        raise ValueError("%s: %s must be [%s, 3], got %s" % (who, name, "V" if V is None else V, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    if t.device != device:
        raise RuntimeError("%s: %s is on %s, faces on %s" % (who, name, t.device, device))
    return t.detach().contiguous()


def _count(n, name, who):
    if isinstance(n, bool) or not isinstance(n, int):
        raise TypeError("%s: %s must be an integer, got %r" % (who, name, n))
    if not 0 <= n < 2 ** 31:
        raise ValueError("%s: %s must lie in [0, 2^31), got %r" % (who, name, n))
    return n


def _bad_faces(who, counts, V):
    return ValueError("%s: %d faces index outside the %d vertices" % (who, int(counts[1]), V))


class Components:
    """The connected components of a mesh, on the device: vertex_component [V] int32; per component root [C] (its smallest vertex index;
    components are numbered by ascending root), num_faces [C], num_vertices [C] int32 and, when the vertices were given, area [C] float64
    (else None).  len() = C."""

    def __init__(self, vertex_component, root, num_faces, num_vertices, area):
        self.vertex_component, self.root, self.num_faces, self.num_vertices, self.area = vertex_component, root, num_faces, num_vertices, area

    def __len__(self):
        return int(self.root.shape[0])

    @torch.no_grad()
    def select(self, largest=50, min_faces=50, min_area=None):
        """The rule of 2DGS's post_process_mesh(cluster_to_keep=largest) -> keep [C] bool on the device: a component stays when
        num_faces >= max(min_faces, the `largest`-th largest num_faces) -- with fewer than `largest` components, the smallest count --,
        so ties at the threshold all stay; with min_area also area >= min_area.  Torch operations on the [C] tensors: no read-back."""
        who = "Components.select"
        K, m = _count(largest, "largest", who), _count(min_faces, "min_faces", who)
        if K < 1:
            raise ValueError("%s: largest must be >= 1, got %r" % (who, largest))
        C = len(self)
        if C == 0:
            return torch.zeros(0, dtype=torch.bool, device=self.num_faces.device)
        kth = torch.topk(self.num_faces, min(K, C)).values[-1]
        keep = self.num_faces >= torch.clamp(kth, min=m)
        if min_area is not None:
            if self.area is None:
                raise ValueError("%s: min_area needs the areas: pass vertices to connected_components" % who)
            keep &= self.area >= float(min_area)
        return keep


@torch.no_grad()
def connected_components(faces, num_vertices, vertices=None):
    """The components of the mesh (faces [F, 3] int32 over num_vertices vertices) by vertex connectivity -> Components.  vertices
    ([V, 3] float32): also the area of every component.  Synchronises once, to learn C; a face with an index outside [0, V) is never
    dereferenced and raises ValueError naming how many there are."""
    who = "connected_components"
    f = _check_faces(faces, who)
    V, F, dev = _count(num_vertices, "num_vertices", who), int(f.shape[0]), f.device
    v = None if vertices is None else _check_rows(vertices, "vertices", V, dev, who)
    _need_device(f, who)
    vc = torch.empty(V, dtype=torch.int32, device=dev)
    counts = (ctypes.c_longlong * 2)(0, 0)
    temp = None
    if V or F:
        temp = torch.empty(int(_lib.lib().adgs_mesh_label_temp_bytes(V, F)), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            code = _lib.lib().adgs_mesh_label(V, F, _ptr(f), temp.data_ptr(), _ptr(vc), counts, _lib.stream_ptr(dev))
        if code < 0 and counts[1] > 0:
            raise _bad_faces(who, counts, V)
        _lib.check(code, "adgs_mesh_label")
    C = int(counts[0])
    root, nf, nv = (torch.empty(C, dtype=torch.int32, device=dev) for _ in range(3))
    area = None if v is None else torch.empty(C, dtype=torch.float64, device=dev)
    if C:
        _lib.call("adgs_mesh_table", dev, V, F, C, _ptr(f), _ptr(v), vc.data_ptr(), temp.data_ptr(), root.data_ptr(), nf.data_ptr(), nv.data_ptr(),
                  _ptr(area))
    return Components(vc, root, nf, nv, area)


@torch.no_grad()
def keep_components(comps, keep, vertices, faces, colors=None, normals=None):
    """Drops every vertex and face of the components with keep [C] False -> (vertices, faces, colors or None, normals or None): the
    remaining vertices renumbered densely in their order, the faces in their order with their corner order, the attributes gathered bit
    for bit.  A mesh in extract_mesh's canonical order stays canonical.  Synchronises once, to learn the sizes."""
    who = "keep_components"
    if not isinstance(comps, Components):
        raise TypeError("%s: comps must be the Components of connected_components, got %s" % (who, type(comps).__name__))
    f = _check_faces(faces, who)
    dev, F, C = f.device, int(f.shape[0]), len(comps)
    V = int(comps.vertex_component.shape[0])
    v = _check_rows(vertices, "vertices", V, dev, who)
    c = None if colors is None else _check_rows(colors, "colors", V, dev, who)
    n = None if normals is None else _check_rows(normals, "normals", V, dev, who)
    if not torch.is_tensor(keep) or keep.dtype != torch.bool or tuple(keep.shape) != (C,):
        raise ValueError("%s: keep must be a bool [C] = [%d] tensor (Components.select)" % (who, C))
    if keep.device != dev or comps.vertex_component.device != dev:
        raise RuntimeError("%s: keep is on %s, the components on %s, faces on %s" % (who, keep.device, comps.vertex_component.device, dev))
    _need_device(f, who)
    k8 = keep.detach().contiguous().view(torch.uint8)
    counts = (ctypes.c_longlong * 2)(0, 0)
    temp = None
    if V:
        temp = torch.empty(int(_lib.lib().adgs_mesh_keep_temp_bytes(V, F)), dtype=torch.uint8, device=dev)
        _lib.call("adgs_mesh_keep_count", dev, V, F, C, _ptr(f), comps.vertex_component.data_ptr(), _ptr(k8), temp.data_ptr(), counts)
    V2, F2 = int(counts[0]), int(counts[1])
    vo = torch.empty((V2, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((F2, 3), dtype=torch.int32, device=dev)
    co = None if c is None else torch.empty((V2, 3), dtype=torch.float32, device=dev)
    no = None if n is None else torch.empty((V2, 3), dtype=torch.float32, device=dev)
    if V2:
        _lib.call("adgs_mesh_keep_emit", dev, V, F, _ptr(f), v.data_ptr(), _ptr(c), _ptr(n), temp.data_ptr(), counts, vo.data_ptr(), _ptr(fo), _ptr(co),
                  _ptr(no))
    return vo, fo, co, no


@torch.no_grad()
def keep_faces(keep, vertices, faces, colors=None, normals=None):
    """Keeps the faces with keep [F] True (for example adgs.zbuffer.FaceVisibility.seen()) and the vertices they use -> (vertices, faces,
    colors or None, normals or None), shaped like keep_components' result: the remaining vertices renumbered densely in their order, the
    faces in their order with their corner order, the attributes gathered bit for bit; a canonical mesh stays canonical.  A face with an
    index outside [0, V) is never dereferenced and never kept.  Synchronises once, to learn the sizes."""
    who = "keep_faces"
    f = _check_faces(faces, who)
    dev, F = f.device, int(f.shape[0])
    v = _check_rows(vertices, "vertices", None, dev, who)
    V = int(v.shape[0])
    c = None if colors is None else _check_rows(colors, "colors", V, dev, who)
    n = None if normals is None else _check_rows(normals, "normals", V, dev, who)
    if not torch.is_tensor(keep) or keep.dtype != torch.bool or tuple(keep.shape) != (F,):
        raise ValueError("%s: keep must be a bool [F] = [%d] tensor" % (who, F))
    if keep.device != dev:
        raise RuntimeError("%s: keep is on %s, faces on %s" % (who, keep.device, dev))
    if V >= 2 ** 31:
        raise ValueError("%s: V must be below 2^31" % who)
    _need_device(f, who)
    k8 = keep.detach().contiguous().view(torch.uint8)
    counts = (ctypes.c_longlong * 3)(0, 0, 0)
    temp = None
    if F:
        temp = torch.empty(int(_lib.lib().adgs_mesh_keep_temp_bytes(V, F)), dtype=torch.uint8, device=dev)
        _lib.call("adgs_zbuffer_keep_faces_count", dev, V, F, _ptr(f), _ptr(k8), temp.data_ptr(), counts)
    V2, F2 = int(counts[0]), int(counts[1])
    vo = torch.empty((V2, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((F2, 3), dtype=torch.int32, device=dev)
    co = None if c is None else torch.empty((V2, 3), dtype=torch.float32, device=dev)
    no = None if n is None else torch.empty((V2, 3), dtype=torch.float32, device=dev)
    if V2:
        _lib.call("adgs_mesh_keep_emit", dev, V, F, _ptr(f), v.data_ptr(), _ptr(c), _ptr(n), temp.data_ptr(), counts, vo.data_ptr(), _ptr(fo), _ptr(co),
                  _ptr(no))
    return vo, fo, co, no


@torch.no_grad()
def remove_small_components(vertices, faces, colors=None, largest=50, min_faces=50, min_area=None):
    """connected_components, Components.select and keep_components in one call -> (vertices, faces, colors or None): the floaters of a
    fused mesh removed by the 2DGS rule.  Two synchronisations (C, then the sizes)."""
    who = "remove_small_components"
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    if colors is not None:
        _check_rows(colors, "colors", int(v.shape[0]), f.device, who)
    comps = connected_components(f, int(v.shape[0]), vertices=v if min_area is not None else None)
    vo, fo, co, _ = keep_components(comps, comps.select(largest, min_faces, min_area), v, f, colors=colors)
    return vo, fo, co


@torch.no_grad()
def vertex_normals(vertices, faces, check=True):
    """Area-weighted vertex normals [V, 3] float32: the normalised sum of (p1 - p0) x (p2 - p0) over the faces around a vertex, summed
    in double in face order (reproducible to the bit, no atomics); (0, 0, 0) for a vertex without a face of non-zero area.  Faces from
    extract_mesh are oriented towards free space, so these normals are too.  No read-back with check=False; check=True validates the
    index range with one torch min / max (ValueError).  The kernels skip a face with an index outside [0, V) either way."""
    who = "vertex_normals"
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    V, F, dev = int(v.shape[0]), int(f.shape[0]), f.device
    if V >= 2 ** 31:
        raise ValueError("%s: V must be below 2^31" % who)
    _need_device(f, who)
    if check and F:
        lo, hi = torch.aminmax(f)
        if int(lo) < 0 or int(hi) >= V:
            raise ValueError("%s: faces index outside the %d vertices (min %d, max %d)" % (who, V, int(lo), int(hi)))
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if V:
        temp = torch.empty(int(_lib.lib().adgs_mesh_normals_temp_bytes(V, F)), dtype=torch.uint8, device=dev) if F else None
        _lib.call("adgs_mesh_vertex_normals", dev, V, F, v.data_ptr(), _ptr(f), _ptr(temp), out.data_ptr())
    return out
