"""Mesh simplification on the device (include/adgs_simplify.h): vertex clustering on a world-anchored lattice (Rossignac & Borrel) with
quadric placement of the representative (Lindstrom), what Open3D's simplify_vertex_clustering(contraction=Quadric) does on the host.

    vertices, faces, colors = adgs.mesh.remove_small_components(vertices, faces, colors)
    vertices, faces, colors = adgs.simplify.simplify_mesh(vertices, faces, colors, cell_size=2 * voxel_size)
    normals = adgs.mesh.vertex_normals(vertices, faces)

With a cell far below the vertex spacing the same call only welds coincident vertices: concatenate block meshes (faces offset) and
simplify_mesh(..., cell_size=voxel_size / 64).  The default origin (0, 0, 0) anchors the lattice in the world, so meshes simplified with
the same cell_size and origin share it.

Faces keep their order and their corner order, but a face can fold over when its corners move.  Every output is reproducible to the bit
(no float atomics).  NOTHING HERE IS DIFFERENTIABLE: everything runs under no_grad on detached inputs.  There is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _ptr
from .mesh import _check_faces, _check_rows, _need_device

PLACEMENTS = {"average": 0, "quadric": 1}
COUNT_NAMES = ("nonfinite_vertices", "dropped_faces", "degenerate_faces", "duplicate_faces")


def _positive(x, name, who):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise TypeError("%s: %s must be a number, got %r" % (who, name, x))
    x = float(x)
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError("%s: %s must be a positive finite number, got %r" % (who, name, x))
    return x


def _cell(cell_size, who):
    x = _positive(cell_size, "cell_size", who)
    f = ctypes.c_float(x).value                                 # the value the device uses
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError("%s: cell_size must be a positive finite float32, got %r" % (who, cell_size))
    return f


def _origin(origin, who):
    try:
        o = [float(x) for x in origin]
    except (TypeError, ValueError):
        raise TypeError("%s: origin must be three numbers, got %r" % (who, origin)) from None
    if len(o) != 3:
        raise ValueError("%s: origin must be three numbers, got %d" % (who, len(o)))
    o = [ctypes.c_float(x).value for x in o]
    if not all(math.isfinite(x) for x in o):
        raise ValueError("%s: origin must be finite float32 values, got %r" % (who, origin))
    return tuple(o)


def _placement(placement, who):
    if not isinstance(placement, str) or placement not in PLACEMENTS:
        raise ValueError("%s: placement must be 'quadric' or 'average', got %r" % (who, placement))
    return PLACEMENTS[placement]


class Clustering:
    """The clusters of a mesh on a lattice, on the device: vertex_cluster [V] int32 (the output vertex of every input vertex, -1 for a
    vertex that is not in the output); per output vertex root [V2] (its smallest member; output vertices are numbered by ascending root)
    and num_vertices [V2]; members [sum num_vertices] with member_starts [V2 + 1]: the CSR of the members in ascending vertex id, for
    carrying any other attribute across; faces [F2, 3] over the output vertices and face_source [F2], the input face of each.  counts: host
    ints nonfinite_vertices, dropped_faces, degenerate_faces, duplicate_faces.  cell_size and origin are the float32 values used.  len() = V2."""

    def __init__(self, vertex_cluster, root, num_vertices, members, member_starts, faces, face_source, counts, cell_size, origin):
        self.vertex_cluster, self.root, self.num_vertices, self.members, self.member_starts = vertex_cluster, root, num_vertices, members, member_starts
        self.faces, self.face_source, self.counts, self.cell_size, self.origin = faces, face_source, counts, cell_size, origin

    def __len__(self):
        return int(self.root.shape[0])


@torch.no_grad()
def cluster_vertices(vertices, faces, cell_size, origin=(0., 0., 0.)):
    """Steps 1-4 of include/adgs_simplify.h -> Clustering.  Synchronises exactly once: the sizes and the counts come back together.  A
    face with an index outside [0, V) is never dereferenced and raises ValueError naming how many there are; so does a finite vertex
    2^20 cells or more from the origin ("enlarge cell_size or move origin").  Vertices with a non-finite coordinate are dropped with
    their faces, and counted."""
    who = "cluster_vertices"
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    cell, org = _cell(cell_size, who), _origin(origin, who)
    V, F, dev = int(v.shape[0]), int(f.shape[0]), f.device
    if V >= 2 ** 31:
        raise ValueError("%s: V must be below 2^31" % who)
    _need_device(f, who)
    vc = torch.empty(V, dtype=torch.int32, device=dev)
    counts = (ctypes.c_longlong * 9)(*([0] * 9))
    corg = (ctypes.c_float * 3)(*org)
    temp = None
    if V or F:
        temp = torch.empty(int(_lib.lib().adgs_simplify_cluster_temp_bytes(V, F)), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            code = _lib.lib().adgs_simplify_cluster(V, F, _ptr(v), _ptr(f), cell, corg, temp.data_ptr(), _ptr(vc), counts, _lib.stream_ptr(dev))
        if code < 0 and counts[5] > 0:
            raise ValueError("%s: %d faces index outside the %d vertices" % (who, int(counts[5]), V))
        if code < 0 and counts[4] > 0:
            raise ValueError("%s: %d vertices lie 2^20 cells or more from the origin: enlarge cell_size or move origin" % (who, int(counts[4])))
        _lib.check(code, "adgs_simplify_cluster")
    V2, F2, M = int(counts[0]), int(counts[1]), int(counts[2])
    root, nv = (torch.empty(V2, dtype=torch.int32, device=dev) for _ in range(2))
    starts = torch.zeros(V2 + 1, dtype=torch.int32, device=dev)
    members = torch.empty(M, dtype=torch.int32, device=dev)
    fo = torch.empty((F2, 3), dtype=torch.int32, device=dev)
    src = torch.empty(F2, dtype=torch.int32, device=dev)
    if V:
        _lib.call("adgs_simplify_cluster_emit", dev, V, F, _ptr(f), _ptr(vc), temp.data_ptr(), counts, _ptr(root), _ptr(nv), starts.data_ptr(),
                  _ptr(members), _ptr(fo), _ptr(src))
    host = dict(zip(COUNT_NAMES, (int(counts[3]), int(counts[6]), int(counts[7]), int(counts[8]))))
    return Clustering(vc, root, nv, members, starts, fo, src, host, cell, org)


@torch.no_grad()
def place_vertices(clustering, vertices, faces, colors=None, placement="quadric", regularization=1e-3):
    """Step 5 of include/adgs_simplify.h -> (vertices2 [V2, 3], colors2 [V2, 3] or None) for the Clustering of the same vertices and
    faces: "average" is the mean of the members, "quadric" moves it onto the planes of the faces around them (kept inside the cell);
    the colours are always the mean of the member colours.  No read-back."""
    who = "place_vertices"
    if not isinstance(clustering, Clustering):
        raise TypeError("%s: clustering must be the Clustering of cluster_vertices, got %s" % (who, type(clustering).__name__))
    f = _check_faces(faces, who)
    V, V2, M = int(clustering.vertex_cluster.shape[0]), len(clustering), int(clustering.members.shape[0])
    v = _check_rows(vertices, "vertices", V, f.device, who)
    c = None if colors is None else _check_rows(colors, "colors", V, f.device, who)
    mode = _placement(placement, who)
    lam = _positive(regularization, "regularization", who)
    F, dev = int(f.shape[0]), f.device
    if clustering.vertex_cluster.device != dev:
        raise RuntimeError("%s: the clustering is on %s, faces on %s" % (who, clustering.vertex_cluster.device, dev))
    if 3 * F >= 2 ** 32:
        raise ValueError("%s: 3 F must be below 2^32" % who)
    _need_device(f, who)
    vo = torch.empty((V2, 3), dtype=torch.float32, device=dev)
    co = None if c is None else torch.empty((V2, 3), dtype=torch.float32, device=dev)
    if V2:
        temp = torch.empty(int(_lib.lib().adgs_simplify_place_temp_bytes(V, F)), dtype=torch.uint8, device=dev) if F else None
        corg = (ctypes.c_float * 3)(*clustering.origin)
        _lib.call("adgs_simplify_place", dev, V, F, V2, M, v.data_ptr(), _ptr(f), _ptr(c), clustering.vertex_cluster.data_ptr(),
                  clustering.member_starts.data_ptr(), clustering.members.data_ptr(), clustering.cell_size, corg, mode, lam, _ptr(temp), vo.data_ptr(),
                  _ptr(co))
    return vo, co


@torch.no_grad()
def simplify_mesh(vertices, faces, colors=None, *, cell_size, origin=(0., 0., 0.), placement="quadric", regularization=1e-3):
    """cluster_vertices and place_vertices in one call -> (vertices, faces, colors or None).  One synchronisation."""
    who = "simplify_mesh"
    f = _check_faces(faces, who)
    v = _check_rows(vertices, "vertices", None, f.device, who)
    if colors is not None:
        _check_rows(colors, "colors", int(v.shape[0]), f.device, who)
    _cell(cell_size, who), _origin(origin, who), _placement(placement, who), _positive(regularization, "regularization", who)
    cl = cluster_vertices(v, f, cell_size, origin)
    vo, co = place_vertices(cl, v, f, colors=colors, placement=placement, regularization=regularization)
    return vo, cl.faces, co
