"""A block-sparse TSDF volume (include/adgs_sparse_tsdf.h): the fusion and the marching tetrahedra of adgs.tsdf on an UNBOUNDED lattice
of which only the 8 x 8 x 8 blocks near an observed surface are stored -- what Open3D's VoxelBlockGrid, nvblox and InfiniTAM do.  One
volume and one welded mesh for a whole street; memory and the work of a view grow with the surface area, not with a bounding box.

    vol = SparseTSDFVolume(voxel_size=0.04)
    for cam, pkg in views:                                                         # first every view's blocks ...
        vol.allocate(pkg["depth"], pkg["img_opacity"], (cam, camera_pose(cam)), weight=static_mask, max_depth=30.0)
    for cam, pkg in views:                                                         # ... then every view into all of them
        vol.integrate(pkg["depth"], pkg["img_opacity"], (cam, camera_pose(cam)), image=pkg["render"], weight=static_mask, max_depth=30.0,
                      allocate=False)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)

FUSING IS ORDER-DEPENDENT WHEN ALLOCATION IS INTERLEAVED WITH INTEGRATION: a block allocated by view 5 never saw the free space of views
1-4, so `integrate(..., allocate=True)` view by view does not give what the dense volume gives.  For the dense result on the allocated
blocks, allocate for all views first, then integrate with allocate=False, as above: every stored value then has the bits a dense
TSDFVolume with the same origin and voxel size holds at that lattice point.

NOTHING HERE IS DIFFERENTIABLE.  There is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib
from .loss import _ptr
from .tsdf import NEAR, TSDFVolume, _positive, _view_arguments, make_view_desc

BLOCK = 8                                    # ADGS_SPARSE_TSDF_BLOCK
BLOCK_POINTS = 512                           # ADGS_SPARSE_TSDF_BLOCK_POINTS
MAX_BLOCKS = 1 << 22                         # ADGS_SPARSE_TSDF_MAX_BLOCKS
COORD_LIMIT = 1 << 20                        # ADGS_SPARSE_TSDF_COORD_LIMIT
MAX_STEPS = 64                               # ADGS_SPARSE_TSDF_MAX_STEPS
# the scratch for the candidate keys a view's allocation starts with: at least MIN_CANDIDATES keys and CANDIDATES_PER_WAVE for every 64
# pixels (a wave of the candidate kernel); a view with more is told so and retried with room (SparseTSDFVolume._allocating_call)
MIN_CANDIDATES = 4096
CANDIDATES_PER_WAVE = 16


class SparseTsdfVolumeDesc(ctypes.Structure):
    """adgs_sparse_tsdf_volume (include/adgs_sparse_tsdf.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int), ("num_blocks", ctypes.c_int), ("capacity", ctypes.c_int), ("table_capacity", ctypes.c_int),
                ("voxel_size", ctypes.c_float), ("origin", ctypes.c_float * 3)]


def make_sparse_volume_desc(num_blocks, capacity, table_capacity, voxel_size, origin):
    """An adgs_sparse_tsdf_volume."""
    return SparseTsdfVolumeDesc(ctypes.sizeof(SparseTsdfVolumeDesc), num_blocks, capacity, table_capacity, voxel_size, (ctypes.c_float * 3)(*origin))


def block_keys(coords):
    """The int64 block keys of [M, 3] integer block coordinates: ((bz + 2^20) << 42) | ((by + 2^20) << 21) | (bx + 2^20)."""
    c = coords.to(torch.int64) + COORD_LIMIT
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


class SparseTSDFVolume:
    """A block-sparse truncated-signed-distance volume on a HIP device.  The lattice is unbounded and anchored in the world:
    X(i, j, k) = origin + voxel_size (i, j, k) with signed indices; block b holds the points 8 b + l, l in [0, 8)^3.  The pool holds
    float32 `tsdf` [NB, 8, 8, 8] (z, y, x), `wsum` [NB, 8, 8, 8] and, with color=True, `color` [NB, 3, 8, 8, 8] in allocation order,
    `block_coords` [NB, 3] int32 names the blocks, and (`keys`, `slots`) is the table: the block keys in ascending order with each
    one's pool row.  A point in no allocated block counts as tsdf 1, wsum 0.  trunc: default 4 voxel_size; margin: how far, in
    voxels, around a sample of a ray blocks are allocated (0 .. 4); capacity: the rows the pool starts with -- it grows
    geometrically and keeps every bit, a block never moves.  At most 2^22 blocks, block coordinates within +-2^20.  Memory: 4 KiB per
    block, 10 KiB with colour (`memory_bytes`).  Not differentiable."""

    def __init__(self, voxel_size, origin=(0.0, 0.0, 0.0), trunc=None, max_weight=64.0, color=True, capacity=4096, margin=2.0, device="cuda"):
        who = "SparseTSDFVolume"
        self.voxel_size = _positive(voxel_size, "voxel_size", who)
        try:
            origin = tuple(float(o) for o in origin)
        except (TypeError, ValueError):
            raise TypeError("%s: origin must be three numbers, got %r" % (who, origin)) from None
        if len(origin) != 3 or not all(abs(o) < float("inf") for o in origin):
            raise ValueError("%s: origin must be three finite numbers, got %r" % (who, origin))
        self.origin = origin
        self.trunc = _positive(4.0 * self.voxel_size if trunc is None else trunc, "trunc", who)
        if math.ceil(self.trunc / self.voxel_size) > MAX_STEPS:
            raise ValueError("%s: trunc must be at most %d voxel_size, got %r" % (who, MAX_STEPS, trunc))
        mw = float(max_weight)
        if not mw > 0.0:
            raise ValueError("%s: max_weight must be > 0, got %r" % (who, max_weight))
        self.max_weight = mw
        if isinstance(capacity, bool) or not isinstance(capacity, int):
            raise TypeError("%s: capacity must be an integer, got %r" % (who, capacity))
        if not (1 <= capacity <= MAX_BLOCKS):
            raise ValueError("%s: capacity must lie in [1, 2^22], got %r" % (who, capacity))
        mg = float(margin)
        if not (0.0 <= mg <= 4.0):
            raise ValueError("%s: margin must lie in [0, 4] (voxels), got %r" % (who, margin))
        self.margin = mg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s: the volume must live on a HIP device; there is no CPU path" % who)
        self._has_color = bool(color)
        self._nb = 0
        self.skipped_samples = 0
        self._pool = self._new_pool(capacity)
        self.device = self._pool[0].device
        self._table = self._new_table(max(capacity, 1024))
        self._block_coords = torch.zeros((self._table[0].shape[0], 3), dtype=torch.int32, device=self.device)
        self._spare = None
        self._temp = None
        self._max_candidates = 0

    # ---- storage ----

    def _new_pool(self, cap):
        dev = self.device
        return (torch.ones((cap, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev),
                torch.zeros((cap, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev),
                torch.zeros((cap, 3, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev) if self._has_color else None)

    def _new_table(self, cap):
        dev = self.device
        return (torch.zeros(cap, dtype=torch.int64, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev))

    @property
    def capacity(self):
        return self._pool[0].shape[0]

    @property
    def num_blocks(self):
        return self._nb

    @property
    def tsdf(self):
        return self._pool[0][:self._nb]

    @property
    def wsum(self):
        return self._pool[1][:self._nb]

    @property
    def color(self):
        return None if self._pool[2] is None else self._pool[2][:self._nb]

    @property
    def block_coords(self):
        return self._block_coords[:self._nb]

    @property
    def keys(self):
        """The block keys in ascending order, int64 [NB]."""
        return self._table[0][:self._nb]

    @property
    def slots(self):
        """The pool row of each key of `keys`, int32 [NB]."""
        return self._table[1][:self._nb]

    @property
    def memory_bytes(self):
        """The bytes the volume holds on the device: the pool at its capacity, the table (both copies) and the block coordinates."""
        held = [t for t in self._pool if t is not None] + list(self._table) + [self._block_coords] + list(self._spare or ())
        return sum(t.numel() * t.element_size() for t in held)

    def reserve(self, capacity):
        """Grows the pool to at least `capacity` rows (never shrinks); the rows keep their bits and a block its row."""
        who = "SparseTSDFVolume.reserve"
        if isinstance(capacity, bool) or not isinstance(capacity, int):
            raise TypeError("%s: capacity must be an integer, got %r" % (who, capacity))
        if not (0 <= capacity <= MAX_BLOCKS):
            raise ValueError("%s: capacity must lie in [0, 2^22], got %r" % (who, capacity))
        if capacity <= self.capacity:
            return
        pool = self._new_pool(capacity)
        for new, old in zip(pool, self._pool):
            if old is not None:
                new[:self._nb].copy_(old[:self._nb])
        self._pool = pool

    def _reserve_table(self, entries):
        """Room for `entries` table entries and block coordinates (at most 2^22)."""
        entries = min(entries, MAX_BLOCKS)
        if entries <= self._table[0].shape[0]:
            return
        table, coords = self._new_table(entries), torch.zeros((entries, 3), dtype=torch.int32, device=self.device)
        for new, old in zip(table, self._table):
            new[:self._nb].copy_(old[:self._nb])
        coords[:self._nb].copy_(self._block_coords[:self._nb])
        self._table, self._block_coords, self._spare = table, coords, None

    def reset(self):
        """Back to the empty volume: no block; the pool keeps its capacity."""
        self._nb = 0
        self.skipped_samples = 0
        self._pool[0].fill_(1.0)
        self._pool[1].zero_()
        if self._pool[2] is not None:
            self._pool[2].zero_()

    def _desc(self):
        return make_sparse_volume_desc(self._nb, self.capacity, self._table[0].shape[0], self.voxel_size, self.origin)

    # ---- allocation ----

    def _allocating_call(self, who, symbol, pixels, candidates, args_before, pass_candidates=False):
        """Runs an allocating entry until it has room (it reports what it needs) -> the number of new blocks.  One read-back per run."""
        for _ in range(4):
            self._reserve_table(self._nb + candidates)
            if self._spare is None or self._spare[0].shape[0] != self._table[0].shape[0]:
                self._spare = self._new_table(self._table[0].shape[0])
            need = int(_lib.lib().adgs_sparse_tsdf_allocate_temp_bytes(pixels, candidates))
            if self._temp is None or self._temp.numel() < need:
                self._temp = torch.empty(need, dtype=torch.uint8, device=self.device)
            counts = (ctypes.c_longlong * 4)(0, 0, 0, 0)
            code = _lib.call(symbol, self.device, ctypes.byref(self._desc()), *args_before, _ptr(self._table[0]), _ptr(self._table[1]),
                             self._spare[0].data_ptr(), self._spare[1].data_ptr(), self._block_coords.data_ptr(), *((candidates,) if pass_candidates else ()),
                             self._temp.data_ptr(), counts)
            new, found, skipped = int(counts[0]), int(counts[1]), int(counts[2])
            if code == 0:
                break
            if found > candidates:                                  # the scratch was too small for the view's candidates: the count of new blocks means nothing yet
                candidates = found + found // 4
                self._max_candidates = max(self._max_candidates, candidates)
            else:                                                   # the table has room for min(NB + candidates, 2^22) entries
                raise RuntimeError("%s: %d new blocks on top of %d exceed the 2^22 blocks a volume can hold; enlarge voxel_size or lower max_depth"
                                   % (who, new, self._nb))
        else:
            raise RuntimeError("%s: the allocation did not settle" % who)
        self.skipped_samples += skipped
        if new:
            if self._nb + new > self.capacity:
                self.reserve(min(MAX_BLOCKS, max(self._nb + new, 2 * self.capacity)))
            self._table, self._spare = self._spare, self._table
            self._nb += new
        return new

    @torch.no_grad()
    def allocate(self, depth, img_opacity, camera, weight=None, inv_depth=True, min_opacity=0.5, max_depth=float("inf"), near=NEAR):
        """Allocates the blocks one rendered view needs -> the number of new blocks.  Synchronises once (twice when the scratch for the
        candidate keys has to grow, which the first view of a volume usually causes; the volume keeps the larger scratch).

        The arguments are those of `integrate` (no image).  Every pixel that integration would use (O >= min_opacity, D > 0, w > 0,
        z_d <= max_depth) marks, along its own ray from trunc in front of the surface to trunc behind it in steps of at most two
        voxels, the blocks within `margin` voxels of each sample.  Beyond z ~ 2 margin voxel_size W / (2 tanfovx) neighbouring rays
        leave gaps between their cubes: bound `max_depth` accordingly.  Samples whose blocks lie outside +-2^20 are counted in
        `skipped_samples` and skipped."""
        who = "SparseTSDFVolume.allocate"
        H, W, tan, pose, mo, nr, md, d, o, _, w = _view_arguments(who, self.device, False, depth, img_opacity, camera, None, weight, min_opacity, max_depth, near)
        return self._allocate_view(who, make_view_desc(H, W, inv_depth, tan, mo, nr, md, self.trunc, self.max_weight, pose), d, o, w)

    def _allocate_view(self, who, view, d, o, w):
        if not d.numel():
            return 0
        pixels = d.numel()
        candidates = max(self._max_candidates, MIN_CANDIDATES, CANDIDATES_PER_WAVE * -(-pixels // 64))
        return self._allocating_call(who, "adgs_sparse_tsdf_allocate_view", pixels, candidates,
                                     (ctypes.byref(view), self.margin, d.data_ptr(), o.data_ptr(), _ptr(w)), pass_candidates=True)

    @torch.no_grad()
    def allocate_blocks(self, coords):
        """Allocates the blocks with the given [M, 3] integer block coordinates (bx, by, bz) -> the number of new blocks.  Duplicates
        and blocks the volume already has are dropped; the rest are appended to the pool in ascending key order.  Synchronises once."""
        who = "SparseTSDFVolume.allocate_blocks"
        if not torch.is_tensor(coords):
            raise TypeError("%s: coords must be a tensor, got %s" % (who, type(coords).__name__))
        if coords.dim() != 2 or coords.shape[1] != 3:
            raise ValueError("%s: coords must be [M, 3], got %s" % (who, tuple(coords.shape)))
        if coords.dtype != torch.int32:
            raise TypeError("%s: coords must be int32, got %s" % (who, coords.dtype))
        if not coords.is_cuda:
            raise RuntimeError("%s: tensors must be on a HIP device; there is no CPU path" % who)
        if coords.device != self.device:
            raise RuntimeError("%s: coords is on %s, the volume on %s" % (who, coords.device, self.device))
        M = coords.shape[0]
        if M == 0:
            return 0
        c = coords.detach().contiguous()
        return self._allocating_call(who, "adgs_sparse_tsdf_allocate_blocks", 0, M, (c.data_ptr(), M))

    # ---- integration ----

    @torch.no_grad()
    def integrate(self, depth, img_opacity, camera, image=None, weight=None, inv_depth=True, min_opacity=0.5, max_depth=float("inf"), near=NEAR,
                  allocate=True):
        """Fuses one rendered view into every allocated block, in place; the arguments are those of TSDFVolume.integrate.  With
        allocate=True the view's blocks are allocated first (one synchronisation; see the module's note on the order); with
        allocate=False the call never synchronises.  ONE launch, a workgroup per block; a block wholly behind the camera or outside
        the frustum is left after a test of its bounding sphere."""
        who = "SparseTSDFVolume.integrate"
        H, W, tan, pose, mo, nr, md, d, o, img, w = _view_arguments(who, self.device, self._has_color, depth, img_opacity, camera, image, weight, min_opacity,
                                                                    max_depth, near)
        view = make_view_desc(H, W, inv_depth, tan, mo, nr, md, self.trunc, self.max_weight, pose)
        if allocate:
            self._allocate_view(who, view, d, o, w)
        if self._nb and d.numel():
            _lib.call("adgs_sparse_tsdf_integrate", self.device, ctypes.byref(self._desc()),
                      ctypes.byref(view), d.data_ptr(), o.data_ptr(), _ptr(img), _ptr(w), self._block_coords.data_ptr(), self._pool[0].data_ptr(),
                      self._pool[1].data_ptr(), _ptr(self._pool[2]))

    # ---- extraction ----

    @torch.no_grad()
    def extract_mesh(self, min_weight=1.0):
        """The surface tsdf = 0 by marching tetrahedra over the cells of the unbounded lattice whose 8 corners all have wsum >=
        min_weight -> (vertices [V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 or None), on the volume's device: the mesh
        TSDFVolume.extract_mesh gives on a dense volume with the same values, in another order -- vertices ascend by (block key of the
        owning lattice point, its index within the block, edge slot), faces by (block key of the cell's lowest corner, index,
        tetrahedron).  Cells reach across blocks, so the mesh is welded across them.  min_weight must be > 0: a point in no block has
        weight 0 and must not count as observed.  Synchronises once, to learn V and F."""
        who = "SparseTSDFVolume.extract_mesh"
        mw = float(min_weight)
        if not mw > 0.0:
            raise ValueError("%s: min_weight must be > 0, got %r" % (who, min_weight))
        dev = self.device
        desc = self._desc()
        counts = (ctypes.c_longlong * 3)(0, 0, 0)
        temp = None
        table = (self._table[0].data_ptr(), self._table[1].data_ptr(), self._pool[0].data_ptr(), self._pool[1].data_ptr())
        if self._nb:
            temp = torch.empty(int(_lib.lib().adgs_sparse_tsdf_extract_temp_bytes(self._nb)), dtype=torch.uint8, device=dev)
            _lib.call("adgs_sparse_tsdf_extract_count", dev, ctypes.byref(desc), *table, mw, temp.data_ptr(), counts)
        V, F, E = int(counts[0]), int(counts[1]), int(counts[2])
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        colors = None if self._pool[2] is None else torch.empty((V, 3), dtype=torch.float32, device=dev)
        if V:
            owners = torch.empty(int(_lib.lib().adgs_sparse_tsdf_extract_owner_bytes(E)), dtype=torch.uint8, device=dev)
            _lib.call("adgs_sparse_tsdf_extract_emit", dev, ctypes.byref(desc), *table, _ptr(self._pool[2]), mw, temp.data_ptr(), owners.data_ptr(), counts,
                      _ptr(vertices), _ptr(faces), _ptr(colors))
        return vertices, faces, colors

    @torch.no_grad()
    def to_dense(self, lo_block, hi_block):
        """A dense TSDFVolume over the blocks lo_block <= b < hi_block (three integers each): its lattice point (i, j, k) is this
        volume's 8 lo_block + (i, j, k), with the stored values where a block is allocated and tsdf 1 / wsum 0 elsewhere.  Its origin
        is origin + 8 voxel_size lo_block rounded to float32, so positions agree to the bit where that is exact."""
        who = "SparseTSDFVolume.to_dense"
        try:
            lo, hi = tuple(lo_block), tuple(hi_block)
        except TypeError:
            raise TypeError("%s: lo_block and hi_block must be three integers each" % who) from None
        if len(lo) != 3 or len(hi) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in lo + hi):
            raise TypeError("%s: lo_block and hi_block must be three integers each, got %r, %r" % (who, lo_block, hi_block))
        if any(not (-COORD_LIMIT <= l <= h <= COORD_LIMIT) for l, h in zip(lo, hi)):
            raise ValueError("%s: need -2^20 <= lo_block <= hi_block <= 2^20, got %r, %r" % (who, lo_block, hi_block))
        n = tuple(h - l for l, h in zip(lo, hi))
        origin = tuple(o + self.voxel_size * BLOCK * l for o, l in zip(self.origin, lo))
        dense = TSDFVolume(origin, self.voxel_size, tuple(BLOCK * v for v in n), trunc=self.trunc, max_weight=self.max_weight, color=self._has_color,
                           device=self.device)
        if self._nb and dense.tsdf.numel():
            b = self.block_coords.to(torch.int64) - torch.tensor(lo, dtype=torch.int64, device=self.device)
            inside = ((b >= 0) & (b < torch.tensor(n, dtype=torch.int64, device=self.device))).all(1)
            b, rows = b[inside], torch.nonzero(inside).reshape(-1)
            split = lambda t: t.view(n[2], BLOCK, n[1], BLOCK, n[0], BLOCK).permute(0, 2, 4, 1, 3, 5)
            split(dense.tsdf)[b[:, 2], b[:, 1], b[:, 0]] = self._pool[0][rows]
            split(dense.wsum)[b[:, 2], b[:, 1], b[:, 0]] = self._pool[1][rows]
            if self._has_color:
                for c in range(3):
                    split(dense.color[c])[b[:, 2], b[:, 1], b[:, 0]] = self._pool[2][rows, c]
        return dense
