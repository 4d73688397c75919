/*
 * adgs_sparse_tsdf.h -- C ABI of the block-sparse TSDF volume (libadgs_hip.so): the fusion and the marching tetrahedra of
 * include/adgs_tsdf.h on an UNBOUNDED lattice of which only the 8 x 8 x 8 blocks near an observed surface are stored.  Memory and the work
 * of a view grow with the surface area, not with a bounding box.
 *
 * Conventions of include/adgs_tsdf.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched; the last parameter is the stream; an empty
 * problem returns 0 and launches nothing.  Nothing here is differentiable.
 *
 * Lattice.  X(i, j, k) = origin + voxel_size (i, j, k) with SIGNED integer indices, formed in double from the float fields exactly as
 * include/adgs_tsdf.h forms it.  The block b = (bx, by, bz) holds the 8 x 8 x 8 points 8 b + l, l in [0, 8)^3, and covers the half-open
 * box [8 b, 8 b + 8) in lattice units.  Each block coordinate lies in [-2^20, 2^20).  The block key is
 *     ((bz + 2^20) << 42) | ((by + 2^20) << 21) | (bx + 2^20)
 * z-major, like the dense linear index.
 *
 * Storage (the caller owns every array).  The pool: tsdf [cap, 8, 8, 8] and wsum [cap, 8, 8, 8] (z, y, x; x fastest) and optionally
 * color [cap, 3, 8, 8, 8], float.  A new block is initialised BY THE CALLER to tsdf 1, wsum 0, colour 0.  block_coords [NB, 3] int32 in
 * pool order.  The TABLE is the NB keys in ascending order (uint64) with each one's pool slot (int32).  Pool order is allocation order:
 * the blocks one call allocates are appended in ascending key order; a block never moves, so a larger pool that holds a copy of the
 * first NB rows is the same volume.  NB <= ADGS_SPARSE_TSDF_MAX_BLOCKS = 2^22.  A lattice point in no allocated block is, by definition,
 * a point with tsdf 1 and wsum 0.
 *
 * adgs_sparse_tsdf_volume: num_blocks = NB; capacity = the rows of the pool (>= NB wherever the pool is given); table_capacity = the
 * entries each of keys_out, slots_out and block_coords has room for in an allocating call.
 *
 * Allocation from a view (adgs_sparse_tsdf_allocate_view).  The view is an adgs_tsdf_view.  A pixel (xi, yi) qualifies when it passes gates
 * 4-5 of include/adgs_tsdf.h: O >= min_opacity, D > 0, w > 0, z_d = O / D (inv_depth) or D / O <= max_depth.  It contributes samples
 * along its own central ray at the camera depths z_m = z_d - trunc + m (2 trunc / n), m = 0..n, n = ceil(trunc / voxel_size) (at most
 * ADGS_SPARSE_TSDF_MAX_STEPS); samples with z_m <= near are dropped.  A sample is X_c = ((xi - cx) / kx, (yi - cy) / ky, 1) z_m with
 * kx = W / (2 tanfovx), cx = (W - 1) / 2 (and so for y), taken to the world with the transposed pose, X_w = R^T (X_c - t), in double.
 * With g = (X_w - origin) / voxel_size and rho = `margin` (in voxels, 0 <= margin <= 4), the sample marks every block that intersects
 * the cube [g - rho, g + rho]^3: per axis floor((g - rho) / 8) .. floor((g + rho) / 8), at most 2 per axis and 8 in all.  A sample
 * with a block coordinate outside [-2^20, 2^20) (or not finite) marks nothing and is COUNTED (counts[2]); it is never wrapped.  The marked
 * blocks that are not in the table are the view's new blocks.
 *   One lane per pixel; per sample a wave reduces its lanes' keys to the distinct ones, drops those in the table (lower-bound search)
 *   and counts the rest; scan; emit; stable radix sort; head flags; compaction; a merge by rank of the old table with the new keys
 *   into keys_out / slots_out (the inputs are left alone, so a failed call changes nothing), and the coordinates of the new blocks into
 *   block_coords [NB ...].  No hash table, no atomics on values.
 *   The candidates (distinct keys per wave and sample, before the sort) go to scratch of `max_candidates` keys.  The call reads counts
 *   back ONCE (it synchronises the stream): counts[0] = the new blocks, counts[1] = the candidates the view has, counts[2] = the skipped
 *   samples, counts[3] = 1 when there was no room, else 0.  When counts[1] > max_candidates or NB + counts[0] > min(table_capacity, 2^22), NOTHING WAS ALLOCATED
 *   (keys_out / slots_out / block_coords [NB ...] hold no result) and the return value is 1: call again with more room.
 *
 * adgs_sparse_tsdf_allocate_blocks: the same from coords [M, 3] int32 on the device; duplicates and blocks in the table are dropped, the
 * rest are appended in ascending key order; a coordinate outside the range is counted in counts[2] and skipped.  max_candidates is M.
 *
 * adgs_sparse_tsdf_integrate: one rendered view into every allocated block, ONE launch, one workgroup per block in pool order, a wave per
 * z-slice of 8 x 8 points (256 contiguous bytes per array).  Every point of every allocated block goes through steps 1-9 of
 * include/adgs_tsdf.h, unchanged, with X from the global index 8 b + l; the chain is the same device function as the dense kernel's,
 * built with the same flags, so where both volumes hold a point and received the same views the stored values are equal as bits.  A
 * skipped point is NOT WRITTEN.  A whole block is skipped only when its bounding sphere proves that every one of its points fails steps
 * 1-3 (behind `near`, or outside the frustum widened by a pixel).  No atomics; there is no table lookup.
 *
 * Extraction: the marching tetrahedra of include/adgs_tsdf.h on the unbounded lattice, with unallocated points as defined above: the
 * same cells, tets, slots, vertex rule, triangle rule and orientation.  min_weight must be > 0: with min_weight <= 0 an unobserved
 * (hence any unallocated) point would count as valid.  Order: vertices ascend by (block key of the owner, local index (lz 8 + ly) 8 +
 * lx, slot); faces by (block key of the cell's lowest corner, local index, tet, triangle).  The mesh is therefore the mesh the dense
 * extraction gives on any dense volume holding the same values (1 / 0 elsewhere), up to this reordering.
 *   adgs_sparse_tsdf_extract_count counts, scans and reads the totals back ONCE: counts[0] = V, counts[1] = F, counts[2] = the blocks
 *   that own a vertex.  adgs_sparse_tsdf_extract_emit writes the mesh; it needs the `temp` the count left behind, the same volume, table
 *   and min_weight, and `owners`.
 *   Scratch.  temp: adgs_sparse_tsdf_extract_temp_bytes(NB) <= 16 NB + 4096 bytes; owners: adgs_sparse_tsdf_extract_owner_bytes(counts[2])
 *   = 2048 counts[2] bytes.  Neither grows with a box.
 *
 * Refused by every entry that takes them: a NULL vol or a NULL required array, struct_bytes too small, a voxel_size that is not finite and
 * > 0, an origin entry that is not finite, num_blocks, capacity or table_capacity negative or above 2^22, num_blocks > capacity (where
 * the pool is given).  By the view entries also what adgs_tsdf_integrate refuses of a view, trunc / voxel_size above
 * ADGS_SPARSE_TSDF_MAX_STEPS, and (allocate_view) a margin outside [0, 4], a max_candidates outside [1, 2^31 - 1].  By integrate:
 * image without color or color without image.  By the extraction: min_weight not > 0 (NaN included); by emit also negative counts or
 * counts above what the count call can return for NB blocks, a NULL owners with counts[2] > 0, a NULL vertices with V > 0 or faces with
 * F > 0, color without colors or colors without color.
 */
#ifndef ADGS_SPARSE_TSDF_H
#define ADGS_SPARSE_TSDF_H
#include <stddef.h>
#include <stdint.h>
#include "adgs_tsdf.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_SPARSE_TSDF_BLOCK 8                    /* lattice points of a block along each axis */
#define ADGS_SPARSE_TSDF_BLOCK_POINTS 512
#define ADGS_SPARSE_TSDF_MAX_BLOCKS 4194304         /* 2^22 */
#define ADGS_SPARSE_TSDF_COORD_LIMIT 1048576        /* 2^20: block coordinates lie in [-2^20, 2^20) */
#define ADGS_SPARSE_TSDF_MAX_STEPS 64               /* the largest n = ceil(trunc / voxel_size) */
#define ADGS_SPARSE_TSDF_OWNER_BYTES_PER_BLOCK 2048

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_sparse_tsdf_volume) of the caller */
	int num_blocks;
	int capacity;
	int table_capacity;
	float voxel_size;
	float origin[3];
} adgs_sparse_tsdf_volume;

size_t adgs_sparse_tsdf_allocate_temp_bytes(long long pixels, long long max_candidates);
int adgs_sparse_tsdf_allocate_view(const adgs_sparse_tsdf_volume* vol, const adgs_tsdf_view* view, float margin, const float* depth,
	const float* opacity, const float* weight, const uint64_t* keys, const int* slots, uint64_t* keys_out, int* slots_out, int* block_coords,
	long long max_candidates, void* temp, long long* counts, void* stream);
int adgs_sparse_tsdf_allocate_blocks(const adgs_sparse_tsdf_volume* vol, const int* coords, long long M, const uint64_t* keys, const int* slots,
	uint64_t* keys_out, int* slots_out, int* block_coords, void* temp, long long* counts, void* stream);
int adgs_sparse_tsdf_integrate(const adgs_sparse_tsdf_volume* vol, const adgs_tsdf_view* view, const float* depth, const float* opacity,
	const float* image, const float* weight, const int* block_coords, float* tsdf, float* wsum, float* color, void* stream);
size_t adgs_sparse_tsdf_extract_temp_bytes(long long num_blocks);
size_t adgs_sparse_tsdf_extract_owner_bytes(long long owner_blocks);
int adgs_sparse_tsdf_extract_count(const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots, const float* tsdf, const float* wsum,
	float min_weight, void* temp, long long* counts, void* stream);
int adgs_sparse_tsdf_extract_emit(const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots, const float* tsdf, const float* wsum,
	const float* color, float min_weight, const void* temp, void* owners, const long long* counts, float* vertices, int* faces, float* colors,
	void* stream);

#ifdef __cplusplus
}
#endif
#endif
