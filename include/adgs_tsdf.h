/*
 * adgs_tsdf.h -- C ABI of the surface extraction step (libadgs_hip.so): TSDF fusion of rendered depth maps (Curless & Levoy 1996) into a
 * dense volume, and marching tetrahedra (Doi & Koide 1991) on that volume, returning an indexed, welded triangle mesh.
 *
 * Conventions of include/adgs_loss.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched (adgs_tsdf_extract_count refuses a mesh
 * that is too large after its one read-back); the last parameter is the stream; an empty problem returns 0 and launches nothing.
 * Nothing here is differentiable.
 *
 * Volume (adgs_tsdf_volume).  A lattice of nx x ny x nz points, X(i, j, k) = origin + voxel_size (i, j, k) in world coordinates, formed in
 * double from the float fields.  Three float device arrays, x fastest: tsdf [nz, ny, nx], initially 1; wsum [nz, ny, nx], initially 0;
 * optionally color [3, nz, ny, nx], initially 0.  The linear index of a lattice point is (k ny + j) nx + i; nx ny nz must be below 2^31.
 *
 * adgs_tsdf_integrate: one rendered view into the volume, ONE launch, one thread per lattice point, lanes along x.
 *   depth [H, W]: D; opacity [H, W]: O, as render() returns them; image [3, H, W] or NULL; weight [H, W] or NULL (= 1): the supervision
 *   weight of adgs.loss (zero over dynamic objects, sky, the ego vehicle); pose: R row-major then t, world to camera, X_c = R X + t.
 *   Per lattice point, in double from the float inputs:
 *   1. X_c = R X + t; skipped unless X_c.z > near
 *   2. (u, v) = the pixel of X_c as include/adgs_multiview.h defines it:
 *      ((X_c.x / X_c.z) / tanfovx * W / 2 + (W - 1) / 2, (X_c.y / X_c.z) / tanfovy * H / 2 + (H - 1) / 2)
 *   3. the NEAREST pixel xi = floor(u + 0.5), yi = floor(v + 0.5) (bilinear depth would smear across depth discontinuities); skipped
 *      unless 0 <= xi < W and 0 <= yi < H
 *   4. skipped unless O >= min_opacity, D > 0 and w > 0 at that pixel
 *   5. z_d = O / D (inv_depth) or D / O; skipped unless z_d <= max_depth (infinity: no limit)
 *   6. sdf = z_d - X_c.z; skipped if sdf < -trunc
 *   7. d = min(1, sdf / trunc)
 *   8. T <- (T Wsum + d w) / (Wsum + w), and each colour channel the same way from image at that pixel
 *   9. Wsum <- min(Wsum + w, max_weight)
 *   each stored value is rounded to float once.  A skipped point is NOT WRITTEN: its values keep their bits.  No atomics (a lattice point
 *   has one owner); nothing outside the images is read.
 *   Refused: a NULL vol / view / depth / opacity / tsdf / wsum, struct_bytes too small, negative sizes, nx ny nz >= 2^31, H W above
 *   INT_MAX, a tanfov, voxel_size or trunc that is not finite and > 0, min_opacity outside (0, 1], max_weight not > 0, near not finite
 *   and >= 0, a pose or origin entry that is not finite, image without color or color without image.
 *
 * Extraction: marching tetrahedra on the lattice.
 *   Cells.  Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is valid when all 8 corners have wsum >= min_weight.  A corner is inside
 *   when tsdf < 0.  A tsdf of exactly 0 is OUTSIDE: it puts vertices on the lattice point itself and may give zero-area triangles.
 *   Tetrahedra.  A cell c splits into the 6 Kuhn tetrahedra around its main diagonal: for the axis orders (x, y, z), (x, z, y), (y, x, z),
 *   (y, z, x), (z, x, y), (z, y, x), in this order, the tet (c, c + e_a, c + e_a + e_b, c + (1, 1, 1)), tet-vertex indices 0..3.  The split
 *   is the same in every cell, so the face diagonals of neighbouring cells agree and the surface has no cracks.
 *   Vertices.  A mesh vertex lies on a lattice edge and belongs to the edge's lower corner p; 7 edges per lattice point, slots in the
 *   order +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z.  The vertex exists when the two ends differ in sign and at least one valid cell contains
 *   the edge; some emitted triangle then uses it, so the mesh has no unused vertex.  Position origin + voxel_size (p + t (q - p)) with
 *   t = T_p / (T_p - T_q), formed in double; the colour is C_p + t (C_q - C_p).
 *   Triangles.  Per tet of a valid cell, e(m, n) being the vertex on the edge between tet vertices m and n:
 *     one inside, a, the outside ones o1 < o2 < o3:      (e(a, o1), e(a, o2), e(a, o3))
 *     three inside, i1 < i2 < i3, the outside one d:     (e(d, i3), e(d, i2), e(d, i1))
 *     two inside, a < b, the outside ones c < d:         q = (e(a, c), e(a, d), e(b, d), e(b, c)) -> (q0, q1, q2), (q0, q2, q3)
 *   and a triangle (p0, p1, p2) becomes (p2, p1, p0) where needed so that its right-hand normal points from the inside corners to the
 *   outside ones: towards free space, hence towards the cameras.  Which (tet, inside set) pairs need it is a constant of the split.
 *   Order.  Vertices ascend by (linear index of the owner, slot); faces by (linear index of the cell, tet, triangle).
 *   vertices [V, 3] float, faces [F, 3] int32, colors [V, 3] float.
 *
 *   adgs_tsdf_extract_count counts, scans and reads the totals back ONCE (it synchronises the stream: the outputs must be allocated;
 *   extraction is not a per-iteration operation): counts[0] = V, counts[1] = F, counts[2] = the number of 256-point chunks of the lattice
 *   that own a vertex.  V or F above INT_MAX is refused here.  adgs_tsdf_extract_emit then writes the mesh; it needs the `temp` the count
 *   left behind, the same volume and min_weight, and `owners`.
 *   Scratch.  temp: adgs_tsdf_extract_temp_bytes(vol) <= 16 ceil(nx ny nz / 256) + 4096 bytes; owners:
 *   adgs_tsdf_extract_owner_bytes(counts[2]) = 1024 counts[2] bytes.  Neither grows with a table over the cells of the lattice.
 *   Refused: a NULL vol / tsdf / wsum / temp / counts, struct_bytes too small, negative sizes, nx ny nz >= 2^31, a voxel_size that is not
 *   finite and > 0, an origin entry that is not finite; by emit also negative counts, a NULL owners with counts[2] > 0, a NULL vertices
 *   with V > 0 or faces with F > 0, color without colors or colors without color.
 */
#ifndef ADGS_TSDF_H
#define ADGS_TSDF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_TSDF_CHUNK 256                 /* lattice points of one workgroup of the extraction */
#define ADGS_TSDF_OWNER_BYTES_PER_CHUNK 1024

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_tsdf_volume) of the caller */
	int nx, ny, nz;
	float voxel_size;
	float origin[3];
} adgs_tsdf_volume;

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_tsdf_view) of the caller */
	int H, W;
	int inv_depth;
	float tanfovx, tanfovy;
	float min_opacity, near, max_depth;
	float trunc, max_weight;
	int reserved;                       /* keeps pose 8-byte aligned; 0 */
	double pose[12];                    /* R row-major, then t: world to camera */
} adgs_tsdf_view;

int adgs_tsdf_integrate(const adgs_tsdf_volume* vol, const adgs_tsdf_view* view, const float* depth, const float* opacity, const float* image,
	const float* weight, float* tsdf, float* wsum, float* color, void* stream);
size_t adgs_tsdf_extract_temp_bytes(const adgs_tsdf_volume* vol);
size_t adgs_tsdf_extract_owner_bytes(long long nonempty_chunks);
int adgs_tsdf_extract_count(const adgs_tsdf_volume* vol, const float* tsdf, const float* wsum, float min_weight, void* temp, long long* counts,
	void* stream);
int adgs_tsdf_extract_emit(const adgs_tsdf_volume* vol, const float* tsdf, const float* wsum, const float* color, float min_weight,
	const void* temp, void* owners, const long long* counts, float* vertices, int* faces, float* colors, void* stream);

#ifdef __cplusplus
}
#endif
#endif
