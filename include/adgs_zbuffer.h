/*
 * adgs_zbuffer.h -- C ABI of the triangle-mesh z-buffer (libadgs_hip.so): the nearest face and its camera depth per pixel of a pinhole
 * view of an indexed triangle mesh, optionally its normal; perspective-correct interpolation of vertex attributes for the winners; per-face
 * visibility counts over views; and the compaction of a mesh by a per-face mask.  It is what culls the faces no camera saw after
 * adgs_tsdf_extract, and what gives depth / normal maps of the final surface.
 *
 * Conventions of include/adgs_mesh.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched; the last parameter is the stream; an empty
 * problem (H W = 0; for count_faces also F = 0) returns 0 and launches nothing.  Only adgs_zbuffer_keep_faces_count reads back (once).
 * Nothing here is differentiable.
 *
 * Input.  vertices [V, 3] float, faces [F, 3] int32, on the device; V, F < 2^31.  A view (adgs_zbuffer_view): H, W with H W < 2^31, tanfovx,
 * tanfovy, pose = R row-major then t, world to camera (as adgs_tsdf_view), near > 0, max_depth > 0 (infinity: no limit), cull (0: none,
 * 1: back faces), small_max (0: the default; see Work distribution) and stages (0: everything; see there).
 *
 * Per face, its corners in their own order:
 *   1. a face with an index outside [0, V) is NEVER DEREFERENCED; it is counted in counts[0].
 *   2. X_c = ((r0 x + r1 y) + r2 z) + t per row, in double from the float inputs.  If any corner has a component of X_c that is not finite,
 *      or X_c.z < near, the whole face is rejected and counted in counts[1].  THERE IS NO NEAR-PLANE CLIPPING: a face that crosses the near
 *      plane is not drawn at all.  (The near plane of the pipeline is 0.2 m and fused triangles are voxel-sized: the lost band lies outside
 *      any real image.)
 *   3. u = (X_c.x / X_c.z) / tanfovx * (W / 2) + (W - 1) / 2, v likewise with tanfovy and H, in double in that order: the pixel convention of
 *      adgs_tsdf.h and adgs_multiview.h, pixel centres at the integers.
 *   4. guard band: unless |u| <= 16384 and |v| <= 16384 for all three corners (NaN and infinity fail), the face is rejected and counted in
 *      counts[2].
 *   5. snap to a 1/256-pixel lattice: U = rint(256 u), V = rint(256 v), round half to even, as integers.  All differences fit in int32 and
 *      every product below is 32 x 32 -> 64 bits.
 *   6. A = (U1 - U0)(V2 - V0) - (V1 - V0)(U2 - U0).  A = 0: degenerate, not drawn, counted in counts[3].
 *   7. facing: A has the sign of det[p0, p1, p2] / (z0 z1 z2), so a face whose geometric normal (p1 - p0) x (p2 - p0) points towards the
 *      camera has A < 0.  With cull = 1 the faces with A > 0 are not drawn and are counted in counts[4].
 *   A face is counted in the first of the five counters that applies.
 *
 * Coverage.  Pixel (px, py) samples P = (256 px, 256 py).  With s = sign(A), for the edges (a, b) = (1, 2), (2, 0), (0, 1):
 *   d = s (U_b - U_a, V_b - V_a),  E = d.x (P.y - V_a) - d.y (P.x - U_a);  E0 + E1 + E2 = |A|.
 *   The pixel is covered iff for every edge E > 0, or E = 0 and (d.y > 0, or d.y = 0 and d.x > 0).  Integer-exact: of two equally oriented
 *   faces that share an edge exactly one takes a centre on it.
 * Depth.  q_i = 1 / z_i in double, once per face; S = (E0 q0 + E1 q1) + E2 q2, the E_i converted exactly and every product rounded on its
 *   own; depth = (float)((double)|A| / S), the camera z at the sample.  The sample is dropped unless depth <= max_depth.
 * Winner.  key = (uint64)bits(depth) << 32 | f; a pixel's result is the MINIMUM key over the faces that cover it: the nearest depth, ties to
 *   the lowest face index.  The minimum commutes: every output is a function of the inputs alone, equal as bits from run to run and in any
 *   face order.  face [H, W] int32 (-1: nothing), depth [H, W] float (0: nothing).
 * Normal map [3, H, W] (optional): for the winner n = R ((p1 - p0) x (p2 - p0)), differences, products and sums in double, normalised in
 *   double, negated when n . X_c(p0) > 0 (so a fronto-parallel plane gives (0, 0, -1), the convention of adgs_normals.h), rounded once.
 *   0 where there is no winner.
 * The object file is built without FMA contraction: face is equal as integers, depth and the interpolated attributes as bits, to a
 * float64 / int64 evaluation in the stated order (only IEEE + - * /, rint and conversions occur); the normals take a square root and are
 * within 2^-23 absolute.
 *
 * adgs_zbuffer_draw: fill, draw, resolve on the stream; no read-back, no synchronisation.  counts [5] int64 ON THE DEVICE is set (not
 *   added to).  temp: adgs_zbuffer_temp_bytes(H, W, F) <= 8 H W + 4 F + 2048 bytes: the keys, the list of big faces, its counters.
 *   Work distribution.  Setup is one lane per face; a face whose clipped bounding box holds no pixel centre (n = 0) ends there.  Faces with
 *   n <= small_max (default 64; at most 4096) are expanded by their wave: a prefix sum of n over the wave, then the lanes walk the (face,
 *   pixel) pairs 64 at a time.  The others go to a list (one atomic per wave) that a second launch with a fixed grid works through: a
 *   workgroup per listed face, its waves on 8 x 8 pixel tiles; faces of more than 256 tiles are shared by all workgroups.  A tile is rejected
 *   from the edge functions' maxima over it before a pixel is touched.  A sample loads the pixel's key and only issues the 64-bit atomic
 *   minimum when its own is smaller.
 *   stages: a bit mask for timing experiments, 1 fill, 2 setup + small faces, 4 big faces, 8 resolve; 0 = 15 = all.  With a partial mask
 *   the outputs are not what is defined above.
 *   Refused: a NULL view, struct_bytes too small, negative H, W, V or F, H W >= 2^31, a tanfov or near that is not finite and > 0, max_depth
 *   not > 0, a pose entry that is not finite, cull outside {0, 1}, small_max outside [0, 4096], stages outside [0, 15], a NULL faces with
 *   F > 0, a NULL vertices with V > 0 and F > 0, a NULL temp / face / depth / counts.
 *
 * adgs_zbuffer_interpolate: attributes [V, C] float -> out [C, H, W] for the winners in face_map (what draw wrote for THIS mesh and view):
 *   E_i and q_i are recomputed by the same device functions; a = (((E0 q0) a0 + (E1 q1) a1) + (E2 q2) a2) / S in double, rounded once.
 *   `background` where face_map is negative (or, defensively, names a face the view would not draw).
 *   Refused: as draw for the view and sizes, C < 0, a NULL face_map or out with C > 0, a NULL attributes / vertices with V > 0, F > 0 and
 *   C > 0, a NULL faces with F > 0 and C > 0.  C = 0 returns 0.
 *
 * adgs_zbuffer_count_faces: for one resolved face_map [H, W] adds into views [F] int32 1 for every face that won at least one pixel and
 *   into pixels [F] int64 the number of pixels it won.  scratch [F] int32 must be ZERO on entry and is left zero.  Integer atomics only,
 *   aggregated per run of equal faces along a wave's pixels: exact and reproducible.  Entries of face_map outside [0, F) are ignored.
 *   Refused: negative H, W or F, H W >= 2^31, a NULL pointer with H W > 0 and F > 0.
 *
 * adgs_zbuffer_keep_faces_count: the face-mask twin of adgs_mesh_keep_count (it lives in csrc/mesh.hip and fills the SAME temp,
 *   adgs_mesh_keep_temp_bytes(V, F)): face f stays when face_keep[f] != 0 and its three indices lie in [0, V); a vertex stays when a face
 *   that stays uses it.  Two scans and ONE read-back (it synchronises the stream): counts[0] = V', counts[1] = F', counts[2] = the number of
 *   faces with face_keep[f] != 0 that were dropped for an index outside [0, V).  adgs_mesh_keep_emit(V, F, ..., temp, counts, ...) then
 *   writes the mesh, unchanged: faces in their order and corner order, vertices renumbered densely in their order, attributes bit for bit;
 *   a canonical mesh stays canonical.
 *   Refused: negative V or F, a NULL faces or face_keep with F > 0, a NULL temp with V > 0 or F > 0, a NULL counts.
 */
#ifndef ADGS_ZBUFFER_H
#define ADGS_ZBUFFER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_ZBUFFER_GUARD 16384            /* |u|, |v| of every corner, in pixels */
#define ADGS_ZBUFFER_SUBPIXEL 256           /* lattice points per pixel */
#define ADGS_ZBUFFER_SMALL_MAX 64           /* the default of small_max (tools/zbuffer_ab.py; EXPERIMENTS.md) */

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_zbuffer_view) of the caller */
	int H, W;
	int cull;                           /* 0: none, 1: back faces (A > 0) */
	int small_max;                      /* 0: ADGS_ZBUFFER_SMALL_MAX */
	int stages;                         /* 0: all */
	double tanfovx, tanfovy;
	double near;
	float max_depth;
	int reserved;                       /* keeps pose 8-byte aligned; 0 */
	double pose[12];                    /* R row-major, then t: world to camera */
} adgs_zbuffer_view;

size_t adgs_zbuffer_temp_bytes(long long H, long long W, long long F);
int adgs_zbuffer_draw(const adgs_zbuffer_view* view, int V, int F, const float* vertices, const int* faces, void* temp, int* face, float* depth,
	float* normal, long long* counts, void* stream);
int adgs_zbuffer_interpolate(const adgs_zbuffer_view* view, int V, int F, const float* vertices, const int* faces, const int* face_map, int C,
	const float* attributes, float background, float* out, void* stream);
int adgs_zbuffer_count_faces(int H, int W, int F, const int* face_map, int* scratch, int* views, long long* pixels, void* stream);
int adgs_zbuffer_keep_faces_count(int V, int F, const int* faces, const unsigned char* face_keep, void* temp, long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
