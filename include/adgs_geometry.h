/*
 * adgs_geometry.h -- C ABI of the geometry evaluation (libadgs_hip.so): an exact bounded nearest-neighbour search over a uniform grid of a
 * point set, area-weighted sampling of a triangle mesh, and the sums behind accuracy / completeness / Chamfer distance (the DTU protocol)
 * and precision / recall / F-score (the Tanks-and-Temples protocol).  What the published pipelines do with KD-trees on the host.
 *
 * Conventions of include/adgs_mesh.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched (adgs_geometry_grid_plan, the one entry that
 * reads back, refuses AFTER its read-back a box with more than 2^21 cells on an axis); the last parameter is the stream; an empty problem
 * returns 0 and launches nothing.  Nothing here is differentiable.  Counts M, N, V, F, n < 2^31.
 *
 * ---- Nearest neighbour ----
 * Definition.  d2(q, p) = (dx * dx + dy * dy) + dz * dz in float, ONE ROUNDING PER OPERATION (the object is built without FMA contraction),
 * dx = q.x - p.x.  A target p is a neighbour of q when (double)d2 <= (double)max_dist * (double)max_dist: the boundary is inclusive.  The
 * result is the neighbour with the smallest d2; ties go to the LOWEST ORIGINAL INDEX, whatever cell it lives in.  Without a neighbour
 * idx = -1 and dist2 = +inf.  A target with a non-finite coordinate is never a neighbour; a query with one gets -1 / +inf.  The results
 * are a function of the arguments alone: equal from run to run.
 *
 * Grid.  Cell coordinate = floor(((double)x - (double)origin) / (double)cell_size) per axis; origin = the minimum over the finite targets
 * (float); dims = the cell coordinate of the maximum + 1.  Key = (z * ny + y) * nx + x as uint64; a target that is not finite (or lies
 * outside origin / dims as passed) gets the key nx * ny * nz, sorts behind every cell and is read by nobody.
 *   adgs_geometry_grid_plan: one launch (minimum, maximum, number of finite targets) and ONE read-back (it synchronises the stream):
 *     origin[3], dims[3], *num_finite.  With no finite target (or M = 0, which launches nothing) dims = {0, 0, 0}.  Refused after the
 *     read-back: an axis with more than 2^21 cells ("... enlarge cell_size").
 *   adgs_geometry_grid_build: keys, the stable radix sort by key, a gather into sorted order as 16-byte records (x, y, z, original index
 *     as bits), and a COMPACT table of the occupied cells: cell_keys [<= M] ascending, cell_starts [<= M + 1] (the first record of the
 *     cell; one entry behind the last cell = the number of records in cells), counts[0] = the number of occupied cells, counts[1] = the
 *     number of records in cells.  Nothing dense in the number of cells.  No read-back.  x is the minor digit, so the up to 2 R + 1 cells
 *     of one (y, z) row are one contiguous run of the records: one lower-bound search of cell_keys per row.
 *   adgs_geometry_nearest: the queries are processed in the order of their own cell key (sorted by the same code), one lane per query,
 *     so the lanes of a wave walk the same rows; the update is (d2 < best) || (d2 == best && index < best_index).  No read-back.
 *
 * Search radius.  R = ceil(max_dist * (1 + 2^-20) / cell_size) cells, in double on the host.  Why no neighbour is missed: if the float d2
 * passes the test, |fl(dx)| <= max_dist (1 + 2^-23), and fl(dx) is within 2^-24 relative of the real difference, so the real |dx| is below
 * max_dist (1 + 2^-22); in cells that is below R (1 + 2^-22) / (1 + 2^-20) < R - R 2^-21.  The two cell coordinates are each formed with an
 * error below 2^-30 (three roundings at 2^-53 relative, coordinates below 2^21 cells), far less than that slack, and two reals less than R
 * apart have floors at most R apart.  So a pair that passes the test -- a pair exactly max_dist apart included -- is never separated by more
 * than R cells on any axis.  Every loop of the kernel is bounded by (2 R + 1)^2 rows, 2 R + 1 cells per row and the records in them; there
 * is no open-ended ring expansion.
 *   Refused: cell_size or max_dist not finite and positive; a dim outside [0, 2^21] ("... enlarge cell_size"); R > 8 ("... enlarge
 *   cell_size"); negative M or N; a NULL pointer that would be followed.
 *   M = 0 or dims = {0, 0, 0} gives every query -1 / +inf (one fill launch).  N = 0 launches nothing.
 *   Scratch: adgs_geometry_grid_temp_bytes(M) <= 30 M + 65536 (two copies of the keys and values, the head flags, the sort's histograms);
 *   adgs_geometry_nearest_temp_bytes(N) <= 26 N + 65536.  Both are 0 for a count outside [0, 2^31).
 *
 * ---- Surface sampling ----  All arithmetic in double from the float positions.
 *   Area (adgs_geometry_face_areas).  areas[f] = 0.5 |(p1 - p0) x (p2 - p0)|; the cross product is (ay bz - az by, az bx - ax bz,
 *     ax by - ay bx) with a = p1 - p0, b = p2 - p0, the norm sqrt((nx nx + ny ny) + nz nz).  A face with an index outside [0, V) is checked
 *     before every dereference, has area 0 and is therefore never sampled.
 *   Random words of sample k: u_j, j = 0, 1, 2, from the splitmix64 finaliser: z = seed + 0x9E3779B97F4A7C15 * (3 k + j + 1) (mod 2^64);
 *     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31; u_j = (z >> 11) * 2^-53.
 *   Face (adgs_geometry_sample).  cdf [F] double is the inclusive running sum of the areas, total = cdf[F - 1] (passed by the caller, so
 *     that it can be refused on the host).  t = min(u0 * total, the next double below total); the face is the first f with cdf[f] > t.  A
 *     face that adds nothing to the cdf is never chosen, the last face included.
 *   Point.  If u1 + u2 > 1 then u1 = 1 - u1, u2 = 1 - u2.  p = (p0 + u1 (p1 - p0)) + u2 (p2 - p0) per coordinate, rounded to float ONCE.
 *     Should a caller's cdf step at a face with an index outside [0, V), that sample is face -1 and point NaN; nothing is dereferenced.
 *   Refused: negative V, F or n; n > 0 with F = 0, or with a total that is not finite and positive; a NULL pointer that would be followed.
 *   n = 0 (and F = 0 for the areas) launches nothing.
 *
 * ---- Distance statistics ----
 *   adgs_geometry_distance_stats over dist2 [N] float (adgs_geometry_nearest's), thresholds[num_thresholds <= 4] and max_dist (doubles):
 *     out[0] = sum of min(d, max_dist), d = sqrt((double)d2); an element that is not below +inf (no neighbour) contributes max_dist
 *     out[1] = N;   out[2] = the number of elements without a neighbour
 *     out[3 + k] = the number of elements with (double)d2 < thresholds[k] * thresholds[k]: strict, in double, no square root
 *   out is 8 doubles on the device; the counts are summed as integers and are exact.  One kernel writes one partial row per workgroup over
 *   a FIXED partition of the index range (a function of N alone), a one-workgroup finish adds the rows in index order: no atomics, and
 *   out is REPRODUCIBLE TO THE BIT from run to run.  N = 0 launches only the finish, which writes zeros.  No read-back.
 *   Scratch: adgs_geometry_stats_temp_bytes(N) <= 65536.
 *   Refused: negative N, num_thresholds outside [0, 4], a threshold or max_dist that is not finite and positive, a NULL pointer.
 */
#ifndef ADGS_GEOMETRY_H
#define ADGS_GEOMETRY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t adgs_geometry_grid_temp_bytes(long long M);
int adgs_geometry_grid_plan(int M, const float* points, float cell_size, void* temp, float* origin, int* dims, long long* num_finite, void* stream);
int adgs_geometry_grid_build(int M, const float* points, float cell_size, const float* origin, const int* dims, void* temp, float* records,
	unsigned long long* cell_keys, unsigned int* cell_starts, unsigned int* counts, void* stream);
size_t adgs_geometry_nearest_temp_bytes(long long N);
int adgs_geometry_nearest(int M, int N, const float* queries, float max_dist, float cell_size, const float* origin, const int* dims,
	const float* records, const unsigned long long* cell_keys, const unsigned int* cell_starts, const unsigned int* counts, void* temp,
	float* dist2, int* idx, void* stream);
int adgs_geometry_face_areas(int V, int F, const float* vertices, const int* faces, double* areas, void* stream);
int adgs_geometry_sample(int V, int F, int n, const float* vertices, const int* faces, const double* cdf, double total,
	unsigned long long seed, float* points, int* face, void* stream);
size_t adgs_geometry_stats_temp_bytes(long long N);
int adgs_geometry_distance_stats(int N, const float* dist2, int num_thresholds, const double* thresholds, double max_dist, void* temp,
	double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
