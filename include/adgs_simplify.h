/*
 * adgs_simplify.h -- C ABI of mesh simplification by vertex clustering (libadgs_hip.so): Rossignac & Borrel's clustering of the vertices
 * on a lattice with Lindstrom's quadric placement of the representative, which is what Open3D's
 * simplify_vertex_clustering(contraction=Quadric) does on the host.  With a cell far below the vertex spacing the same operation only
 * welds coincident vertices (the duplicated seam vertices of meshes fused in blocks).
 *
 * Conventions of include/adgs_mesh.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * -1 is a malformed call, decided on the host from the arguments alone before anything is launched; the last parameter is the stream; an
 * empty problem returns 0.  adgs_simplify_cluster reads back ONCE and refuses after that read-back, with codes of their own,
 *   -2  a mesh with faces that index outside the vertices ("... N faces index outside the V vertices"),
 *   -3  a mesh with finite vertices whose cell cannot be keyed ("... enlarge cell_size or move origin"),
 * in both cases AFTER filling counts.  Nothing here is differentiable.
 *
 * Input.  vertices [V, 3] float, faces [F, 3] int32, optionally colors [V, 3] float, on the device; V, F < 2^31 (the placement also needs
 * 3 F < 2^32: corner ids are 32 bits).  cell_size > 0 (a float, used as a double), origin: three floats ON THE HOST (used as doubles).
 * The lattice is anchored at origin, not at the mesh: two meshes simplified with the same cell_size and origin share it.
 *
 * 1. Cell of a vertex.  Per axis c = floor(((double)x - origin) / (double)cell_size).  A vertex with a non-finite coordinate is DROPPED
 *    and counted (counts[3]).  A finite vertex with |c| >= 2^20 on an axis cannot be keyed in 63 bits: it is counted (counts[4]) and the
 *    call is refused (-3) after the read-back.  The key of a kept vertex is ((cx + 2^20) << 42) | ((cy + 2^20) << 21) | (cz + 2^20); every
 *    field lies in [1, 2^21), so the key 0 is free and marks a vertex that is not kept.
 * 2. Clusters.  A cluster is the set of kept vertices of one cell.  The (key, vertex id) pairs are sorted by key with the stable radix
 *    sort over 63 bits, always: the members of a cluster are in ascending vertex id, the smallest is the cluster's `root`.
 * 3. Faces.  A face with an index outside [0, V) is NEVER DEREFERENCED: the three indices are checked first; it is counted (counts[5])
 *    and the call is refused (-2) after the read-back.  A face with a corner on a dropped vertex is dropped (counts[6]).  The corners are
 *    mapped to clusters; a face with two corners in one cluster is degenerate and dropped (counts[7]).  Two remaining faces are duplicates
 *    when their cluster triples are equal after rotating the smallest index to the front -- the orientation is kept: (a, b, c) and
 *    (a, c, b) are NOT duplicates --; the first in face order stays, the others are dropped (counts[8]).  Two stable passes bring equal
 *    triples together in face order: a 32-bit sort on the third index, then a 64-bit sort on (first << 32 | second).  Kept faces keep
 *    their input order and their own corner order; the rotation is for the comparison only.
 * 4. Output numbering.  Only clusters used by a kept face become vertices (no unused vertex), numbered by ascending root: the used roots
 *    are flagged over the vertices and scanned.  A mesh in adgs_tsdf_extract's canonical order stays canonical; a mesh whose vertices all
 *    have cells of their own, every one used by a face, and without duplicate faces comes back unchanged.
 * 5. Placement (adgs_simplify_place), all in double from the float inputs, every result rounded to float ONCE.
 *    cbar = (sum of the members in ascending vertex id) / their number; the colour of the vertex is that mean of the member colours.
 *    placement 0 "average": the position is cbar.
 *    placement 1 "quadric": over every (face, corner) pair whose corner vertex is a member of the cluster, of a face with valid indices
 *      and nine finite coordinates -- the faces later dropped as degenerate or duplicate included, and a face with two corners in the
 *      cluster counted twice, as in Open3D --, in ascending corner id 3 f + k:
 *        a = p1 - p0, b = p2 - p0, k = a x b, L = |k|; skipped unless L > 0; n = k / L, w = L / 2, e = n . (p_corner - cbar)
 *        A += w n n^T, g += w e n, t += w
 *      e is taken at the corner's own vertex, so a cluster of one member has e = 0 exactly.  With t > 0, (A + lambda t I) delta = g is solved
 *      by Cholesky (SPD, condition number at most (1 + lambda) / lambda); otherwise delta = 0.  delta_k is clamped into
 *      [min(lo_k - cbar_k, 0), max(hi_k - cbar_k, 0)], lo_k = origin_k + c_k cell, hi_k = origin_k + (c_k + 1) cell, c the cell of the
 *      cluster: the clamp is continuous and delta = 0 survives it.  The position is cbar + delta.  The file is built without FMA
 *      contraction: every operation above rounds once.
 *    The 3 F (cluster, corner id) pairs are sorted by cluster with the stable 32-bit radix sort; one thread per cluster bisects to its row
 *    and sums it in order.  NO FLOAT ATOMICS anywhere; flags written by several lanes are plain stores of the same value; every device
 *    loop is a bisection or a run bounded by the array length; nothing waits on another workgroup.  Every output is REPRODUCIBLE TO THE BIT.
 *
 * Entries.
 *   adgs_simplify_cluster: steps 1-4 up to the ONE read-back (it synchronises the stream: the outputs must be allocated).  It writes
 *     vertex_cluster [V] int32 (the output vertex of each input vertex, -1 for a vertex that is not in the output) and
 *       counts[0] = V2, counts[1] = F2, counts[2] = M = the sum of the member counts of the V2 clusters,
 *       counts[3] = non-finite vertices, counts[4] = vertices that cannot be keyed, counts[5] = faces with an index outside [0, V),
 *       counts[6] = dropped faces, counts[7] = degenerate faces, counts[8] = duplicate faces.
 *   adgs_simplify_cluster_emit: from the `temp` the former left behind and its counts: root [V2], num_vertices [V2], member_starts [V2 + 1],
 *     members [M] (the CSR of the members in ascending vertex id), faces_out [F2, 3], face_source [F2] (the input face of each output face).
 *   adgs_simplify_place: step 5; no read-back, no synchronisation.  colors and colors_out are given together or not at all.
 *   Scratch: 28 V + 24 F + 16 max(V, F) <= adgs_simplify_cluster_temp_bytes(V, F) <= 45 (V + F) + 65536;
 *            48 F <= adgs_simplify_place_temp_bytes(V, F) <= 49 F + 16384.  Both are 0 for sizes outside [0, 2^31).
 *   Refused (-1): negative V or F; a cell_size that is not a positive finite number; a NULL origin or counts; a NULL vertices / temp /
 *   vertex_cluster with V > 0; a NULL faces with F > 0; by emit also counts outside [0, V] x [0, F] x [0, V] or with M < V2, a NULL output
 *   of a non-empty result (member_starts whenever V > 0); by place V2 outside [0, V], M outside [V2, V], 3 F >= 2^32, a placement other
 *   than 0 or 1, a regularization that is not a positive finite number, a NULL input or output of a non-empty result, colors without
 *   colors_out or the reverse, a NULL temp with F > 0.
 */
#ifndef ADGS_SIMPLIFY_H
#define ADGS_SIMPLIFY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t adgs_simplify_cluster_temp_bytes(long long V, long long F);
int adgs_simplify_cluster(int V, int F, const float* vertices, const int* faces, float cell_size, const float* origin, void* temp,
	int* vertex_cluster, long long* counts, void* stream);
int adgs_simplify_cluster_emit(int V, int F, const int* faces, const int* vertex_cluster, const void* temp, const long long* counts, int* root,
	int* num_vertices, int* member_starts, int* members, int* faces_out, int* face_source, void* stream);
size_t adgs_simplify_place_temp_bytes(long long V, long long F);
int adgs_simplify_place(int V, int F, int V2, int M, const float* vertices, const int* faces, const float* colors, const int* vertex_cluster,
	const int* member_starts, const int* members, float cell_size, const float* origin, int placement, double regularization, void* temp,
	float* vertices_out, float* colors_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
