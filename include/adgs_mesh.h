/*
 * adgs_mesh.h -- C ABI of the mesh clean-up step (libadgs_hip.so): connected components of an indexed triangle mesh on the device, the
 * removal of components (what 2DGS's post_process_mesh does with Open3D on the host), and area-weighted vertex normals.
 *
 * Conventions of include/adgs_loss.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched (of the two entries that read back,
 * adgs_mesh_label refuses after its one read-back a mesh whose "faces index outside the vertices"; both would refuse a count above
 * INT_MAX, which cannot occur: the counts are bounded by V and F); the last parameter is the stream; an empty problem returns 0 and
 * launches nothing.
 * Nothing here is differentiable.
 *
 * Input.  vertices [V, 3] float, faces [F, 3] int32, optionally colors [V, 3] and normals [V, 3] float, on the device; V, F < 2^31.
 * Unused vertices and faces with a repeated index are allowed.  A face with an index outside [0, V) is NEVER DEREFERENCED: every kernel
 * checks the three indices before use and skips the face (a check, not a clamp).  adgs_mesh_label counts such faces and refuses the mesh.
 *
 * Components.  Two vertices are connected when a face contains both; a component is a connected set of vertices with all faces on them;
 * an unused vertex is a component with 0 faces.  This is VERTEX connectivity: Open3D's cluster_connected_triangles joins triangles that
 * share an EDGE.  On a welded marching-tetrahedra mesh the two differ only at pinch points (two sheets that touch in one vertex are one
 * component here, two there).  Components are numbered 0 .. C-1 by ascending smallest vertex index, the component's "root".
 *   adgs_mesh_label: lock-free union-find over the faces (csrc/mesh.hip), flatten, root flags, scan, vertex_component [V] int32; reads
 *     back ONCE (it synchronises the stream): counts[0] = C, counts[1] = the number of faces with an index outside [0, V); with
 *     counts[1] > 0 it returns a negative code AFTER filling counts ("... N faces index outside the V vertices").
 *   adgs_mesh_table: root [C], num_faces [C], num_vertices [C] int32 and, with vertices, area [C] double: the sum over the component's
 *     faces of 0.5 |(p1 - p0) x (p2 - p0)|, formed in double from the float positions.  It needs the `temp` the label left behind.
 *   vertex_component, root, num_faces and num_vertices are a function of the mesh alone, EQUAL from run to run; area is summed with double
 *   atomics in arrival order and is NOT (its error is bounded by (n_c + 8) 2^-52 sum 0.5 |p1 - p0| |p2 - p0|).
 *   Scratch: adgs_mesh_label_temp_bytes(V, F) <= 4 V + (V / 256 + 8192): the parent array, the scan's block sums, the counters.
 *   Refused: negative V or F, a NULL faces with F > 0, a NULL temp / vertex_component with V > 0, a NULL counts; by the table also C outside
 *   [0, V], a NULL root / num_faces / num_vertices with C > 0, area without vertices or vertices without area.
 *
 * Keep.  Given keep [C] (one byte per component, non-zero = kept), every vertex and face of a component that is not kept is dropped, the
 * remaining vertices are renumbered densely in their order, the faces keep their order and their corner order, and vertices, colors and
 * normals are gathered bit for bit.  A mesh in adgs_tsdf_extract's canonical order stays canonical; faces is reproducible to the integer.
 *   adgs_mesh_keep_count: flags, two scans, ONE read-back (it synchronises the stream: the outputs must be allocated): counts[0] = V',
 *     counts[1] = F'.  adgs_mesh_keep_emit writes the outputs from the `temp` the count left behind.
 *   Scratch: adgs_mesh_keep_temp_bytes(V, F) <= 4 (V + F) + ((V + F) / 256 + 16384): the two flag arrays, scanned in place, and the scan's block sums.
 *   Refused: negative V, F or C, C > V, a NULL faces with F > 0, a NULL vertex_component with V > 0, a NULL keep with C > 0, a NULL temp
 *   with V > 0, a NULL counts; by emit also counts outside [0, V] x [0, F], a NULL vertices with V > 0, a NULL output with a non-empty result,
 *   colors without colors_out (or the reverse), the same for normals.
 *
 * Vertex normals.  n_v = normalise(sum over the corners (f, c) with faces[f][c] = v, in ascending (f, c), of (p1 - p0) x (p2 - p0)), p0, p1, p2
 * the corners of f in its own order: area-weighted.  Differences, products and the sum are double from the float positions; the result is
 * rounded to float ONCE.  With S_v = sum |p1 - p0| |p2 - p0| over the same corners, n_v = (0, 0, 0) when S_v = 0 or |sum| <= 2^-40 S_v.
 * Faces from adgs_tsdf_extract are oriented towards free space, so these normals are too.  NO FLOAT ATOMICS: the 3 F (vertex, corner id =
 * 3 f + c) pairs are sorted by vertex with the stable radix sort, so every vertex's row ascends in (f, c), and one thread per vertex sums
 * its row in that order: the result is REPRODUCIBLE TO THE BIT.  Corners of a face with an index outside [0, V) get the key V and are read
 * by nobody.  No read-back, no synchronisation.
 *   Scratch: adgs_mesh_normals_temp_bytes(V, F) <= 49 F + 16384: two copies of the 3 F keys and values (the sort ping-pongs) and
 *   the sort's histograms.
 *   Refused: negative V or F, a NULL normals / vertices with V > 0, a NULL faces or temp with F > 0.
 */
#ifndef ADGS_MESH_H
#define ADGS_MESH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t adgs_mesh_label_temp_bytes(long long V, long long F);
int adgs_mesh_label(int V, int F, const int* faces, void* temp, int* vertex_component, long long* counts, void* stream);
int adgs_mesh_table(int V, int F, int C, const int* faces, const float* vertices, const int* vertex_component, const void* temp, int* root,
	int* num_faces, int* num_vertices, double* area, void* stream);
size_t adgs_mesh_keep_temp_bytes(long long V, long long F);
int adgs_mesh_keep_count(int V, int F, int C, const int* faces, const int* vertex_component, const unsigned char* keep, void* temp,
	long long* counts, void* stream);
int adgs_mesh_keep_emit(int V, int F, const int* faces, const float* vertices, const float* colors, const float* normals, const void* temp,
	const long long* counts, float* vertices_out, int* faces_out, float* colors_out, float* normals_out, void* stream);
size_t adgs_mesh_normals_temp_bytes(long long V, long long F);
int adgs_mesh_vertex_normals(int V, int F, const float* vertices, const int* faces, void* temp, float* normals, void* stream);

#ifdef __cplusplus
}
#endif
#endif
