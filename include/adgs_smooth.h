/*
 * adgs_smooth.h -- C ABI of the one-ring adjacency of a triangle mesh and of Laplacian / Taubin smoothing over it (libadgs_hip.so): what
 * Open3D's filter_smooth_laplacian / filter_smooth_taubin do on the host, with uniform (umbrella) weights, and the structure that answers
 * "who are the neighbours of vertex v", "is v on a boundary" and "how many boundary or non-manifold edges does this mesh have".
 *
 * Conventions of include/adgs_simplify.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * -1 is a malformed call, decided on the host from the arguments alone before anything is launched; the last parameter is the stream; an
 * empty problem returns 0 and launches nothing.  adgs_smooth_adjacency_count reads back ONCE and refuses after that read-back with
 *   -2  a mesh with faces that index outside the vertices ("... N faces index outside the V vertices"), AFTER filling counts.
 * Nothing here is differentiable.
 *
 * Input.  faces [F, 3] int32 over V vertices, on the device; V < 2^31 and 6 F < 2^31 (a face emits six directed pairs, and the rows of the
 * adjacency are indexed with int32).
 *
 * ADJACENCY.
 * 1. Edges.  A face with an index outside [0, V) is NEVER DEREFERENCED: the three indices are checked first; it is counted (bad_faces), it
 *    contributes nothing, and the call is refused (-2) after the read-back.  Every other face contributes its three undirected edges
 *    {i0, i1}, {i1, i2}, {i2, i0}.  An edge with both ends equal is dropped; the face is then counted ONCE as degenerate
 *    (degenerate_faces) and its other edges still count, so (a, a, b) contributes {a, b} twice.  Duplicate faces contribute again:
 *    multiplicity counts.
 * 2. Incidence.  The incidence of an edge is the number of (face, edge slot) contributions to it.  An edge with incidence 1 is a BOUNDARY
 *    edge and both its ends are boundary vertices (boundary [V], one byte each, 0 or 1); an edge with incidence > 2 is NON-MANIFOLD.
 * 3. Rows.  neighbors of v is the SET of the vertices that share an edge with v, ascending and unique; starts [V + 1] is the CSR row
 *    table, starts[V] = len(neighbors) = 2 E with E the number of distinct edges.  A vertex with an empty row is isolated.
 * 4. How.  Every contribution emits both directed pairs as the keys (a << n | b) and (b << n | a), n the number of bits of V; a dropped
 *    pair gets the key V << n, which sorts behind every pair.  The 6 F keys are sorted with the radix sort on 2 n bits (five passes for a
 *    mesh of 2^19 vertices, where 32-bit fields would take seven).  A run of equal keys is one directed
 *    edge and its length is the incidence of the edge, since every contribution emitted both directions; the head of a run is an entry of
 *    neighbors, numbered by an exclusive scan of the head flags, whose total and the counters are the ONE read-back.  boundary is
 *    zero-filled and a run of length 1 stores 1 at its first end: plain stores of the same value, no atomics.  The counters are integer
 *    atomics, one per wave.  starts[v] is the first entry whose first end is >= v, found by bisection.
 *    Everything is an integer function of the mesh alone: REPRODUCIBLE TO THE INTEGER from run to run and in any face order.
 *
 * SMOOTHING.  The state is one DOUBLE triple per vertex; the float input is widened once.  One step with the factor s is, per component,
 *      S = ((0.0 + x_j1) + x_j2) + ...    over the row of i in ascending neighbour order
 *      x_i' = x_i + s * (S / d_i - x_i)   d_i the row length as a double
 *    -- one division, one subtraction, one multiplication, one addition, each rounded once: the file is built without FMA contraction.  A
 *    vertex with d_i = 0 or with fixed[i] != 0 keeps its value.  Every vertex of a step reads the state the PREVIOUS step left (Jacobi:
 *    two buffers, never in place).  adgs_smooth_steps runs `steps` steps, step k (from 0) with the factor s_even for even k and s_odd for
 *    odd k: Laplacian smoothing is `iterations` steps with s_even = s_odd = lambda, Taubin smoothing 2 * iterations steps with
 *    s_even = lambda, s_odd = mu.  The result is rounded to float ONCE at the end; steps = 0 copies the input's bits.  Non-finite values
 *    propagate as IEEE arithmetic dictates.  One lane per vertex walks its row in order (the order is part of the definition); one launch
 *    per step, the widening in the first and the rounding in the last; no atomics.  The output is REPRODUCIBLE TO THE BIT and equal to a
 *    plain double evaluation of the above.  The rows are read as given: an entry outside [0, V) is skipped, a row table that runs
 *    backwards or past N is clamped, so no table makes a kernel read outside the arrays -- but only adgs_smooth_adjacency_emit's output
 *    gives the definition above.
 *
 * Entries.
 *   adgs_smooth_adjacency_count: steps 1-4 up to the ONE read-back (it synchronises the stream).  Writes boundary [V] and
 *       counts[0] = N = 2 E, counts[1] = bad_faces, counts[2] = edges E, counts[3] = boundary_edges, counts[4] = nonmanifold_edges,
 *       counts[5] = degenerate_faces, counts[6] = isolated_vertices.
 *     V = 0 with F > 0: every face is outside the (empty) vertex set; counts[1] = F without reading any, and -2.
 *   adgs_smooth_adjacency_emit: from the `temp` the former left behind and its counts: starts [V + 1], neighbors [N].  No read-back.
 *   adgs_smooth_steps: the smoothing; no read-back, no synchronisation.  fixed [V] bytes or NULL (nothing fixed); out [V, 3] float, not
 *     the input.
 *   Scratch: 144 F <= adgs_smooth_adjacency_temp_bytes(V, F) <= 148 F + 16384, independent of V;
 *            64 V <= adgs_smooth_steps_temp_bytes(V, N) <= 64 V + 1024 (two buffers of one 32-byte row per vertex), independent of N.
 *     Both are 0 for sizes outside [0, 2^31), the former also for 6 F >= 2^31.
 *   Refused (-1): negative V or F; 6 F >= 2^31; a NULL counts; a NULL faces with F > 0; a NULL boundary with V > 0 (and temp, with F > 0 too); by emit also
 *   counts[0] negative, odd or above 6 F, a NULL starts with V > 0 or neighbors with N > 0; by steps a negative V, N or steps, steps above
 *   20000, a factor that is not finite, a NULL vertices / starts / out / temp with V > 0 (temp only with steps > 0), a NULL neighbors with
 *   N > 0, out == vertices.
 */
#ifndef ADGS_SMOOTH_H
#define ADGS_SMOOTH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t adgs_smooth_adjacency_temp_bytes(long long V, long long F);
int adgs_smooth_adjacency_count(int V, int F, const int* faces, void* temp, unsigned char* boundary, long long* counts, void* stream);
int adgs_smooth_adjacency_emit(int V, int F, const void* temp, const long long* counts, int* starts, int* neighbors, void* stream);
size_t adgs_smooth_steps_temp_bytes(long long V, long long N);
int adgs_smooth_steps(int V, int N, const float* vertices, const int* starts, const int* neighbors, const unsigned char* fixed, int steps,
	double s_even, double s_odd, void* temp, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
