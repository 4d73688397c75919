// Mesh simplification by vertex clustering on the device for gfx950 (wave64).  The definition is in include/adgs_simplify.h.
//
//   cluster  cell keys -> stable 63-bit sort of (key, vertex) -> head flags -> scan -> cluster of every vertex, start of every cluster
//   faces    cluster triples, smallest first -> stable sort on the third index, then on (first, second) -> equal triples adjacent, in face
//            order -> keep flags -> used roots flagged over the vertices -> three scans (vertices, member counts, faces) -> ONE read-back
//   emit     roots, member CSR, renumbered faces from the scans
//   place    3 F (cluster, corner) pairs -> stable sort by cluster -> one thread per cluster sums its members and its corner row in order
// Every kernel that reads `faces` checks the three indices against V before it uses them (load_face, mesh_shared.h).  Counters are integer
// atomics (one per wave); there is no float atomic, and a flag written by several lanes is a plain store of the same value.
#include "common.h"
#include "mesh_shared.h"
#include "../../include/adgs_simplify.h"
#include <cmath>

namespace adgs {
namespace {

constexpr int SIMP_THREADS = MESH_THREADS;                     // blocks_of (mesh_shared.h) counts workgroups of this size
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr double AXIS_LIMIT = 1048576.0;                       // 2^20: |c| below it is keyed in 21 bits per axis
constexpr int KEY_BITS = 63;
// the counters read back beside the three scan totals
enum { CNT_NONFINITE = 0, CNT_UNKEYED, CNT_BAD, CNT_DROPPED, CNT_DEGENERATE, CNT_DUPLICATE, CNT_COUNT };
constexpr int TOTALS = 3 * SCAN_AUX_SLOTS + CNT_COUNT;

struct CellLattice { double origin[3]; double cell; };

// adds the number of lanes of the wave with `p` to *counter: one atomic per wave that has any
__device__ __forceinline__ void count_lanes(bool p, unsigned long long* __restrict__ counter) {
	const unsigned long long m = __ballot(p);
	if (m && (int)(threadIdx.x & (WAVE - 1)) == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// ---- clusters ----

__global__ void __launch_bounds__(SIMP_THREADS) simplify_keys_kernel(const float* __restrict__ vertices, uint32_t V, CellLattice g, uint64_t* __restrict__ keys,
	uint32_t* __restrict__ vals, unsigned long long* __restrict__ counters) {
	const uint32_t v = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	bool nonfinite = false, unkeyed = false;
	if (v < V) {
		uint64_t key = 0;
		double c[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const float x = vertices[3 * (size_t)v + k];
			nonfinite = nonfinite || !isfinite(x);
			c[k] = floor(((double)x - g.origin[k]) / g.cell);
		}
		if (!nonfinite) {
			unkeyed = !(fabs(c[0]) < AXIS_LIMIT) || !(fabs(c[1]) < AXIS_LIMIT) || !(fabs(c[2]) < AXIS_LIMIT);
			if (!unkeyed) key = ((uint64_t)(long long)(c[0] + AXIS_LIMIT) << 42) | ((uint64_t)(long long)(c[1] + AXIS_LIMIT) << 21) | (uint64_t)(long long)(c[2] + AXIS_LIMIT);
		}
		keys[v] = key; vals[v] = v;
	}
	count_lanes(nonfinite, counters + CNT_NONFINITE);
	count_lanes(unkeyed, counters + CNT_UNKEYED);
}

// position i of the sorted keys starts a cluster
__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ sk, uint32_t i) { return sk[i] != 0 && (i == 0 || sk[i - 1] != sk[i]); }

__global__ void __launch_bounds__(SIMP_THREADS) simplify_heads_kernel(const uint64_t* __restrict__ sk, uint32_t V, uint32_t* __restrict__ head) {
	const uint32_t i = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (i < V) head[i] = is_head(sk, i) ? 1u : 0u;
}

// scan[]: the exclusive scan of the head flags.  kc[v]: the cluster (in key order) of vertex v, NONE when it is not kept; cstart[c]: the
// first sorted position of cluster c, cstart[number of clusters] = V.  The keys 0 sort first, so the kept vertices are a suffix.
__global__ void __launch_bounds__(SIMP_THREADS) simplify_assign_kernel(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ sv,
	const uint32_t* __restrict__ scan, uint32_t V, uint32_t* __restrict__ kc, uint32_t* __restrict__ cstart) {
	const uint32_t i = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (i >= V) return;
	const uint32_t v = sv[i];
	uint32_t c = NONE;
	if (sk[i] != 0) {
		const bool head = is_head(sk, i);
		c = scan[i] - (head ? 0u : 1u);                             // a member behind its head: the scan already counted the head
		if (c >= V) c = NONE;                                       // cannot happen: there are at most V heads
		else if (head) cstart[c] = i;
	}
	if (v < V) kc[v] = c;
	if (i == V - 1) cstart[c == NONE ? 0u : c + 1u] = V;            // c + 1 <= V: cstart holds V + 1 entries
}

// ---- faces ----

enum { FACE_OK = 0, FACE_BAD, FACE_DROPPED, FACE_DEGENERATE };

// the cluster triple of face f with the smallest index rotated to the front
__device__ __forceinline__ int face_triple(const int* __restrict__ faces, const uint32_t* __restrict__ kc, uint32_t f, uint32_t V, uint32_t t[3]) {
	uint32_t i[3];
	if (!load_face(faces, f, V, i)) return FACE_BAD;
	const uint32_t a = kc[i[0]], b = kc[i[1]], c = kc[i[2]];
	if (a == NONE || b == NONE || c == NONE) return FACE_DROPPED;
	if (a == b || b == c || a == c) return FACE_DEGENERATE;
	if (a < b && a < c) { t[0] = a; t[1] = b; t[2] = c; }
	else if (b < a && b < c) { t[0] = b; t[1] = c; t[2] = a; }
	else { t[0] = c; t[1] = a; t[2] = b; }
	return FACE_OK;
}

__global__ void __launch_bounds__(SIMP_THREADS) simplify_face_third_kernel(const int* __restrict__ faces, const uint32_t* __restrict__ kc, uint32_t F, uint32_t V,
	uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, unsigned long long* __restrict__ counters) {
	const uint32_t f = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	int why = -1;
	if (f < F) {
		uint32_t t[3];
		why = face_triple(faces, kc, f, V, t);
		keys[f] = why == FACE_OK ? t[2] : V; vals[f] = f;
	}
	count_lanes(why == FACE_BAD, counters + CNT_BAD);
	count_lanes(why == FACE_DROPPED, counters + CNT_DROPPED);
	count_lanes(why == FACE_DEGENERATE, counters + CNT_DEGENERATE);
}

// order[]: the faces sorted by their third index; a face that does not stay gets the key V << 32, above every (first, second)
__global__ void __launch_bounds__(SIMP_THREADS) simplify_face_pair_kernel(const int* __restrict__ faces, const uint32_t* __restrict__ kc,
	const uint32_t* __restrict__ order, uint32_t F, uint32_t V, uint64_t* __restrict__ keys) {
	const uint32_t j = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (j >= F) return;
	const uint32_t f = order[j];
	uint32_t t[3];
	const bool ok = f < F && face_triple(faces, kc, f, V, t) == FACE_OK;
	keys[j] = ok ? ((uint64_t)t[0] << 32) | (uint64_t)t[1] : (uint64_t)V << 32;
}

// keys / order: sorted by (first, second), then third, then face: a face is a duplicate when its predecessor has the same triple
__global__ void __launch_bounds__(SIMP_THREADS) simplify_face_keep_kernel(const int* __restrict__ faces, const uint32_t* __restrict__ kc,
	const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t F, uint32_t V, uint32_t* __restrict__ fkeep,
	unsigned long long* __restrict__ counters) {
	const uint32_t j = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	bool dup = false;
	if (j < F) {
		const uint32_t f = order[j];
		const uint64_t key = keys[j];
		uint32_t t[3], u[3];
		const bool ok = f < F && (key >> 32) < (uint64_t)V && face_triple(faces, kc, f, V, t) == FACE_OK;
		if (ok && j > 0 && keys[j - 1] == key) {
			const uint32_t fp = order[j - 1];
			dup = fp < F && face_triple(faces, kc, fp, V, u) == FACE_OK && u[2] == t[2];
		}
		if (f < F) fkeep[f] = ok && !dup ? 1u : 0u;
	}
	count_lanes(dup, counters + CNT_DUPLICATE);
}

// the root of cluster c: its first member
__device__ __forceinline__ uint32_t root_of(const uint32_t* __restrict__ sv, const uint32_t* __restrict__ cstart, uint32_t c, uint32_t V) {
	const uint32_t s = cstart[c];
	return s < V ? sv[s] : NONE;
}

__global__ void __launch_bounds__(SIMP_THREADS) simplify_used_kernel(const int* __restrict__ faces, const uint32_t* __restrict__ kc,
	const uint32_t* __restrict__ fkeep, const uint32_t* __restrict__ sv, const uint32_t* __restrict__ cstart, uint32_t F, uint32_t V,
	uint32_t* __restrict__ used) {
	const uint32_t f = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	uint32_t i[3];
	if (f >= F || !fkeep[f] || !load_face(faces, f, V, i)) return;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const uint32_t c = kc[i[k]];
		if (c >= V) continue;                                       // not for a kept face
		const uint32_t r = root_of(sv, cstart, c, V);
		if (r < V) used[r] = 1u;
	}
}

// msize[v]: the member count of the cluster whose used root v is, else 0
__global__ void __launch_bounds__(SIMP_THREADS) simplify_sizes_kernel(const uint32_t* __restrict__ kc, const uint32_t* __restrict__ used,
	const uint32_t* __restrict__ cstart, uint32_t V, uint32_t* __restrict__ msize) {
	const uint32_t v = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (v >= V) return;
	uint32_t n = 0;
	const uint32_t c = kc[v];
	if (used[v] && c < V) {
		const uint32_t s = cstart[c], e = cstart[c + 1];
		if (s < e && e <= V) n = e - s;
	}
	msize[v] = n;
}

__global__ void __launch_bounds__(SIMP_THREADS) simplify_vertex_cluster_kernel(const uint32_t* __restrict__ kc, const uint32_t* __restrict__ used,
	const uint32_t* __restrict__ vmap, const uint32_t* __restrict__ sv, const uint32_t* __restrict__ cstart, uint32_t V, int* __restrict__ vertex_cluster) {
	const uint32_t v = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (v >= V) return;
	int out = -1;
	const uint32_t c = kc[v];
	if (c < V) {
		const uint32_t r = root_of(sv, cstart, c, V);
		if (r < V && used[r]) out = (int)vmap[r];
	}
	vertex_cluster[v] = out;
}

// ---- emit ----

// one thread per sorted position: the root writes its cluster's row of the tables, every member its slot of the CSR
__global__ void __launch_bounds__(SIMP_THREADS) simplify_emit_vertices_kernel(const uint32_t* __restrict__ sv, const uint32_t* __restrict__ kc,
	const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ used, const uint32_t* __restrict__ vmap, const uint32_t* __restrict__ mscan,
	uint32_t V, uint32_t V2, uint32_t M, int* __restrict__ root, int* __restrict__ num_vertices, int* __restrict__ member_starts, int* __restrict__ members) {
	const uint32_t i = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (i == 0) member_starts[V2] = (int)M;
	if (i >= V) return;
	const uint32_t v = sv[i];
	if (v >= V) return;
	const uint32_t c = kc[v];
	if (c >= V) return;
	const uint32_t s = cstart[c], e = cstart[c + 1];
	if (!(s <= i && i < e && e <= V)) return;                       // cannot happen: i lies in its own cluster's run
	const uint32_t r = sv[s];
	if (r >= V || !used[r]) return;
	const uint32_t d = vmap[r], m0 = mscan[r];
	if (d >= V2 || (size_t)m0 + (e - s) > (size_t)M) return;        // neither happens for the flags that were counted
	members[m0 + (i - s)] = (int)v;
	if (i == s) { root[d] = (int)r; num_vertices[d] = (int)(e - s); member_starts[d] = (int)m0; }
}

__global__ void __launch_bounds__(SIMP_THREADS) simplify_emit_faces_kernel(const int* __restrict__ faces, const int* __restrict__ vertex_cluster,
	const uint32_t* __restrict__ fkeep, const uint32_t* __restrict__ fmap, uint32_t F, uint32_t V, uint32_t F2, int* __restrict__ faces_out,
	int* __restrict__ face_source) {
	const uint32_t f = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	uint32_t i[3];
	if (f >= F || !fkeep[f] || !load_face(faces, f, V, i)) return;
	const uint32_t d = fmap[f];
	if (d >= F2) return;                                            // does not happen for the flags that were counted
#pragma unroll
	for (int k = 0; k < 3; k++) faces_out[3 * (size_t)d + k] = vertex_cluster[i[k]];
	face_source[d] = (int)f;
}

// ---- placement ----

__device__ __forceinline__ bool finite3(const double p[3]) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the (cluster, corner id) pairs; the key V2 is for a corner that no cluster sums
__global__ void __launch_bounds__(SIMP_THREADS) simplify_corner_pairs_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
	const int* __restrict__ vertex_cluster, uint32_t F, uint32_t V, uint32_t V2, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
	const uint32_t f = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (f >= F) return;
	uint32_t i[3];
	bool ok = load_face(faces, f, V, i);
	if (ok) {
		double p[3];
#pragma unroll
		for (int k = 0; k < 3; k++) { load_point(vertices, i[k], p); ok = ok && finite3(p); }
	}
#pragma unroll
	for (int k = 0; k < 3; k++) {
		uint32_t key = V2;
		if (ok) {
			const uint32_t c = (uint32_t)vertex_cluster[i[k]];
			if (c < V2) key = c;
		}
		keys[3 * (size_t)f + k] = key; vals[3 * (size_t)f + k] = 3u * f + (uint32_t)k;
	}
}

// keys [n]: ascending, the corners of cluster d are the run of keys equal to d; vals: their corner ids 3 f + k, ascending within the run
template <bool QUADRIC>
__global__ void __launch_bounds__(SIMP_THREADS) simplify_place_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
	const float* __restrict__ colors, const int* __restrict__ member_starts, const int* __restrict__ members, const uint32_t* __restrict__ keys,
	const uint32_t* __restrict__ vals, uint32_t V, uint32_t F, uint32_t V2, uint32_t M, CellLattice g, double lambda, float* __restrict__ vertices_out,
	float* __restrict__ colors_out) {
	const uint32_t d = blockIdx.x * (uint32_t)SIMP_THREADS + threadIdx.x;
	if (d >= V2) return;
	uint32_t s = (uint32_t)member_starts[d], e = (uint32_t)member_starts[d + 1];
	if (e > M) e = M;
	if (s > e) s = e;
	double sum[3] = { 0.0, 0.0, 0.0 }, col[3] = { 0.0, 0.0, 0.0 }, first[3] = { 0.0, 0.0, 0.0 };
	uint32_t count = 0;
	for (uint32_t j = s; j < e; j++) {                              // ascending vertex id
		const uint32_t v = (uint32_t)members[j];
		if (v >= V) continue;
		double p[3];
		load_point(vertices, v, p);
		if (count == 0) { first[0] = p[0]; first[1] = p[1]; first[2] = p[2]; }
		sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2];
		if (colors) { load_point(colors, v, p); col[0] += p[0]; col[1] += p[1]; col[2] += p[2]; }
		count++;
	}
	const double n = count ? (double)count : 1.0;
	const double cbar[3] = { sum[0] / n, sum[1] / n, sum[2] / n };
	double delta[3] = { 0.0, 0.0, 0.0 };
	if (QUADRIC && count) {
		const size_t len = 3 * (size_t)F;
		double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, t = 0.0;
		for (size_t j = first_at_least(keys, len, d); j < len && keys[j] == d; j++) {
			const uint32_t f = vals[j] / 3u, k = vals[j] % 3u;
			uint32_t i[3];
			if (f >= F || !load_face(faces, f, V, i)) continue;
			double p[3][3];
#pragma unroll
			for (int c = 0; c < 3; c++) load_point(vertices, i[c], p[c]);      // as load_corners does; through it the compiler emits other (equal-valued) code here
			const FaceEdges e = face_edges(p[0], p[1], p[2]);
			const double kx = e.cross_x(), ky = e.cross_y(), kz = e.cross_z();
			const double L = sqrt(kx * kx + ky * ky + kz * kz);
			if (!(L > 0.0)) continue;
			const double nx = kx / L, ny = ky / L, nz = kz / L, w = L / 2.0;
			const double* pc = k == 0 ? p[0] : (k == 1 ? p[1] : p[2]);
			const double err = nx * (pc[0] - cbar[0]) + ny * (pc[1] - cbar[1]) + nz * (pc[2] - cbar[2]);
			a00 += w * nx * nx; a01 += w * nx * ny; a02 += w * nx * nz; a11 += w * ny * ny; a12 += w * ny * nz; a22 += w * nz * nz;
			g0 += w * err * nx; g1 += w * err * ny; g2 += w * err * nz;
			t += w;
		}
		if (t > 0.0) {
			const double r = lambda * t;
			const double m00 = a00 + r, m11 = a11 + r, m22 = a22 + r;
			// Cholesky M = L L^T, then L y = g, L^T delta = y
			const double l00 = sqrt(m00), l10 = a01 / l00, l20 = a02 / l00;
			const double l11 = sqrt(m11 - l10 * l10), l21 = (a12 - l20 * l10) / l11;
			const double l22 = sqrt(m22 - l20 * l20 - l21 * l21);
			const double y0 = g0 / l00, y1 = (g1 - l10 * y0) / l11, y2 = (g2 - l20 * y0 - l21 * y1) / l22;
			delta[2] = y2 / l22;
			delta[1] = (y1 - l21 * delta[2]) / l11;
			delta[0] = (y0 - l10 * delta[1] - l20 * delta[2]) / l00;
#pragma unroll
			for (int c = 0; c < 3; c++) {
				if (!isfinite(delta[c])) delta[c] = 0.0;            // not for an SPD matrix
				const double cell = floor((first[c] - g.origin[c]) / g.cell);
				const double lo_c = g.origin[c] + cell * g.cell, hi_c = g.origin[c] + (cell + 1.0) * g.cell;
				delta[c] = fmin(fmax(delta[c], fmin(lo_c - cbar[c], 0.0)), fmax(hi_c - cbar[c], 0.0));
			}
		}
	}
#pragma unroll
	for (int c = 0; c < 3; c++) {
		vertices_out[3 * (size_t)d + c] = (float)(cbar[c] + delta[c]);
		if (colors) colors_out[3 * (size_t)d + c] = (float)(col[c] / n);
	}
}

// ---- host ----

// cluster: the sort's ping-pong buffers (the 64-bit keys serve the vertices, then the faces), the maps that emit reads, the totals (three
// rows of SCAN_AUX_SLOTS partial totals: V2, M, F2; then the counters), the sort's and the scan's scratch (one user at a time)
struct ClusterTemp {
	uint64_t *k0, *k1; uint32_t *sv0, *sv; uint32_t *kc, *head, *cstart, *used, *vmap, *mscan;
	uint32_t *fa0, *fa1, *fb0, *fb1, *fkeep, *fmap; unsigned long long* totals; char *sort, *scan; size_t bytes;
};
ClusterTemp carve_cluster(char* base, size_t V, size_t F) {
	Carver c(base);
	ClusterTemp t;
	const size_t n = V > F ? V : F;
	t.k0 = c.take<uint64_t>(n); t.k1 = c.take<uint64_t>(n);
	t.sv0 = c.take<uint32_t>(V); t.sv = c.take<uint32_t>(V);
	t.kc = c.take<uint32_t>(V); t.head = c.take<uint32_t>(V); t.cstart = c.take<uint32_t>(V + 1);
	t.used = c.take<uint32_t>(V); t.vmap = c.take<uint32_t>(V); t.mscan = t.head;      // the head flags are done with when the sizes are written
	t.fa0 = c.take<uint32_t>(F); t.fa1 = c.take<uint32_t>(F); t.fb0 = c.take<uint32_t>(F); t.fb1 = c.take<uint32_t>(F);
	t.fkeep = c.take<uint32_t>(F); t.fmap = c.take<uint32_t>(F);
	t.totals = c.take<unsigned long long>(TOTALS);
	t.sort = c.take<char>(sort_temp_bytes(n));
	t.scan = c.take<char>(scan_temp_bytes(n));
	t.bytes = c.size();
	return t;
}

// place: the (cluster, corner) pairs and their sort, CornerPairTemp of mesh_shared.h

bool lattice_of(float cell_size, const float* origin, CellLattice& g) {
	if (!origin || !(cell_size > 0.f) || !std::isfinite(cell_size)) return false;
	for (int k = 0; k < 3; k++) {
		if (!std::isfinite(origin[k])) return false;
		g.origin[k] = (double)origin[k];
	}
	g.cell = (double)cell_size;
	return true;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_simplify_cluster_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) ? carve_cluster(nullptr, (size_t)V, (size_t)F).bytes : 0;
}

extern "C" int adgs_simplify_cluster(int V, int F, const float* vertices, const int* faces, float cell_size, const float* origin, void* temp,
	int* vertex_cluster, long long* counts, void* stream_) {
	const std::string name("adgs_simplify_cluster");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	CellLattice g;
	if (!lattice_of(cell_size, origin, g)) { set_error(name + ": cell_size must be a positive finite number and origin three finite floats"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!vertices || !temp || !vertex_cluster))) { set_error(name + ": NULL pointer"); return -1; }
	for (int k = 0; k < 9; k++) counts[k] = 0;
	if (V == 0 && F == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (V == 0) {                                               // every face is outside the (empty) vertex set: nothing to read
		counts[5] = F;
	} else {
		const ClusterTemp t = carve_cluster((char*)temp, (size_t)V, (size_t)F);
		unsigned long long* counters = t.totals + 3 * SCAN_AUX_SLOTS;
		const uint32_t uV = (uint32_t)V, uF = (uint32_t)F;
		ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, TOTALS * sizeof(unsigned long long), stream));
		ADGS_HIP_CHECK(hipMemsetAsync(t.used, 0, (size_t)V * sizeof(uint32_t), stream));
		ADGS_LAUNCH(simplify_keys_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, vertices, uV, g, t.k0, t.sv0, counters);
		if (radix_sort_pairs_u64(t.k0, t.k1, t.sv0, t.sv, (size_t)V, KEY_BITS, t.sort, stream) != 0) return -1;
		ADGS_LAUNCH(simplify_heads_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, (const uint64_t*)t.k1, uV, t.head);
		if (exclusive_scan_u32(t.head, t.head, (size_t)V, t.scan, stream) != 0) return -1;
		ADGS_LAUNCH(simplify_assign_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, (const uint64_t*)t.k1, (const uint32_t*)t.sv,
			(const uint32_t*)t.head, uV, t.kc, t.cstart);
		if (F > 0) {
			ADGS_LAUNCH(simplify_face_third_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, faces, (const uint32_t*)t.kc, uF, uV, t.fa0, t.fb0,
				counters);
			const int vbits = bits_of((unsigned long long)V);
			if (radix_sort_pairs_u32(t.fa0, t.fa1, t.fb0, t.fb1, (size_t)F, vbits, t.sort, stream) != 0) return -1;
			ADGS_LAUNCH(simplify_face_pair_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, faces, (const uint32_t*)t.kc, (const uint32_t*)t.fb1,
				uF, uV, t.k0);
			if (radix_sort_pairs_u64(t.k0, t.k1, t.fb1, t.fb0, (size_t)F, 32 + vbits, t.sort, stream) != 0) return -1;
			ADGS_LAUNCH(simplify_face_keep_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, faces, (const uint32_t*)t.kc, (const uint64_t*)t.k1,
				(const uint32_t*)t.fb0, uF, uV, t.fkeep, counters);
			ADGS_LAUNCH(simplify_used_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, faces, (const uint32_t*)t.kc, (const uint32_t*)t.fkeep,
				(const uint32_t*)t.sv, (const uint32_t*)t.cstart, uF, uV, t.used);
		}
		ADGS_LAUNCH(simplify_sizes_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, (const uint32_t*)t.kc, (const uint32_t*)t.used,
			(const uint32_t*)t.cstart, uV, t.mscan);
		if (exclusive_scan_u32_sum(t.used, t.vmap, (size_t)V, t.scan, t.used, t.totals, stream) != 0) return -1;
		if (exclusive_scan_u32_sum(t.mscan, t.mscan, (size_t)V, t.scan, t.mscan, t.totals + SCAN_AUX_SLOTS, stream) != 0) return -1;
		if (F > 0 && exclusive_scan_u32_sum(t.fkeep, t.fmap, (size_t)F, t.scan, t.fkeep, t.totals + 2 * SCAN_AUX_SLOTS, stream) != 0) return -1;
		ADGS_LAUNCH(simplify_vertex_cluster_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, (const uint32_t*)t.kc, (const uint32_t*)t.used,
			(const uint32_t*)t.vmap, (const uint32_t*)t.sv, (const uint32_t*)t.cstart, uV, vertex_cluster);
		unsigned long long sum[3], cnt[CNT_COUNT];
		if (read_scan_totals<3, CNT_COUNT>(t.totals, stream, sum, cnt) != 0) return -1;
		bool fits = sum[0] <= (unsigned long long)V && sum[1] <= (unsigned long long)V && sum[2] <= (unsigned long long)F && sum[0] <= sum[1];
		for (int k = 0; k < CNT_COUNT; k++) fits = fits && cnt[k] <= (unsigned long long)(k < CNT_BAD ? V : F);
		if (!fits) { set_error(name + ": a count exceeds its bound"); return -1; }     // cannot happen: bounded by V and F < 2^31
		counts[0] = (long long)sum[0]; counts[1] = (long long)sum[2]; counts[2] = (long long)sum[1];
		for (int k = 0; k < CNT_COUNT; k++) counts[3 + k] = (long long)cnt[k];
	}
	if (counts[5] > 0) {
		set_error(name + ": " + std::to_string(counts[5]) + " faces index outside the " + std::to_string(V) + " vertices");
		return -2;
	}
	if (counts[4] > 0) {
		set_error(name + ": " + std::to_string(counts[4]) + " vertices lie 2^20 cells or more from the origin: enlarge cell_size or move origin");
		return -3;
	}
	return 0;
}

extern "C" int adgs_simplify_cluster_emit(int V, int F, const int* faces, const int* vertex_cluster, const void* temp, const long long* counts, int* root,
	int* num_vertices, int* member_starts, int* members, int* faces_out, int* face_source, void* stream_) {
	const std::string name("adgs_simplify_cluster_emit");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	const long long V2 = counts[0], F2 = counts[1], M = counts[2];
	if (V2 < 0 || F2 < 0 || V2 > V || F2 > F || M < V2 || M > V) {
		set_error(name + ": counts are not what adgs_simplify_cluster returned for this mesh"); return -1;
	}
	if ((F > 0 && !faces) || (V > 0 && (!temp || !vertex_cluster || !member_starts))) { set_error(name + ": NULL pointer"); return -1; }
	if ((V2 > 0 && (!root || !num_vertices || !members)) || (F2 > 0 && (!faces_out || !face_source))) { set_error(name + ": NULL output"); return -1; }
	if (V == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const ClusterTemp t = carve_cluster((char*)temp, (size_t)V, (size_t)F);
	ADGS_LAUNCH(simplify_emit_vertices_kernel, dim3(blocks_of(V)), dim3(SIMP_THREADS), 0, stream, (const uint32_t*)t.sv, (const uint32_t*)t.kc,
		(const uint32_t*)t.cstart, (const uint32_t*)t.used, (const uint32_t*)t.vmap, (const uint32_t*)t.mscan, (uint32_t)V, (uint32_t)V2, (uint32_t)M, root,
		num_vertices, member_starts, members);
	if (F2 > 0) ADGS_LAUNCH(simplify_emit_faces_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, faces, vertex_cluster, (const uint32_t*)t.fkeep,
		(const uint32_t*)t.fmap, (uint32_t)F, (uint32_t)V, (uint32_t)F2, faces_out, face_source);
	return 0;
}

extern "C" size_t adgs_simplify_place_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) ? carve_corner_pairs(nullptr, (size_t)F).bytes : 0;
}

extern "C" int adgs_simplify_place(int V, int F, int V2, int M, const float* vertices, const int* faces, const float* colors, const int* vertex_cluster,
	const int* member_starts, const int* members, float cell_size, const float* origin, int placement, double regularization, void* temp,
	float* vertices_out, float* colors_out, void* stream_) {
	const std::string name("adgs_simplify_place");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (V2 < 0 || V2 > V || M < V2 || M > V) { set_error(name + ": V2 must lie in [0, V] and M in [V2, V]"); return -1; }
	if (3ull * (unsigned long long)F > 0xFFFFFFFFull) { set_error(name + ": 3 F must be below 2^32"); return -1; }
	if (placement != 0 && placement != 1) { set_error(name + ": placement must be 0 (average) or 1 (quadric)"); return -1; }
	if (!(regularization > 0.0) || !std::isfinite(regularization)) { set_error(name + ": regularization must be a positive finite number"); return -1; }
	CellLattice g;
	if (!lattice_of(cell_size, origin, g)) { set_error(name + ": cell_size must be a positive finite number and origin three finite floats"); return -1; }
	if ((colors != nullptr) != (colors_out != nullptr)) { set_error(name + ": colors and colors_out must be given together"); return -1; }
	if (V2 > 0 && (!vertices || !vertex_cluster || !member_starts || !members || !vertices_out || (F > 0 && (!faces || !temp)))) {
		set_error(name + ": NULL pointer"); return -1;
	}
	if (V2 == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const CornerPairTemp t = carve_corner_pairs((char*)temp, (size_t)F);
	const bool quadric = placement == 1 && F > 0;               // without a face there is no quadric: delta = 0
	if (quadric) {
		ADGS_LAUNCH(simplify_corner_pairs_kernel, dim3(blocks_of(F)), dim3(SIMP_THREADS), 0, stream, vertices, faces, vertex_cluster, (uint32_t)F,
			(uint32_t)V, (uint32_t)V2, t.k0, t.v0);
		if (radix_sort_pairs_u32(t.k0, t.k1, t.v0, t.v1, 3 * (size_t)F, bits_of((unsigned long long)V2), t.sort, stream) != 0) return -1;
		ADGS_LAUNCH(simplify_place_kernel<true>, dim3(blocks_of(V2)), dim3(SIMP_THREADS), 0, stream, vertices, faces, colors, member_starts, members,
			(const uint32_t*)t.k1, (const uint32_t*)t.v1, (uint32_t)V, (uint32_t)F, (uint32_t)V2, (uint32_t)M, g, regularization, vertices_out, colors_out);
	} else {
		ADGS_LAUNCH(simplify_place_kernel<false>, dim3(blocks_of(V2)), dim3(SIMP_THREADS), 0, stream, vertices, faces, colors, member_starts, members,
			(const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t)V, (uint32_t)F, (uint32_t)V2, (uint32_t)M, g, regularization, vertices_out,
			colors_out);
	}
	return 0;
}
