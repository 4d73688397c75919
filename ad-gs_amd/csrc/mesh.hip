// Mesh clean-up on the device for gfx950 (wave64): connected components (lock-free union-find), component table, keep / compaction and
// area-weighted vertex normals of an indexed triangle mesh.  The definition is in include/adgs_mesh.h.
//
//   label    init parent -> link (one launch over the faces) -> flatten (one launch over the vertices) -> root flags -> scan -> component ids
//   table    one launch over the vertices (root, vertex counts), one over the faces (face counts, areas): one atomic per run of a component
//   keep     flags from keep[vertex_component] (or, adgs_zbuffer_keep_faces_count, from a per-face mask) -> two scans -> one emit launch
//            for the vertex attributes, one for the faces
//   normals  3 F (vertex, corner) pairs -> stable radix sort by vertex -> one thread per vertex finds its row by bisection and sums it in order
// Every kernel that reads `faces` checks the three indices against V before it uses them (load_face, mesh_shared.h) and skips the face otherwise.
#include "common.h"
#include "mesh_shared.h"
#include "../../include/adgs_mesh.h"
#include "../../include/adgs_zbuffer.h"

namespace adgs {
namespace {

constexpr uint32_t NO_COMPONENT = 0xFFFFFFFFu;

// ---- union-find ----
//
// parent[] is a forest over the vertices; the rules that make the two launches terminate and give the right answer:
//   (1) parent[x] <= x always: a root is its own parent, every other node points to a smaller index.
//   (2) A link is made ONLY by atomicCAS(&parent[r], r, s) on a node r that is still its own parent, with s < r and s a root found for the
//       other vertex: always from the larger root to the smaller.  A node that stopped being a root never becomes one again.
//   (3) Path compression only replaces a NON-root's parent by a smaller node of the same tree that was its ancestor when it was read
//       (atomicMin in the link launch, a store of the root in the flatten launch).  A root is touched by the CAS of (2) and by nothing else.
//   (4) find() walks strictly decreasing indices (1), so it ends after at most x steps.
//   (5) A CAS fails only because another lane linked that root away in the meantime (2): over the whole launch there are fewer than V links,
//       so the retries are bounded by the number of links.  No other loop on the device is unbounded; nothing spins on a value another
//       workgroup must write.
// Trees only merge and (3) keeps a node in its tree, so when the link launch is over two vertices are in one tree exactly when a chain of
// faces connects them; by (2) the root of a tree is the smallest index in it, which is what makes the numbering a function of the mesh.
// The eight XCDs have private L2s: every access to parent[] is an agent-scope atomic (relaxed load, CAS, min, store), never a plain load or
// store.  A stale value would still be a node of the same tree with a smaller index, so it could cost retries but not the result; with
// atomic accesses the argument above needs no such case.
__device__ __forceinline__ uint32_t uf_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t uf_find(uint32_t* __restrict__ parent, uint32_t x) {
	uint32_t p = uf_load(parent + x);
	while (p != x) {                                            // p < x: x is not a root
		const uint32_t g = uf_load(parent + p);                 // g <= p
		if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (3): halve the path
		x = p; p = g;
	}
	return x;
}

__device__ __forceinline__ void uf_union(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
	for (;;) {
		a = uf_find(parent, a); b = uf_find(parent, b);
		if (a == b) return;
		const uint32_t r = max(a, b), s = min(a, b);
		uint32_t expected = r;
		if (__hip_atomic_compare_exchange_strong(parent + r, &expected, s, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
		a = r; b = s;                                           // r was linked away by another lane: find both roots again
	}
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_init_kernel(uint32_t* __restrict__ parent, uint32_t V) {
	const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (v < V) parent[v] = v;
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_link_kernel(const int* __restrict__ faces, uint32_t F, uint32_t V, uint32_t* __restrict__ parent,
	unsigned long long* __restrict__ bad) {
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (f >= F) return;
	uint32_t i[3];
	if (!load_face(faces, f, V, i)) { atomicAdd(bad, 1ull); return; }
	uf_union(parent, i[0], i[1]);
	uf_union(parent, i[1], i[2]);
}

// parent[v] <- the root of v: the smallest vertex of its component.  No link is made in this launch, so the root of every tree is fixed;
// a concurrent reader sees either the old parent or the root, both nodes of its tree with a smaller index.
__global__ void __launch_bounds__(MESH_THREADS) mesh_flatten_kernel(uint32_t* __restrict__ parent, uint32_t V, uint32_t* __restrict__ flag) {
	const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (v >= V) return;
	uint32_t x = v, p = uf_load(parent + x);
	while (p != x) { x = p; p = uf_load(parent + x); }
	if (x != v) __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	flag[v] = x == v ? 1u : 0u;
}

// comp[]: the exclusive scan of the root flags, so comp[r] is the number of a root r already; every other vertex takes its root's.  In place:
// a root's entry is read by others and rewritten by nobody.
__global__ void __launch_bounds__(MESH_THREADS) mesh_component_kernel(const uint32_t* __restrict__ parent, uint32_t V, uint32_t* comp) {
	const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (v >= V) return;
	const uint32_t r = parent[v];                               // <= v: flattened by the previous launch
	if (r != v) comp[v] = comp[r];
}

// ---- component table ----

// Same-address atomics serialise in the L2 (primitives.hip), and faces arrive ordered by cell, vertices by lattice point, so neighbours
// mostly share a component -- but on a noisy fused mesh a third of the vertices lie in floaters, and nearly every group of 64 neighbours holds
// a few components beside the large one (measured: per-lane atomics in such groups cost 1.4 ms for 565 k faces, all on one address).  So a
// wave walks TABLE_ITERS consecutive groups of 64 items and keeps a running (component, count, area).  Per group it takes the distinct
// components of its lanes one at a time (one ballot each, at most 64): the lanes that agree are reduced across the wave; the sum joins the run
// when it is the run's component, and is ONE atomic otherwise.  The run is flushed, one atomic, when a group no longer holds its component
// and at the end.  When the lanes of a group all agree this is one ballot and one reduction.  Everything branched on is wave-uniform.
constexpr int TABLE_ITERS = 32;
constexpr int TABLE_ITEMS = MESH_THREADS * TABLE_ITERS;        // per workgroup

template <bool AREA>
struct ComponentRun {
	uint32_t c = NO_COMPONENT; int n = 0; double a = 0.0;
	__device__ __forceinline__ void flush(int* __restrict__ count, double* __restrict__ area) {
		if (c != NO_COMPONENT && (threadIdx.x & (WAVE - 1)) == 0) {
			atomicAdd(count + c, n);
			if (AREA) atomicAdd(area + c, a);
		}
		c = NO_COMPONENT; n = 0; a = 0.0;
	}
	// every lane of the wave calls it; lane_c = NO_COMPONENT: the lane has nothing to add
	__device__ __forceinline__ void add(uint32_t lane_c, double lane_a, int* __restrict__ count, double* __restrict__ area) {
		const bool has = lane_c != NO_COMPONENT;
		unsigned long long rest = __ballot(has);
		if (rest == 0) return;
		if (__ballot(has && lane_c == c) == 0) {                // the run's component is not in this group: the first lane's becomes the run
			flush(count, area);
			c = (uint32_t)__shfl((int)lane_c, __ffsll((long long)rest) - 1, WAVE);
		}
		while (rest) {                                          // one round per distinct component of the group: at most 64
			const uint32_t pick = (uint32_t)__shfl((int)lane_c, __ffsll((long long)rest) - 1, WAVE);
			const bool mine = has && lane_c == pick;
			const unsigned long long sub = __ballot(mine);
			double sum = 0.0;
			if (AREA) {
				sum = mine ? lane_a : 0.0;
#pragma unroll
				for (int off = WAVE / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, WAVE);
			}
			if (pick == c) {
				n += (int)__popcll(sub);
				if (AREA) a += sum;
			} else if ((threadIdx.x & (WAVE - 1)) == 0) {
				atomicAdd(count + pick, (int)__popcll(sub));
				if (AREA) atomicAdd(area + pick, sum);
			}
			rest &= ~sub;
		}
	}
};

// the first item of this wave's TABLE_ITERS groups of 64
__device__ __forceinline__ size_t table_wave_base() {
	return (size_t)blockIdx.x * TABLE_ITEMS + (size_t)(threadIdx.x / WAVE) * (WAVE * TABLE_ITERS);
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_table_vertices_kernel(const uint32_t* __restrict__ parent, const int* __restrict__ comp, uint32_t V,
	uint32_t C, int* __restrict__ root, int* __restrict__ num_vertices) {
	ComponentRun<false> run;
	const size_t base = table_wave_base() + (threadIdx.x & (WAVE - 1));
	for (int it = 0; it < TABLE_ITERS; it++) {
		const size_t v = base + (size_t)it * WAVE;
		uint32_t c = NO_COMPONENT;
		if (v < V) {
			const uint32_t cv = (uint32_t)comp[v];
			if (cv < C) { c = cv; if (parent[v] == (uint32_t)v) root[c] = (int)v; }
		}
		run.add(c, 0.0, num_vertices, nullptr);
	}
	run.flush(num_vertices, nullptr);
}

template <bool AREA>
__global__ void __launch_bounds__(MESH_THREADS) mesh_table_faces_kernel(const int* __restrict__ faces, const float* __restrict__ vertices,
	const int* __restrict__ comp, uint32_t F, uint32_t V, uint32_t C, int* __restrict__ num_faces, double* __restrict__ area) {
	ComponentRun<AREA> run;
	const size_t base = table_wave_base() + (threadIdx.x & (WAVE - 1));
	for (int it = 0; it < TABLE_ITERS; it++) {
		const size_t f = base + (size_t)it * WAVE;
		uint32_t c = NO_COMPONENT;
		double a = 0.0;
		uint32_t i[3];
		if (f < F && load_face(faces, (uint32_t)f, V, i)) {
			const uint32_t cv = (uint32_t)comp[i[0]];
			if (cv < C) {
				c = cv;
				if (AREA) {
					double p[3][3];
					load_corners(vertices, i, p);
					const FaceEdges e = face_edges(p[0], p[1], p[2]);
					const double nx = e.cross_x(), ny = e.cross_y(), nz = e.cross_z();
					a = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
				}
			}
		}
		run.add(c, a, num_faces, area);
	}
	run.flush(num_faces, area);
}

// ---- keep ----

__global__ void __launch_bounds__(MESH_THREADS) mesh_keep_flags_kernel(const int* __restrict__ faces, const int* __restrict__ comp,
	const unsigned char* __restrict__ keep, uint32_t V, uint32_t F, uint32_t C, uint32_t* __restrict__ vflag, uint32_t* __restrict__ fflag) {
	const uint32_t t = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (t < V) {
		const uint32_t c = (uint32_t)comp[t];
		vflag[t] = c < C && keep[c] ? 1u : 0u;
	}
	if (t < F) {
		uint32_t i[3], k = 0;
		if (load_face(faces, t, V, i)) {
			const uint32_t c = (uint32_t)comp[i[0]];                // the three corners share it
			k = c < C && keep[c] ? 1u : 0u;
		}
		fflag[t] = k;
	}
}

// The flags of a per-face mask (adgs_zbuffer_keep_faces_count): a face stays when face_keep[f] != 0 and its indices are in range; a vertex
// when a face that stays uses it -- plain stores of 1 into vflag, which the host zeroed.  The faces that the mask kept and the index check
// dropped are counted in the UPPER 32 bits of the face row of the scan totals (F' < 2^31 stays below them), one atomic per wave that has any:
// the KeepTemp layout needs no counter of its own.
__global__ void __launch_bounds__(MESH_THREADS) mesh_keep_mask_flags_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ face_keep,
	uint32_t V, uint32_t F, uint32_t* __restrict__ vflag, uint32_t* __restrict__ fflag, unsigned long long* __restrict__ face_totals) {
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	uint32_t i[3], k = 0;
	bool dropped = false;
	if (f < F && face_keep[f]) {
		if (load_face(faces, f, V, i)) { k = 1u; vflag[i[0]] = 1u; vflag[i[1]] = 1u; vflag[i[2]] = 1u; }
		else dropped = true;
	}
	if (f < F) fflag[f] = k;
	const unsigned long long m = __ballot(dropped);
	if (m && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(face_totals + (blockIdx.x % SCAN_AUX_SLOTS), (unsigned long long)__popcll(m) << 32);
}

// map[]: the exclusive scan of the flags; element t was kept when the scan steps behind it
__device__ __forceinline__ bool kept(const uint32_t* __restrict__ map, uint32_t t, uint32_t n, uint32_t total) {
	return (t + 1 < n ? map[t + 1] : total) != map[t];
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_keep_vertices_kernel(const uint32_t* __restrict__ vmap, uint32_t V, uint32_t V2,
	const float* __restrict__ a0, const float* __restrict__ a1, const float* __restrict__ a2, float* __restrict__ o0, float* __restrict__ o1,
	float* __restrict__ o2) {
	const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (v >= V || !kept(vmap, v, V, V2)) return;
	const uint32_t d = vmap[v];
	if (d >= V2) return;                                        // d < V2 for the flags that were counted
#pragma unroll
	for (int k = 0; k < 3; k++) {
		o0[3 * (size_t)d + k] = a0[3 * (size_t)v + k];
		if (a1) o1[3 * (size_t)d + k] = a1[3 * (size_t)v + k];
		if (a2) o2[3 * (size_t)d + k] = a2[3 * (size_t)v + k];
	}
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_keep_faces_kernel(const int* __restrict__ faces, const uint32_t* __restrict__ vmap,
	const uint32_t* __restrict__ fmap, uint32_t V, uint32_t F, uint32_t V2, uint32_t F2, int* __restrict__ faces_out) {
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (f >= F || !kept(fmap, f, F, F2)) return;
	const uint32_t d = fmap[f];
	uint32_t i[3];
	if (d >= F2 || !load_face(faces, f, V, i)) return;          // neither happens for the flags that were counted
#pragma unroll
	for (int k = 0; k < 3; k++) faces_out[3 * (size_t)d + k] = (int)vmap[i[k]];
}

// ---- vertex normals ----

__global__ void __launch_bounds__(MESH_THREADS) mesh_corner_pairs_kernel(const int* __restrict__ faces, uint32_t F, uint32_t V, uint32_t* __restrict__ keys,
	uint32_t* __restrict__ vals) {
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (f >= F) return;
	uint32_t i[3];
	const bool ok = load_face(faces, f, V, i);
#pragma unroll
	for (int k = 0; k < 3; k++) { keys[3 * (size_t)f + k] = ok ? i[k] : V; vals[3 * (size_t)f + k] = 3u * f + (uint32_t)k; }
}

// keys [n]: ascending, the corners of vertex v are the run of keys equal to v; vals: their corner ids 3 f + c, ascending within the run (the
// sort is stable).  A corner id below 3 F whose key is below V belongs to a face whose three indices were checked when the pairs were made.
__global__ void __launch_bounds__(MESH_THREADS) mesh_normals_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
	const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t V, uint32_t F, float* __restrict__ normals) {
	const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (v >= V) return;
	const size_t n = 3 * (size_t)F;
	double sx = 0.0, sy = 0.0, sz = 0.0, S = 0.0;
	for (size_t j = first_at_least(keys, n, v); j < n && keys[j] == v; j++) {
		const uint32_t f = vals[j] / 3u;
		uint32_t i[3];
		if (f >= F || !load_face(faces, f, V, i)) continue;
		double p[3][3];
		load_corners(vertices, i, p);
		const FaceEdges e = face_edges(p[0], p[1], p[2]);
		sx += e.cross_x(); sy += e.cross_y(); sz += e.cross_z();
		S += sqrt(e.ax * e.ax + e.ay * e.ay + e.az * e.az) * sqrt(e.bx * e.bx + e.by * e.by + e.bz * e.bz);
	}
	const double len = sqrt(sx * sx + sy * sy + sz * sz);
	const bool zero = !(S > 0.0) || !(len > 0x1p-40 * S);
	normals[3 * (size_t)v + 0] = zero ? 0.f : (float)(sx / len);
	normals[3 * (size_t)v + 1] = zero ? 0.f : (float)(sy / len);
	normals[3 * (size_t)v + 2] = zero ? 0.f : (float)(sz / len);
}

// ---- host ----

unsigned table_blocks_of(size_t n) { return (unsigned)((n + TABLE_ITEMS - 1) / TABLE_ITEMS); }

// label: the parent array, the counters (the scan's SCAN_AUX_SLOTS partial totals of C, then the bad-face count), the scan's scratch
struct LabelTemp { uint32_t* parent; unsigned long long* totals; char* scan; size_t bytes; };
LabelTemp carve_label(char* base, size_t V) {
	Carver c(base);
	LabelTemp t;
	t.parent = c.take<uint32_t>(V);
	t.totals = c.take<unsigned long long>(2 * SCAN_AUX_SLOTS);
	t.scan = c.take<char>(scan_temp_bytes(V));
	t.bytes = c.size();
	return t;
}

// keep: the vertex and face flags (scanned in place), the 2 x SCAN_AUX_SLOTS partial totals, the scan's scratch (used by one scan at a time)
struct KeepTemp { uint32_t *vmap, *fmap; unsigned long long* totals; char* scan; size_t bytes; };
KeepTemp carve_keep(char* base, size_t V, size_t F) {
	Carver c(base);
	KeepTemp t;
	t.vmap = c.take<uint32_t>(V); t.fmap = c.take<uint32_t>(F);
	t.totals = c.take<unsigned long long>(2 * SCAN_AUX_SLOTS);
	t.scan = c.take<char>(scan_temp_bytes(V > F ? V : F));
	t.bytes = c.size();
	return t;
}

// normals: the (vertex, corner) pairs and their sort, CornerPairTemp of mesh_shared.h

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_mesh_label_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) ? carve_label(nullptr, (size_t)V).bytes : 0;
}

extern "C" int adgs_mesh_label(int V, int F, const int* faces, void* temp, int* vertex_component, long long* counts, void* stream_) {
	const std::string name("adgs_mesh_label");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!temp || !vertex_component))) { set_error(name + ": NULL pointer"); return -1; }
	counts[0] = counts[1] = 0;
	if (V == 0 && F == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (V == 0) {                                               // every face is outside the (empty) vertex set: nothing to read
		counts[1] = F;
	} else {
		const LabelTemp t = carve_label((char*)temp, (size_t)V);
		unsigned long long* bad = t.totals + SCAN_AUX_SLOTS;
		uint32_t* comp = reinterpret_cast<uint32_t*>(vertex_component);
		ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, 2 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
		ADGS_LAUNCH(mesh_init_kernel, dim3(blocks_of(V)), dim3(MESH_THREADS), 0, stream, t.parent, (uint32_t)V);
		if (F > 0) ADGS_LAUNCH(mesh_link_kernel, dim3(blocks_of(F)), dim3(MESH_THREADS), 0, stream, faces, (uint32_t)F, (uint32_t)V, t.parent, bad);
		ADGS_LAUNCH(mesh_flatten_kernel, dim3(blocks_of(V)), dim3(MESH_THREADS), 0, stream, t.parent, (uint32_t)V, comp);
		if (exclusive_scan_u32_sum(comp, comp, (size_t)V, t.scan, comp, t.totals, stream) != 0) return -1;
		ADGS_LAUNCH(mesh_component_kernel, dim3(blocks_of(V)), dim3(MESH_THREADS), 0, stream, (const uint32_t*)t.parent, (uint32_t)V, comp);
		unsigned long long C[1], nbad;
		if (read_scan_totals<1, 1>(t.totals, stream, C, &nbad) != 0) return -1;
		if (C[0] > (unsigned long long)V || nbad > (unsigned long long)F) {      // cannot happen: bounded by V and F < 2^31
			set_error(name + ": a count exceeds INT_MAX"); return -1;
		}
		counts[0] = (long long)C[0]; counts[1] = (long long)nbad;
	}
	if (counts[1] > 0) {
		set_error(name + ": " + std::to_string(counts[1]) + " faces index outside the " + std::to_string(V) + " vertices");
		return -2;
	}
	return 0;
}

extern "C" int adgs_mesh_table(int V, int F, int C, const int* faces, const float* vertices, const int* vertex_component, const void* temp, int* root,
	int* num_faces, int* num_vertices, double* area, void* stream_) {
	const std::string name("adgs_mesh_table");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (C < 0 || C > V) { set_error(name + ": C must lie in [0, V]"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!temp || !vertex_component)) || (C > 0 && (!root || !num_faces || !num_vertices))) {
		set_error(name + ": NULL pointer"); return -1;
	}
	if ((vertices != nullptr) != (area != nullptr)) { set_error(name + ": vertices and area must be given together"); return -1; }
	if (V == 0 || C == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const LabelTemp t = carve_label((char*)temp, (size_t)V);
	ADGS_HIP_CHECK(hipMemsetAsync(num_faces, 0, (size_t)C * sizeof(int), stream));
	ADGS_HIP_CHECK(hipMemsetAsync(num_vertices, 0, (size_t)C * sizeof(int), stream));
	if (area) ADGS_HIP_CHECK(hipMemsetAsync(area, 0, (size_t)C * sizeof(double), stream));
	ADGS_LAUNCH(mesh_table_vertices_kernel, dim3(table_blocks_of(V)), dim3(MESH_THREADS), 0, stream, (const uint32_t*)t.parent, vertex_component, (uint32_t)V,
		(uint32_t)C, root, num_vertices);
	if (F > 0) {
		if (area) ADGS_LAUNCH(mesh_table_faces_kernel<true>, dim3(table_blocks_of(F)), dim3(MESH_THREADS), 0, stream, faces, vertices, vertex_component,
			(uint32_t)F, (uint32_t)V, (uint32_t)C, num_faces, area);
		else ADGS_LAUNCH(mesh_table_faces_kernel<false>, dim3(table_blocks_of(F)), dim3(MESH_THREADS), 0, stream, faces, vertices, vertex_component,
			(uint32_t)F, (uint32_t)V, (uint32_t)C, num_faces, area);
	}
	return 0;
}

extern "C" size_t adgs_mesh_keep_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) ? carve_keep(nullptr, (size_t)V, (size_t)F).bytes : 0;
}

extern "C" int adgs_mesh_keep_count(int V, int F, int C, const int* faces, const int* vertex_component, const unsigned char* keep, void* temp,
	long long* counts, void* stream_) {
	const std::string name("adgs_mesh_keep_count");
	if (V < 0 || F < 0 || C < 0) { set_error(name + ": negative V, F or C"); return -1; }
	if (C > V) { set_error(name + ": C must lie in [0, V]"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!temp || !vertex_component)) || (C > 0 && !keep)) { set_error(name + ": NULL pointer"); return -1; }
	counts[0] = counts[1] = 0;
	if (V == 0) return 0;                                       // no vertex, hence no face that can stay
	hipStream_t stream = (hipStream_t)stream_;
	const KeepTemp t = carve_keep((char*)temp, (size_t)V, (size_t)F);
	ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, 2 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
	ADGS_LAUNCH(mesh_keep_flags_kernel, dim3(blocks_of((size_t)(V > F ? V : F))), dim3(MESH_THREADS), 0, stream, faces, vertex_component, keep,
		(uint32_t)V, (uint32_t)F, (uint32_t)C, t.vmap, t.fmap);
	if (exclusive_scan_u32_sum(t.vmap, t.vmap, (size_t)V, t.scan, t.vmap, t.totals, stream) != 0) return -1;
	if (F > 0 && exclusive_scan_u32_sum(t.fmap, t.fmap, (size_t)F, t.scan, t.fmap, t.totals + SCAN_AUX_SLOTS, stream) != 0) return -1;
	unsigned long long sum[2];
	if (read_scan_totals<2, 0>(t.totals, stream, sum, nullptr) != 0) return -1;
	if (sum[0] > (unsigned long long)V || sum[1] > (unsigned long long)F) { set_error(name + ": a count exceeds INT_MAX"); return -1; }     // cannot happen
	counts[0] = (long long)sum[0]; counts[1] = (long long)sum[1];
	return 0;
}

extern "C" int adgs_zbuffer_keep_faces_count(int V, int F, const int* faces, const unsigned char* face_keep, void* temp, long long* counts, void* stream_) {
	const std::string name("adgs_zbuffer_keep_faces_count");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	if ((F > 0 && (!faces || !face_keep)) || ((V > 0 || F > 0) && !temp)) { set_error(name + ": NULL pointer"); return -1; }
	counts[0] = counts[1] = counts[2] = 0;
	if (F == 0) return 0;                                       // no face stays, hence no vertex
	hipStream_t stream = (hipStream_t)stream_;
	const KeepTemp t = carve_keep((char*)temp, (size_t)V, (size_t)F);
	ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, 2 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
	if (V > 0) ADGS_HIP_CHECK(hipMemsetAsync(t.vmap, 0, (size_t)V * sizeof(uint32_t), stream));
	ADGS_LAUNCH(mesh_keep_mask_flags_kernel, dim3(blocks_of((size_t)F)), dim3(MESH_THREADS), 0, stream, faces, face_keep, (uint32_t)V, (uint32_t)F, t.vmap,
		t.fmap, t.totals + SCAN_AUX_SLOTS);
	if (V > 0 && exclusive_scan_u32_sum(t.vmap, t.vmap, (size_t)V, t.scan, t.vmap, t.totals, stream) != 0) return -1;
	if (exclusive_scan_u32_sum(t.fmap, t.fmap, (size_t)F, t.scan, t.fmap, t.totals + SCAN_AUX_SLOTS, stream) != 0) return -1;
	unsigned long long sum[2];
	if (read_scan_totals<2, 0>(t.totals, stream, sum, nullptr) != 0) return -1;
	const unsigned long long kept = sum[1] & 0xFFFFFFFFull, dropped = sum[1] >> 32;
	if (sum[0] > (unsigned long long)V || kept + dropped > (unsigned long long)F) { set_error(name + ": a count exceeds INT_MAX"); return -1; }      // cannot happen
	counts[0] = (long long)sum[0]; counts[1] = (long long)kept; counts[2] = (long long)dropped;
	return 0;
}

extern "C" int adgs_mesh_keep_emit(int V, int F, const int* faces, const float* vertices, const float* colors, const float* normals, const void* temp,
	const long long* counts, float* vertices_out, int* faces_out, float* colors_out, float* normals_out, void* stream_) {
	const std::string name("adgs_mesh_keep_emit");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	const long long V2 = counts[0], F2 = counts[1];
	if (V2 < 0 || F2 < 0 || V2 > V || F2 > F) { set_error(name + ": counts are not what adgs_mesh_keep_count returned for this mesh"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!temp || !vertices))) { set_error(name + ": NULL pointer"); return -1; }
	if ((colors != nullptr) != (colors_out != nullptr)) { set_error(name + ": colors and colors_out must be given together"); return -1; }
	if ((normals != nullptr) != (normals_out != nullptr)) { set_error(name + ": normals and normals_out must be given together"); return -1; }
	if ((V2 > 0 && !vertices_out) || (F2 > 0 && !faces_out)) { set_error(name + ": NULL vertices_out or faces_out"); return -1; }
	if (V2 == 0) return 0;                                      // no vertex stays, hence no face
	hipStream_t stream = (hipStream_t)stream_;
	const KeepTemp t = carve_keep((char*)temp, (size_t)V, (size_t)F);
	ADGS_LAUNCH(mesh_keep_vertices_kernel, dim3(blocks_of(V)), dim3(MESH_THREADS), 0, stream, (const uint32_t*)t.vmap, (uint32_t)V, (uint32_t)V2, vertices,
		colors, normals, vertices_out, colors_out, normals_out);
	if (F2 > 0) ADGS_LAUNCH(mesh_keep_faces_kernel, dim3(blocks_of(F)), dim3(MESH_THREADS), 0, stream, faces, (const uint32_t*)t.vmap, (const uint32_t*)t.fmap,
		(uint32_t)V, (uint32_t)F, (uint32_t)V2, (uint32_t)F2, faces_out);
	return 0;
}

extern "C" size_t adgs_mesh_normals_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) ? carve_corner_pairs(nullptr, (size_t)F).bytes : 0;
}

extern "C" int adgs_mesh_vertex_normals(int V, int F, const float* vertices, const int* faces, void* temp, float* normals, void* stream_) {
	const std::string name("adgs_mesh_vertex_normals");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if ((V > 0 && (!vertices || !normals)) || (F > 0 && (!faces || !temp))) { set_error(name + ": NULL pointer"); return -1; }
	if (V == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const CornerPairTemp t = carve_corner_pairs((char*)temp, (size_t)F);
	const uint32_t* keys = t.k1;
	const uint32_t* vals = t.v1;
	if (F > 0) {
		ADGS_LAUNCH(mesh_corner_pairs_kernel, dim3(blocks_of(F)), dim3(MESH_THREADS), 0, stream, faces, (uint32_t)F, (uint32_t)V, t.k0, t.v0);
		if (radix_sort_pairs_u32(t.k0, t.k1, t.v0, t.v1, 3 * (size_t)F, bits_of((unsigned long long)V), t.sort, stream) != 0) return -1;      // the keys are 0 .. V
	}
	ADGS_LAUNCH(mesh_normals_kernel, dim3(blocks_of(V)), dim3(MESH_THREADS), 0, stream, vertices, faces, keys, vals, (uint32_t)V, (uint32_t)F, normals);
	return 0;
}
