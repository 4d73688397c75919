// One-ring adjacency of a triangle mesh and Laplacian / Taubin smoothing over it on the device for gfx950 (wave64).  The definition is in
// include/adgs_smooth.h.
//
//   count   six directed pairs (a << bits(V) | b) per face -> radix sort on 2 bits(V) bits -> head flags of the runs of equal keys, the
//           run length is the edge's incidence (boundary bytes, counters) -> scan of the head flags -> ONE read-back
//   emit    neighbors and the first end of every entry from the numbered heads; starts by bisection over the first ends
//   steps   one lane per vertex sums its row in ascending neighbour order in double; two ping-pong buffers of 32-byte rows, one launch per
//           step, the float -> double widening in the first and the rounding in the last
// Every kernel that reads `faces` checks the three indices against V before it uses them (load_face, mesh_shared.h).  Counters are integer
// atomics (one per wave); there is no float atomic, and a boundary byte written by several lanes is a plain store of the same value.
#include "common.h"
#include "mesh_shared.h"
#include "../../include/adgs_smooth.h"
#include <cmath>

namespace adgs {
namespace {

constexpr int SMOOTH_THREADS = MESH_THREADS;                   // blocks_of (mesh_shared.h) counts workgroups of this size
constexpr long long MAX_STEPS = 20000;
// Every counter is COUNTER_SLOTS partial counts that the host adds up, as the scan's totals are: nearly every wave of the head pass counts
// an edge and a row, and with one address per counter those 10^5 atomics queue up behind each other (measured: the head pass took 1.67 ms
// on 4.4 M keys, and mesh_adjacency on 3.4 M keys 1.82 ms with one address per counter against 0.62 ms with the slots).
enum { CNT_BAD = 0, CNT_DEGENERATE, CNT_EDGES, CNT_BOUNDARY, CNT_NONMANIFOLD, CNT_ROWS, CNT_COUNT };
constexpr int COUNTER_SLOTS = 32;
constexpr int TOTALS = SCAN_AUX_SLOTS + CNT_COUNT * COUNTER_SLOTS;

// adds the number of lanes of the wave with `p` to the workgroup's slot of counter `which`: one atomic per wave that has any
__device__ __forceinline__ void add_lanes(bool p, unsigned long long* __restrict__ counters, int which) {
	const unsigned long long m = __ballot(p);
	if (m && (int)(threadIdx.x & (WAVE - 1)) == __ffsll((long long)m) - 1)
		atomicAdd(counters + which * COUNTER_SLOTS + (blockIdx.x & (COUNTER_SLOTS - 1)), (unsigned long long)__popcll(m));
}

// ---- adjacency ----

// A directed pair (a, b) as the key a << bits | b, bits = bits_of(V): every index and V itself fit a field, so the key of a dropped pair,
// V << bits, sorts behind every pair, and the sort runs over 2 bits(V) key bits instead of 64.
struct PairKeys {
	uint32_t V; int bits;
	__device__ __forceinline__ uint64_t pack(uint32_t a, uint32_t b) const { return ((uint64_t)a << bits) | (uint64_t)b; }
	__device__ __forceinline__ uint64_t dropped() const { return (uint64_t)V << bits; }
	__device__ __forceinline__ uint32_t first(uint64_t key) const { return (uint32_t)(key >> bits); }
	__device__ __forceinline__ uint32_t second(uint64_t key) const { return (uint32_t)(key & ((1ull << bits) - 1ull)); }
	__device__ __forceinline__ bool valid(uint64_t key) const { return first(key) < V && second(key) < V; }      // a pair that was not dropped
};

__global__ void __launch_bounds__(SMOOTH_THREADS) smooth_pairs_kernel(const int* __restrict__ faces, uint32_t F, PairKeys pk, uint64_t* __restrict__ keys,
	unsigned long long* __restrict__ counters) {
	const uint32_t f = blockIdx.x * (uint32_t)SMOOTH_THREADS + threadIdx.x;
	bool bad = false, degenerate = false;
	if (f < F) {
		uint32_t i[3];
		bad = !load_face(faces, f, pk.V, i);
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const uint32_t a = i[k], b = i[(k + 1) % 3];
			const bool drop = bad || a == b;
			degenerate = degenerate || (!bad && a == b);
			keys[6 * (size_t)f + 2 * k + 0] = drop ? pk.dropped() : pk.pack(a, b);
			keys[6 * (size_t)f + 2 * k + 1] = drop ? pk.dropped() : pk.pack(b, a);
		}
	}
	add_lanes(bad, counters, CNT_BAD);
	add_lanes(degenerate, counters, CNT_DEGENERATE);
}

// position i of the sorted keys is the first of a run of equal pairs: an entry of `neighbors`
__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ sk, uint32_t i, const PairKeys& pk) {
	return pk.valid(sk[i]) && (i == 0 || sk[i - 1] != sk[i]);
}

// head[i]; the run behind a head is as long as the edge's incidence.  Every edge has two runs, (a, b) and (b, a): the one with a < b counts
// it, and each stores its own first end's boundary byte.
__global__ void __launch_bounds__(SMOOTH_THREADS) smooth_heads_kernel(const uint64_t* __restrict__ sk, uint32_t n, PairKeys pk, uint32_t* __restrict__ head,
	unsigned char* __restrict__ boundary, unsigned long long* __restrict__ counters) {
	const uint32_t i = blockIdx.x * (uint32_t)SMOOTH_THREADS + threadIdx.x;
	bool edge = false, single = false, many = false, row = false;
	if (i < n) {
		const uint64_t key = sk[i];
		const uint32_t a = pk.first(key), b = pk.second(key);
		const bool h = is_head(sk, i, pk);
		head[i] = h ? 1u : 0u;
		if (h) {
			const bool two = i + 1 < n && sk[i + 1] == key, three = two && i + 2 < n && sk[i + 2] == key;
			if (!two) boundary[a] = 1;
			edge = a < b; single = edge && !two; many = edge && three;
			row = i == 0 || pk.first(sk[i - 1]) != a;
		}
	}
	add_lanes(edge, counters, CNT_EDGES);
	add_lanes(single, counters, CNT_BOUNDARY);
	add_lanes(many, counters, CNT_NONMANIFOLD);
	add_lanes(row, counters, CNT_ROWS);
}

// scan[]: the exclusive scan of the head flags.  Entry scan[i] of a head: its second end into neighbors, its first end into first_end.
__global__ void __launch_bounds__(SMOOTH_THREADS) smooth_emit_kernel(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ scan, uint32_t n, PairKeys pk,
	uint32_t N, int* __restrict__ neighbors, uint32_t* __restrict__ first_end) {
	const uint32_t i = blockIdx.x * (uint32_t)SMOOTH_THREADS + threadIdx.x;
	if (i >= n || !is_head(sk, i, pk)) return;
	const uint64_t key = sk[i];
	const uint32_t a = pk.first(key), b = pk.second(key), d = scan[i];
	if (d >= N) return;                                             // does not happen for the heads that were counted
	neighbors[d] = (int)b; first_end[d] = a;
}

// first_end [N]: ascending.  The row of v starts at the first entry whose first end is >= v, so an isolated vertex has an empty row.
__global__ void __launch_bounds__(SMOOTH_THREADS) smooth_starts_kernel(const uint32_t* __restrict__ first_end, uint32_t V, uint32_t N, int* __restrict__ starts) {
	const uint32_t v = blockIdx.x * (uint32_t)SMOOTH_THREADS + threadIdx.x;
	if (v > V) return;
	starts[v] = v == V ? (int)N : (int)first_at_least(first_end, (size_t)N, v);
}

// ---- smoothing ----

// the state of one vertex: a 32-byte row, so that a neighbour is one aligned fetch
struct alignas(32) Row { double x, y, z, w; };

template <bool FIRST>
__device__ __forceinline__ Row load_state(const float* __restrict__ vin, const Row* __restrict__ cur, uint32_t v) {
	if constexpr (FIRST) {
		double p[3];
		load_point(vin, v, p);
		return Row{ p[0], p[1], p[2], 0.0 };
	}
	return cur[v];
}

// One step: x' = x + s * (S / d - x), S the sum of the row of v in ascending neighbour order from 0.0.  Four neighbours are fetched
// together and added one after the other; a neighbour outside [0, V) (not in a row of adgs_smooth_adjacency_emit) adds +0.0, which
// changes no sum that started from +0.0.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(SMOOTH_THREADS) smooth_step_kernel(const float* __restrict__ vin, const Row* __restrict__ cur, const int* __restrict__ starts,
	const int* __restrict__ neighbors, const unsigned char* __restrict__ fixed, uint32_t V, uint32_t N, double s, Row* __restrict__ next, float* __restrict__ out) {
	const uint32_t v = blockIdx.x * (uint32_t)SMOOTH_THREADS + threadIdx.x;
	if (v >= V) return;
	Row x = load_state<FIRST>(vin, cur, v);
	uint32_t lo = (uint32_t)starts[v], hi = (uint32_t)starts[v + 1];
	if (hi > N) hi = N;
	if (lo > hi) lo = hi;
	const uint32_t d = hi - lo;
	if (d != 0 && !(fixed && fixed[v])) {
		const Row zero{ 0.0, 0.0, 0.0, 0.0 };
		double S0 = 0.0, S1 = 0.0, S2 = 0.0;
		uint32_t j = lo;
		for (; j + 4 <= hi; j += 4) {
			uint32_t u[4];
			Row r[4];
#pragma unroll
			for (int k = 0; k < 4; k++) u[k] = (uint32_t)neighbors[j + k];
#pragma unroll
			for (int k = 0; k < 4; k++) r[k] = u[k] < V ? load_state<FIRST>(vin, cur, u[k]) : zero;
#pragma unroll
			for (int k = 0; k < 4; k++) { S0 += r[k].x; S1 += r[k].y; S2 += r[k].z; }
		}
		for (; j < hi; j++) {
			const uint32_t u = (uint32_t)neighbors[j];
			const Row r = u < V ? load_state<FIRST>(vin, cur, u) : zero;
			S0 += r.x; S1 += r.y; S2 += r.z;
		}
		const double n = (double)d;
		x.x = x.x + s * (S0 / n - x.x);
		x.y = x.y + s * (S1 / n - x.y);
		x.z = x.z + s * (S2 / n - x.z);
	}
	if (LAST) {
		out[3 * (size_t)v + 0] = (float)x.x; out[3 * (size_t)v + 1] = (float)x.y; out[3 * (size_t)v + 2] = (float)x.z;
	} else {
		next[v] = x;
	}
}

// ---- host ----

PairKeys pair_keys(int V) { return PairKeys{ (uint32_t)V, bits_of((unsigned long long)V) }; }
// 6 F < 2^31: the pairs, the entries of neighbors and the rows of starts are indexed with 32 bits (starts is int32)
bool faces_ok(long long F) { return F >= 0 && 6 * F <= (long long)INT_MAX; }

// the sort's ping-pong buffers and its own scratch, the totals (one row of partial scan totals, then the counters), the scan's scratch.
// The sort carries values nobody needs: after it v0 holds the head flags, then their scan, and v1 the first end of every entry.
struct AdjacencyTemp { uint64_t *k0, *k1; uint32_t *v0, *v1; unsigned long long* totals; char *sort, *scan; size_t bytes; };
AdjacencyTemp carve_adjacency(char* base, size_t F) {
	Carver c(base);
	AdjacencyTemp t;
	const size_t n = 6 * F;
	t.k0 = c.take<uint64_t>(n); t.k1 = c.take<uint64_t>(n);
	t.v0 = c.take<uint32_t>(n); t.v1 = c.take<uint32_t>(n);
	t.totals = c.take<unsigned long long>(TOTALS);
	t.sort = c.take<char>(sort_temp_bytes(n));
	t.scan = c.take<char>(scan_temp_bytes(n));
	t.bytes = c.size();
	return t;
}

struct StepsTemp { Row *a, *b; size_t bytes; };
StepsTemp carve_steps(char* base, size_t V) {
	Carver c(base);
	StepsTemp t;
	t.a = c.take<Row>(V); t.b = c.take<Row>(V);
	t.bytes = c.size();
	return t;
}

template <bool FIRST, bool LAST>
int launch_step(const float* vin, const Row* cur, const int* starts, const int* neighbors, const unsigned char* fixed, int V, int N, double s, Row* next,
	float* out, hipStream_t stream) {
	ADGS_LAUNCH((smooth_step_kernel<FIRST, LAST>), dim3(blocks_of(V)), dim3(SMOOTH_THREADS), 0, stream, vin, cur, starts, neighbors, fixed, (uint32_t)V,
		(uint32_t)N, s, next, out);
	return 0;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_smooth_adjacency_temp_bytes(long long V, long long F) {
	return sizes_ok(V, F) && faces_ok(F) ? carve_adjacency(nullptr, (size_t)F).bytes : 0;
}

extern "C" int adgs_smooth_adjacency_count(int V, int F, const int* faces, void* temp, unsigned char* boundary, long long* counts, void* stream_) {
	const std::string name("adgs_smooth_adjacency_count");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!faces_ok(F)) { set_error(name + ": 6 F must be below 2^31"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	if ((F > 0 && !faces) || (V > 0 && (!boundary || (F > 0 && !temp)))) { set_error(name + ": NULL pointer"); return -1; }
	for (int k = 0; k < 7; k++) counts[k] = 0;
	if (V == 0 && F == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (V == 0) {                                               // every face is outside the (empty) vertex set: nothing to read
		counts[1] = F;
	} else {
		ADGS_HIP_CHECK(hipMemsetAsync(boundary, 0, (size_t)V, stream));
		counts[6] = V;
		if (F > 0) {
			const AdjacencyTemp t = carve_adjacency((char*)temp, (size_t)F);
			unsigned long long* counters = t.totals + SCAN_AUX_SLOTS;
			const size_t n = 6 * (size_t)F;
			const PairKeys pk = pair_keys(V);
			ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, TOTALS * sizeof(unsigned long long), stream));
			ADGS_LAUNCH(smooth_pairs_kernel, dim3(blocks_of(F)), dim3(SMOOTH_THREADS), 0, stream, faces, (uint32_t)F, pk, t.k0, counters);
			if (radix_sort_pairs_u64(t.k0, t.k1, t.v0, t.v1, n, 2 * pk.bits, t.sort, stream) != 0) return -1;
			ADGS_LAUNCH(smooth_heads_kernel, dim3(blocks_of(n)), dim3(SMOOTH_THREADS), 0, stream, (const uint64_t*)t.k1, (uint32_t)n, pk, t.v0, boundary,
				counters);
			if (exclusive_scan_u32_sum(t.v0, t.v0, n, t.scan, t.v0, t.totals, stream) != 0) return -1;
			unsigned long long sum[1], slots[CNT_COUNT * COUNTER_SLOTS], cnt[CNT_COUNT] = {};
			if (read_scan_totals<1, CNT_COUNT * COUNTER_SLOTS>(t.totals, stream, sum, slots) != 0) return -1;
			for (int k = 0; k < CNT_COUNT * COUNTER_SLOTS; k++) cnt[k / COUNTER_SLOTS] += slots[k];
			bool fits = sum[0] <= n && sum[0] == 2 * cnt[CNT_EDGES] && cnt[CNT_BAD] <= (unsigned long long)F && cnt[CNT_DEGENERATE] <= (unsigned long long)F &&
				cnt[CNT_BOUNDARY] + cnt[CNT_NONMANIFOLD] <= cnt[CNT_EDGES] && cnt[CNT_ROWS] <= (unsigned long long)V;
			if (!fits) { set_error(name + ": a count exceeds its bound"); return -1; }     // cannot happen: every edge has its two runs
			counts[0] = (long long)sum[0]; counts[1] = (long long)cnt[CNT_BAD]; counts[2] = (long long)cnt[CNT_EDGES];
			counts[3] = (long long)cnt[CNT_BOUNDARY]; counts[4] = (long long)cnt[CNT_NONMANIFOLD]; counts[5] = (long long)cnt[CNT_DEGENERATE];
			counts[6] = (long long)V - (long long)cnt[CNT_ROWS];
		}
	}
	if (counts[1] > 0) {
		set_error(name + ": " + std::to_string(counts[1]) + " faces index outside the " + std::to_string(V) + " vertices");
		return -2;
	}
	return 0;
}

extern "C" int adgs_smooth_adjacency_emit(int V, int F, const void* temp, const long long* counts, int* starts, int* neighbors, void* stream_) {
	const std::string name("adgs_smooth_adjacency_emit");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (!faces_ok(F)) { set_error(name + ": 6 F must be below 2^31"); return -1; }
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	const long long N = counts[0];
	if (N < 0 || N % 2 != 0 || N > 6 * (long long)F || (V == 0 && N > 0)) {
		set_error(name + ": counts are not what adgs_smooth_adjacency_count returned for this mesh"); return -1;
	}
	if ((V > 0 && !starts) || (N > 0 && (!neighbors || !temp))) { set_error(name + ": NULL pointer"); return -1; }
	if (V == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (N == 0) {
		ADGS_HIP_CHECK(hipMemsetAsync(starts, 0, ((size_t)V + 1) * sizeof(int), stream));
		return 0;
	}
	const AdjacencyTemp t = carve_adjacency((char*)temp, (size_t)F);
	const size_t n = 6 * (size_t)F;
	ADGS_LAUNCH(smooth_emit_kernel, dim3(blocks_of(n)), dim3(SMOOTH_THREADS), 0, stream, (const uint64_t*)t.k1, (const uint32_t*)t.v0, (uint32_t)n, pair_keys(V),
		(uint32_t)N, neighbors, t.v1);
	ADGS_LAUNCH(smooth_starts_kernel, dim3(blocks_of((size_t)V + 1)), dim3(SMOOTH_THREADS), 0, stream, (const uint32_t*)t.v1, (uint32_t)V, (uint32_t)N, starts);
	return 0;
}

extern "C" size_t adgs_smooth_steps_temp_bytes(long long V, long long N) {
	return sizes_ok(V, N) ? carve_steps(nullptr, (size_t)V).bytes : 0;
}

extern "C" int adgs_smooth_steps(int V, int N, const float* vertices, const int* starts, const int* neighbors, const unsigned char* fixed, int steps,
	double s_even, double s_odd, void* temp, float* out, void* stream_) {
	const std::string name("adgs_smooth_steps");
	if (V < 0 || N < 0) { set_error(name + ": negative V or N"); return -1; }
	if (steps < 0 || steps > MAX_STEPS) { set_error(name + ": steps must lie in [0, " + std::to_string(MAX_STEPS) + "]"); return -1; }
	if (!std::isfinite(s_even) || !std::isfinite(s_odd)) { set_error(name + ": the factors must be finite"); return -1; }
	if ((V > 0 && (!vertices || !starts || !out || (steps > 0 && !temp))) || (N > 0 && !neighbors)) { set_error(name + ": NULL pointer"); return -1; }
	if (V > 0 && out == vertices) { set_error(name + ": out must not be the input"); return -1; }
	if (V == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (steps == 0) {
		ADGS_HIP_CHECK(hipMemcpyAsync(out, vertices, 3 * (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, stream));
		return 0;
	}
	const StepsTemp t = carve_steps((char*)temp, (size_t)V);
	for (int k = 0; k < steps; k++) {
		const bool first = k == 0, last = k == steps - 1;
		const double s = k % 2 == 0 ? s_even : s_odd;
		const Row* cur = k % 2 == 0 ? t.b : t.a;                    // step 0 reads the float input and writes a
		Row* next = k % 2 == 0 ? t.a : t.b;
		int code;
		if (first && last) code = launch_step<true, true>(vertices, cur, starts, neighbors, fixed, V, N, s, next, out, stream);
		else if (first) code = launch_step<true, false>(vertices, cur, starts, neighbors, fixed, V, N, s, next, out, stream);
		else if (last) code = launch_step<false, true>(vertices, cur, starts, neighbors, fixed, V, N, s, next, out, stream);
		else code = launch_step<false, false>(vertices, cur, starts, neighbors, fixed, V, N, s, next, out, stream);
		if (code != 0) return -1;
	}
	return 0;
}
