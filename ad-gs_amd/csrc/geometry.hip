// Geometry evaluation on the device for gfx950 (wave64): exact bounded nearest neighbour over a uniform grid, area-weighted surface sampling,
// distance statistics.  The definitions are in include/adgs_geometry.h; this object is built with -ffp-contract=off.
//
//   plan     one launch: minimum, maximum and count of the finite points (order-independent atomics on ordered bit patterns) -> one read-back
//   build    keys -> stable radix sort -> gather into 16-byte records + head flags -> scan -> compact table of the occupied cells
//   nearest  keys of the queries -> the same sort -> one lane per query in key order: (2 R + 1)^2 rows, one lower-bound search per row
//   sample   one thread per sample: three splitmix64 words, an upper-bound search of the cdf, one point
//   stats    one partial row per workgroup over a fixed partition, a one-workgroup finish: no atomics
#include "common.h"
#include "mesh_shared.h"
#include "../../include/adgs_geometry.h"
#include <cmath>

namespace adgs {
namespace {

constexpr int GEO_THREADS = MESH_THREADS;                      // blocks_of (mesh_shared.h) counts workgroups of this size
constexpr int MAX_AXIS_CELLS = 1 << 21;
constexpr int MAX_RADIUS = 8;
constexpr int MAX_THRESHOLDS = 4;
constexpr int STATS_MAX_BLOCKS = 1024;
constexpr int STATS_ROW = 1 + MAX_THRESHOLDS;                 // integer columns of a partial row: the count without a neighbour, below each threshold

struct GridDesc { double origin[3]; double cell; int n[3]; };

// float <-> uint32 whose unsigned order is the order of the floats (finite values only reach it)
__device__ __forceinline__ uint32_t ordered_bits(float f) {
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float ordered_float(uint32_t o) {
	const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
	union { uint32_t u; float f; } v;
	v.u = u;
	return v.f;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// floor(((double)x - origin) / cell), clamped to [-2^22, 2^22] so that it is an int whatever the point
__device__ __forceinline__ int cell_of(float x, double origin, double cell) {
	const double c = floor(((double)x - origin) / cell);
	return (int)fmin(fmax(c, -4194304.0), 4194304.0);
}

// ---- plan ----

// box[0..2] minimum, box[3..5] maximum as ordered bits, box[6] the number of finite points.  Minimum, maximum and an integer count do
// not depend on the order of the atomics.
__global__ void __launch_bounds__(GEO_THREADS) geometry_box_kernel(const float* __restrict__ points, uint32_t M, uint32_t* __restrict__ box) {
	__shared__ uint32_t s[7];
	if (threadIdx.x < 7) s[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
	__syncthreads();
	const uint32_t i = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (i < M) {
		const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
		if (finite3(x, y, z)) {
			const uint32_t o[3] = { ordered_bits(x), ordered_bits(y), ordered_bits(z) };
#pragma unroll
			for (int k = 0; k < 3; k++) { atomicMin(&s[k], o[k]); atomicMax(&s[3 + k], o[k]); }
			atomicAdd(&s[6], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 7 && s[6] != 0u) {
		if (threadIdx.x < 3) atomicMin(box + threadIdx.x, s[threadIdx.x]);
		else if (threadIdx.x < 6) atomicMax(box + threadIdx.x, s[threadIdx.x]);
		else atomicAdd(box + 6, s[6]);
	}
}

// ---- keys (targets and queries) ----

// CLAMP false (targets): a point that is not finite or lies outside the grid gets the key `total` = nx ny nz.  CLAMP true (queries): the
// cell is clamped into the grid -- the key only orders the work --, and only a point that is not finite gets `total`.
template <bool CLAMP>
__global__ void __launch_bounds__(GEO_THREADS) geometry_keys_kernel(const float* __restrict__ points, uint32_t n, GridDesc g, uint64_t total,
	uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
	const uint32_t i = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (i >= n) return;
	const float p[3] = { points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2] };
	uint64_t key = total;
	if (finite3(p[0], p[1], p[2])) {
		int c[3];
		bool inside = true;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			c[k] = cell_of(p[k], g.origin[k], g.cell);
			if (CLAMP) c[k] = min(max(c[k], 0), g.n[k] - 1);
			else inside = inside && c[k] >= 0 && c[k] < g.n[k];
		}
		if (inside) key = ((uint64_t)c[2] * (uint64_t)g.n[1] + (uint64_t)c[1]) * (uint64_t)g.n[0] + (uint64_t)c[0];
	}
	keys[i] = key;
	vals[i] = i;
}

// ---- build ----

// records in sorted order, and flag[j] = 1 where a cell begins
__global__ void __launch_bounds__(GEO_THREADS) geometry_gather_kernel(const float* __restrict__ points, const uint64_t* __restrict__ keys,
	const uint32_t* __restrict__ vals, uint32_t M, uint64_t total, float4* __restrict__ records, uint32_t* __restrict__ flag) {
	const uint32_t j = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (j >= M) return;
	const uint32_t i = vals[j];
	const uint64_t key = keys[j];
	float4 r = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
	if (i < M) r = make_float4(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], __int_as_float((int)i));
	records[j] = r;
	flag[j] = (key < total && (j == 0 || keys[j - 1] != key)) ? 1u : 0u;
}

// pos[]: the exclusive scan of the head flags.  A head writes its cell; the last record in a cell writes the counts and the table's end.
// counts[] was zeroed before: it stays {0, 0} when no record lies in a cell.
__global__ void __launch_bounds__(GEO_THREADS) geometry_cells_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint32_t M,
	uint64_t total, uint64_t* __restrict__ cell_keys, uint32_t* __restrict__ cell_starts, uint32_t* __restrict__ counts) {
	const uint32_t j = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (j >= M) return;
	const uint64_t key = keys[j];
	if (key >= total) return;
	const bool head = j == 0 || keys[j - 1] != key;
	const uint32_t c = pos[j];                                  // < M: at most one head per record
	if (head && c < M) { cell_keys[c] = key; cell_starts[c] = j; }
	if (j + 1 == M || keys[j + 1] >= total) {
		const uint32_t C = c + (head ? 1u : 0u);
		if (C <= M) cell_starts[C] = j + 1;
		counts[0] = C; counts[1] = j + 1;
	}
}

// ---- nearest ----

__global__ void __launch_bounds__(GEO_THREADS) geometry_fill_kernel(uint32_t N, float* __restrict__ dist2, int* __restrict__ idx) {
	const uint32_t i = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (i < N) { dist2[i] = INFINITY; idx[i] = -1; }
}

// order[t]: the query handled by thread t (the queries sorted by their cell key).  One lane per query; every loop is bounded: (2 R + 1)^2
// rows, a bisection of the cell table (at most 32 steps), at most 2 R + 1 cells of the row, and the records of those cells.
__global__ void __launch_bounds__(GEO_THREADS) geometry_nearest_kernel(const float* __restrict__ queries, const uint32_t* __restrict__ order, uint32_t N,
	uint32_t M, GridDesc g, int R, float limit, const float4* __restrict__ records, const uint64_t* __restrict__ cell_keys,
	const uint32_t* __restrict__ cell_starts, const uint32_t* __restrict__ counts, float* __restrict__ dist2, int* __restrict__ idx) {
	const uint32_t t = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (t >= N) return;
	const uint32_t qi = order[t];
	if (qi >= N) return;                                        // cannot happen: order is a permutation of 0 .. N-1
	const float qx = queries[3 * (size_t)qi], qy = queries[3 * (size_t)qi + 1], qz = queries[3 * (size_t)qi + 2];
	// `limit` is the largest float with (double)limit <= (double)max_dist^2, so d2 <= limit is the definition's test without a double in the
	// loop; starting from (limit, INT_MAX) the update rule alone applies it: a d2 above limit never wins, one equal to it wins on the index.
	float best = limit;
	int best_index = INT_MAX;
	const uint32_t C = min(counts[0], M), n_rec = min(counts[1], M);
	if (finite3(qx, qy, qz) && C > 0) {
		const int cx = cell_of(qx, g.origin[0], g.cell), cy = cell_of(qy, g.origin[1], g.cell), cz = cell_of(qz, g.origin[2], g.cell);
		const int x0 = max(cx - R, 0), x1 = min(cx + R, g.n[0] - 1);
		for (int z = max(cz - R, 0); z <= min(cz + R, g.n[2] - 1) && x0 <= x1; z++) {
			for (int y = max(cy - R, 0); y <= min(cy + R, g.n[1] - 1); y++) {
				const uint64_t row = ((uint64_t)z * (uint64_t)g.n[1] + (uint64_t)y) * (uint64_t)g.n[0];
				const uint64_t klo = row + (uint64_t)x0, khi = row + (uint64_t)x1;
				uint32_t lo = 0, hi = C;                            // the first cell with a key >= klo
				while (lo < hi) {
					const uint32_t mid = lo + (hi - lo) / 2;
					if (cell_keys[mid] < klo) lo = mid + 1; else hi = mid;
				}
				uint32_t end = lo;                                  // the cells of the row: at most x1 - x0 + 1 of them
				for (int s = 0; s <= x1 - x0 && end < C && cell_keys[end] <= khi; s++) end++;
				if (end == lo) continue;
				const uint32_t j1 = min(cell_starts[end], n_rec);
				for (uint32_t j = cell_starts[lo]; j < j1; j++) {
					const float4 r = records[j];
					const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
					const float d2 = (dx * dx + dy * dy) + dz * dz;
					const int index = __float_as_int(r.w);
					if (d2 < best || (d2 == best && index < best_index)) { best = d2; best_index = index; }
				}
			}
		}
	}
	dist2[qi] = best_index == INT_MAX ? INFINITY : best;
	idx[qi] = best_index == INT_MAX ? -1 : best_index;
}

// ---- surface sampling (load_face, load_corners, face_edges: mesh_shared.h) ----

__global__ void __launch_bounds__(GEO_THREADS) geometry_areas_kernel(const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V, uint32_t F,
	double* __restrict__ areas) {
	const uint32_t f = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (f >= F) return;
	uint32_t i[3];
	double a = 0.0;
	if (load_face(faces, f, V, i)) {
		double p[3][3];
		load_corners(vertices, i, p);
		const FaceEdges e = face_edges(p[0], p[1], p[2]);
		const double nx = e.cross_x(), ny = e.cross_y(), nz = e.cross_z();
		a = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
	}
	areas[f] = a;
}

__device__ __forceinline__ double splitmix_unit(uint64_t seed, uint64_t counter) {
	uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (double)(z >> 11) * 0x1p-53;
}

__global__ void __launch_bounds__(GEO_THREADS) geometry_sample_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
	const double* __restrict__ cdf, uint32_t V, uint32_t F, uint32_t n, double total, double below_total, uint64_t seed, float* __restrict__ points,
	int* __restrict__ face) {
	const uint32_t k = blockIdx.x * (uint32_t)GEO_THREADS + threadIdx.x;
	if (k >= n) return;
	const double u0 = splitmix_unit(seed, 3ull * k + 1);
	double u1 = splitmix_unit(seed, 3ull * k + 2), u2 = splitmix_unit(seed, 3ull * k + 3);
	const double t = fmin(u0 * total, below_total);
	uint32_t lo = 0, hi = F;                                    // the first face with cdf[f] > t: at most 31 steps
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (cdf[mid] > t) hi = mid; else lo = mid + 1;
	}
	const uint32_t f = min(lo, F - 1);                          // lo < F whenever cdf[F - 1] = total
	if (u1 + u2 > 1.0) { u1 = 1.0 - u1; u2 = 1.0 - u2; }
	uint32_t i[3];
	if (!load_face(faces, f, V, i)) {                           // only with a cdf that steps at such a face
		points[3 * (size_t)k] = points[3 * (size_t)k + 1] = points[3 * (size_t)k + 2] = NAN;
		face[k] = -1;
		return;
	}
	double p[3][3];
	load_corners(vertices, i, p);
#pragma unroll
	for (int d = 0; d < 3; d++) points[3 * (size_t)k + d] = (float)((p[0][d] + u1 * (p[1][d] - p[0][d])) + u2 * (p[2][d] - p[0][d]));
	face[k] = (int)f;
}

// ---- distance statistics ----

struct StatsArgs { double tau2[MAX_THRESHOLDS]; double max_dist; int nt; };

// sums over the workgroup in a fixed order: the wave's butterfly, then the waves in order; valid in thread 0
__device__ __forceinline__ void block_sums(double& sum, unsigned long long (&cnt)[STATS_ROW]) {
	__shared__ double s_sum[GEO_THREADS / WAVE];
	__shared__ unsigned long long s_cnt[STATS_ROW][GEO_THREADS / WAVE];
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1) {
		sum += __shfl_xor(sum, off, WAVE);
#pragma unroll
		for (int q = 0; q < STATS_ROW; q++) cnt[q] += __shfl_xor(cnt[q], off, WAVE);
	}
	if ((threadIdx.x & (WAVE - 1)) == 0) {
		s_sum[threadIdx.x / WAVE] = sum;
#pragma unroll
		for (int q = 0; q < STATS_ROW; q++) s_cnt[q][threadIdx.x / WAVE] = cnt[q];
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		sum = 0.0;
		for (int w = 0; w < GEO_THREADS / WAVE; w++) sum += s_sum[w];
#pragma unroll
		for (int q = 0; q < STATS_ROW; q++) { cnt[q] = 0; for (int w = 0; w < GEO_THREADS / WAVE; w++) cnt[q] += s_cnt[q][w]; }
	}
}

// workgroup b sums the elements [b * chunk, (b + 1) * chunk), chunk a multiple of the workgroup: thread t takes t, t + 256, ... in order
__global__ void __launch_bounds__(GEO_THREADS) geometry_stats_kernel(const float* __restrict__ dist2, uint32_t N, uint32_t chunk, StatsArgs a,
	double* __restrict__ part_sum, unsigned long long* __restrict__ part_cnt) {
	double sum = 0.0;
	unsigned long long cnt[STATS_ROW];
#pragma unroll
	for (int q = 0; q < STATS_ROW; q++) cnt[q] = 0;
	const size_t begin = (size_t)blockIdx.x * chunk, end = min(begin + (size_t)chunk, (size_t)N);
	for (size_t i = begin + threadIdx.x; i < end; i += GEO_THREADS) {
		const float d2 = dist2[i];
		const bool none = !(d2 < INFINITY);
		const double d = (double)d2;
		sum += none ? a.max_dist : fmin(sqrt(d), a.max_dist);
		cnt[0] += none ? 1u : 0u;
#pragma unroll
		for (int q = 0; q < MAX_THRESHOLDS; q++) cnt[1 + q] += (q < a.nt && d < a.tau2[q]) ? 1u : 0u;
	}
	block_sums(sum, cnt);
	if (threadIdx.x == 0) {
		part_sum[blockIdx.x] = sum;
#pragma unroll
		for (int q = 0; q < STATS_ROW; q++) part_cnt[(size_t)blockIdx.x * STATS_ROW + q] = cnt[q];
	}
}

// one workgroup: thread t adds the rows t, t + 256, ... in order
__global__ void __launch_bounds__(GEO_THREADS) geometry_stats_finish_kernel(const double* __restrict__ part_sum, const unsigned long long* __restrict__ part_cnt,
	uint32_t rows, uint32_t N, double* __restrict__ out) {
	double sum = 0.0;
	unsigned long long cnt[STATS_ROW];
#pragma unroll
	for (int q = 0; q < STATS_ROW; q++) cnt[q] = 0;
	for (uint32_t r = threadIdx.x; r < rows; r += GEO_THREADS) {
		sum += part_sum[r];
#pragma unroll
		for (int q = 0; q < STATS_ROW; q++) cnt[q] += part_cnt[(size_t)r * STATS_ROW + q];
	}
	block_sums(sum, cnt);
	if (threadIdx.x == 0) {
		out[0] = sum; out[1] = (double)N; out[2] = (double)cnt[0];
#pragma unroll
		for (int q = 0; q < MAX_THRESHOLDS; q++) out[3 + q] = (double)cnt[1 + q];
		out[7] = 0.0;
	}
}

// ---- host ----

// build: the box of the plan, two copies of the keys and values (the sort ping-pongs), the head flags (scanned in place), the scratch of the
// sort and of the scan (used one after the other)
struct GridTemp { uint32_t* box; uint64_t *k0, *k1; uint32_t *v0, *v1, *flag; char* prim; size_t bytes; };
GridTemp carve_grid(char* base, size_t M) {
	Carver c(base);
	GridTemp t;
	t.box = c.take<uint32_t>(8);
	t.k0 = c.take<uint64_t>(M); t.k1 = c.take<uint64_t>(M); t.v0 = c.take<uint32_t>(M); t.v1 = c.take<uint32_t>(M); t.flag = c.take<uint32_t>(M);
	const size_t a = sort_temp_bytes(M), b = scan_temp_bytes(M);
	t.prim = c.take<char>(a > b ? a : b);
	t.bytes = c.size();
	return t;
}

struct NearestTemp { uint64_t *k0, *k1; uint32_t *v0, *v1; char* sort; size_t bytes; };
NearestTemp carve_nearest(char* base, size_t N) {
	Carver c(base);
	NearestTemp t;
	t.k0 = c.take<uint64_t>(N); t.k1 = c.take<uint64_t>(N); t.v0 = c.take<uint32_t>(N); t.v1 = c.take<uint32_t>(N);
	t.sort = c.take<char>(sort_temp_bytes(N));
	t.bytes = c.size();
	return t;
}

struct StatsTemp { double* sum; unsigned long long* cnt; size_t bytes; };
StatsTemp carve_stats(char* base) {
	Carver c(base);
	StatsTemp t;
	t.sum = c.take<double>(STATS_MAX_BLOCKS); t.cnt = c.take<unsigned long long>((size_t)STATS_MAX_BLOCKS * STATS_ROW);
	t.bytes = c.size();
	return t;
}

// the grid of the arguments; false with a message when they are refused
bool grid_of(const std::string& name, float cell_size, const float* origin, const int* dims, GridDesc& g, uint64_t& total, int& key_bits) {
	if (!positive(cell_size)) { set_error(name + ": cell_size must be finite and positive"); return false; }
	if (!origin || !dims) { set_error(name + ": NULL origin or dims"); return false; }
	for (int k = 0; k < 3; k++) {
		if (dims[k] < 0 || dims[k] > MAX_AXIS_CELLS) {
			set_error(name + ": " + std::to_string(dims[k]) + " cells on axis " + std::to_string(k) + ", at most 2^21 are supported: enlarge cell_size");
			return false;
		}
		if (!std::isfinite(origin[k])) { set_error(name + ": origin must be finite"); return false; }
		g.origin[k] = (double)origin[k]; g.n[k] = dims[k];
	}
	g.cell = (double)cell_size;
	total = (uint64_t)dims[0] * (uint64_t)dims[1] * (uint64_t)dims[2];      // <= 2^63
	key_bits = bits_of(total, 64);                              // the keys are 0 .. total
	return true;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_geometry_grid_temp_bytes(long long M) { return count_ok(M) ? carve_grid(nullptr, (size_t)M).bytes : 0; }

extern "C" int adgs_geometry_grid_plan(int M, const float* points, float cell_size, void* temp, float* origin, int* dims, long long* num_finite,
	void* stream_) {
	const std::string name("adgs_geometry_grid_plan");
	if (M < 0) { set_error(name + ": negative M"); return -1; }
	if (!positive(cell_size)) { set_error(name + ": cell_size must be finite and positive"); return -1; }
	if (!origin || !dims || !num_finite) { set_error(name + ": NULL origin, dims or num_finite"); return -1; }
	if (M > 0 && (!points || !temp)) { set_error(name + ": NULL pointer"); return -1; }
	for (int k = 0; k < 3; k++) { origin[k] = 0.f; dims[k] = 0; }
	*num_finite = 0;
	if (M == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const GridTemp t = carve_grid((char*)temp, (size_t)M);
	const uint32_t init[8] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u };
	ADGS_HIP_CHECK(hipMemcpyAsync(t.box, init, sizeof(init), hipMemcpyHostToDevice, stream));
	ADGS_LAUNCH(geometry_box_kernel, dim3(blocks_of(M)), dim3(GEO_THREADS), 0, stream, points, (uint32_t)M, t.box);
	uint32_t host[8];
	ADGS_HIP_CHECK(hipMemcpyAsync(host, t.box, sizeof(host), hipMemcpyDeviceToHost, stream));
	ADGS_HIP_CHECK(hipStreamSynchronize(stream));
	if (host[6] == 0u) return 0;
	if (host[6] > (uint32_t)M) { set_error(name + ": a count exceeds M"); return -1; }     // cannot happen
	*num_finite = (long long)host[6];
	for (int k = 0; k < 3; k++) {
		origin[k] = ordered_float(host[k]);
		const double cells = std::floor(((double)ordered_float(host[3 + k]) - (double)origin[k]) / (double)cell_size) + 1.0;
		if (!(cells <= (double)MAX_AXIS_CELLS)) {
			char buf[64];
			snprintf(buf, sizeof buf, "%.0f", cells);
			set_error(name + ": " + buf + " cells on axis " + std::to_string(k) + ", at most 2^21 are supported: enlarge cell_size");
			return -2;
		}
		dims[k] = (int)cells;
	}
	return 0;
}

extern "C" int adgs_geometry_grid_build(int M, const float* points, float cell_size, const float* origin, const int* dims, void* temp, float* records,
	unsigned long long* cell_keys, unsigned int* cell_starts, unsigned int* counts, void* stream_) {
	const std::string name("adgs_geometry_grid_build");
	if (M < 0) { set_error(name + ": negative M"); return -1; }
	GridDesc g; uint64_t total; int bits;
	if (!grid_of(name, cell_size, origin, dims, g, total, bits)) return -1;
	if (!counts) { set_error(name + ": NULL counts"); return -1; }
	if (M > 0 && (!points || !temp || !records || !cell_keys || !cell_starts)) { set_error(name + ": NULL pointer"); return -1; }
	if (M == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const GridTemp t = carve_grid((char*)temp, (size_t)M);
	ADGS_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), stream));
	ADGS_LAUNCH(geometry_keys_kernel<false>, dim3(blocks_of(M)), dim3(GEO_THREADS), 0, stream, points, (uint32_t)M, g, total, t.k0, t.v0);
	if (radix_sort_pairs_u64(t.k0, t.k1, t.v0, t.v1, (size_t)M, bits, t.prim, stream) != 0) return -1;
	ADGS_LAUNCH(geometry_gather_kernel, dim3(blocks_of(M)), dim3(GEO_THREADS), 0, stream, points, (const uint64_t*)t.k1, (const uint32_t*)t.v1, (uint32_t)M,
		total, reinterpret_cast<float4*>(records), t.flag);
	if (exclusive_scan_u32(t.flag, t.flag, (size_t)M, t.prim, stream) != 0) return -1;
	ADGS_LAUNCH(geometry_cells_kernel, dim3(blocks_of(M)), dim3(GEO_THREADS), 0, stream, (const uint64_t*)t.k1, (const uint32_t*)t.flag, (uint32_t)M, total,
		reinterpret_cast<uint64_t*>(cell_keys), cell_starts, counts);
	return 0;
}

extern "C" size_t adgs_geometry_nearest_temp_bytes(long long N) { return count_ok(N) ? carve_nearest(nullptr, (size_t)N).bytes : 0; }

extern "C" int adgs_geometry_nearest(int M, int N, const float* queries, float max_dist, float cell_size, const float* origin, const int* dims,
	const float* records, const unsigned long long* cell_keys, const unsigned int* cell_starts, const unsigned int* counts, void* temp,
	float* dist2, int* idx, void* stream_) {
	const std::string name("adgs_geometry_nearest");
	if (M < 0 || N < 0) { set_error(name + ": negative M or N"); return -1; }
	if (!positive(max_dist)) { set_error(name + ": max_dist must be finite and positive"); return -1; }
	GridDesc g; uint64_t total; int bits;
	if (!grid_of(name, cell_size, origin, dims, g, total, bits)) return -1;
	const double cells = std::ceil((double)max_dist * (1.0 + 0x1p-20) / (double)cell_size);
	if (!(cells <= (double)MAX_RADIUS)) {
		char buf[64];
		snprintf(buf, sizeof buf, "%.0f", cells);
		set_error(name + ": max_dist spans " + buf + " cells, at most 8 are searched: enlarge cell_size");
		return -1;
	}
	const bool empty = M == 0 || total == 0;
	if (N > 0 && (!queries || !dist2 || !idx)) { set_error(name + ": NULL pointer"); return -1; }
	if (N > 0 && !empty && (!records || !cell_keys || !cell_starts || !counts || !temp)) { set_error(name + ": NULL pointer"); return -1; }
	if (N == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	if (empty) {
		ADGS_LAUNCH(geometry_fill_kernel, dim3(blocks_of(N)), dim3(GEO_THREADS), 0, stream, (uint32_t)N, dist2, idx);
		return 0;
	}
	const NearestTemp t = carve_nearest((char*)temp, (size_t)N);
	const double max_dist2 = (double)max_dist * (double)max_dist;
	float limit = (float)max_dist2;                             // the largest float that passes (double)d2 <= max_dist2 ...
	if ((double)limit > max_dist2) limit = std::nextafter(limit, 0.0f);      // ... FLT_MAX when max_dist2 is beyond the floats
	ADGS_LAUNCH(geometry_keys_kernel<true>, dim3(blocks_of(N)), dim3(GEO_THREADS), 0, stream, queries, (uint32_t)N, g, total, t.k0, t.v0);
	if (radix_sort_pairs_u64(t.k0, t.k1, t.v0, t.v1, (size_t)N, bits, t.sort, stream) != 0) return -1;
	ADGS_LAUNCH(geometry_nearest_kernel, dim3(blocks_of(N)), dim3(GEO_THREADS), 0, stream, queries, (const uint32_t*)t.v1, (uint32_t)N, (uint32_t)M, g,
		(int)cells, limit, reinterpret_cast<const float4*>(records), reinterpret_cast<const uint64_t*>(cell_keys), cell_starts,
		counts, dist2, idx);
	return 0;
}

extern "C" int adgs_geometry_face_areas(int V, int F, const float* vertices, const int* faces, double* areas, void* stream_) {
	const std::string name("adgs_geometry_face_areas");
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if (F > 0 && (!faces || !areas || (V > 0 && !vertices))) { set_error(name + ": NULL pointer"); return -1; }
	if (F == 0) return 0;
	ADGS_LAUNCH(geometry_areas_kernel, dim3(blocks_of(F)), dim3(GEO_THREADS), 0, (hipStream_t)stream_, vertices, faces, (uint32_t)V, (uint32_t)F, areas);
	return 0;
}

extern "C" int adgs_geometry_sample(int V, int F, int n, const float* vertices, const int* faces, const double* cdf, double total,
	unsigned long long seed, float* points, int* face, void* stream_) {
	const std::string name("adgs_geometry_sample");
	if (V < 0 || F < 0 || n < 0) { set_error(name + ": negative V, F or n"); return -1; }
	if (n == 0) return 0;
	if (F == 0) { set_error(name + ": no face to sample from"); return -1; }
	if (!positive(total)) { set_error(name + ": the total area (cdf[F - 1]) must be finite and positive"); return -1; }
	if (!faces || !cdf || !points || !face || (V > 0 && !vertices)) { set_error(name + ": NULL pointer"); return -1; }
	ADGS_LAUNCH(geometry_sample_kernel, dim3(blocks_of(n)), dim3(GEO_THREADS), 0, (hipStream_t)stream_, vertices, faces, cdf, (uint32_t)V, (uint32_t)F,
		(uint32_t)n, total, std::nextafter(total, 0.0), (uint64_t)seed, points, face);
	return 0;
}

extern "C" size_t adgs_geometry_stats_temp_bytes(long long N) { return count_ok(N) ? carve_stats(nullptr).bytes : 0; }

extern "C" int adgs_geometry_distance_stats(int N, const float* dist2, int num_thresholds, const double* thresholds, double max_dist, void* temp,
	double* out, void* stream_) {
	const std::string name("adgs_geometry_distance_stats");
	if (N < 0) { set_error(name + ": negative N"); return -1; }
	if (num_thresholds < 0 || num_thresholds > MAX_THRESHOLDS) { set_error(name + ": num_thresholds must lie in [0, 4]"); return -1; }
	if (!positive(max_dist)) { set_error(name + ": max_dist must be finite and positive"); return -1; }
	if (num_thresholds > 0 && !thresholds) { set_error(name + ": NULL thresholds"); return -1; }
	StatsArgs a;
	a.max_dist = max_dist; a.nt = num_thresholds;
	for (int q = 0; q < MAX_THRESHOLDS; q++) {
		a.tau2[q] = 0.0;
		if (q >= num_thresholds) continue;
		if (!positive(thresholds[q])) { set_error(name + ": thresholds must be finite and positive"); return -1; }
		a.tau2[q] = thresholds[q] * thresholds[q];
	}
	if (!out || !temp || (N > 0 && !dist2)) { set_error(name + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const StatsTemp t = carve_stats((char*)temp);
	// the partition is a function of N alone: rows workgroups of `chunk` elements, chunk a multiple of the workgroup
	uint32_t rows = 0, chunk = 0;
	if (N > 0) {
		const size_t groups = ((size_t)N + GEO_THREADS - 1) / GEO_THREADS;
		const size_t per = (groups + STATS_MAX_BLOCKS - 1) / STATS_MAX_BLOCKS;
		chunk = (uint32_t)(per * GEO_THREADS);
		rows = (uint32_t)(((size_t)N + chunk - 1) / chunk);
		ADGS_LAUNCH(geometry_stats_kernel, dim3(rows), dim3(GEO_THREADS), 0, stream, dist2, (uint32_t)N, chunk, a, t.sum, t.cnt);
	}
	ADGS_LAUNCH(geometry_stats_finish_kernel, dim3(1), dim3(GEO_THREADS), 0, stream, (const double*)t.sum, (const unsigned long long*)t.cnt, rows, (uint32_t)N, out);
	return 0;
}
