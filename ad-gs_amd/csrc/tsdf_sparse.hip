// The block-sparse TSDF volume for gfx950 (wave64): allocation of 8 x 8 x 8 blocks from a view, integration over the allocated blocks and
// marching tetrahedra on the unbounded lattice.  The definition is in include/adgs_sparse_tsdf.h; the per-point update chain, classify,
// cell_faces and the faces of a cell are the dense volume's own device functions (tsdf_shared.h), and this file is built with tsdf.o's flags.
//
// Allocate: count, scan, emit, sort, flag, scan, merge -- no hash table, no atomics on values.
//   candidates   one lane per pixel; per sample and cube corner the wave reduces its lanes' block keys to the distinct ones (a first-lane
//                broadcast loop over the remaining lanes), drops those among the wave's last 64 distinct keys (one per lane) and those in the
//                table (lower-bound search) and counts the rest per wave; a lane skips a corner whose key it had at the previous sample.
//                Run twice: count, then (after the scan) emit.
//   sort         radix_sort_pairs_u64 over the device-side candidate count
//   flag + scan  a head flag per distinct new key; exclusive_scan_u32_sum gives each new key its rank and the number of new blocks
//   merge        by rank: an old entry moves up by the new keys below it, a new key by the old entries below it; the new blocks' slots are
//                NB + rank.  The merged table goes to the OUTPUT arrays, so a call that runs out of room leaves the volume alone.
// Integrate: one workgroup of 256 per allocated block in pool order; a wave owns a z-slice of 8 x 8 points (256 contiguous bytes per array)
// and each thread two slices.  The block test (bounding sphere against `near` and the frustum) is workgroup-uniform and comes first.
// Extract: one workgroup of 512 per block in key order.  The 27 neighbour blocks are resolved once per workgroup; tsdf and wsum of the
// 10 x 10 x 10 neighbourhood (-1 .. +8) are staged in LDS (8 KB), unallocated points as tsdf 1 / wsum 0, and classify runs on that little
// lattice.  Owner words are per block that owns a vertex, as the dense volume keeps them per chunk.
#include "common.h"
#include "tsdf_shared.h"
#include "../../include/adgs_sparse_tsdf.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

constexpr int SB = ADGS_SPARSE_TSDF_BLOCK, SBP = ADGS_SPARSE_TSDF_BLOCK_POINTS, SN = SB + 2, SNP = SN * SN * SN;
constexpr int COORD_LIMIT = ADGS_SPARSE_TSDF_COORD_LIMIT, MAX_BLOCKS = ADGS_SPARSE_TSDF_MAX_BLOCKS;
constexpr int ALLOC_THREADS = 256, INTEGRATE_THREADS = 256, EXTRACT_THREADS = SBP;
constexpr uint64_t NO_KEY = ~0ull;                              // no block key (those have 63 bits, and 2^63 - 1 is one); sorts last
static_assert(SB == 8 && SBP == SB * SB * SB && ADGS_SPARSE_TSDF_OWNER_BYTES_PER_BLOCK == SBP * sizeof(uint32_t), "one word per owner of a block");
static_assert(COORD_LIMIT == 1 << 20 && MAX_BLOCKS == 1 << 22, "21 bits per block coordinate");

// |b| < 2^20 on every axis
__host__ __device__ __forceinline__ uint64_t block_key(int bx, int by, int bz) {
	return ((uint64_t)(uint32_t)(bz + COORD_LIMIT) << 42) | ((uint64_t)(uint32_t)(by + COORD_LIMIT) << 21) | (uint64_t)(uint32_t)(bx + COORD_LIMIT);
}
__device__ __forceinline__ void key_coords(uint64_t key, int& bx, int& by, int& bz) {
	bx = (int)(key & 0x1FFFFFu) - COORD_LIMIT; by = (int)((key >> 21) & 0x1FFFFFu) - COORD_LIMIT; bz = (int)((key >> 42) & 0x1FFFFFu) - COORD_LIMIT;
}
// the first index of the ascending keys[0, n) with keys[index] >= k: at most 23 steps
__device__ __forceinline__ uint32_t lower_bound_key(const uint64_t* __restrict__ keys, uint32_t n, uint64_t k) {
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (keys[mid] < k) lo = mid + 1; else hi = mid;
	}
	return lo;
}
__device__ __forceinline__ bool in_table(const uint64_t* __restrict__ keys, uint32_t n, uint64_t k) {
	const uint32_t r = lower_bound_key(keys, n, k);
	return r < n && keys[r] == k;
}

// ---- allocation ----

struct AllocView {
	int H, W, inv_depth, steps;         // steps: n
	double kx, ky, cx, cy;
	double R[9], t[3];
	double near, max_depth, trunc, dz;  // dz = 2 trunc / n
	double o[3], vs, rho;               // rho: the margin in voxels
	float min_opacity;
};

// what the allocation keeps on the device between its kernels, and reads back
struct AllocState {
	unsigned long long counts[4];       // new blocks, candidates, skipped samples, 1 when nothing was allocated
	uint32_t n_sort;                    // min(candidates, max_candidates)
	uint32_t n_new;                     // 0 when nothing is allocated
};

// EMIT false: wave_base[w] = the number of candidate keys of wave w.  EMIT true: wave_base is scanned; writes the candidates.
template <bool EMIT>
__global__ void __launch_bounds__(ALLOC_THREADS) sparse_candidates_kernel(AllocView v, const float* __restrict__ depth, const float* __restrict__ opacity,
	const float* __restrict__ weight, const uint64_t* __restrict__ keys, uint32_t NB, uint32_t* __restrict__ wave_base, uint64_t* __restrict__ cand,
	uint32_t cand_cap, AllocState* __restrict__ state) {
	const int lane = threadIdx.x & (WAVE - 1);
	const size_t wave = (size_t)blockIdx.x * (ALLOC_THREADS / WAVE) + threadIdx.x / WAVE;
	const long long pix = (long long)blockIdx.x * ALLOC_THREADS + threadIdx.x, npix = (long long)v.H * v.W;
	bool ok = pix < npix;
	double zd = 0.0, rx = 0.0, ry = 0.0;
	if (ok) {
		const float Of = opacity[pix], Df = depth[pix];
		ok = Of >= v.min_opacity && Df > 0.f;
		if (ok && weight) ok = weight[pix] > 0.f;
		if (ok) {
			zd = v.inv_depth ? (double)Of / (double)Df : (double)Df / (double)Of;
			ok = zd <= v.max_depth;
			const int yi = (int)(pix / v.W), xi = (int)(pix - (long long)yi * v.W);
			rx = ((double)xi - v.cx) / v.kx; ry = ((double)yi - v.cy) / v.ky;
		}
	}
	uint64_t prev[8];
#pragma unroll
	for (int c = 0; c < 8; c++) prev[c] = NO_KEY;
	const uint32_t base = EMIT ? wave_base[wave] : 0u;
	uint32_t cnt = 0, nskip = 0, head = 0;                        // cnt and head are wave-uniform
	uint64_t recent = NO_KEY;
	for (int m = 0; m <= v.steps; m++) {                          // every lane of the wave takes every turn: the ballots below need them all
		const double zm = zd - v.trunc + (double)m * v.dz;
		bool s = ok && zm > v.near;
		int lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
		if (s) {
			const double c0 = rx * zm - v.t[0], c1 = ry * zm - v.t[1], c2 = zm - v.t[2];
#pragma unroll
			for (int a = 0; a < 3; a++) {
				const double g = ((v.R[a] * c0 + v.R[3 + a] * c1 + v.R[6 + a] * c2) - v.o[a]) / v.vs;
				const double l = floor((g - v.rho) * 0.125), h = floor((g + v.rho) * 0.125);
				if (!(l >= -(double)COORD_LIMIT && h < (double)COORD_LIMIT)) s = false;     // false for NaN
				else { lo[a] = (int)l; hi[a] = (int)h; }
			}
			if (!s) nskip++;
		}
#pragma unroll
		for (int c = 0; c < 8; c++) {
			// corner c of the cube: the upper block on the axes of its bits; a repeat of a lower corner where the cube stays inside one block
			const bool fresh = s && !((c & 1) && hi[0] == lo[0]) && !((c & 2) && hi[1] == lo[1]) && !((c & 4) && hi[2] == lo[2]);
			const uint64_t key = fresh ? block_key(c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2]) : NO_KEY;
			const bool cv = fresh && key != prev[c];              // the key it had at the previous sample went through the wave then
			prev[c] = key;
			bool mine = false;
			unsigned long long left = __ballot(cv);
			while (left) {                                          // wave-uniform
				const int leader = __ffsll(left) - 1;
				const uint64_t k = ((uint64_t)__shfl((uint32_t)(key >> 32), leader, WAVE) << 32) | (uint64_t)__shfl((uint32_t)key, leader, WAVE);
				const unsigned long long same = __ballot(cv && key == k);
				// the wave's last 64 distinct keys, one per lane: another corner or an earlier sample has usually been here
				const bool seen = __ballot(recent == k) != 0ull;
				if (!seen) {
					if (lane == (int)(head & (WAVE - 1))) recent = k;
					head++;
					if (lane == leader) mine = true;
				}
				left &= ~same;                                      // the leader is among them
			}
			if (mine && in_table(keys, NB, key)) mine = false;
			const unsigned long long mm = __ballot(mine);
			if (EMIT && mine) {
				const uint32_t pos = base + cnt + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
				if (pos < cand_cap) cand[pos] = key;
			}
			cnt += (uint32_t)__popcll(mm);
		}
	}
	if (!EMIT) {
		if (lane == 0) wave_base[wave] = cnt;
		if (nskip) atomicAdd(&state->counts[2], (unsigned long long)nskip);
	}
}

// coords [M, 3] -> keys (NO_KEY outside the range)
__global__ void __launch_bounds__(ALLOC_THREADS) sparse_coord_keys_kernel(const int* __restrict__ coords, uint32_t M, uint64_t* __restrict__ cand,
	AllocState* __restrict__ state) {
	const uint32_t i = blockIdx.x * (uint32_t)ALLOC_THREADS + threadIdx.x;
	if (i == 0) { state->counts[1] = M; state->n_sort = M; }
	if (i >= M) return;
	const int bx = coords[3 * (size_t)i], by = coords[3 * (size_t)i + 1], bz = coords[3 * (size_t)i + 2];
	const bool good = bx >= -COORD_LIMIT && bx < COORD_LIMIT && by >= -COORD_LIMIT && by < COORD_LIMIT && bz >= -COORD_LIMIT && bz < COORD_LIMIT;
	cand[i] = good ? block_key(bx, by, bz) : NO_KEY;
	if (!good) atomicAdd(&state->counts[2], 1ull);
}

__global__ void sparse_candidate_total_kernel(const unsigned long long* __restrict__ aux, uint32_t cand_cap, AllocState* __restrict__ state) {
	unsigned long long total = 0;
	for (int s = 0; s < SCAN_AUX_SLOTS; s++) total += aux[s];
	state->counts[1] = total;
	state->n_sort = (uint32_t)(total < (unsigned long long)cand_cap ? total : (unsigned long long)cand_cap);
}

// flags[i] = 1 where sorted[i] is the first of its key, a block key, and not in the table; 0 up to cand_cap
__global__ void __launch_bounds__(ALLOC_THREADS) sparse_head_flags_kernel(const uint64_t* __restrict__ sorted, uint32_t cand_cap, const uint64_t* __restrict__ keys,
	uint32_t NB, const AllocState* __restrict__ state, uint32_t* __restrict__ flags) {
	const uint32_t i = blockIdx.x * (uint32_t)ALLOC_THREADS + threadIdx.x;
	if (i >= cand_cap) return;
	uint32_t f = 0;
	if (i < state->n_sort) {
		const uint64_t k = sorted[i];
		f = k != NO_KEY && (i == 0 || sorted[i - 1] != k) && !in_table(keys, NB, k) ? 1u : 0u;
	}
	flags[i] = f;
}

__global__ void sparse_new_total_kernel(const unsigned long long* __restrict__ aux, uint32_t cand_cap, uint32_t NB, uint32_t room, AllocState* __restrict__ state) {
	unsigned long long n = 0;
	for (int s = 0; s < SCAN_AUX_SLOTS; s++) n += aux[s];
	const bool fits = state->counts[1] <= (unsigned long long)cand_cap && (unsigned long long)NB + n <= (unsigned long long)room;
	state->counts[0] = n;
	state->counts[3] = fits ? 0ull : 1ull;
	state->n_new = fits ? (uint32_t)n : 0u;
}

// thread i: the old table entry i and the sorted candidate i.  room >= NB + n_new wherever n_new > 0.
__global__ void __launch_bounds__(ALLOC_THREADS) sparse_merge_kernel(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
	const uint64_t* __restrict__ keys, const int* __restrict__ slots, uint32_t NB, uint32_t room, const AllocState* __restrict__ state,
	uint64_t* __restrict__ keys_out, int* __restrict__ slots_out, int* __restrict__ block_coords) {
	const uint32_t i = blockIdx.x * (uint32_t)ALLOC_THREADS + threadIdx.x;
	const uint32_t n_new = state->n_new, n_sort = state->n_sort;
	if (state->counts[3]) return;                               // no room: nothing is allocated
	if (i < NB) {
		const uint64_t k = keys[i];
		const uint32_t q = lower_bound_key(sorted, n_sort, k);      // the new keys below k are the flagged candidates before q
		const uint32_t p = i + (q < n_sort ? pos[q] : n_new);
		if (p < room) { keys_out[p] = k; slots_out[p] = slots[i]; }
	}
	if (i < n_sort && flags[i]) {
		const uint64_t k = sorted[i];
		const uint32_t j = pos[i], p = j + lower_bound_key(keys, NB, k), slot = NB + j;
		if (j < n_new && p < room && slot < room) {
			keys_out[p] = k; slots_out[p] = (int)slot;
			int bx, by, bz;
			key_coords(k, bx, by, bz);
			block_coords[3 * (size_t)slot] = bx; block_coords[3 * (size_t)slot + 1] = by; block_coords[3 * (size_t)slot + 2] = bz;
		}
	}
}

// ---- integration ----

// the block test: a block's points lie within `radius` of its centre; the four side planes of the frustum, widened by a pixel as the per-point
// cull is, are f(X_c) = a x + b z >= 0 (or y for x), and |grad f| radius bounds f over the sphere
struct BlockCull { double radius, left_b, right_b, top_b, bottom_b, left_r, right_r, top_r, bottom_r; };

__global__ void __launch_bounds__(INTEGRATE_THREADS) sparse_integrate_kernel(Lattice L, TsdfView v, BlockCull cull, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ image, const float* __restrict__ weight, const int* __restrict__ block_coords,
	float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ color) {
	const size_t slot = blockIdx.x;
	const int bx = block_coords[3 * slot], by = block_coords[3 * slot + 1], bz = block_coords[3 * slot + 2];
	{	// workgroup-uniform; skips only a block whose every point fails steps 1-3
		const double h = 0.5 * (double)(SB - 1);
		const double C0 = L.o[0] + L.vs * ((double)(SB * bx) + h), C1 = L.o[1] + L.vs * ((double)(SB * by) + h), C2 = L.o[2] + L.vs * ((double)(SB * bz) + h);
		const double z = v.R[6] * C0 + v.R[7] * C1 + v.R[8] * C2 + v.t[2];
		if (z + cull.radius <= v.near) return;
		const double xk = (v.R[0] * C0 + v.R[1] * C1 + v.R[2] * C2 + v.t[0]) * v.kx, yk = (v.R[3] * C0 + v.R[4] * C1 + v.R[5] * C2 + v.t[1]) * v.ky;
		if (xk + cull.left_b * z < -cull.left_r || xk - cull.right_b * z > cull.right_r || yk + cull.top_b * z < -cull.top_r || yk - cull.bottom_b * z > cull.bottom_r)
			return;
	}
	const int lx = threadIdx.x & (SB - 1), ly = (threadIdx.x >> 3) & (SB - 1);
#pragma unroll
	for (int half = 0; half < 2; half++) {
		const int lz = (int)(threadIdx.x >> 6) + half * (INTEGRATE_THREADS / WAVE);
		const size_t local = (size_t)((lz * SB + ly) * SB + lx);
		tsdf_update_point(L, v, SB * bx + lx, SB * by + ly, SB * bz + lz, depth, opacity, image, weight, tsdf + slot * SBP + local, wsum + slot * SBP + local,
			color ? color + slot * (3 * SBP) + local : nullptr, (size_t)SBP);
	}
}

// ---- extraction ----

struct BlockStage {
	float t[SNP], w[SNP];               // the points 8 b - 1 .. 8 b + 8 on every axis, x fastest
	int slot[27], rank[27];             // of the neighbour block b + d, index ((dz + 1) 3 + dy + 1) 3 + dx + 1; -1: not allocated
	uint32_t wave[EXTRACT_THREADS / WAVE];
};

// every thread of the workgroup calls it; r < NB.  Every index into the pool comes from a slot checked against the capacity.
__device__ __forceinline__ void stage_block(BlockStage& S, const uint64_t* __restrict__ keys, const int* __restrict__ slots, uint32_t NB, uint32_t cap,
	const float* __restrict__ tsdf, const float* __restrict__ wsum, uint32_t r, int& bx, int& by, int& bz) {
	key_coords(keys[r], bx, by, bz);
	if (threadIdx.x < 27) {
		const int d = threadIdx.x, nx = bx + d % 3 - 1, ny = by + (d / 3) % 3 - 1, nz = bz + d / 9 - 1;
		int slot = -1, rank = -1;
		if (nx >= -COORD_LIMIT && nx < COORD_LIMIT && ny >= -COORD_LIMIT && ny < COORD_LIMIT && nz >= -COORD_LIMIT && nz < COORD_LIMIT) {
			const uint64_t k = block_key(nx, ny, nz);
			const uint32_t q = lower_bound_key(keys, NB, k);
			if (q < NB && keys[q] == k) {
				const int s = slots[q];
				if (s >= 0 && (uint32_t)s < cap) { slot = s; rank = (int)q; }
			}
		}
		S.slot[d] = slot; S.rank[d] = rank;
	}
	__syncthreads();
	for (int e = threadIdx.x; e < SNP; e += EXTRACT_THREADS) {
		const int x = e % SN - 1, y = (e / SN) % SN - 1, z = e / (SN * SN) - 1;
		const int s = S.slot[((z < 0 ? 0 : (z >= SB ? 2 : 1)) * 3 + (y < 0 ? 0 : (y >= SB ? 2 : 1))) * 3 + (x < 0 ? 0 : (x >= SB ? 2 : 1))];
		const size_t at = (size_t)(s < 0 ? 0 : s) * SBP + (size_t)((((z & (SB - 1)) * SB) + (y & (SB - 1))) * SB + (x & (SB - 1)));
		S.t[e] = s < 0 ? 1.f : tsdf[at];
		S.w[e] = s < 0 ? 0.f : wsum[at];
	}
	__syncthreads();
}

__device__ __forceinline__ Lattice stage_lattice() {
	Lattice L; L.nx = L.ny = L.nz = SN; L.n = SNP; L.vs = 1.0; L.o[0] = L.o[1] = L.o[2] = 0.0;
	return L;
}

// the block index (0, 1, 2) -> (-1, 0, +1) of a staged coordinate -1 .. 8
__device__ __forceinline__ int side(int c) { return c < 0 ? 0 : (c >= SB ? 2 : 1); }

// EMIT false: the three counts of the block of rank blockIdx.x.  EMIT true: its vertices and, when it has any, its owner words.
template <bool EMIT>
__global__ void __launch_bounds__(EXTRACT_THREADS) sparse_points_kernel(Lattice G, const uint64_t* __restrict__ keys, const int* __restrict__ slots, uint32_t NB,
	uint32_t cap, const float* __restrict__ tsdf, const float* __restrict__ wsum, const float* __restrict__ color, float min_weight, uint32_t* __restrict__ cv,
	uint32_t* __restrict__ cf, uint32_t* __restrict__ ce, uint32_t* __restrict__ owners, unsigned n_owner_blocks, size_t n_vertices,
	float* __restrict__ vertices, float* __restrict__ colors) {
	__shared__ BlockStage S;
	const uint32_t r = blockIdx.x;
	int bx, by, bz;
	stage_block(S, keys, slots, NB, cap, tsdf, wsum, r, bx, by, bz);
	const int lx = threadIdx.x & (SB - 1), ly = (threadIdx.x >> 3) & (SB - 1), lz = threadIdx.x >> 6;
	const unsigned at = (unsigned)(((lz + 1) * SN + ly + 1) * SN + lx + 1);
	const PointClass pc = classify(stage_lattice(), S.t, S.w, min_weight, at, lx + 1, ly + 1, lz + 1);
	uint32_t nv_block, nf_block;
	const uint32_t local = block_exclusive<EXTRACT_THREADS>((uint32_t)__popc(pc.vmask), S.wave, nv_block);
	if (!EMIT) {
		block_exclusive<EXTRACT_THREADS>(pc.cell ? cell_faces(pc.in8) : 0u, S.wave, nf_block);
		if (threadIdx.x == 0) { cv[r] = nv_block; cf[r] = nf_block; ce[r] = nv_block ? 1u : 0u; }
		return;
	}
	if (nv_block == 0) return;                                  // workgroup-uniform
	// cv, ce: scanned.  ce[r] < n_owner_blocks for a block with vertices
	owners[(size_t)min(ce[r], n_owner_blocks - 1u) * SBP + threadIdx.x] = (local << 8) | pc.vmask;
	if (!pc.vmask) return;
	const int i = SB * bx + lx, j = SB * by + ly, k = SB * bz + lz;
	const int own = S.slot[13];                                 // this block: allocated, or it would own no vertex
	const double Tp = (double)S.t[at];
	size_t id = (size_t)cv[r] + local;
#pragma unroll
	for (int s = 0; s < 7; s++) {
		if (!((pc.vmask >> s) & 1u) || id >= n_vertices) continue;      // id < n_vertices for the volume that was counted
		const int ob = BITS_OF_SLOT[s], dx = ob & 1, dy = (ob >> 1) & 1, dz = ob >> 2;
		const double Tq = (double)S.t[at + dx + dy * SN + dz * SN * SN], t = Tp / (Tp - Tq);      // the signs differ: Tp != Tq
		vertices[3 * id + 0] = (float)(G.o[0] + G.vs * ((double)i + t * (double)dx));
		vertices[3 * id + 1] = (float)(G.o[1] + G.vs * ((double)j + t * (double)dy));
		vertices[3 * id + 2] = (float)(G.o[2] + G.vs * ((double)k + t * (double)dz));
		if (colors) {
			// the other end lies in a valid cell, hence in an allocated block
			const int qx = lx + dx, qy = ly + dy, qz = lz + dz, qs = S.slot[(side(qz) * 3 + side(qy)) * 3 + side(qx)];
			const size_t ql = (size_t)((((qz & (SB - 1)) * SB) + (qy & (SB - 1))) * SB + (qx & (SB - 1)));
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const double Cp = own < 0 ? 0.0 : (double)color[(size_t)own * (3 * SBP) + (size_t)c * SBP + threadIdx.x];
				const double Cq = qs < 0 ? 0.0 : (double)color[(size_t)qs * (3 * SBP) + (size_t)c * SBP + ql];
				colors[3 * id + c] = (float)(Cp + t * (Cq - Cp));
			}
		}
		id++;
	}
}

__global__ void __launch_bounds__(EXTRACT_THREADS) sparse_faces_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ slots, uint32_t NB, uint32_t cap,
	const float* __restrict__ tsdf, const float* __restrict__ wsum, float min_weight, const uint32_t* __restrict__ cv, const uint32_t* __restrict__ cf,
	const uint32_t* __restrict__ ce, const uint32_t* __restrict__ owners, unsigned n_owner_blocks, size_t n_faces, int* __restrict__ faces) {
	__shared__ BlockStage S;
	const uint32_t r = blockIdx.x;
	int bx, by, bz;
	stage_block(S, keys, slots, NB, cap, tsdf, wsum, r, bx, by, bz);
	const int lx = threadIdx.x & (SB - 1), ly = (threadIdx.x >> 3) & (SB - 1), lz = threadIdx.x >> 6;
	const unsigned at = (unsigned)(((lz + 1) * SN + ly + 1) * SN + lx + 1);
	const PointClass pc = classify(stage_lattice(), S.t, S.w, min_weight, at, lx + 1, ly + 1, lz + 1);
	uint32_t nf_block;
	const uint32_t local = block_exclusive<EXTRACT_THREADS>(pc.cell ? cell_faces(pc.in8) : 0u, S.wave, nf_block);
	if (!pc.cell) return;
	// the vertex on the edge between corners lo < hi (corner bits, lo a subset of hi) of this cell: it exists, so its owner's block is allocated
	// and has an owner word
	auto vid = [&](int lo, int hi) -> int {
		const int ox = lx + (lo & 1), oy = ly + ((lo >> 1) & 1), oz = lz + (lo >> 2);
		const int orank = S.rank[(side(oz) * 3 + side(oy)) * 3 + side(ox)];
		if (orank < 0) return 0;
		const uint32_t ol = (uint32_t)((((oz & (SB - 1)) * SB) + (oy & (SB - 1))) * SB + (ox & (SB - 1)));
		const uint32_t word = owners[(size_t)min(ce[orank], n_owner_blocks - 1u) * SBP + ol];
		return (int)(cv[orank] + (word >> 8) + (uint32_t)__popc(word & ((1u << ((SLOT_OF_BITS >> (4 * (hi ^ lo))) & 15u)) - 1u)));
	};
	cell_emit_faces(pc.in8, vid, (size_t)cf[r] + local, n_faces, faces);
}

// ---- host ----

// 0: fine; -1: refused.  with_pool: num_blocks <= capacity is required
int check_volume(const std::string& name, const adgs_sparse_tsdf_volume* vol, bool with_pool, Lattice& L) {
	if (vol->struct_bytes < (int)sizeof(adgs_sparse_tsdf_volume)) { set_error(name + ": struct_bytes is smaller than adgs_sparse_tsdf_volume"); return -1; }
	if (vol->num_blocks < 0 || vol->capacity < 0 || vol->table_capacity < 0) { set_error(name + ": negative num_blocks, capacity or table_capacity"); return -1; }
	if (vol->num_blocks > MAX_BLOCKS || vol->capacity > MAX_BLOCKS || vol->table_capacity > MAX_BLOCKS) {
		set_error(name + ": num_blocks, capacity and table_capacity must be at most 2^22"); return -1;
	}
	if (with_pool && vol->num_blocks > vol->capacity) { set_error(name + ": num_blocks exceeds the capacity of the pool"); return -1; }
	if (!positive(vol->voxel_size)) { set_error(name + ": voxel_size must be finite and > 0"); return -1; }
	for (int a = 0; a < 3; a++)
		if (!std::isfinite(vol->origin[a])) { set_error(name + ": the origin must be finite"); return -1; }
	L.nx = L.ny = L.nz = 0; L.n = 0;
	L.vs = (double)vol->voxel_size;
	for (int a = 0; a < 3; a++) L.o[a] = (double)vol->origin[a];
	return 0;
}

// the shared check of a view (check_view, tsdf_shared.h), then trunc / voxel_size above the limit; steps: n
int check_view_steps(const std::string& name, const adgs_tsdf_view* view, const Lattice& L, TsdfView& v, int& steps) {
	if (check_view(name, view, v) < 0) return -1;
	const double n = std::ceil((double)view->trunc / L.vs);
	if (!(n <= (double)ADGS_SPARSE_TSDF_MAX_STEPS)) { set_error(name + ": trunc / voxel_size exceeds ADGS_SPARSE_TSDF_MAX_STEPS"); return -1; }
	steps = n < 1.0 ? 1 : (int)n;
	return 0;
}

unsigned blocks_for(size_t n, int threads) { return (unsigned)((n + (size_t)threads - 1) / (size_t)threads); }

// the scratch of an allocating call
struct AllocTemp {
	uint32_t* wave_base; uint64_t *cand, *sorted; uint32_t *flags, *pos;        // flags and pos double as the sort's value arrays
	unsigned long long* aux; AllocState* state; char *scan, *sort; size_t bytes;
};
size_t alloc_waves(long long pixels) { return (size_t)blocks_for((size_t)pixels, ALLOC_THREADS) * (ALLOC_THREADS / WAVE); }
AllocTemp carve_alloc(char* base, long long pixels, long long cand_cap) {
	Carver c(base);
	AllocTemp t;
	const size_t nw = alloc_waves(pixels), cc = (size_t)cand_cap;
	t.wave_base = c.take<uint32_t>(nw);
	t.cand = c.take<uint64_t>(cc); t.sorted = c.take<uint64_t>(cc);
	t.flags = c.take<uint32_t>(cc); t.pos = c.take<uint32_t>(cc);
	t.aux = c.take<unsigned long long>(2 * SCAN_AUX_SLOTS);
	t.state = c.take<AllocState>(1);
	t.scan = c.take<char>(scan_temp_bytes(nw > cc ? nw : cc));
	t.sort = c.take<char>(sort_temp_bytes(cc));
	t.bytes = c.size();
	return t;
}

// sort, flag, scan, merge and the one read-back; the candidates and state->counts[1], n_sort are in place.  -> 0, 1 (no room) or -1
int allocate_tail(const std::string& name, const AllocTemp& t, uint32_t cand_cap, const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots,
	uint64_t* keys_out, int* slots_out, int* block_coords, long long* counts, hipStream_t stream) {
	const uint32_t NB = (uint32_t)vol->num_blocks, room = (uint32_t)vol->table_capacity;
	if (radix_sort_pairs_u64_dn(t.cand, t.sorted, t.flags, t.pos, cand_cap, &t.state->n_sort, 64, t.sort, stream) != 0) return -1;
	ADGS_LAUNCH(sparse_head_flags_kernel, dim3(blocks_for(cand_cap, ALLOC_THREADS)), dim3(ALLOC_THREADS), 0, stream, (const uint64_t*)t.sorted, cand_cap, keys, NB,
		(const AllocState*)t.state, t.flags);
	if (exclusive_scan_u32_sum(t.flags, t.pos, cand_cap, t.scan, t.flags, t.aux + SCAN_AUX_SLOTS, stream) != 0) return -1;
	ADGS_LAUNCH(sparse_new_total_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)(t.aux + SCAN_AUX_SLOTS), cand_cap, NB, room, t.state);
	const size_t n = NB > cand_cap ? NB : cand_cap;
	ADGS_LAUNCH(sparse_merge_kernel, dim3(blocks_for(n, ALLOC_THREADS)), dim3(ALLOC_THREADS), 0, stream, (const uint64_t*)t.sorted, (const uint32_t*)t.flags,
		(const uint32_t*)t.pos, keys, slots, NB, room, (const AllocState*)t.state, keys_out, slots_out, block_coords);
	unsigned long long host[4];
	ADGS_HIP_CHECK(hipMemcpyAsync(host, t.state->counts, sizeof(host), hipMemcpyDeviceToHost, stream));
	ADGS_HIP_CHECK(hipStreamSynchronize(stream));
	for (int i = 0; i < 4; i++) counts[i] = (long long)host[i];
	return host[3] ? 1 : 0;
}

// NULL tables are fine for an empty volume only
bool table_missing(const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots) { return vol->num_blocks > 0 && (!keys || !slots); }

// the scratch of the extraction: ExtractTemp of tsdf_shared.h, one row per block

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_sparse_tsdf_allocate_temp_bytes(long long pixels, long long max_candidates) {
	if (pixels < 0 || pixels > (long long)INT_MAX || max_candidates < 0 || max_candidates > (long long)INT_MAX) return 0;
	return carve_alloc(nullptr, pixels, max_candidates).bytes;
}

extern "C" int adgs_sparse_tsdf_allocate_view(const adgs_sparse_tsdf_volume* vol, const adgs_tsdf_view* view, float margin, const float* depth,
	const float* opacity, const float* weight, const uint64_t* keys, const int* slots, uint64_t* keys_out, int* slots_out, int* block_coords,
	long long max_candidates, void* temp, long long* counts, void* stream_) {
	const std::string name("adgs_sparse_tsdf_allocate_view");
	if (!vol || !view || !depth || !opacity || !keys_out || !slots_out || !block_coords || !temp || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	if (check_volume(name, vol, false, L) < 0) return -1;
	if (table_missing(vol, keys, slots)) { set_error(name + ": NULL pointer"); return -1; }
	TsdfView tv;
	int steps;
	if (check_view_steps(name, view, L, tv, steps) < 0) return -1;
	if (!(margin >= 0.f && margin <= 4.f)) { set_error(name + ": margin must lie in [0, 4]"); return -1; }
	if (max_candidates < 1 || max_candidates > (long long)INT_MAX) { set_error(name + ": max_candidates must lie in [1, 2^31 - 1]"); return -1; }
	counts[0] = counts[1] = counts[2] = counts[3] = 0;
	if (view->H == 0 || view->W == 0) return 0;
	AllocView v;
	v.H = tv.H; v.W = tv.W; v.inv_depth = tv.inv_depth; v.steps = steps;
	v.kx = tv.kx; v.ky = tv.ky; v.cx = tv.cx; v.cy = tv.cy;
	for (int i = 0; i < 9; i++) v.R[i] = tv.R[i];
	for (int i = 0; i < 3; i++) { v.t[i] = tv.t[i]; v.o[i] = L.o[i]; }
	v.near = tv.near; v.max_depth = tv.max_depth; v.trunc = tv.trunc; v.dz = 2.0 * tv.trunc / (double)steps;
	v.vs = L.vs; v.rho = (double)margin; v.min_opacity = tv.min_opacity;
	hipStream_t stream = (hipStream_t)stream_;
	const long long pixels = (long long)view->H * view->W;
	const uint32_t cand_cap = (uint32_t)max_candidates, NB = (uint32_t)vol->num_blocks;
	const AllocTemp t = carve_alloc((char*)temp, pixels, max_candidates);
	const size_t nw = alloc_waves(pixels);
	const unsigned grid = blocks_for((size_t)pixels, ALLOC_THREADS);
	ADGS_HIP_CHECK(hipMemsetAsync(t.aux, 0, 2 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
	ADGS_HIP_CHECK(hipMemsetAsync(t.state, 0, sizeof(AllocState), stream));
	ADGS_LAUNCH(sparse_candidates_kernel<false>, dim3(grid), dim3(ALLOC_THREADS), 0, stream, v, depth, opacity, weight, keys, NB, t.wave_base, t.cand, cand_cap,
		t.state);
	if (exclusive_scan_u32_sum(t.wave_base, t.wave_base, nw, t.scan, t.wave_base, t.aux, stream) != 0) return -1;
	ADGS_LAUNCH(sparse_candidate_total_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)t.aux, cand_cap, t.state);
	ADGS_LAUNCH(sparse_candidates_kernel<true>, dim3(grid), dim3(ALLOC_THREADS), 0, stream, v, depth, opacity, weight, keys, NB, t.wave_base, t.cand, cand_cap,
		t.state);
	return allocate_tail(name, t, cand_cap, vol, keys, slots, keys_out, slots_out, block_coords, counts, stream);
}

extern "C" int adgs_sparse_tsdf_allocate_blocks(const adgs_sparse_tsdf_volume* vol, const int* coords, long long M, const uint64_t* keys, const int* slots,
	uint64_t* keys_out, int* slots_out, int* block_coords, void* temp, long long* counts, void* stream_) {
	const std::string name("adgs_sparse_tsdf_allocate_blocks");
	if (!vol || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	if (check_volume(name, vol, false, L) < 0) return -1;
	if (M < 0 || M > (long long)INT_MAX) { set_error(name + ": M must lie in [0, 2^31 - 1]"); return -1; }
	counts[0] = counts[1] = counts[2] = counts[3] = 0;
	if (M == 0) return 0;
	if (!coords || !keys_out || !slots_out || !block_coords || !temp || table_missing(vol, keys, slots)) { set_error(name + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const AllocTemp t = carve_alloc((char*)temp, 0, M);
	ADGS_HIP_CHECK(hipMemsetAsync(t.aux, 0, 2 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
	ADGS_HIP_CHECK(hipMemsetAsync(t.state, 0, sizeof(AllocState), stream));
	ADGS_LAUNCH(sparse_coord_keys_kernel, dim3(blocks_for((size_t)M, ALLOC_THREADS)), dim3(ALLOC_THREADS), 0, stream, coords, (uint32_t)M, t.cand, t.state);
	return allocate_tail(name, t, (uint32_t)M, vol, keys, slots, keys_out, slots_out, block_coords, counts, stream);
}

extern "C" int adgs_sparse_tsdf_integrate(const adgs_sparse_tsdf_volume* vol, const adgs_tsdf_view* view, const float* depth, const float* opacity,
	const float* image, const float* weight, const int* block_coords, float* tsdf, float* wsum, float* color, void* stream_) {
	const std::string name("adgs_sparse_tsdf_integrate");
	if (!vol || !view || !depth || !opacity) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	if (check_volume(name, vol, true, L) < 0) return -1;
	TsdfView v;
	int steps;
	if (check_view_steps(name, view, L, v, steps) < 0) return -1;
	if ((image != nullptr) != (color != nullptr)) { set_error(name + ": image and color must be given together"); return -1; }
	if (vol->num_blocks == 0 || view->H == 0 || view->W == 0) return 0;
	if (!block_coords || !tsdf || !wsum) { set_error(name + ": NULL pointer"); return -1; }
	BlockCull cull;
	// the points of a block lie within 3.5 sqrt(3) voxels of its centre; the slack covers the rounding of the centre's projection many times over
	cull.radius = L.vs * 0.5 * (double)(SB - 1) * std::sqrt(3.0) * (1.0 + 1e-6);
	cull.left_b = v.cx + 1.5; cull.right_b = (double)v.W + 0.5 - v.cx; cull.top_b = v.cy + 1.5; cull.bottom_b = (double)v.H + 0.5 - v.cy;
	const double slack = 1.0 + 1e-6;
	cull.left_r = cull.radius * std::sqrt(v.kx * v.kx + cull.left_b * cull.left_b) * slack;
	cull.right_r = cull.radius * std::sqrt(v.kx * v.kx + cull.right_b * cull.right_b) * slack;
	cull.top_r = cull.radius * std::sqrt(v.ky * v.ky + cull.top_b * cull.top_b) * slack;
	cull.bottom_r = cull.radius * std::sqrt(v.ky * v.ky + cull.bottom_b * cull.bottom_b) * slack;
	ADGS_LAUNCH(sparse_integrate_kernel, dim3((unsigned)vol->num_blocks), dim3(INTEGRATE_THREADS), 0, (hipStream_t)stream_, L, v, cull, depth, opacity, image,
		weight, block_coords, tsdf, wsum, color);
	return 0;
}

extern "C" size_t adgs_sparse_tsdf_extract_temp_bytes(long long num_blocks) {
	if (num_blocks < 0 || num_blocks > (long long)MAX_BLOCKS) return 0;
	return carve_extract(nullptr, (size_t)num_blocks).bytes;
}

extern "C" size_t adgs_sparse_tsdf_extract_owner_bytes(long long owner_blocks) {
	return owner_blocks > 0 ? (size_t)owner_blocks * ADGS_SPARSE_TSDF_OWNER_BYTES_PER_BLOCK : 0;
}

extern "C" int adgs_sparse_tsdf_extract_count(const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots, const float* tsdf, const float* wsum,
	float min_weight, void* temp, long long* counts, void* stream_) {
	const std::string name("adgs_sparse_tsdf_extract_count");
	if (!vol || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	if (check_volume(name, vol, true, L) < 0) return -1;
	if (!(min_weight > 0.f)) { set_error(name + ": min_weight must be > 0"); return -1; }
	counts[0] = counts[1] = counts[2] = 0;
	if (vol->num_blocks == 0) return 0;
	if (!keys || !slots || !tsdf || !wsum || !temp) { set_error(name + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const uint32_t NB = (uint32_t)vol->num_blocks;
	const ExtractTemp t = carve_extract((char*)temp, NB);
	ADGS_LAUNCH(sparse_points_kernel<false>, dim3(NB), dim3(EXTRACT_THREADS), 0, stream, L, keys, slots, NB, (uint32_t)vol->capacity, tsdf, wsum,
		(const float*)nullptr, min_weight, t.cv, t.cf, t.ce, (uint32_t*)nullptr, 0u, (size_t)0, (float*)nullptr, (float*)nullptr);
	return extract_count_tail(name, t, NB, stream, counts);
}

extern "C" int adgs_sparse_tsdf_extract_emit(const adgs_sparse_tsdf_volume* vol, const uint64_t* keys, const int* slots, const float* tsdf, const float* wsum,
	const float* color, float min_weight, const void* temp, void* owners, const long long* counts, float* vertices, int* faces, float* colors,
	void* stream_) {
	const std::string name("adgs_sparse_tsdf_extract_emit");
	if (!vol || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	if (check_volume(name, vol, true, L) < 0) return -1;
	if (!(min_weight > 0.f)) { set_error(name + ": min_weight must be > 0"); return -1; }
	const long long V = counts[0], F = counts[1], E = counts[2], NB = vol->num_blocks;
	// a point owns at most 7 vertices, a cell has at most 12 faces
	if (check_emit(name, "adgs_sparse_tsdf_extract_count", counts, 7 * SBP * NB, 12 * SBP * NB, NB, vertices, faces, owners, color, colors) < 0) return -1;
	if (V == 0 || E == 0) return 0;                              // no vertex, hence no face
	if (!keys || !slots || !tsdf || !wsum || !temp) { set_error(name + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const ExtractTemp t = carve_extract((char*)temp, (size_t)NB);
	ADGS_LAUNCH(sparse_points_kernel<true>, dim3((unsigned)NB), dim3(EXTRACT_THREADS), 0, stream, L, keys, slots, (uint32_t)NB, (uint32_t)vol->capacity, tsdf,
		wsum, color, min_weight, t.cv, t.cf, t.ce, (uint32_t*)owners, (unsigned)E, (size_t)V, vertices, colors);
	if (F > 0) ADGS_LAUNCH(sparse_faces_kernel, dim3((unsigned)NB), dim3(EXTRACT_THREADS), 0, stream, keys, slots, (uint32_t)NB, (uint32_t)vol->capacity, tsdf, wsum,
		min_weight, (const uint32_t*)t.cv, (const uint32_t*)t.cf, (const uint32_t*)t.ce, (const uint32_t*)owners, (unsigned)E, (size_t)F, faces);
	return 0;
}
