// The zero rows of a frame's dense gradient tensors, written beside the blend backward instead of behind it (api.hip: the v2 branch of
// raster_backward_impl; switch: ADGS_GRAD_PREFILL=0, read by the frame's FORWARD).
//
// With the forward's published mask (PreprocessBwdArgs::published) nine Gaussians in ten of a C3 frame receive no gradient: their rows of
// every gradient tensor are +0, and no such zero depends on the blend backward.  The Gaussians are taken in GROUPS of 256 consecutive ids
// (the preprocess backward's block).  A group whose published count is below PREFILL_SPARSE_NUM / PREFILL_SPARSE_DEN of its size is SPARSE:
//   - a fill workgroup stores +0 over the group's whole row range of every destination of the frame's FillPlan (full 16-byte stores) -- inside
//     the grid of the blend backward, which is VALU-bound and leaves the memory system idle, or in a launch of its own where there is no
//     blend backward to ride on;
//   - the preprocess backward and the SH-deformation row kernel, which run behind it, then store the rows of the published Gaussians only.
// Every other group is DENSE: nobody fills it, and the two kernels write every row of it as they always did.  The three of them apply
// prefill_group_sparse() to the same 256 bytes of a mask that is final before the first of them runs.
#pragma once
#include "common.h"
#include "stream_access.h"

namespace adgs {

constexpr int PREFILL_GROUP = 256;            // Gaussians per group: BW_THREADS of preprocess_bwd.hip
#ifndef ADGS_PREFILL_SPARSE_NUM
#define ADGS_PREFILL_SPARSE_NUM 1
#endif
#ifndef ADGS_PREFILL_SPARSE_DEN
#define ADGS_PREFILL_SPARSE_DEN 2
#endif
constexpr int PREFILL_SPARSE_NUM = ADGS_PREFILL_SPARSE_NUM, PREFILL_SPARSE_DEN = ADGS_PREFILL_SPARSE_DEN;
// the one group rule: `published` of the group's `valid` Gaussians (256 but for the frame's last group) have their mask byte set
__host__ __device__ __forceinline__ bool prefill_group_sparse(int published, int valid) { return published * PREFILL_SPARSE_DEN < valid * PREFILL_SPARSE_NUM; }

// where the fill workgroups sit in the blend backward's grid: in front of its last PREFILL_TILES_BEHIND tile workgroups (0: behind the last
// tile).  The tiles are dealt longest first, so the fill goes where the kernel's tail begins; in front of the long tiles (behind the first
// 4096 workgroups, the first refill of the chip's wave slots) it delays them by more than it saves (EXPERIMENTS.md: the placements measured).
#ifndef ADGS_PREFILL_TILES_BEHIND
#define ADGS_PREFILL_TILES_BEHIND 0u
#endif
constexpr uint32_t PREFILL_TILES_BEHIND = ADGS_PREFILL_TILES_BEHIND;
#ifdef ADGS_PREFILL_AFTER_BLOCKS            // experiment builds: behind this many tile workgroups instead
constexpr uint32_t PREFILL_AFTER_BLOCKS = ADGS_PREFILL_AFTER_BLOCKS;
#endif
__host__ inline uint32_t prefill_start(uint32_t tiles) {
#ifdef ADGS_PREFILL_AFTER_BLOCKS
	return tiles < PREFILL_AFTER_BLOCKS ? tiles : PREFILL_AFTER_BLOCKS;
#else
	return tiles > PREFILL_TILES_BEHIND ? tiles - PREFILL_TILES_BEHIND : 0u;
#endif
}

// One destination: the rows of Gaussians [first, first + count); Gaussian g's row is the `row` floats at p + (g - first) * stride
// (stride == row: the rows are one contiguous slab).  4-byte aligned, no more is asked.
struct FillEntry { float* p; int row, stride, first, count; };
constexpr int PREFILL_MAX_ENTRIES = 26;
struct FillPlan {
	const uint8_t* published;         // nullptr: no plan (every group dense)
	int P, n;                         // Gaussians of the frame, entries in use
	uint32_t start, groups;           // in-grid: workgroups [start, start + groups) of the launch are fill workgroups, one group each
	FillEntry e[PREFILL_MAX_ENTRIES];
};
inline void fill_plan_add(FillPlan& fp, float* p, int row, int stride, int first, int count) {
	if (!p || row <= 0 || count <= 0 || fp.n >= PREFILL_MAX_ENTRIES) return;
	fp.e[fp.n++] = FillEntry{ p, row, stride, first, count };
}

#if defined(__HIPCC__)
#ifndef ADGS_PREFILL_STREAM
#define ADGS_PREFILL_STREAM 1         // 1: the streaming (non-temporal) store policy of stream_access.h, 0: the default one
#endif
__device__ __forceinline__ void prefill_st(float* p) {
#if ADGS_PREFILL_STREAM
	st_stream(p, 0.f);
#else
	*p = 0.f;
#endif
}
__device__ __forceinline__ void prefill_st4(float4* p) {
#if ADGS_PREFILL_STREAM
	st_stream4(p, make_float4(0.f, 0.f, 0.f, 0.f));
#else
	*p = make_float4(0.f, 0.f, 0.f, 0.f);
#endif
}
// how many of the mask bytes [base, base + PREFILL_GROUP) (below P) are set: called by all `nthreads` threads of a workgroup of ONE wave
__device__ __forceinline__ int prefill_wave_count(const uint8_t* __restrict__ published, int base, int P, int lane) {
	int n = 0;
#pragma unroll
	for (int j = 0; j < PREFILL_GROUP / WAVE; j++) {
		const int i = base + j * WAVE + lane;
		const bool set = i < P && published[i] != 0;
		n += __popcll(__builtin_amdgcn_ballot_w64(set));
	}
	return n;
}
// The fill of one group by one wave (fp is read, never written: a store to a by-value kernel argument moves all of it into scratch memory).
__device__ __forceinline__ void prefill_group(const FillPlan& fp, const uint32_t group, const int lane) {
	const int base = (int)group * PREFILL_GROUP;
	if (base >= fp.P) return;
	const int end = min(base + PREFILL_GROUP, fp.P);
	if (!prefill_group_sparse(prefill_wave_count(fp.published, base, fp.P, lane), end - base)) return;
	for (int i = 0; i < fp.n; i++) {
		float* const p = fp.e[i].p;
		const int row = fp.e[i].row, stride = fp.e[i].stride, first = fp.e[i].first;
		const int lo = max(base, first), hi = min(end, first + fp.e[i].count);      // a group that straddles Ns has a range in the scene AND the object entry
		if (lo >= hi) continue;
		if (stride != row) {            // strided rows (channel 0 of [P, D_S]): one row per lane
			for (int g = lo + lane; g < hi; g += WAVE)
				for (int c = 0; c < row; c++) prefill_st(p + (size_t)(g - first) * stride + c);
			continue;
		}
		float* const d = p + (size_t)(lo - first) * row;
		const int n = (hi - lo) * row;                                              // <= 256 rows: fits an int for any row below 8 M floats
		const int head = min(n, (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2);      // dwords up to the first 16-byte boundary
		if (lane < head) prefill_st(d + lane);
		const int n4 = (n - head) >> 2;
		float4* const d4 = reinterpret_cast<float4*>(d + head);
		for (int q = lane; q < n4; q += WAVE) prefill_st4(d4 + q);                  // 1 KiB of consecutive bytes per wave and instruction
		const int tail0 = head + (n4 << 2);
		if (tail0 + lane < n) prefill_st(d + tail0 + lane);                         // at most three dwords
	}
}
#endif

} // namespace adgs
