// Slot-row reductions: how a scalar loss or statistic is summed over a grid without a fill per call and without atomics on one address.
// The ABI-level description (who zeroes what, what the backward may read) is in include/adgs_loss.h; this header is the device side.
//
// Every thread accumulates in double.  wave_sum forms the wave's sums (__shfl_xor butterfly); one lane adds them with atomicAdd into a
// SLOT ROW of a zero-initialised work buffer: SLOTS rows of ROW doubles, row (block * 4 + wave) % SLOTS from a wave (slot_add_wave), row
// block % SLOTS from a whole workgroup (slot_add_block).  A finish kernel of ONE workgroup of SLOT_THREADS threads calls slot_finish:
// thread t reads row t and stores 0.0 over it ("consumed": the rows are zero again for the next call on the buffer), the rows are summed
// by wave and then through LDS in wave order, and thread 0 holds the totals.  What the finish kernel does with them -- store them behind
// the rows for the backward, form the loss -- is its own epilogue.
// The order of the additions is fixed (offsets 32, 16, ..., 1; waves 0, 1, 2, 3), so a term whose rows receive one add each (no more
// workgroups than its rows can take) is deterministic to the bit.
#pragma once
#include "common.h"
#include <algorithm>

namespace adgs {

constexpr int SLOT_THREADS = 256;         // workgroup size of the kernels that call slot_add_wave and of every finish kernel

// workgroups of a one-dimensional sum kernel over n elements; beyond 2048 of them a thread strides over the elements
inline unsigned reduce_blocks(long long n) { return (unsigned)std::min<long long>((n + SLOT_THREADS - 1) / SLOT_THREADS, 2048); }

// every lane receives the sum over its wave
__device__ __forceinline__ void wave_sum(double& v) {
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
}
template <int K> __device__ __forceinline__ void wave_sum(double (&v)[K]) {
#pragma unroll
	for (int q = 0; q < K; q++) wave_sum(v[q]);
}

// Each wave of a SLOT_THREADS workgroup (one-dimensional grid) adds its K sums to columns first .. first + K - 1 of its slot row.
template <int SLOTS, int ROW, int K> __device__ __forceinline__ void slot_add_wave(double* __restrict__ work, double (&v)[K], int first = 0) {
#pragma unroll
	for (int q = 0; q < K; q++) {
		wave_sum(v[q]);
		if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(work + (size_t)((blockIdx.x * (SLOT_THREADS / WAVE) + threadIdx.x / WAVE) % SLOTS) * ROW + first + q, v[q]);
	}
}

// A workgroup of LT threads (any grid) adds its K sums to its slot row with one atomic per sum: thread q adds the waves' sums in wave
// order.  A total of exactly 0.0 is skipped: a row starts at +0.0 and can never become -0.0 (x + -x and +0.0 + -0.0 are +0.0), and
// adding +0.0 or -0.0 to such a row leaves every bit of it as it was.  Every thread of the workgroup must call this (it has a barrier).
template <int SLOTS, int ROW, int LT, int K> __device__ __forceinline__ void slot_add_block(double* __restrict__ work, double (&v)[K]) {
	__shared__ double red[K][LT / WAVE];
	const int tid = threadIdx.x;
	wave_sum(v);
	if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
		for (int q = 0; q < K; q++) red[q][tid / WAVE] = v[q];
	}
	__syncthreads();
	if (tid < K) {
		double t = 0.0;
		for (int w = 0; w < LT / WAVE; w++) t += red[tid][w];
		const unsigned b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		if (t != 0.0) atomicAdd(work + (size_t)(b % SLOTS) * ROW + tid, t);
	}
}

// The finish kernel's read (one workgroup of SLOT_THREADS threads): columns first .. first + K - 1 of every slot row are summed into
// tot, valid in thread 0 only, and left zero.
template <int SLOTS, int ROW, int K> __device__ __forceinline__ void slot_finish(double* __restrict__ work, double (&tot)[K], int first = 0) {
	static_assert(SLOTS == SLOT_THREADS, "one finish thread per slot row");
	__shared__ double s[K][SLOT_THREADS / WAVE];
	double* row = work + (size_t)threadIdx.x * ROW + first;
#pragma unroll
	for (int q = 0; q < K; q++) {
		tot[q] = row[q];
		row[q] = 0.0;
		wave_sum(tot[q]);
		if ((threadIdx.x & (WAVE - 1)) == 0) s[q][threadIdx.x / WAVE] = tot[q];
	}
	__syncthreads();
	if (threadIdx.x == 0) {
#pragma unroll
		for (int q = 0; q < K; q++) { tot[q] = 0.0; for (int w = 0; w < SLOT_THREADS / WAVE; w++) tot[q] += s[q][w]; }
	}
}

} // namespace adgs
