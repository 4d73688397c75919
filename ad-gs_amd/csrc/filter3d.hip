// The 3D smoothing filter of Mip-Splatting for gfx950 (include/adgs_filter3d.h): the per-Gaussian maximal sampling rate over a set
// of cameras, the filter size from it, and the fused activation (with its analytic backward) that applies the filter to scales and
// opacity between the deformation pass and the rasterizer.
//
// accumulate: a thread holds FOUR consecutive Gaussians (48 contiguous bytes of positions: three 16-byte non-temporal loads -- the
// positions are touched once per launch, stream_access.h) and walks the camera table once for the four; the table index is the
// loop counter, so a camera record arrives through the scalar data cache (one 64-byte scalar load per camera and wave, no LDS, no
// chunking: any camera count is one loop).  Rows in front of / behind the 16-byte aligned middle of [row0, row0 + rows) -- at most
// three each -- are taken by single-Gaussian threads of the same launch.
// This file is built without FMA contraction (Makefile: EXACT): z and fx / z round once per operation in the order the header states,
// which is what makes a rate a pure function of (position, camera) and the maximum independent of how cameras are split over calls.
//
// apply: pure streaming, 16-byte accesses over the flattened [P*3] and [P] arrays -- a thread takes four Gaussians (three float4 of
// scales, one each of opacity and filter) -- with single-Gaussian threads for the last P % 4 rows, and for every row when a
// pointer is not 16-byte aligned.  The outputs feed the next kernel (preprocess, or the deformation backward): ordinary stores;
// the upstream gradients are read once: non-temporal loads.
#include "common.h"
#include "stream_access.h"
#include "../../include/adgs_filter3d.h"
#include <algorithm>
#include <initializer_list>

namespace adgs {
namespace {

constexpr int F3_BLOCK = 256;
constexpr int CAM = ADGS_FILTER3D_CAMERA_FLOATS;
constexpr float F3_SQRT02 = 0.44721359549995793f;      // sqrt(0.2): the filter's variance is 0.2 pixels^2 at the sampling rate

// rows [row0, row0 + head) and [row0 + head + 4 groups, ... + tail) one per thread, `groups` aligned groups of four in between
struct F3Range { int row0, head, groups, tail; };

struct alignas(16) F3Camera { float c[CAM]; };      // R | t, fx, fy, W, H

__device__ __forceinline__ float f3_rate(const float* c, float px, float py, float pz) {
	const float x = ((c[0] * px + c[1] * py) + c[2] * pz) + c[9];
	const float y = ((c[3] * px + c[4] * py) + c[5] * pz) + c[10];
	const float z = ((c[6] * px + c[7] * py) + c[8] * pz) + c[11];
	const float fx = c[12], fy = c[13], wx = 0.65f * c[14], wy = 0.65f * c[15];
	// every comparison is false for a NaN: such a position is seen by nobody
	const bool seen = (z > 0.2f) & (fabsf(x * fx) <= wx * z) & (fabsf(y * fy) <= wy * z);
	return seen ? fx / z : 0.f;
}

__global__ void __launch_bounds__(F3_BLOCK) f3_accumulate_kernel(const float* __restrict__ xyz, F3Range r, const F3Camera* __restrict__ cams, int ncams,
	float* __restrict__ rate, int init) {
	const int tid = blockIdx.x * F3_BLOCK + threadIdx.x;
	float p[12], best[4] = {0.f, 0.f, 0.f, 0.f};
	size_t row;
	const bool group = tid < r.groups;
	if (group) {
		row = (size_t)r.row0 + r.head + 4 * (size_t)tid;
		const float4* src = reinterpret_cast<const float4*>(xyz + 3 * row);
		const float4 a = ld_stream4(src), b = ld_stream4(src + 1), c = ld_stream4(src + 2);
		p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w; p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
		if (!init) { const float4 o = *reinterpret_cast<const float4*>(rate + row); best[0] = o.x; best[1] = o.y; best[2] = o.z; best[3] = o.w; }
	} else {
		const int k = tid - r.groups;
		if (k >= r.head + r.tail) return;
		row = (size_t)r.row0 + (k < r.head ? k : r.head + 4 * (size_t)r.groups + (k - r.head));
#pragma unroll
		for (int j = 0; j < 12; j++) p[j] = j < 3 ? ld_stream(xyz + 3 * row + j) : 0.f;
		if (!init) best[0] = rate[row];
	}
	for (int n = 0; n < ncams; n++) {
		const F3Camera cam = cams[n];      // wave-uniform address: one 64-byte scalar load
		const float* c = cam.c;
#pragma unroll
		for (int j = 0; j < 4; j++) best[j] = fmaxf(best[j], f3_rate(c, p[3 * j], p[3 * j + 1], p[3 * j + 2]));      // a NaN `old` loses to any rate
	}
	if (group) *reinterpret_cast<float4*>(rate + row) = make_float4(best[0], best[1], best[2], best[3]);
	else rate[row] = best[0];
}

// Positive floats order like their bit patterns: the minimum positive rate is the maximum of ~bits, and 0 says "none" -- one word,
// one unsigned maximum, whatever the order of the workgroups.
__global__ void __launch_bounds__(F3_BLOCK) f3_min_rate_kernel(const float* __restrict__ rate, int P, uint32_t* __restrict__ work) {
	uint32_t key = 0u;
	for (size_t i = (size_t)blockIdx.x * F3_BLOCK + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * F3_BLOCK) {
		const float v = rate[i];
		if (v > 0.f) key = max(key, ~__float_as_uint(v));
	}
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, off, WAVE));
	if ((threadIdx.x & (WAVE - 1)) == 0 && key != 0u) atomicMax(work, key);
}

// rate and out may be the same buffer: an element is read and written by one thread
__global__ void __launch_bounds__(F3_BLOCK) f3_filter_kernel(const float* rate, int P, float* out, const uint32_t* __restrict__ work) {
	const size_t i = (size_t)blockIdx.x * F3_BLOCK + threadIdx.x;
	if (i >= (size_t)P) return;
	const uint32_t key = work[0];
	const float unseen = key != 0u ? F3_SQRT02 / __uint_as_float(~key) : 0.f;
	const float v = rate[i];
	out[i] = v > 0.f ? F3_SQRT02 / v : unseen;
}

struct F3Row { float S[3], O, coef, d[3], f2; };
__device__ __forceinline__ F3Row f3_row(const float* s, float o, float f) {
	F3Row r;
	r.f2 = f * f;
	float ratio[3];
#pragma unroll
	for (int i = 0; i < 3; i++) {
		const float q = s[i] * s[i];
		r.d[i] = q + r.f2;
		r.S[i] = sqrtf(r.d[i]);
		ratio[i] = q / r.d[i];      // <= 1; exactly 1 for f = 0.  Three ratios, not a ratio of two products: prod s_i^2 reaches 1e-36
	}
	r.coef = sqrtf((ratio[0] * ratio[1]) * ratio[2]);
	r.O = o * r.coef;
	return r;
}
__device__ __forceinline__ void f3_row_bwd(const float* s, float o, float f, const float* gS, float gO, float* gs, float& go) {
	const F3Row r = f3_row(s, o, f);
	const float t = gO * r.O;
#pragma unroll
	for (int i = 0; i < 3; i++) gs[i] = gS[i] * (s[i] / r.S[i]) + t * (r.f2 / (s[i] * r.d[i]));
	go = gO * r.coef;
}

__device__ __forceinline__ void f3_unpack12(const float4* p, float* v, bool stream) {
	const float4 a = stream ? ld_stream4(p) : p[0], b = stream ? ld_stream4(p + 1) : p[1], c = stream ? ld_stream4(p + 2) : p[2];
	v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
}
__device__ __forceinline__ void f3_unpack4(const float4* p, float* v, bool stream) {
	const float4 a = stream ? ld_stream4(p) : p[0];
	v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void f3_pack12(float4* p, const float* v) {
	p[0] = make_float4(v[0], v[1], v[2], v[3]); p[1] = make_float4(v[4], v[5], v[6], v[7]); p[2] = make_float4(v[8], v[9], v[10], v[11]);
}

// threads [0, groups): Gaussians 4 t .. 4 t + 3 with 16-byte accesses; threads [groups, groups + P - 4 groups): one Gaussian each
__global__ void __launch_bounds__(F3_BLOCK) f3_apply_fwd_kernel(int P, int groups, const float* __restrict__ scales, const float* __restrict__ opacity,
	const float* __restrict__ filter, float* __restrict__ scales_out, float* __restrict__ opacity_out) {
	const int tid = blockIdx.x * F3_BLOCK + threadIdx.x;
	if (tid < groups) {
		float s[12], o[4], f[4], S[12], O[4];
		f3_unpack12(reinterpret_cast<const float4*>(scales) + 3 * (size_t)tid, s, false);
		f3_unpack4(reinterpret_cast<const float4*>(opacity) + tid, o, false);
		f3_unpack4(reinterpret_cast<const float4*>(filter) + tid, f, false);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const F3Row r = f3_row(s + 3 * j, o[j], f[j]);
			S[3 * j] = r.S[0]; S[3 * j + 1] = r.S[1]; S[3 * j + 2] = r.S[2]; O[j] = r.O;
		}
		f3_pack12(reinterpret_cast<float4*>(scales_out) + 3 * (size_t)tid, S);
		reinterpret_cast<float4*>(opacity_out)[tid] = make_float4(O[0], O[1], O[2], O[3]);
		return;
	}
	const size_t row = 4 * (size_t)groups + (size_t)(tid - groups);
	if (row >= (size_t)P) return;
	const float s[3] = {scales[3 * row], scales[3 * row + 1], scales[3 * row + 2]};
	const F3Row r = f3_row(s, opacity[row], filter[row]);
	scales_out[3 * row] = r.S[0]; scales_out[3 * row + 1] = r.S[1]; scales_out[3 * row + 2] = r.S[2];
	opacity_out[row] = r.O;
}

__global__ void __launch_bounds__(F3_BLOCK) f3_apply_bwd_kernel(int P, int groups, const float* __restrict__ scales, const float* __restrict__ opacity,
	const float* __restrict__ filter, const float* __restrict__ g_scales_out, const float* __restrict__ g_opacity_out, float* __restrict__ g_scales,
	float* __restrict__ g_opacity) {
	const int tid = blockIdx.x * F3_BLOCK + threadIdx.x;
	if (tid < groups) {
		float s[12], o[4], f[4], gS[12], gO[4], gs[12], go[4];
		f3_unpack12(reinterpret_cast<const float4*>(scales) + 3 * (size_t)tid, s, false);
		f3_unpack4(reinterpret_cast<const float4*>(opacity) + tid, o, false);
		f3_unpack4(reinterpret_cast<const float4*>(filter) + tid, f, false);
		f3_unpack12(reinterpret_cast<const float4*>(g_scales_out) + 3 * (size_t)tid, gS, true);
		f3_unpack4(reinterpret_cast<const float4*>(g_opacity_out) + tid, gO, true);
#pragma unroll
		for (int j = 0; j < 4; j++) f3_row_bwd(s + 3 * j, o[j], f[j], gS + 3 * j, gO[j], gs + 3 * j, go[j]);      // a row's values stay in its row
		f3_pack12(reinterpret_cast<float4*>(g_scales) + 3 * (size_t)tid, gs);
		reinterpret_cast<float4*>(g_opacity)[tid] = make_float4(go[0], go[1], go[2], go[3]);
		return;
	}
	const size_t row = 4 * (size_t)groups + (size_t)(tid - groups);
	if (row >= (size_t)P) return;
	const float s[3] = {scales[3 * row], scales[3 * row + 1], scales[3 * row + 2]};
	const float gS[3] = {ld_stream(g_scales_out + 3 * row), ld_stream(g_scales_out + 3 * row + 1), ld_stream(g_scales_out + 3 * row + 2)};
	float gs[3], go;
	f3_row_bwd(s, opacity[row], filter[row], gS, ld_stream(g_opacity_out + row), gs, go);
	g_scales[3 * row] = gs[0]; g_scales[3 * row + 1] = gs[1]; g_scales[3 * row + 2] = gs[2];
	g_opacity[row] = go;
}

bool f3_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
unsigned f3_blocks(long long threads) { return (unsigned)((threads + F3_BLOCK - 1) / F3_BLOCK); }

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_filter3d_accumulate(const float* xyz, int row0, int rows, const float* cams, int ncams, float* rate_inout, int init, void* stream) {
	if (!xyz || !cams || !rate_inout) { set_error("adgs_filter3d_accumulate: NULL xyz / cams / rate_inout"); return -1; }
	if (row0 < 0 || rows < 0 || ncams < 0) { set_error("adgs_filter3d_accumulate: negative row0 / rows / ncams"); return -1; }
	if ((long long)row0 + rows > 0x7fffffffll) { set_error("adgs_filter3d_accumulate: row0 + rows exceeds 2^31 - 1"); return -1; }
	if (!f3_aligned16(cams)) { set_error("adgs_filter3d_accumulate: cams must be 16-byte aligned"); return -1; }
	if (rows == 0) return 0;
	// the aligned middle: row a0 is the first multiple of four (then 3 a0 floats of xyz and a0 floats of rate are multiples of 16 bytes)
	F3Range r{row0, rows, 0, 0};
	if (f3_aligned16(xyz) && f3_aligned16(rate_inout)) {
		const long long end = (long long)row0 + rows, a0 = ((long long)row0 + 3) / 4 * 4, a1 = end / 4 * 4;
		if (a0 < a1) r = F3Range{row0, (int)(a0 - row0), (int)((a1 - a0) / 4), (int)(end - a1)};
	}
	hipLaunchKernelGGL(f3_accumulate_kernel, dim3(f3_blocks((long long)r.groups + r.head + r.tail)), dim3(F3_BLOCK), 0, (hipStream_t)stream,
		xyz, r, reinterpret_cast<const F3Camera*>(cams), ncams, rate_inout, init);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_filter3d_finalize(const float* rate, int P, float* filter_out, uint32_t* work, void* stream_) {
	if (!rate || !filter_out || !work) { set_error("adgs_filter3d_finalize: NULL rate / filter_out / work"); return -1; }
	if (P < 0) { set_error("adgs_filter3d_finalize: negative P"); return -1; }
	if (P == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	ADGS_HIP_CHECK(hipMemsetAsync(work, 0, sizeof(uint32_t), stream));
	hipLaunchKernelGGL(f3_min_rate_kernel, dim3(std::min(f3_blocks(P), 1024u)), dim3(F3_BLOCK), 0, stream, rate, P, work);
	hipLaunchKernelGGL(f3_filter_kernel, dim3(f3_blocks(P)), dim3(F3_BLOCK), 0, stream, rate, P, filter_out, work);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

static int f3_apply_groups(int P, std::initializer_list<const void*> ptrs) {
	for (const void* p : ptrs) if (!f3_aligned16(p)) return 0;
	return P / 4;
}

extern "C" int adgs_filter3d_apply_forward(int P, const float* scales, const float* opacity, const float* filter, float* scales_out, float* opacity_out,
	void* stream) {
	if (!scales || !opacity || !filter || !scales_out || !opacity_out) { set_error("adgs_filter3d_apply_forward: NULL scales / opacity / filter / scales_out / opacity_out"); return -1; }
	if (P < 0) { set_error("adgs_filter3d_apply_forward: negative P"); return -1; }
	if (P == 0) return 0;
	const int groups = f3_apply_groups(P, {scales, opacity, filter, scales_out, opacity_out});
	hipLaunchKernelGGL(f3_apply_fwd_kernel, dim3(f3_blocks((long long)groups + (P - 4 * groups))), dim3(F3_BLOCK), 0, (hipStream_t)stream,
		P, groups, scales, opacity, filter, scales_out, opacity_out);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_filter3d_apply_backward(int P, const float* scales, const float* opacity, const float* filter, const float* g_scales_out,
	const float* g_opacity_out, float* g_scales, float* g_opacity, void* stream) {
	if (!scales || !opacity || !filter || !g_scales_out || !g_opacity_out || !g_scales || !g_opacity) {
		set_error("adgs_filter3d_apply_backward: NULL scales / opacity / filter / g_scales_out / g_opacity_out / g_scales / g_opacity"); return -1;
	}
	if (P < 0) { set_error("adgs_filter3d_apply_backward: negative P"); return -1; }
	if (P == 0) return 0;
	const int groups = f3_apply_groups(P, {scales, opacity, filter, g_scales_out, g_opacity_out, g_scales, g_opacity});
	hipLaunchKernelGGL(f3_apply_bwd_kernel, dim3(f3_blocks((long long)groups + (P - 4 * groups))), dim3(F3_BLOCK), 0, (hipStream_t)stream,
		P, groups, scales, opacity, filter, g_scales_out, g_opacity_out, g_scales, g_opacity);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
