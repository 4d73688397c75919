// Tile geometry, halo staging and the separable 11-tap Gaussian window of the SSIM kernels (loss.hip: the training loss and its backward;
// metrics.hip: the evaluation pass).  One 32x16 output tile per workgroup of 256 threads: the 42x26 input halo is staged in LDS, the window
// runs as a horizontal pass (into LDS) and a vertical pass, both as sliding windows in registers (loss.hip's header comment).
#pragma once
#include "common.h"
#include <cmath>

namespace adgs {
namespace ssimwin {

constexpr int TSX = 32, TSY = 16;         // output tile
constexpr int WR = 5;                     // window radius (11 taps)
constexpr int NT = 2 * WR + 1;
constexpr int HSX = TSX + 2 * WR, HSY = TSY + 2 * WR;      // halo 42 x 26
constexpr int SSTR = 44;                  // floats per staged row (16-byte aligned; 4 sx + 15 <= 43)
constexpr int HSTR = TSX + 4;             // floats per row of the horizontally filtered images
constexpr int LT = 256;                   // threads per workgroup
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

// gaussian(11, 1.5) of utils/loss_utils.py:26-28: exp(-(x-5)^2 / (2 sigma^2)) normalised by the sum (float32)
struct Window { float g[NT]; };
static Window make_window() {
	Window w; float s = 0.f;
	for (int x = 0; x < 2 * WR + 1; x++) { w.g[x] = (float)std::exp(-(double)((x - WR) * (x - WR)) / (2.0 * 1.5 * 1.5)); s += w.g[x]; }
	for (int x = 0; x < 2 * WR + 1; x++) w.g[x] = w.g[x] / s;
	return w;
}

// what stage_halos does to an element inside the image before it stores it: nothing
struct StageAsIs { __device__ __forceinline__ float operator()(int, float v, int, int) const { return v; } };

// Staging of NA halo images at once: zero padding outside the image (F.conv2d padding=5).  All loads of a thread (5 per image, at
// clamped addresses, unconditional) are issued before the first LDS store: a rolled loop of conditional loads paid one L2 round
// trip per element and image -- the staging, not the window arithmetic, was what these kernels' time went into.
// An element inside the image is stored as op(a, value, ly, lx) (a: which image; ly, lx: its place in the halo); the padding stays zero.
template <int NA, class Op = StageAsIs>
__device__ __forceinline__ void stage_halos(float (*const (&s)[NA])[SSTR], const float* const (&src)[NA], size_t plane, int x0, int y0, int H, int W, int tid,
	const Op& op = Op()) {
	constexpr int NIT = (HSY * HSX + LT - 1) / LT;
	float v[NA][NIT];
#pragma unroll
	for (int it = 0; it < NIT; it++) {
		const int i = min(tid + it * LT, HSY * HSX - 1);
		const int ly = i / HSX, lx = i - ly * HSX;
		const int gy = min(max(y0 + ly - WR, 0), H - 1), gx = min(max(x0 + lx - WR, 0), W - 1);
#pragma unroll
		for (int a = 0; a < NA; a++) v[a][it] = src[a][plane + (size_t)gy * W + gx];
	}
#pragma unroll
	for (int it = 0; it < NIT; it++) {
		const int i = tid + it * LT;
		if (i >= HSY * HSX) break;
		const int ly = i / HSX, lx = i - ly * HSX, gy = y0 + ly - WR, gx = x0 + lx - WR;
		const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
		for (int a = 0; a < NA; a++) s[a][ly][lx] = in ? op(a, v[a][it], ly, lx) : 0.f;
	}
}
// 16 consecutive floats of a staged row (14 are used) as four 16-byte LDS reads
__device__ __forceinline__ void load_run(const float* row, float (&u)[16]) {
	const float4* r = reinterpret_cast<const float4*>(row);
#pragma unroll
	for (int q = 0; q < 4; q++) { const float4 v = r[q]; u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w; }
}
__device__ __forceinline__ float4 window4(const Window& win, const float (&u)[16]) {
	float o[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		float a = 0.f;
#pragma unroll
		for (int k = 0; k < NT; k++) a += win.g[k] * u[j + k];
		o[j] = a;
	}
	return make_float4(o[0], o[1], o[2], o[3]);
}

} // namespace ssimwin
} // namespace adgs
