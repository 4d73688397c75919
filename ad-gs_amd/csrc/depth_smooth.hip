// Edge-aware smoothness of the rendered (inverse) depth, first and second order, forward and backward, for gfx950 (wave64).
// The definition is in include/adgs_loss.h (adgs_depth_smooth_forward).  One 32x16 tile per workgroup of 256 threads, two pixels per thread.
//
// Staging.  Depth, weight and -- one channel after the other -- the guide are staged ONCE per workgroup with their halo in LDS (the halo
// is re-read from L2 by the neighbouring tiles, not from HBM).  A guide channel is only ever needed as the two forward differences
// |I(p) - I(p + e_x)|, |I(p) - I(p + e_y)|, summed over the channels: the channel buffer is reused, the loads of up to four channels are in
// flight at once (with those of depth and weight: one round trip for an RGB guide), and what stays is two images ex, ey however many channels
// the guide has.  Both orders read their edge weight from them:
//   order 1, pair (p, p + e):       a = exp(-gamma / C * e(p))
//   order 2, triple centred at p:   a = exp(-gamma / (2 C) * (e(p - e) + e(p)))
// Outside the image the staged weight is 0 (and 1 inside when there is no weight), so a term that leaves the image has v = 0 and drops out of
// every sum without a test; depth and guide are staged as 0 there, which keeps 0 * a * |delta| finite.
//
// Ownership.  A pair belongs to its first pixel, a triple to its centre: a term that straddles a tile border is summed by exactly one workgroup.
// delta is formed in double from the float inputs (its sign is then the float64 reference's), the products v a |delta| in float, the six sums
// (sum w d, sum w, S_x, V_x, S_y, V_y) in double per thread, then through the slot rows (slot_reduce.h); the finish kernel stores the totals,
// s and L behind the rows.
//
// Backward: a gather.  Every staged pixel that owns a term stores sign(delta) v a once (cx, cy in LDS); a pixel then collects the <= 4 (order 1)
// or <= 6 (order 2) coefficients of the terms it takes part in -- halo 1 or 2 -- and writes its element of dL_ddepth once: no atomics, no zero fill.
//
// Byte model (HBM): forward reads (1 + C + [weight]) * 4 * H * W bytes and writes nothing but the slot rows; backward reads the same and
// writes 4 * H * W.  No intermediate image goes to global memory.
#include "common.h"
#include "slot_reduce.h"
#include "../../include/adgs_loss.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

constexpr int DS_TX = 32, DS_TY = 16, DS_LT = 256;
constexpr int DS_CH = 4;                                        // guide channels in flight per thread
constexpr int DS_ROW = 8;                                       // doubles per slot row (six used)
constexpr int DS_MAX_TILES = (1 << 24) - 1;                     // tiles * 256 threads must stay below 2^32
static_assert(DS_LT == SLOT_THREADS && ADGS_SMOOTH_WORK_DOUBLES >= ADGS_LOSS_SLOTS * DS_ROW + 8, "slot_add_wave's workgroup; eight scalars behind the rows");
// scalars behind the rows: sum w d, sum w, S_x, V_x, S_y, V_y, s, L
enum { DS_SWD = 0, DS_SW, DS_SX, DS_VX, DS_SY, DS_VY, DS_S, DS_L };

// halo of the staged region: what lies before (HL) and behind (HR) the tile along each axis
template <int ORDER, bool BWD> struct Region {
	static constexpr int HL = BWD ? ORDER : ORDER - 1, HR = BWD ? ORDER : 1;
	static constexpr int RX = DS_TX + HL + HR, RY = DS_TY + HL + HR, RN = RX * RY;
	static constexpr int NI = (RN + DS_LT - 1) / DS_LT;          // staged elements per thread
};

// one term along one axis (st: 1 or the row stride), owned by staged element i: delta, v = product of the weights, a = the edge weight
template <int ORDER>
__device__ __forceinline__ void smooth_term(const float* sd, const float* sw, const float* e, int i, int st, float k, double& delta, float& v, float& a) {
	if constexpr (ORDER == 1) {
		delta = (double)sd[i] - (double)sd[i + st];
		v = sw[i] * sw[i + st];
		a = expf(-k * e[i]);
	} else {
		delta = (double)sd[i - st] - 2.0 * (double)sd[i] + (double)sd[i + st];
		v = sw[i - st] * sw[i] * sw[i + st];
		a = expf(-k * (e[i - st] + e[i]));
	}
}

// Stages depth, weight and the guide's difference sums ex, ey of the region around tile (x0, y0).  Ends with a barrier.
template <class R>
__device__ __forceinline__ void stage_region(int H, int W, int C, const float* __restrict__ depth, const float* __restrict__ guide, const float* __restrict__ weight,
	int x0, int y0, int tid, float* sd, float* sw, float* buf, float* ex, float* ey) {
	int off[R::NI];                                             // clamped offset into a plane (H * W <= INT_MAX)
	bool in[R::NI];
#pragma unroll
	for (int it = 0; it < R::NI; it++) {
		const int i = min(tid + it * DS_LT, R::RN - 1);
		const int ry = i / R::RX, rx = i - ry * R::RX;
		const int gy = y0 - R::HL + ry, gx = x0 - R::HL + rx;
		in[it] = gy >= 0 && gy < H && gx >= 0 && gx < W;
		off[it] = min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
	}
	// every load a thread can issue is in flight before its first LDS store: depth, weight and the first DS_CH guide channels are one
	// round trip; register set j is refilled with channel c + DS_CH as soon as channel c has gone to LDS
	float vd[R::NI], vw[R::NI], vg[DS_CH][R::NI];
#pragma unroll
	for (int it = 0; it < R::NI; it++) {
		vd[it] = depth[off[it]];
		vw[it] = weight ? weight[off[it]] : 1.f;
	}
#pragma unroll
	for (int j = 0; j < DS_CH; j++) {
		if (j < C) {
			const float* src = guide + (size_t)j * H * W;
#pragma unroll
			for (int it = 0; it < R::NI; it++) vg[j][it] = src[off[it]];
		}
	}
#pragma unroll
	for (int it = 0; it < R::NI; it++) {
		const int i = tid + it * DS_LT;
		if (i < R::RN) { sd[i] = in[it] ? vd[it] : 0.f; sw[i] = in[it] ? vw[it] : 0.f; }
	}
	float ax[R::NI], ay[R::NI];
#pragma unroll
	for (int it = 0; it < R::NI; it++) { ax[it] = 0.f; ay[it] = 0.f; }
	for (int c0 = 0; c0 < C; c0 += DS_CH) {
#pragma unroll
		for (int j = 0; j < DS_CH; j++) {
			const int c = c0 + j;
			if (c >= C) break;
			if (c) __syncthreads();                             // channel c - 1 has been read
#pragma unroll
			for (int it = 0; it < R::NI; it++) {
				const int i = tid + it * DS_LT;
				if (i < R::RN) buf[i] = in[it] ? vg[j][it] : 0.f;
			}
			if (c + DS_CH < C) {
				const float* nxt = guide + (size_t)(c + DS_CH) * H * W;
#pragma unroll
				for (int it = 0; it < R::NI; it++) vg[j][it] = nxt[off[it]];
			}
			__syncthreads();
#pragma unroll
			for (int it = 0; it < R::NI; it++) {
				const int i = tid + it * DS_LT;
				if (i >= R::RN) continue;
				const int ry = i / R::RX, rx = i - ry * R::RX;
				const float b = buf[i];
				if (rx + 1 < R::RX) ax[it] += fabsf(b - buf[i + 1]);
				if (ry + 1 < R::RY) ay[it] += fabsf(b - buf[i + R::RX]);
			}
		}
	}
#pragma unroll
	for (int it = 0; it < R::NI; it++) {
		const int i = tid + it * DS_LT;
		if (i < R::RN) { ex[i] = ax[it]; ey[i] = ay[it]; }
	}
	__syncthreads();
}

template <int ORDER>
__global__ void __launch_bounds__(DS_LT) depth_smooth_sum_kernel(int H, int W, int C, int tiles_x, const float* __restrict__ depth, const float* __restrict__ guide,
	const float* __restrict__ weight, float kx, double* __restrict__ work) {
	using R = Region<ORDER, false>;
	__shared__ float sd[R::RN], sw[R::RN], buf[R::RN], ex[R::RN], ey[R::RN];
	const int tid = threadIdx.x;
	const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
	stage_region<R>(H, W, C, depth, guide, weight, bx * DS_TX, by * DS_TY, tid, sd, sw, buf, ex, ey);
	double acc[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int i = (2 * (tid >> 5) + o + R::HL) * R::RX + (tid & (DS_TX - 1)) + R::HL;
		acc[DS_SWD] += (double)(sw[i] * sd[i]);
		acc[DS_SW] += (double)sw[i];
		double delta; float v, a;
		smooth_term<ORDER>(sd, sw, ex, i, 1, kx, delta, v, a);
		acc[DS_SX] += (double)(v * a * (float)fabs(delta)); acc[DS_VX] += (double)v;
		smooth_term<ORDER>(sd, sw, ey, i, R::RX, kx, delta, v, a);
		acc[DS_SY] += (double)(v * a * (float)fabs(delta)); acc[DS_VY] += (double)v;
	}
	slot_add_wave<ADGS_LOSS_SLOTS, DS_ROW>(work, acc);
}

// one block: totals of the slot rows (left zero) -> the eight scalars behind them and the loss
__global__ void __launch_bounds__(SLOT_THREADS) depth_smooth_finish_kernel(double* __restrict__ work, int normalize, float* __restrict__ loss) {
	double t[6];
	slot_finish<ADGS_LOSS_SLOTS, DS_ROW>(work, t);
	if (threadIdx.x == 0) {
		double* tot = work + (size_t)ADGS_LOSS_SLOTS * DS_ROW;
		for (int q = 0; q < 6; q++) tot[q] = t[q];
		double sc = 0.0, L = 0.0;
		if (tot[DS_SW] > 0.0) {
			sc = normalize ? 1.0 / (tot[DS_SWD] / tot[DS_SW] + 1e-7) : 1.0;
			L = sc * ((tot[DS_VX] > 0.0 ? tot[DS_SX] / tot[DS_VX] : 0.0) + (tot[DS_VY] > 0.0 ? tot[DS_SY] / tot[DS_VY] : 0.0));
		}
		tot[DS_S] = sc; tot[DS_L] = L;
		loss[0] = (float)L;
	}
}

template <int ORDER>
__global__ void __launch_bounds__(DS_LT) depth_smooth_bwd_kernel(int H, int W, int C, int tiles_x, const float* __restrict__ depth, const float* __restrict__ guide,
	const float* __restrict__ weight, float kx, int normalize, const double* __restrict__ work, const float* __restrict__ g_loss, float* __restrict__ out) {
	using R = Region<ORDER, true>;
	__shared__ float sd[R::RN], sw[R::RN], buf[R::RN], ex[R::RN], ey[R::RN], cx[R::RN], cy[R::RN];
	const int tid = threadIdx.x;
	const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
	const int x0 = bx * DS_TX, y0 = by * DS_TY;
	stage_region<R>(H, W, C, depth, guide, weight, x0, y0, tid, sd, sw, buf, ex, ey);
	// the coefficient sign(delta) v a of the term each staged element owns, where the region holds the whole term
#pragma unroll
	for (int it = 0; it < R::NI; it++) {
		const int i = tid + it * DS_LT;
		if (i >= R::RN) continue;
		const int ry = i / R::RX, rx = i - ry * R::RX;
		double delta; float v, a, tx = 0.f, ty = 0.f;
		if (rx >= ORDER - 1 && rx + 1 < R::RX) {
			smooth_term<ORDER>(sd, sw, ex, i, 1, kx, delta, v, a);
			tx = sgn(delta) * (v * a);
		}
		if (ry >= ORDER - 1 && ry + 1 < R::RY) {
			smooth_term<ORDER>(sd, sw, ey, i, R::RX, kx, delta, v, a);
			ty = sgn(delta) * (v * a);
		}
		cx[i] = tx; cy[i] = ty;
	}
	__syncthreads();
	const double* tot = work + (size_t)ADGS_LOSS_SLOTS * DS_ROW;
	const double sum_w = tot[DS_SW], vx = tot[DS_VX], vy = tot[DS_VY];
	const float inv_vx = vx > 0.0 ? (float)(1.0 / vx) : 0.f, inv_vy = vy > 0.0 ? (float)(1.0 / vy) : 0.f;
	const float gs = g_loss[0] * (float)tot[DS_S];                                     // s = 0 when sum w = 0
	const float through_mean = normalize && sum_w > 0.0 ? (float)(tot[DS_L] / sum_w) : 0.f;
	const int gx = x0 + (tid & (DS_TX - 1));
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int ly = 2 * (tid >> 5) + o, gy = y0 + ly;
		if (gx >= W || gy >= H) continue;
		const int i = (ly + R::HL) * R::RX + (tid & (DS_TX - 1)) + R::HL;
		float G;
		if constexpr (ORDER == 1) G = inv_vx * (cx[i] - cx[i - 1]) + inv_vy * (cy[i] - cy[i - R::RX]);
		else G = inv_vx * (cx[i - 1] - 2.f * cx[i] + cx[i + 1]) + inv_vy * (cy[i - R::RX] - 2.f * cy[i] + cy[i + R::RX]);
		out[(size_t)gy * W + gx] = gs * (G - through_mean * sw[i]);
	}
}

// what both entry points refuse, from the arguments alone; tiles: the number of workgroups
int smooth_check(const char* who, int H, int W, int C, const float* guide, int order, float gamma, bool null_pointer, long long& tiles) {
	const std::string name(who);
	if (null_pointer) { set_error(name + ": NULL pointer"); return -1; }
	if (H < 0 || W < 0) { set_error(name + ": negative H or W"); return -1; }
	if ((long long)H * W > (long long)INT_MAX) { set_error(name + ": H * W exceeds INT_MAX"); return -1; }
	if (order != 1 && order != 2) { set_error(name + ": order must be 1 or 2"); return -1; }
	if (C < 0 || C > 8) { set_error(name + ": C must lie in [0, 8]"); return -1; }
	if ((guide != nullptr) != (C > 0)) { set_error(name + ": a guide needs 1 <= C <= 8 channels, no guide C = 0"); return -1; }
	if (!(gamma >= 0.f) || !std::isfinite(gamma)) { set_error(name + ": gamma must be finite and >= 0"); return -1; }
	tiles = (long long)((W + DS_TX - 1) / DS_TX) * ((H + DS_TY - 1) / DS_TY);
	if (tiles > DS_MAX_TILES) { set_error(name + ": more than 16777215 tiles of 32 x 16 pixels"); return -1; }
	return 0;
}
// the factor of the summed guide differences in the exponent: gamma / C at order 1, gamma / (2 C) at order 2
float smooth_k(int C, int order, float gamma) { return C ? gamma / (float)(order * C) : 0.f; }

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_depth_smooth_forward(int H, int W, int C, const float* depth, const float* guide, const float* weight,
	int order, int normalize, float gamma, double* work, float* loss, void* stream_) {
	long long tiles = 0;
	if (smooth_check("adgs_depth_smooth_forward", H, W, C, guide, order, gamma, !depth || !work || !loss, tiles)) return -1;
	if (tiles == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const int tiles_x = (W + DS_TX - 1) / DS_TX;
	const float k = smooth_k(C, order, gamma);
	if (order == 1) hipLaunchKernelGGL(depth_smooth_sum_kernel<1>, dim3((unsigned)tiles), dim3(DS_LT), 0, stream, H, W, C, tiles_x, depth, guide, weight, k, work);
	else hipLaunchKernelGGL(depth_smooth_sum_kernel<2>, dim3((unsigned)tiles), dim3(DS_LT), 0, stream, H, W, C, tiles_x, depth, guide, weight, k, work);
	hipLaunchKernelGGL(depth_smooth_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, normalize ? 1 : 0, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_depth_smooth_backward(int H, int W, int C, const float* depth, const float* guide, const float* weight,
	int order, int normalize, float gamma, const double* work, const float* g_loss, float* dL_ddepth, void* stream_) {
	long long tiles = 0;
	if (smooth_check("adgs_depth_smooth_backward", H, W, C, guide, order, gamma, !depth || !work || !g_loss || !dL_ddepth, tiles)) return -1;
	if (tiles == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const int tiles_x = (W + DS_TX - 1) / DS_TX;
	const float k = smooth_k(C, order, gamma);
	if (order == 1) hipLaunchKernelGGL(depth_smooth_bwd_kernel<1>, dim3((unsigned)tiles), dim3(DS_LT), 0, stream, H, W, C, tiles_x, depth, guide, weight, k,
		normalize ? 1 : 0, work, g_loss, dL_ddepth);
	else hipLaunchKernelGGL(depth_smooth_bwd_kernel<2>, dim3((unsigned)tiles), dim3(DS_LT), 0, stream, H, W, C, tiles_x, depth, guide, weight, k,
		normalize ? 1 : 0, work, g_loss, dL_ddepth);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
