// Fused L1 + SSIM (11x11 Gaussian window, sigma 1.5, zero padding) forward and backward for gfx950.
// Reference: utils/loss_utils.py:20-68 (called at train.py:79-80).  One 32x16 output tile per workgroup:
// the 42x26 input halo is staged in LDS, the separable window runs as a horizontal pass (into LDS) and a
// vertical pass, both as SLIDING WINDOWS IN REGISTERS: a thread forms 4 neighbouring outputs of a row from
// 14 inputs read as four 16-byte LDS words (instead of 4 x 11 scalar reads), and 2 outputs of a column from
// 12 reads (instead of 22).  The 16x16-tile, one-output-per-thread form of round 2 was LDS-bound (11 reads
// per output and pass, 2-way bank conflicts, one L2 round trip per staged element): 129 + 93 us per C3 frame;
// now 99 + 75.  The arithmetic per output (tap order, fused multiply-adds) is unchanged.
#include "common.h"
#include "ssim_window.h"
#include "slot_reduce.h"
#include "../../include/adgs_loss.h"

namespace adgs {
namespace {

using namespace ssimwin;                  // tile geometry, Window, stage_halos, load_run, window4: shared with metrics.hip

// WEIGHTED: a per-pixel supervision weight w [H, W], shared by every plane, applies to the MAP and to |image - gt| (the images enter the
// windows unweighted: the region definition of metrics.hip).  The thread reads w at its two output pixels only; the sums are
// (sum w |d|, sum w ssim, sum w) with sum w counted by the workgroups of plane 0 alone, and the three maps are stored times w, so the
// backward's convolutions are those of the unweighted form.  A workgroup whose whole tile has w = 0 (an ego-vehicle mask is whole rows of
// them) writes zero maps and skips the staging and the windows.
template <bool WEIGHTED>
__global__ void __launch_bounds__(LT) l1_ssim_fwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ weight,
	Window win, double* __restrict__ sums, float* __restrict__ d_mu1, float* __restrict__ d_e11, float* __restrict__ d_e12) {
	constexpr int NS = WEIGHTED ? 3 : 2;
	__shared__ __attribute__((aligned(16))) float s1[HSY][SSTR], s2[HSY][SSTR];
	__shared__ __attribute__((aligned(16))) float h[5][HSY][HSTR];      // horizontally filtered x1, x2, x1^2, x2^2, x1 x2
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * TSX, y0 = blockIdx.y * TSY;
	const size_t plane = (size_t)blockIdx.z * H * W;
	float wv[2] = { 1.f, 1.f };
	if constexpr (WEIGHTED) {
		const int gx = x0 + (tid & (TSX - 1)), gy = y0 + 2 * (tid >> 5);
#pragma unroll
		for (int o = 0; o < 2; o++) wv[o] = (gx < W && gy + o < H) ? weight[(size_t)(gy + o) * W + gx] : 0.f;
		if (!__syncthreads_or(wv[0] != 0.f || wv[1] != 0.f)) {
			if (d_mu1 && gx < W) {
#pragma unroll
				for (int o = 0; o < 2; o++) {
					if (gy + o >= H) continue;
					const size_t oo = plane + (size_t)(gy + o) * W + gx;
					d_mu1[oo] = 0.f; d_e11[oo] = 0.f; d_e12[oo] = 0.f;
				}
			}
			return;
		}
	}
	{
		float (*const dst[2])[SSTR] = { s1, s2 };
		const float* const src[2] = { img, gt };
		stage_halos<2>(dst, src, plane, x0, y0, H, W, tid);
	}
	__syncthreads();
	{	// horizontal pass: row r, outputs 4 sx .. 4 sx + 3
		const int r = tid >> 3, sx = tid & 7;
		if (r < HSY) {
			float u[16], v[16], t[16];
			load_run(&s1[r][4 * sx], u); load_run(&s2[r][4 * sx], v);
			*reinterpret_cast<float4*>(&h[0][r][4 * sx]) = window4(win, u);
			*reinterpret_cast<float4*>(&h[1][r][4 * sx]) = window4(win, v);
#pragma unroll
			for (int i = 0; i < 16; i++) t[i] = u[i] * u[i];
			*reinterpret_cast<float4*>(&h[2][r][4 * sx]) = window4(win, t);
#pragma unroll
			for (int i = 0; i < 16; i++) t[i] = v[i] * v[i];
			*reinterpret_cast<float4*>(&h[3][r][4 * sx]) = window4(win, t);
#pragma unroll
			for (int i = 0; i < 16; i++) t[i] = u[i] * v[i];
			*reinterpret_cast<float4*>(&h[4][r][4 * sx]) = window4(win, t);
		}
	}
	__syncthreads();
	// vertical pass: column tx, outputs rows 2 g and 2 g + 1
	const int tx = tid & (TSX - 1), g = tid >> 5;
	float acc[5][2];
#pragma unroll
	for (int q = 0; q < 5; q++) {
		float c[NT + 1];
#pragma unroll
		for (int j = 0; j < NT + 1; j++) c[j] = h[q][2 * g + j][tx];
#pragma unroll
		for (int o = 0; o < 2; o++) {
			float a = 0.f;
#pragma unroll
			for (int k = 0; k < NT; k++) a += win.g[k] * c[o + k];
			acc[q][o] = a;
		}
	}
	double l1 = 0.0, sm = 0.0, sw = 0.0;
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int ty = 2 * g + o, gx = x0 + tx, gy = y0 + ty;
		if (gx >= W || gy >= H) continue;
		const float mu1 = acc[0][o], mu2 = acc[1][o], e11 = acc[2][o], e22 = acc[3][o], e12 = acc[4][o];
		const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
		const float sg1 = e11 - mu1_sq, sg2 = e22 - mu2_sq, sg12 = e12 - mu12;
		const float A1 = 2.f * mu12 + C1, A2 = 2.f * sg12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = sg1 + sg2 + C2;
		const float D = B1 * B2, inv = 1.f / D;
		double map = (double)((A1 * A2) * inv), ad = (double)fabsf(s1[ty + WR][tx + WR] - s2[ty + WR][tx + WR]);
		if constexpr (WEIGHTED) {
			map *= (double)wv[o]; ad *= (double)wv[o];
			if (blockIdx.z == 0) sw += (double)wv[o];
		}
		sm += map;
		l1 += ad;
		if (d_mu1) {
			const size_t oo = plane + (size_t)gy * W + gx;
			// partial derivatives of the map w.r.t. the window means mu1, E[x1^2], E[x1 x2] (mu2, E[x2^2] belong to gt)
			const float num = A1 * A2;
			const float dnum = 2.f * mu2 * A2 - 2.f * mu2 * A1;           // dA1 = 2 mu2, dA2 = -2 mu2
			const float dden = 2.f * mu1 * B2 - 2.f * mu1 * B1;           // dB1 = 2 mu1, dB2 = -2 mu1
			float p_mu1 = (dnum * D - num * dden) * (inv * inv);
			float p_e11 = -num * inv / B2;                                // dB2 = 1
			float p_e12 = 2.f * A1 * inv;                                 // dA2 = 2
			if constexpr (WEIGHTED) { p_mu1 *= wv[o]; p_e11 *= wv[o]; p_e12 *= wv[o]; }
			d_mu1[oo] = p_mu1; d_e11[oo] = p_e11; d_e12[oo] = p_e12;
		}
	}
	double v[NS] = { l1, sm };
	if constexpr (WEIGHTED) v[2] = sw;
	slot_add_block<ADGS_LOSS_SLOTS, NS, LT>(sums, v);
}

// WEIGHTED: the maps arrive times w (see the forward), the L1 term takes w at the pixel, and 1 / (planes sum w) replaces inv_n: sum w is
// read from the totals the forward's finish kernel left in the work buffer (0 -> an all-zero gradient).
template <bool WEIGHTED>
__global__ void __launch_bounds__(LT) l1_ssim_bwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ weight,
	const double* __restrict__ totals, Window win, const float* __restrict__ d_mu1, const float* __restrict__ d_e11, const float* __restrict__ d_e12,
	const float* __restrict__ g_l1, const float* __restrict__ g_ssim, float inv_n, float* __restrict__ out) {
	__shared__ __attribute__((aligned(16))) float s[3][HSY][SSTR];
	__shared__ __attribute__((aligned(16))) float h[3][HSY][HSTR];
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * TSX, y0 = blockIdx.y * TSY;
	const size_t plane = (size_t)blockIdx.z * H * W;
	// map pixels outside the image do not exist: contribute 0
	{
		float (*const dst[3])[SSTR] = { s[0], s[1], s[2] };
		const float* const src[3] = { d_mu1, d_e11, d_e12 };
		stage_halos<3>(dst, src, plane, x0, y0, H, W, tid);
	}
	__syncthreads();
	{
		const int r = tid >> 3, sx = tid & 7;
		if (r < HSY) {
#pragma unroll
			for (int q = 0; q < 3; q++) {
				float u[16];
				load_run(&s[q][r][4 * sx], u);
				*reinterpret_cast<float4*>(&h[q][r][4 * sx]) = window4(win, u);
			}
		}
	}
	__syncthreads();
	const int tx = tid & (TSX - 1), g = tid >> 5;
	float acc[3][2];
#pragma unroll
	for (int q = 0; q < 3; q++) {
		float c[NT + 1];
#pragma unroll
		for (int j = 0; j < NT + 1; j++) c[j] = h[q][2 * g + j][tx];
#pragma unroll
		for (int o = 0; o < 2; o++) {
			float a = 0.f;
#pragma unroll
			for (int k = 0; k < NT; k++) a += win.g[k] * c[o + k];
			acc[q][o] = a;
		}
	}
	const float gs = g_ssim ? g_ssim[0] : 0.f, gl = g_l1 ? g_l1[0] : 0.f;
	if constexpr (WEIGHTED) {
		const double sw = totals[2];
		inv_n = sw > 0.0 ? (float)(1.0 / ((double)gridDim.z * sw)) : 0.f;
	}
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int gx = x0 + tx, gy = y0 + 2 * g + o;
		if (gx >= W || gy >= H) continue;
		const size_t oo = plane + (size_t)gy * W + gx;
		const float x1 = img[oo], x2 = gt[oo];
		const float dx = x1 - x2;
		float sg = sgn(dx);
		if constexpr (WEIGHTED) sg *= weight[(size_t)gy * W + gx];
		out[oo] = gl * sg * inv_n + gs * inv_n * (acc[0][o] + 2.f * x1 * acc[1][o] + x2 * acc[2][o]);
	}
}

// ---------------------------------------------------------------- scale/shift-invariant depth loss
// work layout (doubles): [slot][DEPTH_ROW] partial sums (a00, a01, a11, b0, b1 of pass 1; L1, A = sum m sgn p, B = sum m sgn of pass 2),
// then 16 scalars: [0..4] the five totals, [5] s, [6] t, [7] det, [8] L1 total, [9] A, [10] B.
constexpr int DEPTH_ROW = 8, DEPTH_TOTALS = ADGS_LOSS_SLOTS * DEPTH_ROW;
struct DepthScalars { double a00, a01, a11, b0, b1, s, t, det; };

__global__ void __launch_bounds__(SLOT_THREADS) depth_sums_kernel(int n, const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, double* __restrict__ work) {
	double a00 = 0, a01 = 0, a11 = 0, b0 = 0, b1 = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const double w = m ? (double)m[i] : 1.0, x = p[i], y = g[i];
		a00 += w * x * x; a01 += w * x; a11 += w; b0 += w * x * y; b1 += w * y;
	}
	double v[5] = { a00, a01, a11, b0, b1 };
	slot_add_wave<ADGS_LOSS_SLOTS, DEPTH_ROW>(work, v);
}
// one block: totals of the slots -> scale, shift (depth_utils.py:30-45)
__global__ void __launch_bounds__(SLOT_THREADS) depth_solve_kernel(double* __restrict__ work) {
	double* out = work + DEPTH_TOTALS;
	double t[5];
	slot_finish<ADGS_LOSS_SLOTS, DEPTH_ROW>(work, t);
	if (threadIdx.x == 0) {
		for (int q = 0; q < 5; q++) out[q] = t[q];
		// the reference forms the sums and the determinant in fp32 (torch.sum of fp32 tensors): round the totals first
		const float a00 = (float)t[0], a01 = (float)t[1], a11 = (float)t[2], b0 = (float)t[3], b1 = (float)t[4];
		const float det = a00 * a11 - a01 * a01;
		float sc = 0.f, sh = 0.f;
		if (det != 0.f) { sc = (a11 * b0 - a01 * b1) / det; sh = (-a01 * b0 + a00 * b1) / det; }
		out[5] = sc; out[6] = sh; out[7] = det;
	}
}
__global__ void __launch_bounds__(SLOT_THREADS) depth_l1_kernel(int n, const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m, double* __restrict__ work) {
	const double* sc = work + DEPTH_TOTALS;
	const float s = (float)sc[5], t = (float)sc[6];
	double L = 0, A = 0, B = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const float w = m ? m[i] : 1.f, x = p[i];
		const float d = (s * x + t) - g[i];
		const float sg = sgn(d);
		L += (double)(fabsf(d) * w); A += (double)(w * sg * x); B += (double)(w * sg);
	}
	double v[3] = { L, A, B };
	slot_add_wave<ADGS_LOSS_SLOTS, DEPTH_ROW>(work, v, 5);      // columns 5 .. 7 of the rows
}
__global__ void __launch_bounds__(SLOT_THREADS) depth_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double* out = work + DEPTH_TOTALS;
	double t[3];
	slot_finish<ADGS_LOSS_SLOTS, DEPTH_ROW>(work, t, 5);
	if (threadIdx.x == 0) {
		for (int q = 0; q < 3; q++) out[8 + q] = t[q];
		loss[0] = (float)(out[8] / out[2]);                       // sum(|.| m) / sum(m)
	}
}
__global__ void __launch_bounds__(256) depth_bwd_kernel(int n, const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
	const double* __restrict__ work, const float* __restrict__ g_loss, float* __restrict__ out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double* sc = work + DEPTH_TOTALS;
	const double a00 = sc[0], a01 = sc[1], a11 = sc[2], b0 = sc[3], b1 = sc[4], s = sc[5], t = sc[6], det = sc[7], A = sc[9], B = sc[10];
	const float w = m ? m[i] : 1.f, x = p[i], y = g[i];
	const float d = ((float)s * x + (float)t) - y;
	const float sg = sgn(d);
	double grad = (double)sg * s;
	if (det != 0.0) {
		// through the least-squares solution: s, t depend on a00 = sum m p^2, a01 = sum m p, b0 = sum m p g
		const double s_a00 = -s * a11 / det, s_a01 = (-b1 + 2.0 * a01 * s) / det, s_b0 = a11 / det;
		const double t_a00 = (b1 - t * a11) / det, t_a01 = (-b0 + 2.0 * a01 * t) / det, t_b0 = -a01 / det;
		grad += (A * s_a00 + B * t_a00) * 2.0 * x + (A * s_a01 + B * t_a01) + (A * s_b0 + B * t_b0) * y;
	} else grad = 0.0;                                             // the reference returns python floats (0.0, 0.0): no graph
	out[i] = (float)((double)g_loss[0] * (double)w * grad / a11);
	(void)a00;
}

// ---------------------------------------------------------------- flow re-projection loss and clipped BCE
// Pixel-wise losses of train.py:88-103 that the reference builds from nonzero() (a host synchronisation), gathers and half a
// dozen elementwise kernels each.  Here: one reduction pass (slot_reduce.h) + a one-block finish, and one elementwise backward.
// aux work layout (doubles): [slot][AUX_ROW] = (sum, count), then [AUX_TOTALS] = sum, [+1] = count.
constexpr int AUX_ROW = 2, AUX_TOTALS = ADGS_LOSS_SLOTS * AUX_ROW;
struct FlowCam { float M[9]; float KT[3]; float dist; };          // M = K R, KT = K T (3x3 row-major products formed on the host in fp32)
// The camera of the flow target as DEVICE pointers (the reference keeps K / R / T on the GPU, train.py:68-71): nothing is read back
// and nothing is cached on the host.  K == nullptr: the by-value FlowCam is used.
struct FlowCamDev { const float* K; const float* R; const float* T; };
// the same products, in the same order and without contraction, as make_flow_cam forms on the host: both entry points agree bit for bit
__device__ __forceinline__ FlowCam flow_cam_load(const FlowCam& host, const FlowCamDev& d) {
	if (!d.K) return host;
	FlowCam c;
#pragma unroll
	for (int i = 0; i < 3; i++) {
#pragma unroll
		for (int j = 0; j < 3; j++)
			c.M[3 * i + j] = __fadd_rn(__fadd_rn(__fmul_rn(d.K[3 * i], d.R[j]), __fmul_rn(d.K[3 * i + 1], d.R[3 + j])), __fmul_rn(d.K[3 * i + 2], d.R[6 + j]));
		c.KT[i] = __fadd_rn(__fadd_rn(__fmul_rn(d.K[3 * i], d.T[0]), __fmul_rn(d.K[3 * i + 1], d.T[1])), __fmul_rn(d.K[3 * i + 2], d.T[2]));
	}
	c.dist = host.dist;
	return c;
}

struct FlowPix { bool sel; float w, u, v, z, px, py; bool front; };
__device__ __forceinline__ FlowPix flow_pixel(int i, int HW, int W, int H, const float* __restrict__ f, const float* __restrict__ fl,
	const float* __restrict__ vis, const float* __restrict__ op, const FlowCam& c) {
	FlowPix r;
	const float t0 = fl[i], t1 = fl[HW + i];
	r.sel = (vis[i] > 0.5f) && (t0 <= (float)W - 1.0f) && (t0 >= 0.f) && (t1 <= (float)H - 1.0f) && (t1 >= 0.f);       // loss_utils.py:90
	r.w = 0.f; r.u = r.v = r.z = r.px = r.py = 0.f; r.front = false;
	if (!r.sel) return r;
	const float x = f[i], y = f[HW + i], z = f[2 * HW + i];
	r.px = c.M[0] * x + c.M[1] * y + c.M[2] * z + c.KT[0];
	r.py = c.M[3] * x + c.M[4] * y + c.M[5] * z + c.KT[1];
	const float pz = c.M[6] * x + c.M[7] * y + c.M[8] * z + c.KT[2];
	r.front = pz > c.dist;                                         // flow_utils.py:8
	r.z = fmaxf(pz, c.dist);                                       // clamp_min, :9
	r.u = r.px / r.z; r.v = r.py / r.z;
	r.w = (op ? op[i] : 1.f) * (r.front ? 1.f : 0.f);
	return r;
}
__global__ void __launch_bounds__(SLOT_THREADS) flow_loss_sum_kernel(int H, int W, const float* __restrict__ f, const float* __restrict__ fl,
	const float* __restrict__ vis, const float* __restrict__ op, FlowCam c0, FlowCamDev cd, double* __restrict__ work) {
	const int HW = H * W;
	const FlowCam c = flow_cam_load(c0, cd);
	double sum = 0, cnt = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
		const FlowPix p = flow_pixel(i, HW, W, H, f, fl, vis, op, c);
		if (p.sel) {
			cnt += 1.0;
			sum += (double)((fabsf(p.u - fl[i]) / (float)W + fabsf(p.v - fl[HW + i]) / (float)H) * p.w);      // :103-105
		}
	}
	double v[2] = { sum, cnt };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
}
// the finish kernel every (sum, count) term shares: the two totals behind the rows, loss = sum / count
__global__ void __launch_bounds__(SLOT_THREADS) aux_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double t[2];
	slot_finish<ADGS_LOSS_SLOTS, AUX_ROW>(work, t);
	if (threadIdx.x == 0) {
		work[AUX_TOTALS] = t[0]; work[AUX_TOTALS + 1] = t[1];
		loss[0] = t[1] > 0 ? (float)(t[0] / t[1]) : 0.f;             // mean over the selected pixels; 0.0 when none (:92-93)
	}
}
__global__ void __launch_bounds__(256) flow_loss_bwd_kernel(int H, int W, const float* __restrict__ f, const float* __restrict__ fl,
	const float* __restrict__ vis, const float* __restrict__ op, FlowCam c0, FlowCamDev cd, const double* __restrict__ work, const float* __restrict__ g_loss,
	float* __restrict__ g_f, float* __restrict__ g_op) {
	const int HW = H * W;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= HW) return;
	const FlowCam c = flow_cam_load(c0, cd);
	const double n = work[AUX_TOTALS + 1];
	const FlowPix p = flow_pixel(i, HW, W, H, f, fl, vis, op, c);
	float gx = 0.f, gy = 0.f, gz = 0.f, go = 0.f;
	if (p.sel && n > 0) {
		const float gl = (float)((double)g_loss[0] / n);
		const float du = p.u - fl[i], dv = p.v - fl[HW + i];
		go = gl * (fabsf(du) / (float)W + fabsf(dv) / (float)H) * (p.front ? 1.f : 0.f);
		const float gu = gl * sgn(du) * p.w / (float)W, gv = gl * sgn(dv) * p.w / (float)H;
		// u = px / z, v = py / z; z = max(pz, dist) passes the gradient where pz > dist (the weight is 0 elsewhere)
		const float gpx = gu / p.z, gpy = gv / p.z, gpz = -(gu * p.px + gv * p.py) / (p.z * p.z);
		gx = c.M[0] * gpx + c.M[3] * gpy + c.M[6] * gpz;
		gy = c.M[1] * gpx + c.M[4] * gpy + c.M[7] * gpz;
		gz = c.M[2] * gpx + c.M[5] * gpy + c.M[8] * gpz;
	}
	g_f[i] = gx; g_f[HW + i] = gy; g_f[2 * HW + i] = gz;
	if (g_op) g_op[i] = go;
}

// mean BCE of q = clip(pred, lo, hi) (or 1 - clip) against t = target (or target > 0): train.py:95-103
__device__ __forceinline__ float bce_target(float t, int positive) { return positive ? (t > 0.f ? 1.f : 0.f) : t; }
__device__ __forceinline__ float bce_value(float pred, float target, float lo, float hi, int invert, int positive) {
	const float c = fminf(fmaxf(pred, lo), hi);
	const float q = invert ? 1.0f - c : c;
	const float t = bce_target(target, positive);
	return -(t * fmaxf(logf(q), -100.f) + (1.f - t) * fmaxf(logf(1.f - q), -100.f));     // torch clamps the logs at -100
}
// d BCE / d pred: (q - t) / (q (1 - q)) with torch's eps-clamped denominator; clamp passes the gradient on [lo, hi]
__device__ __forceinline__ float bce_dpred(float x, float target, float lo, float hi, int invert, int positive, bool& inside) {
	const float c = fminf(fmaxf(x, lo), hi);
	const float q = invert ? 1.0f - c : c;
	const float t = bce_target(target, positive);
	const float dq = (q - t) / fmaxf(q * (1.f - q), 1e-12f);
	inside = x >= lo && x <= hi;
	return invert ? -dq : dq;
}
__global__ void __launch_bounds__(SLOT_THREADS) bce_clip_sum_kernel(int n, const float* __restrict__ pred, const float* __restrict__ target, float lo, float hi,
	int invert, int positive, double* __restrict__ work) {
	double sum = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
		sum += (double)bce_value(pred[i], target[i], lo, hi, invert, positive);
	double v[1] = { sum };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
	if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(work + 1, (double)n);      // the "count" of the shared finish kernel
}
__global__ void __launch_bounds__(256) bce_clip_bwd_kernel(int n, const float* __restrict__ pred, const float* __restrict__ target, float lo, float hi,
	int invert, int positive, const float* __restrict__ g_loss, float* __restrict__ out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	bool inside;
	const float d = bce_dpred(pred[i], target[i], lo, hi, invert, positive, inside);
	out[i] = inside ? g_loss[0] * d / (float)n : 0.f;
}
// the same with a per-element weight: sum w bce / sum w; the finish kernel's "count" is sum w, which the backward reads from the work buffer
__global__ void __launch_bounds__(SLOT_THREADS) bce_clip_weighted_sum_kernel(int n, const float* __restrict__ pred, const float* __restrict__ target,
	const float* __restrict__ weight, float lo, float hi, int invert, int positive, double* __restrict__ work) {
	double sum = 0, cnt = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const float w = weight[i];
		sum += (double)w * (double)bce_value(pred[i], target[i], lo, hi, invert, positive);
		cnt += (double)w;
	}
	double v[2] = { sum, cnt };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
}
__global__ void __launch_bounds__(256) bce_clip_weighted_bwd_kernel(int n, const float* __restrict__ pred, const float* __restrict__ target,
	const float* __restrict__ weight, float lo, float hi, int invert, int positive, const double* __restrict__ work, const float* __restrict__ g_loss,
	float* __restrict__ out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double sw = work[AUX_TOTALS + 1];
	bool inside;
	const float d = bce_dpred(pred[i], target[i], lo, hi, invert, positive, inside);
	out[i] = inside && sw > 0.0 ? g_loss[0] * weight[i] * d * (float)(1.0 / sw) : 0.f;
}

// ---------------------------------------------------------------- sparse metric depth (the lidar_depth/*.npz arrays of the preparation scripts)
// sum m |depth - target| / sum m over the pixels with m > 0 and lidar > 0; target = lidar, or 1 / lidar when inverse depth was rendered.
// No scale or shift is fitted.  Same aux work layout: (sum, sum m).
// the target and the residual in double: 1 / lidar next to a rendered inverse depth is a difference of close numbers
__device__ __forceinline__ bool lidar_residual(float depth, float lidar, float m, int inv_depth, double& r) {
	if (!(m > 0.f && lidar > 0.f)) return false;
	r = (double)depth - (inv_depth ? 1.0 / (double)lidar : (double)lidar);
	return true;
}
__global__ void __launch_bounds__(SLOT_THREADS) lidar_depth_sum_kernel(int n, const float* __restrict__ depth, const float* __restrict__ lidar, const float* __restrict__ mask,
	int inv_depth, double* __restrict__ work) {
	double sum = 0, cnt = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const float m = mask[i];
		double r;
		if (lidar_residual(depth[i], lidar[i], m, inv_depth, r)) { sum += (double)m * fabs(r); cnt += (double)m; }
	}
	double v[2] = { sum, cnt };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
}
__global__ void __launch_bounds__(256) lidar_depth_bwd_kernel(int n, const float* __restrict__ depth, const float* __restrict__ lidar, const float* __restrict__ mask,
	int inv_depth, const double* __restrict__ work, const float* __restrict__ g_loss, float* __restrict__ out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double sm = work[AUX_TOTALS + 1];
	const float m = mask[i];
	double r;
	float g = 0.f;
	if (lidar_residual(depth[i], lidar[i], m, inv_depth, r) && sm > 0.0)
		g = g_loss[0] * m * sgn(r) * (float)(1.0 / sm);
	out[i] = g;
}

} // namespace
} // namespace adgs

using namespace adgs;

// ---------------------------------------------------------------- neighbourhood regularisers (train.py:104-113)
//   reg_loss       = mean(sum(var(xyz_deform_param[obj_near_idx], dim=1), dim=-1))     rows of D = 3 C floats, inner = C
//   reg_sigma_loss = mean(sum(var(gs_time_sigma[obj_near_idx], dim=1), dim=-1))        rows of D = 2 floats,   inner = 2
//   sigma_loss     = mean(|frame_gap / mean(exp(gs_time_sigma), dim=-1)|)
// The reference gathers a [G, K, 3, C] copy of the rows (43 MB at C3), runs torch.var / sum / mean over it and scatters the
// gradient back through index_put.  Here one thread owns one (group, column) pair: it reads its K values straight from the K
// gathered rows (consecutive threads = consecutive columns of a row: coalesced), forms the unbiased variance in registers, and
// the backward adds 2 (x - mean) / ((K - 1) denom) to the K rows with one atomic each (a Gaussian can sit in several groups).
// Row indices follow the reference's fancy indexing (`param[obj_near_idx]`): a negative index counts from the end; anything outside
// [-N, N) raises IndexError there.  A kernel cannot raise without a host round trip, so an out-of-range index (a stale obj_near_idx from
// before a prune) makes the LOSS NaN -- and no out-of-bounds access -- and the rows of the affected GROUP receive no gradient (a NaN mean would
// otherwise reach every valid row of the group and, one Adam step later, the parameters and both moments for good).  The host wrapper
// (adgs.loss._GroupVar) validates every new index tensor once and raises IndexError like the reference.
constexpr int GV_MAXK = 32;
__device__ __forceinline__ long long gv_row(long long i, int N) { if (i < 0) i += N; return (i < 0 || i >= N) ? -1 : i; }
__global__ void __launch_bounds__(SLOT_THREADS) group_var_sum_kernel(int N, int G, int K, int D, const float* __restrict__ x, const long long* __restrict__ idx,
	double denom, double* __restrict__ work) {
	const long long total = (long long)G * D;
	double sum = 0;
	for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
		const int g = (int)(t / D), d = (int)(t % D);
		float v[GV_MAXK], mean = 0.f;
		for (int k = 0; k < K; k++) { const long long r = gv_row(idx[(size_t)g * K + k], N); v[k] = r < 0 ? __int_as_float(0x7fc00000) : x[(size_t)r * D + d]; mean += v[k]; }
		mean /= (float)K;
		float ss = 0.f;
		for (int k = 0; k < K; k++) { const float c = v[k] - mean; ss += c * c; }
		sum += (double)(ss / (float)(K - 1));
	}
	double v[1] = { sum };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
	if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(work + 1, denom);      // the "count" of the shared finish kernel
}
__global__ void __launch_bounds__(256) group_var_bwd_kernel(int N, int G, int K, int D, const float* __restrict__ x, const long long* __restrict__ idx,
	float scale, const float* __restrict__ g_loss, float* __restrict__ dx) {
	const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= (long long)G * D) return;
	const int g = (int)(t / D), d = (int)(t % D);
	float v[GV_MAXK], mean = 0.f; long long row[GV_MAXK];
	for (int k = 0; k < K; k++) { row[k] = gv_row(idx[(size_t)g * K + k], N); v[k] = row[k] < 0 ? __int_as_float(0x7fc00000) : x[(size_t)row[k] * D + d]; mean += v[k]; }
	mean /= (float)K;
	const float c = scale * g_loss[0];
	bool valid = true;
	for (int k = 0; k < K; k++) valid = valid && row[k] >= 0;
	if (!valid) return;          // a group with an out-of-range index has no defined variance: its rows receive NO gradient (never NaN) -- the forward's loss is NaN
	for (int k = 0; k < K; k++) atomicAdd(dx + (size_t)row[k] * D + d, c * (v[k] - mean));
}
__global__ void __launch_bounds__(SLOT_THREADS) sigma_loss_sum_kernel(int N, const float* __restrict__ ls, float gap, double* __restrict__ work) {
	double sum = 0;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
		const float m = 0.5f * (expf(ls[2 * i]) + expf(ls[2 * i + 1]));
		sum += (double)fabsf(gap / m);
	}
	double v[1] = { sum };
	slot_add_wave<ADGS_LOSS_SLOTS, AUX_ROW>(work, v);
	if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(work + 1, (double)N);
}
__global__ void __launch_bounds__(256) sigma_loss_bwd_kernel(int N, const float* __restrict__ ls, float gap, const float* __restrict__ g_loss, float* __restrict__ d) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= N) return;
	const float e0 = expf(ls[2 * i]), e1 = expf(ls[2 * i + 1]);
	const float m = 0.5f * (e0 + e1), q = gap / m;
	const float c = -sgn(q) * q / m * 0.5f * g_loss[0] / (float)N;          // d|q|/dm = -sgn q / m;  dm/ds_j = e_j / 2
	d[2 * i] = c * e0; d[2 * i + 1] = c * e1;
}

extern "C" int adgs_depth_loss_forward(int n, const float* prediction, const float* target, const float* mask, double* work, float* loss, void* stream_) {
	if (n <= 0) return 0;
	if (!prediction || !target || !work || !loss) { set_error("adgs_depth_loss_forward: NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const unsigned blocks = reduce_blocks(n);
	hipLaunchKernelGGL(depth_sums_kernel, dim3(blocks), dim3(SLOT_THREADS), 0, stream, n, prediction, target, mask, work);
	hipLaunchKernelGGL(depth_solve_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work);
	hipLaunchKernelGGL(depth_l1_kernel, dim3(blocks), dim3(SLOT_THREADS), 0, stream, n, prediction, target, mask, work);
	hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_depth_loss_backward(int n, const float* prediction, const float* target, const float* mask, const double* work, const float* g_loss,
	float* dL_dprediction, void* stream_) {
	if (n <= 0) return 0;
	if (!prediction || !target || !work || !g_loss || !dL_dprediction) { set_error("adgs_depth_loss_backward: NULL pointer"); return -1; }
	hipLaunchKernelGGL(depth_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, n, prediction, target, mask, work, g_loss, dL_dprediction);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_l1_ssim_forward(int planes, int H, int W, const float* image, const float* gt, double* sums,
	float* d_mu1, float* d_e11, float* d_e12, void* stream) {
	if (planes <= 0 || H <= 0 || W <= 0) return 0;
	if (!image || !gt || !sums) { set_error("adgs_l1_ssim_forward: NULL image / gt / sums"); return -1; }
	if ((d_mu1 != nullptr) != (d_e11 != nullptr) || (d_mu1 != nullptr) != (d_e12 != nullptr)) { set_error("adgs_l1_ssim_forward: pass all three derivative maps or none"); return -1; }
	if (planes > 65535) { set_error("adgs_l1_ssim_forward: more than 65535 planes"); return -1; }
	static const Window win = make_window();
	const dim3 grid((W + TSX - 1) / TSX, (H + TSY - 1) / TSY, planes);
	hipLaunchKernelGGL(l1_ssim_fwd_kernel<false>, grid, dim3(LT), 0, (hipStream_t)stream, H, W, image, gt, (const float*)nullptr, win, sums, d_mu1, d_e11, d_e12);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

// means of the two sums of adgs_l1_ssim_forward: out2 = (sum |image - gt|, sum ssim_map) / n; the slot rows are consumed (zero afterwards)
namespace {
__global__ void __launch_bounds__(SLOT_THREADS) l1_ssim_finish_kernel(double* __restrict__ sums, double inv_n, float* __restrict__ out2) {
	double t[2];
	slot_finish<ADGS_LOSS_SLOTS, 2>(sums, t);
	if (threadIdx.x == 0) { out2[0] = (float)(t[0] * inv_n); out2[1] = (float)(t[1] * inv_n); }
}
}
extern "C" int adgs_l1_ssim_means(double* sums, long long n, float* out2, void* stream) {
	if (!sums || !out2) { set_error("adgs_l1_ssim_means: NULL pointer"); return -1; }
	hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, (hipStream_t)stream, sums, 1.0 / (double)std::max<long long>(n, 1), out2);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_l1_ssim_backward(int planes, int H, int W, const float* image, const float* gt,
	const float* d_mu1, const float* d_e11, const float* d_e12, const float* g_l1, const float* g_ssim, float* dL_dimage, void* stream) {
	if (planes <= 0 || H <= 0 || W <= 0) return 0;
	if (!image || !gt || !d_mu1 || !d_e11 || !d_e12 || !dL_dimage) { set_error("adgs_l1_ssim_backward: NULL pointer"); return -1; }
	if (planes > 65535) { set_error("adgs_l1_ssim_backward: more than 65535 planes"); return -1; }
	static const Window win = make_window();
	const dim3 grid((W + TSX - 1) / TSX, (H + TSY - 1) / TSY, planes);
	const float inv_n = (float)(1.0 / ((double)planes * H * W));
	hipLaunchKernelGGL(l1_ssim_bwd_kernel<false>, grid, dim3(LT), 0, (hipStream_t)stream, H, W, image, gt, (const float*)nullptr, (const double*)nullptr, win, d_mu1, d_e11, d_e12,
		g_l1, g_ssim, inv_n, dL_dimage);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

// ---------------------------------------------------------------- the weighted forms (include/adgs_loss.h)
namespace {
// totals of the three sums -> work[3 * SLOTS ..] = (sum w |d|, sum w ssim, sum w); out2 = the first two over planes * sum w, 0 when sum w = 0
__global__ void __launch_bounds__(SLOT_THREADS) l1_ssim_weighted_finish_kernel(double* __restrict__ work, double planes, float* __restrict__ out2) {
	double t[3];
	slot_finish<ADGS_LOSS_SLOTS, 3>(work, t);
	if (threadIdx.x == 0) {
		double* tot = work + 3 * ADGS_LOSS_SLOTS;
		for (int q = 0; q < 3; q++) tot[q] = t[q];
		const double n = planes * tot[2];
		out2[0] = tot[2] > 0 ? (float)(tot[0] / n) : 0.f; out2[1] = tot[2] > 0 ? (float)(tot[1] / n) : 0.f;
	}
}
}
extern "C" int adgs_l1_ssim_weighted_forward(int planes, int H, int W, const float* image, const float* gt, const float* weight, double* work,
	float* d_mu1, float* d_e11, float* d_e12, float* out2, void* stream) {
	if (planes <= 0 || H <= 0 || W <= 0) return 0;
	if (!image || !gt || !weight || !work || !out2) { set_error("adgs_l1_ssim_weighted_forward: NULL image / gt / weight / work / out2"); return -1; }
	if ((d_mu1 != nullptr) != (d_e11 != nullptr) || (d_mu1 != nullptr) != (d_e12 != nullptr)) { set_error("adgs_l1_ssim_weighted_forward: pass all three derivative maps or none"); return -1; }
	if (planes > 65535) { set_error("adgs_l1_ssim_weighted_forward: more than 65535 planes"); return -1; }
	static_assert(ADGS_L1_SSIM_WEIGHTED_WORK_DOUBLES >= 3 * ADGS_LOSS_SLOTS + 3, "three totals behind the rows");
	static const Window win = make_window();
	const dim3 grid((W + TSX - 1) / TSX, (H + TSY - 1) / TSY, planes);
	hipLaunchKernelGGL(l1_ssim_fwd_kernel<true>, grid, dim3(LT), 0, (hipStream_t)stream, H, W, image, gt, weight, win, work, d_mu1, d_e11, d_e12);
	hipLaunchKernelGGL(l1_ssim_weighted_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, (hipStream_t)stream, work, (double)planes, out2);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_l1_ssim_weighted_backward(int planes, int H, int W, const float* image, const float* gt, const float* weight,
	const float* d_mu1, const float* d_e11, const float* d_e12, const double* work, const float* g_l1, const float* g_ssim, float* dL_dimage, void* stream) {
	if (planes <= 0 || H <= 0 || W <= 0) return 0;
	if (!image || !gt || !weight || !d_mu1 || !d_e11 || !d_e12 || !work || !dL_dimage) { set_error("adgs_l1_ssim_weighted_backward: NULL pointer"); return -1; }
	if (planes > 65535) { set_error("adgs_l1_ssim_weighted_backward: more than 65535 planes"); return -1; }
	static const Window win = make_window();
	const dim3 grid((W + TSX - 1) / TSX, (H + TSY - 1) / TSY, planes);
	hipLaunchKernelGGL(l1_ssim_bwd_kernel<true>, grid, dim3(LT), 0, (hipStream_t)stream, H, W, image, gt, weight, work + 3 * ADGS_LOSS_SLOTS, win, d_mu1, d_e11, d_e12,
		g_l1, g_ssim, 0.f, dL_dimage);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_bce_clip_weighted_forward(int n, const float* pred, const float* target, const float* weight, float lo, float hi, int invert, int positive_target,
	double* work, float* loss, void* stream_) {
	if (n <= 0) return 0;
	if (!pred || !target || !weight || !work || !loss) { set_error("adgs_bce_clip_weighted_forward: NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(bce_clip_weighted_sum_kernel, dim3(reduce_blocks(n)), dim3(SLOT_THREADS), 0, stream, n, pred, target, weight, lo, hi, invert, positive_target, work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_bce_clip_weighted_backward(int n, const float* pred, const float* target, const float* weight, float lo, float hi, int invert, int positive_target,
	const double* work, const float* g_loss, float* dL_dpred, void* stream_) {
	if (n <= 0) return 0;
	if (!pred || !target || !weight || !work || !g_loss || !dL_dpred) { set_error("adgs_bce_clip_weighted_backward: NULL pointer"); return -1; }
	hipLaunchKernelGGL(bce_clip_weighted_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, n, pred, target, weight, lo, hi, invert, positive_target,
		work, g_loss, dL_dpred);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_lidar_depth_loss_forward(int n, const float* depth, const float* lidar_depth, const float* lidar_mask, int inv_depth, double* work, float* loss,
	void* stream_) {
	if (n <= 0) return 0;
	if (!depth || !lidar_depth || !lidar_mask || !work || !loss) { set_error("adgs_lidar_depth_loss_forward: NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(lidar_depth_sum_kernel, dim3(reduce_blocks(n)), dim3(SLOT_THREADS), 0, stream, n, depth, lidar_depth, lidar_mask, inv_depth, work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_lidar_depth_loss_backward(int n, const float* depth, const float* lidar_depth, const float* lidar_mask, int inv_depth, const double* work,
	const float* g_loss, float* dL_ddepth, void* stream_) {
	if (n <= 0) return 0;
	if (!depth || !lidar_depth || !lidar_mask || !work || !g_loss || !dL_ddepth) { set_error("adgs_lidar_depth_loss_backward: NULL pointer"); return -1; }
	hipLaunchKernelGGL(lidar_depth_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, n, depth, lidar_depth, lidar_mask, inv_depth, work, g_loss, dL_ddepth);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

static FlowCam make_flow_cam(const float* K, const float* R, const float* T, float dist) {
	FlowCam c;
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++) c.M[3 * i + j] = K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j] + K[3 * i + 2] * R[6 + j];
		c.KT[i] = K[3 * i] * T[0] + K[3 * i + 1] * T[1] + K[3 * i + 2] * T[2];
	}
	c.dist = dist;
	return c;
}
static int flow_loss_forward_impl(const char* who, bool dev_cam, int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, double* work, float* loss, void* stream_) {
	if (H <= 0 || W <= 0) return 0;
	if (!img_flow || !flow || !flow_vis || !K || !R || !T || !work || !loss) { set_error(std::string(who) + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const int n = H * W;
	FlowCam c; FlowCamDev cd{nullptr, nullptr, nullptr};
	if (dev_cam) { c = FlowCam{}; c.dist = dist; cd = FlowCamDev{K, R, T}; } else c = make_flow_cam(K, R, T, dist);
	hipLaunchKernelGGL(flow_loss_sum_kernel, dim3(reduce_blocks(n)), dim3(SLOT_THREADS), 0, stream, H, W, img_flow, flow, flow_vis, img_opacity, c, cd, work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
static int flow_loss_backward_impl(const char* who, bool dev_cam, int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, const double* work, const float* g_loss, float* dL_dimg_flow, float* dL_dimg_opacity,
	void* stream_) {
	if (H <= 0 || W <= 0) return 0;
	if (!img_flow || !flow || !flow_vis || !K || !R || !T || !work || !g_loss || !dL_dimg_flow) { set_error(std::string(who) + ": NULL pointer"); return -1; }
	const int n = H * W;
	FlowCam c; FlowCamDev cd{nullptr, nullptr, nullptr};
	if (dev_cam) { c = FlowCam{}; c.dist = dist; cd = FlowCamDev{K, R, T}; } else c = make_flow_cam(K, R, T, dist);
	hipLaunchKernelGGL(flow_loss_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, H, W, img_flow, flow, flow_vis, img_opacity,
		c, cd, work, g_loss, dL_dimg_flow, dL_dimg_opacity);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_flow_loss_forward(int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, double* work, float* loss, void* stream) {
	return flow_loss_forward_impl("adgs_flow_loss_forward", false, H, W, img_flow, flow, flow_vis, img_opacity, K, R, T, dist, work, loss, stream);
}
extern "C" int adgs_flow_loss_forward_devcam(int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, double* work, float* loss, void* stream) {
	return flow_loss_forward_impl("adgs_flow_loss_forward_devcam", true, H, W, img_flow, flow, flow_vis, img_opacity, K, R, T, dist, work, loss, stream);
}
extern "C" int adgs_flow_loss_backward(int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, const double* work, const float* g_loss, float* dL_dimg_flow, float* dL_dimg_opacity,
	void* stream) {
	return flow_loss_backward_impl("adgs_flow_loss_backward", false, H, W, img_flow, flow, flow_vis, img_opacity, K, R, T, dist, work, g_loss, dL_dimg_flow,
		dL_dimg_opacity, stream);
}
extern "C" int adgs_flow_loss_backward_devcam(int H, int W, const float* img_flow, const float* flow, const float* flow_vis, const float* img_opacity,
	const float* K, const float* R, const float* T, float dist, const double* work, const float* g_loss, float* dL_dimg_flow, float* dL_dimg_opacity,
	void* stream) {
	return flow_loss_backward_impl("adgs_flow_loss_backward_devcam", true, H, W, img_flow, flow, flow_vis, img_opacity, K, R, T, dist, work, g_loss, dL_dimg_flow,
		dL_dimg_opacity, stream);
}
extern "C" int adgs_bce_clip_forward(int n, const float* pred, const float* target, float lo, float hi, int invert, int positive_target,
	double* work, float* loss, void* stream_) {
	if (n <= 0) return 0;
	if (!pred || !target || !work || !loss) { set_error("adgs_bce_clip_forward: NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(bce_clip_sum_kernel, dim3(reduce_blocks(n)), dim3(SLOT_THREADS), 0, stream, n, pred, target, lo, hi, invert, positive_target, work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_bce_clip_backward(int n, const float* pred, const float* target, float lo, float hi, int invert, int positive_target,
	const float* g_loss, float* dL_dpred, void* stream_) {
	if (n <= 0) return 0;
	if (!pred || !target || !g_loss || !dL_dpred) { set_error("adgs_bce_clip_backward: NULL pointer"); return -1; }
	hipLaunchKernelGGL(bce_clip_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, n, pred, target, lo, hi, invert, positive_target, g_loss, dL_dpred);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_group_var_forward(int N, int G, int K, int D, int inner, const float* x, const int64_t* idx, double* work, float* loss, void* stream_) {
	if (G <= 0 || D <= 0) return 0;
	if (!x || !idx || !work || !loss) { set_error("adgs_group_var_forward: NULL pointer"); return -1; }
	if (K < 2 || K > GV_MAXK || inner <= 0 || D % inner != 0 || N <= 0) { set_error("adgs_group_var_forward: needs 2 <= K <= 32 neighbours and D a multiple of inner"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const long long total = (long long)G * D;
	hipLaunchKernelGGL(group_var_sum_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(SLOT_THREADS), 0, stream, N, G, K, D, x,
		reinterpret_cast<const long long*>(idx), (double)G * (double)(D / inner), work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_group_var_backward(int N, int G, int K, int D, int inner, const float* x, const int64_t* idx, const float* g_loss, float* dL_dx, void* stream_) {
	if (G <= 0 || D <= 0) return 0;
	if (!x || !idx || !g_loss || !dL_dx) { set_error("adgs_group_var_backward: NULL pointer"); return -1; }
	if (K < 2 || K > GV_MAXK || inner <= 0 || D % inner != 0 || N <= 0) { set_error("adgs_group_var_backward: needs 2 <= K <= 32 neighbours and D a multiple of inner"); return -1; }
	const long long total = (long long)G * D;
	const float scale = (float)(2.0 / ((double)(K - 1) * (double)G * (double)(D / inner)));
	hipLaunchKernelGGL(group_var_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, N, G, K, D, x,
		reinterpret_cast<const long long*>(idx), scale, g_loss, dL_dx);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_sigma_loss_forward(int N, const float* log_sigma, float frame_gap, double* work, float* loss, void* stream_) {
	if (N <= 0) return 0;
	if (!log_sigma || !work || !loss) { set_error("adgs_sigma_loss_forward: NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(sigma_loss_sum_kernel, dim3(reduce_blocks(N)), dim3(SLOT_THREADS), 0, stream, N, log_sigma, frame_gap, work);
	hipLaunchKernelGGL(aux_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
extern "C" int adgs_sigma_loss_backward(int N, const float* log_sigma, float frame_gap, const float* g_loss, float* dL_dlog_sigma, void* stream_) {
	if (N <= 0) return 0;
	if (!log_sigma || !g_loss || !dL_dlog_sigma) { set_error("adgs_sigma_loss_backward: NULL pointer"); return -1; }
	hipLaunchKernelGGL(sigma_loss_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream_, N, log_sigma, frame_gap, g_loss, dL_dlog_sigma);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
