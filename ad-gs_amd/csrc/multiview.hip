// Multi-view photometric consistency (plane-warped patch NCC), forward and backward, for gfx950 (wave64).
// The definition is in include/adgs_multiview.h.
//
// One wave per sample, SLOT_THREADS / 64 samples per workgroup and round, lane k = tap k of the (2 r + 1)^2 <= 49 taps; lanes >= T are idle
// and contribute zeros.  Everything that belongs to the sample (index, D, O, N, the plane) is read at a wave-uniform address and is the
// same in every lane, so the gates before the taps end the whole wave's work on the sample; "every tap" is __all.  The per-tap chain and
// the five sums are double (the inputs are exact floats): sum a^2 - Sa^2 / T cancels on low-texture patches.  The volume is S T taps, a
// few million double operations per call: the pass is bound by its gathers (T reads of I_r, 4 T of I_n per sample), not by the fp64 rate.
// Forward: the wave's lane 0 holds (w v e, w v); slot_add_block adds the workgroup's sums to its slot row with one atomic per sum, the
// finish kernel stores the totals and L behind the rows.
// Backward: the same evaluation again, then per lane  g_k = de/db_k (grad I_n . d(u, v)/dm t)  = de/ds_k and four wave sums
// (sum g s, sum g r(q).x, sum g r(q).y, sum g); lane 0 chains through s_k = (Nh . r(q)) / (z c0), the normalisation and z and adds the five
// floats atomically into the maps the entry has zero-filled.
//
// Byte model (HBM, an upper bound: neighbouring samples share lines): forward S (4 + 24 + [4] + 4 T + 16 T) bytes read; backward the
// same plus the zero fill and 20 S bytes of atomics.
#include "common.h"
#include "slot_reduce.h"
#include "../../include/adgs_loss.h"
#include "../../include/adgs_multiview.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

constexpr int MV_ROW = 2;                                       // doubles per slot row
constexpr int MV_WAVES = SLOT_THREADS / WAVE;                   // samples per workgroup and round
constexpr unsigned MV_MAX_BLOCKS = 2048;                        // beyond that a wave strides over the samples
static_assert(ADGS_MULTIVIEW_WORK_DOUBLES >= ADGS_LOSS_SLOTS * MV_ROW + 3, "three scalars behind the rows");
static_assert((2 * ADGS_MULTIVIEW_MAX_RADIUS + 1) * (2 * ADGS_MULTIVIEW_MAX_RADIUS + 1) <= WAVE, "one tap per lane");
enum { MV_SVE = 0, MV_SV, MV_L };                              // the scalars behind the rows: sum w v e, sum w v, L

struct MvView {
	int H, W, Hn, Wn;
	int radius, side, T;    // side = 2 radius + 1, T = side^2
	int inv_depth;
	double tx, ty;          // tanfovx, tanfovy of the reference
	double ku, kv;          // Wn / (2 tanfovx_n), Hn / (2 tanfovy_n)
	double cu, cv;          // (Wn - 1) / 2, (Hn - 1) / 2
	double R[9], t[3];
	double min_cos, max_error, eps;
	float min_opacity;
};

// What a wave knows of its sample after the gates before the error: the first block is the same in every lane, the second is the lane's tap.
struct MvSample {
	double D, O, z, rho, nh[3], r0x, r0y, c0;
	double Sa, Sb, C, Va, Vb, den, e;
	bool on;                // lane < T
	double a, b, s, rqx, rqy;
	double mx, my, mz;      // mx / mz, my / mz, mz
	double gu, gv;          // the gradient of the bilinear sample
};

__device__ __forceinline__ double mv_ray_x(const MvView& v, int gx) { return ((2.0 * (double)gx + 1.0) / (double)v.W - 1.0) * v.tx; }
__device__ __forceinline__ double mv_ray_y(const MvView& v, int gy) { return ((2.0 * (double)gy + 1.0) / (double)v.H - 1.0) * v.ty; }

// Evaluates sample `idx` (wave-uniform) up to e.  false: one of the gates before the error fails (the same answer in every lane); nothing
// outside the two images is read.
__device__ __forceinline__ bool mv_eval(const MvView& v, const float* __restrict__ normal, const float* __restrict__ depth, const float* __restrict__ opacity,
	const float* __restrict__ ref_gray, const float* __restrict__ nbr_gray, int idx, int lane, MvSample& o) {
	const int HW = v.H * v.W;                                   // <= INT_MAX
	if (idx < 0 || idx >= HW) return false;
	const int y0 = idx / v.W, x0 = idx - y0 * v.W;
	const int r = v.radius;
	if (x0 < r || x0 >= v.W - r || y0 < r || y0 >= v.H - r) return false;
	const float Of = opacity[idx], Df = depth[idx];
	if (!(Of >= v.min_opacity) || !(Df > 0.f)) return false;
	const double n0 = normal[idx], n1 = normal[(size_t)HW + idx], n2 = normal[2 * (size_t)HW + idx];
	o.D = Df; o.O = Of;
	o.rho = sqrt(n0 * n0 + n1 * n1 + n2 * n2 + 1e-12);
	o.nh[0] = n0 / o.rho; o.nh[1] = n1 / o.rho; o.nh[2] = n2 / o.rho;
	o.r0x = mv_ray_x(v, x0); o.r0y = mv_ray_y(v, y0);
	o.c0 = o.nh[0] * o.r0x + o.nh[1] * o.r0y + o.nh[2];
	if (!(-o.c0 >= v.min_cos * sqrt(o.r0x * o.r0x + o.r0y * o.r0y + 1.0))) return false;        // c0 < 0 from here on
	o.z = v.inv_depth ? o.O / o.D : o.D / o.O;
	// the lane's tap
	o.on = lane < v.T;
	const int k = o.on ? lane : 0;
	const int ky = k / v.side, kx = k - ky * v.side;
	const int qx = x0 + kx - r, qy = y0 + ky - r;               // inside the reference image
	o.rqx = mv_ray_x(v, qx); o.rqy = mv_ray_y(v, qy);
	o.s = (o.nh[0] * o.rqx + o.nh[1] * o.rqy + o.nh[2]) / (o.z * o.c0);
	const double m0 = v.R[0] * o.rqx + v.R[1] * o.rqy + v.R[2] + v.t[0] * o.s;
	const double m1 = v.R[3] * o.rqx + v.R[4] * o.rqy + v.R[5] + v.t[1] * o.s;
	o.mz = v.R[6] * o.rqx + v.R[7] * o.rqy + v.R[8] + v.t[2] * o.s;
	bool ok = o.mz > 1e-6;
	o.mx = m0 / o.mz; o.my = m1 / o.mz;
	const double pu = o.mx * v.ku + v.cu, pv = o.my * v.kv + v.cv;
	ok = ok && pu >= 0.0 && pu <= (double)(v.Wn - 1) && pv >= 0.0 && pv <= (double)(v.Hn - 1);      // false for NaN
	if (!__all(!o.on || ok)) return false;
	// the bilinear sample: (pu, pv) lies inside the neighbour's image in every lane that is on; lane >= T repeats tap 0
	const int xi = min(max((int)floor(pu), 0), max(v.Wn - 2, 0)), yi = min(max((int)floor(pv), 0), max(v.Hn - 2, 0));
	const int x1 = min(xi + 1, v.Wn - 1), y1 = min(yi + 1, v.Hn - 1);
	const double fx = pu - (double)xi, fy = pv - (double)yi;
	const double i00 = nbr_gray[(size_t)yi * v.Wn + xi], i01 = nbr_gray[(size_t)yi * v.Wn + x1];
	const double i10 = nbr_gray[(size_t)y1 * v.Wn + xi], i11 = nbr_gray[(size_t)y1 * v.Wn + x1];
	const double a = ref_gray[(size_t)qy * v.W + qx];
	const double top = i00 + fx * (i01 - i00), bot = i10 + fx * (i11 - i10);
	o.gu = (1.0 - fy) * (i01 - i00) + fy * (i11 - i10);
	o.gv = bot - top;
	o.a = o.on ? a : 0.0;
	o.b = o.on ? top + fy * (bot - top) : 0.0;
	double sums[5] = { o.a, o.b, o.a * o.b, o.a * o.a, o.b * o.b };
	wave_sum(sums);
	const double T = (double)v.T;
	o.Sa = sums[0]; o.Sb = sums[1];
	o.C = sums[2] - o.Sa * o.Sb / T;
	o.Va = sums[3] - o.Sa * o.Sa / T;
	o.Vb = sums[4] - o.Sb * o.Sb / T;
	o.den = o.Va * o.Vb + v.eps;
	o.e = 1.0 - o.C * o.C / o.den;
	return true;
}

__global__ void __launch_bounds__(SLOT_THREADS) multiview_ncc_fwd_kernel(MvView v, const float* __restrict__ normal, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ ref_gray, const float* __restrict__ nbr_gray, const float* __restrict__ weight,
	const int32_t* __restrict__ samples, int S, double* __restrict__ work, float* __restrict__ e_out, uint8_t* __restrict__ valid_out) {
	const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	double acc[MV_ROW] = { 0.0, 0.0 };                          // sum w v e, sum w v: in lane 0 of every wave
	for (long long s = (long long)blockIdx.x * MV_WAVES + wave; s < (long long)S; s += (long long)gridDim.x * MV_WAVES) {
		const int idx = __builtin_amdgcn_readfirstlane(samples[s]);
		MvSample o;
		const bool geo = mv_eval(v, normal, depth, opacity, ref_gray, nbr_gray, idx, lane, o);
		const bool valid = geo && o.e < v.max_error;
		if (lane == 0) {
			if (valid) {
				const double w = weight ? (double)weight[idx] : 1.0;
				acc[MV_SVE] += w * o.e; acc[MV_SV] += w;
			}
			if (e_out) e_out[s] = geo ? (float)o.e : 0.f;
			if (valid_out) valid_out[s] = valid ? 1 : 0;
		}
	}
	slot_add_block<ADGS_LOSS_SLOTS, MV_ROW, SLOT_THREADS>(work, acc);
}

// one block: totals of the slot rows (left zero) -> the scalars behind them and the loss
__global__ void __launch_bounds__(SLOT_THREADS) multiview_ncc_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double t[MV_ROW];
	slot_finish<ADGS_LOSS_SLOTS, MV_ROW>(work, t);
	if (threadIdx.x == 0) {
		double* tot = work + (size_t)ADGS_LOSS_SLOTS * MV_ROW;
		for (int q = 0; q < MV_ROW; q++) tot[q] = t[q];
		const double L = tot[MV_SV] > 0.0 ? tot[MV_SVE] / tot[MV_SV] : 0.0;
		tot[MV_L] = L;
		loss[0] = (float)L;
	}
}

__global__ void __launch_bounds__(SLOT_THREADS) multiview_ncc_bwd_kernel(MvView v, const float* __restrict__ normal, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ ref_gray, const float* __restrict__ nbr_gray, const float* __restrict__ weight,
	const int32_t* __restrict__ samples, int S, const double* __restrict__ work, const float* __restrict__ g_loss,
	float* __restrict__ dL_dnormal, float* __restrict__ dL_ddepth, float* __restrict__ dL_dopacity) {
	const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	const double sum_v = work[(size_t)ADGS_LOSS_SLOTS * MV_ROW + MV_SV];
	const double gs = sum_v > 0.0 ? (double)g_loss[0] / sum_v : 0.0;
	if (gs == 0.0) return;                                      // the maps are zero already
	const size_t plane = (size_t)v.H * v.W;
	for (long long s = (long long)blockIdx.x * MV_WAVES + wave; s < (long long)S; s += (long long)gridDim.x * MV_WAVES) {
		const int idx = __builtin_amdgcn_readfirstlane(samples[s]);
		MvSample o;
		if (!mv_eval(v, normal, depth, opacity, ref_gray, nbr_gray, idx, lane, o)) continue;
		if (!(o.e < v.max_error)) continue;
		const double ge = gs * (weight ? (double)weight[idx] : 1.0);       // dL/de of this sample
		if (ge == 0.0) continue;
		const double T = (double)v.T;
		// de/db_k through C and Vb, then db_k/ds_k = grad I_n . d(u, v)/dm . t
		const double de_db = -(2.0 * o.C * (o.a - o.Sa / T) / o.den - o.C * o.C * o.Va * 2.0 * (o.b - o.Sb / T) / (o.den * o.den));
		const double db_ds = (o.gu * v.ku * (v.t[0] - o.mx * v.t[2]) + o.gv * v.kv * (v.t[1] - o.my * v.t[2])) / o.mz;
		const double g = o.on ? de_db * db_ds : 0.0;
		double G[4] = { g * o.s, g * o.rqx, g * o.rqy, g };
		wave_sum(G);
		if (lane != 0) continue;
		// s_k = (Nh . r(q)) / (z c0), c0 = Nh . r0:  ds_k/dz = -s_k / z,  ds_k/dNh = r(q) / (z c0) - s_k r0 / c0
		const double gz = -ge * G[0] / o.z;
		const double zc = o.z * o.c0;
		const double gh[3] = { ge * (G[1] / zc - G[0] * o.r0x / o.c0), ge * (G[2] / zc - G[0] * o.r0y / o.c0), ge * (G[3] / zc - G[0] / o.c0) };
		if (dL_dnormal) {                                           // Nh = N / rho: (I - Nh Nh^T) / rho
			const double along = o.nh[0] * gh[0] + o.nh[1] * gh[1] + o.nh[2] * gh[2];
			atomicAdd(dL_dnormal + idx, (float)((gh[0] - o.nh[0] * along) / o.rho));
			atomicAdd(dL_dnormal + plane + idx, (float)((gh[1] - o.nh[1] * along) / o.rho));
			atomicAdd(dL_dnormal + 2 * plane + idx, (float)((gh[2] - o.nh[2] * along) / o.rho));
		}
		if (dL_ddepth) atomicAdd(dL_ddepth + idx, (float)(v.inv_depth ? -gz * o.O / (o.D * o.D) : gz / o.O));
		if (dL_dopacity) atomicAdd(dL_dopacity + idx, (float)(v.inv_depth ? gz / o.D : -gz * o.D / (o.O * o.O)));
	}
}

bool mv_positive(float x) { return std::isfinite(x) && x > 0.f; }
bool mv_unit(float x) { return std::isfinite(x) && x > 0.f && x <= 1.f; }

// 0: launch with `v`; 1: nothing to do; -1: refused
int mv_check(const char* who, const adgs_multiview_desc* d, bool null_pointer, int S, MvView& v) {
	const std::string name(who);
	if (!d || null_pointer) { set_error(name + ": NULL pointer"); return -1; }
	if (d->struct_bytes < (int)sizeof(adgs_multiview_desc)) { set_error(name + ": struct_bytes is smaller than adgs_multiview_desc"); return -1; }
	if (d->H < 0 || d->W < 0 || d->Hn < 0 || d->Wn < 0) { set_error(name + ": negative H, W, Hn or Wn"); return -1; }
	if ((long long)d->H * d->W > (long long)INT_MAX || (long long)d->Hn * d->Wn > (long long)INT_MAX) { set_error(name + ": H * W or Hn * Wn exceeds INT_MAX"); return -1; }
	if (S < 0) { set_error(name + ": negative S"); return -1; }
	if (d->radius < 1 || d->radius > ADGS_MULTIVIEW_MAX_RADIUS) { set_error(name + ": radius must be 1, 2 or 3"); return -1; }
	if (!mv_positive(d->tanfovx) || !mv_positive(d->tanfovy) || !mv_positive(d->tanfovx_n) || !mv_positive(d->tanfovy_n)) {
		set_error(name + ": the four tanfov values must be finite and > 0"); return -1;
	}
	if (!mv_unit(d->min_opacity)) { set_error(name + ": min_opacity must lie in (0, 1]"); return -1; }
	if (!mv_unit(d->min_cos)) { set_error(name + ": min_cos must lie in (0, 1]"); return -1; }
	if (!mv_unit(d->max_error)) { set_error(name + ": max_error must lie in (0, 1]"); return -1; }
	if (!mv_positive(d->eps)) { set_error(name + ": eps must be finite and > 0"); return -1; }
	for (int i = 0; i < 12; i++)
		if (!std::isfinite(d->pose[i])) { set_error(name + ": the pose must be finite"); return -1; }
	if (S == 0 || d->H == 0 || d->W == 0 || d->Hn == 0 || d->Wn == 0) return 1;
	v.H = d->H; v.W = d->W; v.Hn = d->Hn; v.Wn = d->Wn;
	v.radius = d->radius; v.side = 2 * d->radius + 1; v.T = v.side * v.side;
	v.inv_depth = d->inv_depth ? 1 : 0;
	v.tx = (double)d->tanfovx; v.ty = (double)d->tanfovy;
	v.ku = (double)d->Wn / (2.0 * (double)d->tanfovx_n); v.kv = (double)d->Hn / (2.0 * (double)d->tanfovy_n);
	v.cu = 0.5 * (double)(d->Wn - 1); v.cv = 0.5 * (double)(d->Hn - 1);
	for (int i = 0; i < 9; i++) v.R[i] = (double)d->pose[i];
	for (int i = 0; i < 3; i++) v.t[i] = (double)d->pose[9 + i];
	v.min_cos = (double)d->min_cos; v.max_error = (double)d->max_error; v.eps = (double)d->eps;
	v.min_opacity = d->min_opacity;
	return 0;
}

unsigned mv_blocks(int S) { return (unsigned)std::min<long long>(((long long)S + MV_WAVES - 1) / MV_WAVES, (long long)MV_MAX_BLOCKS); }

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_multiview_ncc_forward(const adgs_multiview_desc* desc, const float* normal, const float* depth, const float* opacity,
	const float* ref_gray, const float* nbr_gray, const float* weight, const int32_t* samples, int S, double* work, float* loss,
	float* e_out, uint8_t* valid_out, void* stream_) {
	MvView v;
	const int c = mv_check("adgs_multiview_ncc_forward", desc, !normal || !depth || !opacity || !ref_gray || !nbr_gray || !samples || !work || !loss, S, v);
	if (c) return c < 0 ? -1 : 0;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(multiview_ncc_fwd_kernel, dim3(mv_blocks(S)), dim3(SLOT_THREADS), 0, stream, v, normal, depth, opacity, ref_gray, nbr_gray, weight,
		samples, S, work, e_out, valid_out);
	hipLaunchKernelGGL(multiview_ncc_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_multiview_ncc_backward(const adgs_multiview_desc* desc, const float* normal, const float* depth, const float* opacity,
	const float* ref_gray, const float* nbr_gray, const float* weight, const int32_t* samples, int S, const double* work,
	const float* g_loss, float* dL_dnormal, float* dL_ddepth, float* dL_dopacity, void* stream_) {
	MvView v;
	const int c = mv_check("adgs_multiview_ncc_backward", desc, !normal || !depth || !opacity || !ref_gray || !nbr_gray || !samples || !work || !g_loss, S, v);
	if (c) return c < 0 ? -1 : 0;
	if (!dL_dnormal && !dL_ddepth && !dL_dopacity) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const size_t plane = (size_t)v.H * v.W * sizeof(float);
	if (dL_dnormal) ADGS_HIP_CHECK(hipMemsetAsync(dL_dnormal, 0, 3 * plane, stream));
	if (dL_ddepth) ADGS_HIP_CHECK(hipMemsetAsync(dL_ddepth, 0, plane, stream));
	if (dL_dopacity) ADGS_HIP_CHECK(hipMemsetAsync(dL_dopacity, 0, plane, stream));
	hipLaunchKernelGGL(multiview_ncc_bwd_kernel, dim3(mv_blocks(S)), dim3(SLOT_THREADS), 0, stream, v, normal, depth, opacity, ref_gray, nbr_gray, weight,
		samples, S, work, g_loss, dL_dnormal, dL_ddepth, dL_dopacity);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
