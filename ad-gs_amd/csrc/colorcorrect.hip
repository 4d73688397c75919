// Colour fit behind the colour-corrected metrics, for gfx950 (include/adgs_colorcorrect.h): per iteration ONE accumulate launch forms the
// three weighted Gram matrices and right-hand sides of the image in double (3 x 65 sums), and ONE single-workgroup finishing launch adds
// the slot rows up, leaves them zero and solves the three ridge systems by Cholesky; the warp it writes is read by the next iteration's
// accumulate launch.  No intermediate image: a pixel's x^{k-1} is recomputed from the clipped input by applying the earlier warps in
// registers (30 FMAs per warp, the warp rows as wave-uniform loads).
// The accumulate kernel is a grid of at most MAXG workgroups striding over the image with the CHANNEL LOOP OUTERMOST: 65 double
// accumulators (130 VGPRs) live at a time, and their cross-lane reduction is paid once per workgroup and channel, not per tile.  The
// image is read once per channel; at the evaluation resolution it stays in the Infinity Cache between the three sweeps.
#include "common.h"
#include "slot_reduce.h"
#include "../../include/adgs_colorcorrect.h"
#include <cmath>

namespace adgs {
namespace {

constexpr int NF = ADGS_CC_FEATURES, SLOTS = ADGS_CC_SLOTS, ROW = ADGS_CC_ROW;
constexpr int NG = NF * (NF + 1) / 2;      // unique Gram entries
constexpr int NA = NG + NF;                // sums per channel: the Gram entries, then h; n_c is the Gram entry of the constant feature
constexpr int CT = 256;                    // threads per workgroup
constexpr int MAXG = 512;                  // workgroups of the accumulate launch: two per CU
static_assert(3 * NA <= ROW && 3 * NA <= CT, "a slot row holds three channels; one finishing thread per sum");

// position of Gram entry (i, j), i <= j, in a channel's part of a slot row
__host__ __device__ constexpr int tri(int i, int j) { return i * NF - i * (i - 1) / 2 + (j - i); }

// the features a model fits, as a compact list: affine [r, g, b, 1], quadratic all ten; feat(i): the column of warp row / slot row
template <int MODEL> struct Model {
	static constexpr int N = MODEL == ADGS_CC_QUADRATIC ? NF : 4;
	__host__ __device__ static constexpr int feat(int i) { return MODEL == ADGS_CC_QUADRATIC ? i : (i < 3 ? i : NF - 1); }
};

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

template <int MODEL> __device__ __forceinline__ void features(const double (&x)[3], double (&phi)[Model<MODEL>::N]) {
	phi[0] = x[0]; phi[1] = x[1]; phi[2] = x[2];
	if (MODEL == ADGS_CC_QUADRATIC) {
		phi[3] = x[0] * x[0]; phi[4] = x[0] * x[1]; phi[5] = x[0] * x[2];
		phi[6] = x[1] * x[1]; phi[7] = x[1] * x[2]; phi[8] = x[2] * x[2];
	}
	phi[Model<MODEL>::N - 1] = 1.0;
}

// x <- clip(phi(x) . W_c) for the three channels of one warp ([3][NF], wave-uniform)
template <int MODEL> __device__ __forceinline__ void advance(double (&x)[3], const double* __restrict__ warp) {
	using M = Model<MODEL>;
	double phi[M::N];
	features<MODEL>(x, phi);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		double s = 0.0;
#pragma unroll
		for (int i = 0; i < M::N; i++) s = fma(phi[i], warp[c * NF + M::feat(i)], s);
		x[c] = clip01(s);
	}
}

__device__ __forceinline__ void clipped_pixel(const float* __restrict__ img, size_t HW, size_t p, double (&x)[3]) {
	x[0] = (double)clip01(img[p]); x[1] = (double)clip01(img[HW + p]); x[2] = (double)clip01(img[2 * HW + p]);
}

// what the accumulate sweep of channel c reads of a pixel, as loaded: the loop fetches the next pixel's while it works on this one's (two
// waves per SIMD do not hide a memory round trip per step on their own)
struct RawPixel {
	float r, g, b, y, w;
	__device__ __forceinline__ void load(const float* __restrict__ img, const float* __restrict__ gt_c, const float* __restrict__ weight, size_t HW, size_t p) {
		r = img[p]; g = img[HW + p]; b = img[2 * HW + p]; y = gt_c[p];
		w = weight ? weight[p] : 1.f;
	}
};

template <int MODEL> __global__ void __launch_bounds__(CT) cc_accumulate_kernel(size_t HW, int nprev, float epsf, const float* __restrict__ img,
	const float* __restrict__ gt, const float* __restrict__ weight, const double* __restrict__ warps, double* __restrict__ work) {
	using M = Model<MODEL>;
	constexpr int N = M::N;
	__shared__ double red[NA][CT / WAVE];
	const int tid = threadIdx.x;
	const double eps = (double)epsf, top = 1.0 - eps;
	const size_t stride = (size_t)gridDim.x * CT;
	if (N < NF) {      // the entries a model does not fit stay zero
		for (int i = tid; i < NA * (CT / WAVE); i += CT) (&red[0][0])[i] = 0.0;
		__syncthreads();
	}
#pragma unroll 1
	for (int c = 0; c < 3; c++) {
		double acc[N * (N + 1) / 2 + N];
#pragma unroll
		for (int a = 0; a < N * (N + 1) / 2 + N; a++) acc[a] = 0.0;
		const size_t first = (size_t)blockIdx.x * CT + tid;
		const float* gt_c = gt + (size_t)c * HW;
		RawPixel next;
		if (first < HW) next.load(img, gt_c, weight, HW, first);
#pragma unroll 1
		for (size_t p = first; p < HW; p += stride) {
			const RawPixel raw = next;
			if (p + stride < HW) next.load(img, gt_c, weight, HW, p + stride);
			double x[3] = { (double)clip01(raw.r), (double)clip01(raw.g), (double)clip01(raw.b) };
			const double y = (double)clip01(raw.y), w = (double)raw.w;
			const double x0c = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
			for (int k = 0; k < nprev; k++) advance<MODEL>(x, warps + (size_t)k * 3 * NF);
			const double xc = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
			const bool usable = x0c >= eps && x0c <= top && xc >= eps && xc <= top && y >= eps && y <= top;
			const double m = usable ? w : 0.0;
			double phi[N];
			features<MODEL>(x, phi);
			int a = 0;
#pragma unroll
			for (int i = 0; i < N; i++) {
				const double t = m * phi[i];
#pragma unroll
				for (int j = i; j < N; j++, a++) acc[a] = fma(t, phi[j], acc[a]);
			}
#pragma unroll
			for (int i = 0; i < N; i++) acc[a + i] = fma(m * phi[i], y, acc[a + i]);
		}
		// the workgroup's sums of this channel: lanes, then waves, then one atomic per sum into the slot row
		{
			int a = 0;
#pragma unroll
			for (int i = 0; i < N; i++) {
#pragma unroll
				for (int j = i; j <= N; j++, a++) {      // j == N: h_i
					double v = j < N ? acc[a - i] : acc[N * (N + 1) / 2 + i];
					wave_sum(v);
					if ((tid & (WAVE - 1)) == 0) red[j < N ? tri(M::feat(i), M::feat(j)) : NG + M::feat(i)][tid / WAVE] = v;
				}
			}
		}
		__syncthreads();
		if (tid < NA) {
			double t = 0.0;
#pragma unroll
			for (int wv = 0; wv < CT / WAVE; wv++) t += red[tid][wv];
			if (t != 0.0) atomicAdd(work + (size_t)(blockIdx.x % SLOTS) * ROW + c * NA + tid, t);
		}
		__syncthreads();                  // red is rewritten by the next channel
	}
}

// one workgroup: the slot rows' totals (the rows are consumed: zero afterwards), then one thread per channel solves
// (G + ridge I) W = h + ridge e_c by Cholesky in registers
template <int MODEL> __global__ void __launch_bounds__(CT) cc_finish_kernel(double ridge, double* __restrict__ work, double* __restrict__ warp_out,
	double* __restrict__ support_out) {
	using M = Model<MODEL>;
	constexpr int N = M::N;
	__shared__ double s[3 * NA];
	const int tid = threadIdx.x;
	if (tid < 3 * NA) {
		double t = 0.0;
#pragma unroll 16
		for (int r = 0; r < SLOTS; r++) {
			double* p = work + (size_t)r * ROW + tid;
			t += *p;
			*p = 0.0;
		}
		s[tid] = t;
	}
	__syncthreads();
	if (tid >= 3) return;
	const int c = tid;
	const double* g = s + c * NA;
	const double n = g[tri(NF - 1, NF - 1)];
	support_out[c] = n;
	double wrow[NF];
#pragma unroll
	for (int i = 0; i < NF; i++) wrow[i] = 0.0;
	if (n == 0.0) {                       // no usable pixel (every m_c is 0, the sums with it): exactly the identity
#pragma unroll
		for (int i = 0; i < 3; i++) wrow[i] = i == c ? 1.0 : 0.0;
	} else {
		double a[N][N], b[N];             // the lower triangle, overwritten by its Cholesky factor
#pragma unroll
		for (int i = 0; i < N; i++) {
#pragma unroll
			for (int j = 0; j <= i; j++) a[i][j] = g[tri(M::feat(j), M::feat(i))] + (i == j ? ridge : 0.0);
			b[i] = g[NG + M::feat(i)] + (i == c ? ridge : 0.0);
		}
#pragma unroll
		for (int j = 0; j < N; j++) {
			double d = a[j][j];
#pragma unroll
			for (int k = 0; k < j; k++) d = fma(-a[j][k], a[j][k], d);
			d = sqrt(d);
			a[j][j] = d;
#pragma unroll
			for (int i = j + 1; i < N; i++) {
				double t = a[i][j];
#pragma unroll
				for (int k = 0; k < j; k++) t = fma(-a[i][k], a[j][k], t);
				a[i][j] = t / d;
			}
		}
#pragma unroll
		for (int i = 0; i < N; i++) {         // L z = b
			double t = b[i];
#pragma unroll
			for (int k = 0; k < i; k++) t = fma(-a[i][k], b[k], t);
			b[i] = t / a[i][i];
		}
#pragma unroll
		for (int i = N - 1; i >= 0; i--) {    // L^T w = z
			double t = b[i];
#pragma unroll
			for (int k = i + 1; k < N; k++) t = fma(-a[k][i], b[k], t);
			b[i] = t / a[i][i];
		}
#pragma unroll
		for (int i = 0; i < N; i++) wrow[M::feat(i)] = b[i];
	}
#pragma unroll
	for (int i = 0; i < NF; i++) warp_out[c * NF + i] = wrow[i];
}

template <int MODEL> __global__ void __launch_bounds__(CT) cc_apply_kernel(size_t HW, int n_warps, const float* __restrict__ img,
	const double* __restrict__ warps, float* __restrict__ out) {
	const size_t stride = (size_t)gridDim.x * CT;
	for (size_t p = (size_t)blockIdx.x * CT + threadIdx.x; p < HW; p += stride) {
		double x[3];
		clipped_pixel(img, HW, p, x);
		for (int k = 0; k < n_warps; k++) advance<MODEL>(x, warps + (size_t)k * 3 * NF);
		out[p] = (float)x[0]; out[HW + p] = (float)x[1]; out[2 * HW + p] = (float)x[2];
	}
}

// what both entries refuse; `who` ends in ": "
bool bad_desc(const char* who, const adgs_cc_desc* desc) {
	const std::string w(who);
	if (!desc) { set_error(w + "NULL descriptor"); return true; }
	if (desc->struct_bytes < (int)sizeof(adgs_cc_desc)) { set_error(w + "struct_bytes is smaller than adgs_cc_desc"); return true; }
	if (desc->H < 1 || desc->W < 1) { set_error(w + "H and W must be at least 1"); return true; }
	if (desc->model != ADGS_CC_AFFINE && desc->model != ADGS_CC_QUADRATIC) { set_error(w + "model must be 0 (affine) or 1 (quadratic)"); return true; }
	if (desc->iters < 1 || desc->iters > ADGS_CC_MAX_ITERS) { set_error(w + "iters must be 1 .. " + std::to_string(ADGS_CC_MAX_ITERS)); return true; }
	if (!(desc->eps >= 0.f && desc->eps < 0.5f)) { set_error(w + "eps must be in [0, 0.5)"); return true; }
	if (!(desc->ridge > 0.0) || !std::isfinite(desc->ridge)) { set_error(w + "ridge must be positive and finite"); return true; }
	return false;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_cc_work_doubles(void) { return (size_t)SLOTS * ROW; }

extern "C" int adgs_cc_fit(const adgs_cc_desc* desc, const float* image, const float* gt, const float* weight, double* work, double* warps_out,
	double* support_out, void* stream_) {
	const char* who = "adgs_cc_fit: ";
	if (bad_desc(who, desc)) return -1;
	if (!image || !gt || !work || !warps_out || !support_out) { set_error(std::string(who) + "NULL image / gt / work / warps_out / support_out"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const size_t HW = (size_t)desc->H * desc->W;
	const int grid = (int)std::min<size_t>((HW + CT - 1) / CT, MAXG);
	for (int k = 0; k < desc->iters; k++) {
		double* warp = warps_out + (size_t)k * 3 * NF;
		if (desc->model == ADGS_CC_QUADRATIC) {
			hipLaunchKernelGGL(cc_accumulate_kernel<ADGS_CC_QUADRATIC>, dim3(grid), dim3(CT), 0, stream, HW, k, desc->eps, image, gt, weight, warps_out, work);
			hipLaunchKernelGGL(cc_finish_kernel<ADGS_CC_QUADRATIC>, dim3(1), dim3(CT), 0, stream, desc->ridge, work, warp, support_out + 3 * k);
		} else {
			hipLaunchKernelGGL(cc_accumulate_kernel<ADGS_CC_AFFINE>, dim3(grid), dim3(CT), 0, stream, HW, k, desc->eps, image, gt, weight, warps_out, work);
			hipLaunchKernelGGL(cc_finish_kernel<ADGS_CC_AFFINE>, dim3(1), dim3(CT), 0, stream, desc->ridge, work, warp, support_out + 3 * k);
		}
	}
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_cc_apply(const adgs_cc_desc* desc, const float* image, const double* warps, int n_warps, float* out, void* stream_) {
	const char* who = "adgs_cc_apply: ";
	if (bad_desc(who, desc)) return -1;
	if (!image || !warps || !out) { set_error(std::string(who) + "NULL image / warps / out"); return -1; }
	if (n_warps < 1 || n_warps > desc->iters) { set_error(std::string(who) + "n_warps must be 1 .. iters"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const size_t HW = (size_t)desc->H * desc->W;
	const int grid = (int)std::min<size_t>((HW + CT - 1) / CT, 4 * MAXG);
	if (desc->model == ADGS_CC_QUADRATIC) hipLaunchKernelGGL(cc_apply_kernel<ADGS_CC_QUADRATIC>, dim3(grid), dim3(CT), 0, stream, HW, n_warps, image, warps, out);
	else hipLaunchKernelGGL(cc_apply_kernel<ADGS_CC_AFFINE>, dim3(grid), dim3(CT), 0, stream, HW, n_warps, image, warps, out);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
