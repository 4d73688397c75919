// Multi-view geometric consistency (depth reprojection error), forward and backward, for gfx950 (wave64).
// The definition is in include/adgs_multiview_geo.h.
//
// One thread per reference pixel, 32 x 8 tiles (a wave covers two rows of 32: the reads of D, O, weight and the stores of the outputs
// and of the two reference-view gradients are whole lines).  The chain is double: the inputs are exact floats, and the error is the
// difference of two pixel coordinates of up to 1920 after a round trip through two divisions by a depth.  The float32 restatement of the
// reference at 1280 x 1920 is off by up to 5.2e-4 px in err and by 1.7 times the largest gradient element in the gradients -- the direction
// (dx, dy) / err of an error far below a pixel is rounding noise in float32 -- (tests/test_multiview_geo_ref.py), against tolerances of
// 1e-5 px and 1e-4 of the largest element.  The volume is ~150 double operations per pixel, 0.4 GFLOP per call at 1280 x 1920: the pass
// is bound by its eight gathers per pixel, not by the fp64 rate.
// Forward: the thread holds (w v g err, w v); slot_add_block adds the workgroup's sums to its slot row with one atomic per sum, the finish
// kernel stores the totals and L behind the rows.
// Backward: the same evaluation again, then the chain in reverse.  Every thread stores its pixel's dL/dD and dL/dO (zero when the pixel
// is invalid): the two maps need no fill.  The eight corner contributions to the neighbour's maps go through an LDS window over the
// tile's footprint in the neighbour (bounding box of the corners of its valid pixels, GEO_WIN pixels at most): ds_add_f32 there, then
// one global float atomic per touched pixel and map.  At equal resolutions a 32 x 8 tile lands on ~34 x 10 neighbour pixels, so the
// 2048 corner adds of a tile become ~700 global ones, issued by consecutive lanes on consecutive addresses.  A tile whose footprint does
// not fit (a neighbour of much higher resolution, a depth discontinuity across the tile) adds its corners directly (measured at 1280 x 1920
// against a build that always does: backward 0.079 ms against 0.113 ms, EXPERIMENTS.md).  With no neighbour
// gradient wanted the kernel skips all of this (the same kernel: the reference view's gradients are the same bits either way).
//
// Byte model (HBM; the gathers of neighbouring pixels share lines, so 8 bytes per neighbour pixel that is touched at all):
// forward 8 HW + [4 HW] + 8 HnWn read, [8 HW] written; backward the same read, 8 HW written, plus 8 HnWn of fill and the atomics.
#include "common.h"
#include "slot_reduce.h"
#include "../../include/adgs_loss.h"
#include "../../include/adgs_multiview_geo.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

constexpr int GEO_ROW = 2;                                      // doubles per slot row
constexpr int GEO_TX = 32, GEO_TY = 8;                          // the tile of reference pixels of one workgroup
#ifndef ADGS_GEO_WIN
#define ADGS_GEO_WIN 2048                                       // experiment builds: make fullvariant DEFS=-DADGS_GEO_WIN=1 sends every tile down the direct path
#endif
constexpr int GEO_WIN = ADGS_GEO_WIN;                           // neighbour pixels of the LDS window (x 2 maps x 4 bytes = 16 KiB)
static_assert(GEO_WIN >= 1 && GEO_WIN <= 4096, "the window is static LDS");
static_assert(GEO_TX * GEO_TY == SLOT_THREADS, "one thread per pixel of the tile");
static_assert(ADGS_MULTIVIEW_GEO_WORK_DOUBLES >= ADGS_LOSS_SLOTS * GEO_ROW + 3, "three scalars behind the rows");
enum { GEO_SVE = 0, GEO_SV, GEO_L };                           // the scalars behind the rows: sum w v g err, sum w v, L

struct GeoView {
	int H, W, Hn, Wn;
	int inv_depth;
	int tiles_x;            // tiles per row of tiles
	double tx, ty;          // tanfovx, tanfovy of the reference
	double kx, ky;          // W / (2 tanfovx), H / (2 tanfovy)
	double cx, cy;          // (W - 1) / 2, (H - 1) / 2
	double ku, kv;          // Wn / (2 tanfovx_n), Hn / (2 tanfovy_n)
	double cu, cv;          // (Wn - 1) / 2, (Hn - 1) / 2
	double R[9], t[3];
	double max_err;
	float min_opacity;
};

// What a thread knows of its pixel once every gate before the last has passed.
struct GeoPix {
	double D, O, z, rx, ry;
	double Yz, a, b;        // Y.z, Y.x / Y.z, Y.y / Y.z
	int xi, yi, x1, y1;     // the bilinear cell: inside the neighbour's image
	double fx, fy;
	double Dc[4], Oc[4], zc[4];     // the corners (yi, xi), (yi, x1), (y1, xi), (y1, x1)
	double top, bot, zh;
	double Xx, Xy, Xz;      // X'
	double dx, dy, err;
};

// Evaluates pixel (x, y) of the reference image (inside it) up to err.  false: one of the gates before the last fails; nothing outside
// the two images is read.
__device__ __forceinline__ bool geo_eval(const GeoView& v, const float* __restrict__ depth, const float* __restrict__ opacity,
	const float* __restrict__ nbr_depth, const float* __restrict__ nbr_opacity, int x, int y, GeoPix& o) {
	const size_t idx = (size_t)y * v.W + x;
	const float Of = opacity[idx], Df = depth[idx];
	if (!(Of >= v.min_opacity) || !(Df > 0.f)) return false;
	o.D = Df; o.O = Of;
	o.z = v.inv_depth ? o.O / o.D : o.D / o.O;
	o.rx = ((2.0 * (double)x + 1.0) / (double)v.W - 1.0) * v.tx;
	o.ry = ((2.0 * (double)y + 1.0) / (double)v.H - 1.0) * v.ty;
	const double X0 = o.z * o.rx, X1 = o.z * o.ry, X2 = o.z;
	const double Y0 = v.R[0] * X0 + v.R[1] * X1 + v.R[2] * X2 + v.t[0];
	const double Y1 = v.R[3] * X0 + v.R[4] * X1 + v.R[5] * X2 + v.t[1];
	o.Yz = v.R[6] * X0 + v.R[7] * X1 + v.R[8] * X2 + v.t[2];
	if (!(o.Yz > 1e-6)) return false;
	o.a = Y0 / o.Yz; o.b = Y1 / o.Yz;
	const double pu = o.a * v.ku + v.cu, pv = o.b * v.kv + v.cv;
	if (!(pu >= 0.0 && pu <= (double)(v.Wn - 1) && pv >= 0.0 && pv <= (double)(v.Hn - 1))) return false;      // false for NaN
	// (pu, pv) lies inside the neighbour's image: every index below is in [0, Wn - 1] x [0, Hn - 1]
	o.xi = min(max((int)floor(pu), 0), max(v.Wn - 2, 0)); o.yi = min(max((int)floor(pv), 0), max(v.Hn - 2, 0));
	o.x1 = min(o.xi + 1, v.Wn - 1); o.y1 = min(o.yi + 1, v.Hn - 1);
	o.fx = pu - (double)o.xi; o.fy = pv - (double)o.yi;
	const size_t c[4] = { (size_t)o.yi * v.Wn + o.xi, (size_t)o.yi * v.Wn + o.x1, (size_t)o.y1 * v.Wn + o.xi, (size_t)o.y1 * v.Wn + o.x1 };
	float Dn[4], On[4];
#pragma unroll
	for (int k = 0; k < 4; k++) { Dn[k] = nbr_depth[c[k]]; On[k] = nbr_opacity[c[k]]; }
	bool ok = true;
#pragma unroll
	for (int k = 0; k < 4; k++) ok = ok && On[k] >= v.min_opacity && Dn[k] > 0.f;
	if (!ok) return false;
#pragma unroll
	for (int k = 0; k < 4; k++) { o.Dc[k] = Dn[k]; o.Oc[k] = On[k]; o.zc[k] = v.inv_depth ? o.Oc[k] / o.Dc[k] : o.Dc[k] / o.Oc[k]; }
	o.top = o.zc[0] + o.fx * (o.zc[1] - o.zc[0]);
	o.bot = o.zc[2] + o.fx * (o.zc[3] - o.zc[2]);
	o.zh = o.top + o.fy * (o.bot - o.top);
	const double q0 = o.a * o.zh - v.t[0], q1 = o.b * o.zh - v.t[1], q2 = o.zh - v.t[2];           // Y' - t
	o.Xx = v.R[0] * q0 + v.R[3] * q1 + v.R[6] * q2;
	o.Xy = v.R[1] * q0 + v.R[4] * q1 + v.R[7] * q2;
	o.Xz = v.R[2] * q0 + v.R[5] * q1 + v.R[8] * q2;
	if (!(o.Xz > 1e-6)) return false;
	o.dx = (o.Xx / o.Xz) * v.kx + v.cx - (double)x;
	o.dy = (o.Xy / o.Xz) * v.ky + v.cy - (double)y;
	o.err = sqrt(o.dx * o.dx + o.dy * o.dy);
	return true;
}

__global__ void __launch_bounds__(SLOT_THREADS) multiview_geo_fwd_kernel(GeoView v, const float* __restrict__ depth, const float* __restrict__ opacity,
	const float* __restrict__ nbr_depth, const float* __restrict__ nbr_opacity, const float* __restrict__ weight, double* __restrict__ work,
	float* __restrict__ err_out, float* __restrict__ weight_out) {
	const int by = blockIdx.x / v.tiles_x, bx = blockIdx.x - by * v.tiles_x;
	const int x = bx * GEO_TX + (threadIdx.x & (GEO_TX - 1)), y = by * GEO_TY + threadIdx.x / GEO_TX;
	double acc[GEO_ROW] = { 0.0, 0.0 };                         // sum w v g err, sum w v
	if (x < v.W && y < v.H) {
		const size_t idx = (size_t)y * v.W + x;
		GeoPix o;
		const bool geo = geo_eval(v, depth, opacity, nbr_depth, nbr_opacity, x, y, o);
		const bool valid = geo && o.err < v.max_err;
		const double g = valid ? exp(-o.err) : 0.0;
		if (valid) {
			const double w = weight ? (double)weight[idx] : 1.0;
			acc[GEO_SVE] = w * g * o.err; acc[GEO_SV] = w;
		}
		if (err_out) err_out[idx] = geo ? (float)o.err : 0.f;
		if (weight_out) weight_out[idx] = (float)g;
	}
	slot_add_block<ADGS_LOSS_SLOTS, GEO_ROW, SLOT_THREADS>(work, acc);
}

// one block: totals of the slot rows (left zero) -> the scalars behind them and the loss
__global__ void __launch_bounds__(SLOT_THREADS) multiview_geo_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double t[GEO_ROW];
	slot_finish<ADGS_LOSS_SLOTS, GEO_ROW>(work, t);
	if (threadIdx.x == 0) {
		double* tot = work + (size_t)ADGS_LOSS_SLOTS * GEO_ROW;
		for (int q = 0; q < GEO_ROW; q++) tot[q] = t[q];
		const double L = tot[GEO_SV] > 0.0 ? tot[GEO_SVE] / tot[GEO_SV] : 0.0;
		tot[GEO_L] = L;
		loss[0] = (float)L;
	}
}

// The neighbour's gradient maps that are given are zero on entry.
__global__ void __launch_bounds__(SLOT_THREADS) multiview_geo_bwd_kernel(GeoView v, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ nbr_depth, const float* __restrict__ nbr_opacity, const float* __restrict__ weight,
	const double* __restrict__ work, const float* __restrict__ g_loss, float* __restrict__ dL_ddepth, float* __restrict__ dL_dopacity,
	float* __restrict__ dL_dnbr_depth, float* __restrict__ dL_dnbr_opacity) {
	const int tid = threadIdx.x;
	const bool nbr = dL_dnbr_depth || dL_dnbr_opacity;          // one kernel either way: the reference view's gradients are the same bits
	const int by = blockIdx.x / v.tiles_x, bx = blockIdx.x - by * v.tiles_x;
	const int x = bx * GEO_TX + (tid & (GEO_TX - 1)), y = by * GEO_TY + tid / GEO_TX;
	const bool inside = x < v.W && y < v.H;
	const double sum_v = work[(size_t)ADGS_LOSS_SLOTS * GEO_ROW + GEO_SV];
	const double gs = sum_v > 0.0 ? (double)g_loss[0] / sum_v : 0.0;
	GeoPix o;
	bool live = false;                                          // a valid pixel with a non-zero dL/derr and err > 0
	double ge = 0.0;
	if (inside && gs != 0.0 && geo_eval(v, depth, opacity, nbr_depth, nbr_opacity, x, y, o) && o.err < v.max_err) {
		ge = gs * (weight ? (double)weight[(size_t)y * v.W + x] : 1.0) * exp(-o.err);
		live = ge != 0.0 && o.err > 0.0;
	}
	double gD = 0.0, gO = 0.0, gDn[4] = { 0.0, 0.0, 0.0, 0.0 }, gOn[4] = { 0.0, 0.0, 0.0, 0.0 };
	if (live) {
		// (x', y') = (X'.x / X'.z kx + cx, ...)
		const double A = ge * o.dx / o.err * v.kx / o.Xz, B = ge * o.dy / o.err * v.ky / o.Xz;
		const double gX0 = A, gX1 = B, gX2 = -(A * o.Xx + B * o.Xy) / o.Xz;
		// X' = R^T (Y' - t)
		const double gQ0 = v.R[0] * gX0 + v.R[1] * gX1 + v.R[2] * gX2;
		const double gQ1 = v.R[3] * gX0 + v.R[4] * gX1 + v.R[5] * gX2;
		const double gQ2 = v.R[6] * gX0 + v.R[7] * gX1 + v.R[8] * gX2;
		// Y' = (a zh, b zh, zh)
		const double gzh = gQ0 * o.a + gQ1 * o.b + gQ2;
		double ga = gQ0 * o.zh, gb = gQ1 * o.zh;
		// zh through its sampling position: u = a ku + cu, v = b kv + cv
		ga += gzh * ((1.0 - o.fy) * (o.zc[1] - o.zc[0]) + o.fy * (o.zc[3] - o.zc[2])) * v.ku;
		gb += gzh * (o.bot - o.top) * v.kv;
		// a = Y.x / Y.z, b = Y.y / Y.z;  Y = R X + t;  X = z r
		const double gY0 = ga / o.Yz, gY1 = gb / o.Yz, gY2 = -(ga * o.a + gb * o.b) / o.Yz;
		const double gx0 = v.R[0] * gY0 + v.R[3] * gY1 + v.R[6] * gY2;
		const double gx1 = v.R[1] * gY0 + v.R[4] * gY1 + v.R[7] * gY2;
		const double gx2 = v.R[2] * gY0 + v.R[5] * gY1 + v.R[8] * gY2;
		const double gz = gx0 * o.rx + gx1 * o.ry + gx2;
		gD = v.inv_depth ? -gz * o.O / (o.D * o.D) : gz / o.O;
		gO = v.inv_depth ? gz / o.D : -gz * o.D / (o.O * o.O);
		if (nbr) {
			const double wc[4] = { (1.0 - o.fx) * (1.0 - o.fy), o.fx * (1.0 - o.fy), (1.0 - o.fx) * o.fy, o.fx * o.fy };
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const double gzc = gzh * wc[k];
				gDn[k] = v.inv_depth ? -gzc * o.Oc[k] / (o.Dc[k] * o.Dc[k]) : gzc / o.Oc[k];
				gOn[k] = v.inv_depth ? gzc / o.Dc[k] : -gzc * o.Dc[k] / (o.Oc[k] * o.Oc[k]);
			}
		}
	}
	if (inside) {
		const size_t idx = (size_t)y * v.W + x;
		if (dL_ddepth) dL_ddepth[idx] = (float)gD;
		if (dL_dopacity) dL_dopacity[idx] = (float)gO;
	}
	if (!nbr) return;

	__shared__ float s_acc[2][GEO_WIN];
	__shared__ int s_box[4];                                    // minx, miny, maxx, maxy over the cells of the tile's live pixels
	if (tid == 0) { s_box[0] = 0x7fffffff; s_box[1] = 0x7fffffff; s_box[2] = -1; s_box[3] = -1; }
	__syncthreads();
	{
		int lox = live ? o.xi : 0x7fffffff, loy = live ? o.yi : 0x7fffffff, hix = live ? o.x1 : -1, hiy = live ? o.y1 : -1;
#pragma unroll
		for (int off = WAVE / 2; off > 0; off >>= 1) {
			lox = min(lox, __shfl_xor(lox, off, WAVE)); loy = min(loy, __shfl_xor(loy, off, WAVE));
			hix = max(hix, __shfl_xor(hix, off, WAVE)); hiy = max(hiy, __shfl_xor(hiy, off, WAVE));
		}
		if ((tid & (WAVE - 1)) == 0 && lox <= hix) { atomicMin(&s_box[0], lox); atomicMin(&s_box[1], loy); atomicMax(&s_box[2], hix); atomicMax(&s_box[3], hiy); }
	}
	__syncthreads();
	const int minx = s_box[0], miny = s_box[1];
	if (s_box[2] < 0) return;                                   // no live pixel in this tile (block-uniform)
	const int fw = s_box[2] - minx + 1, fh = s_box[3] - miny + 1;      // block-uniform; the box lies inside the neighbour's image
	if ((long long)fw * fh <= GEO_WIN) {
		const int n = fw * fh;
		for (int i = tid; i < n; i += SLOT_THREADS) { s_acc[0][i] = 0.f; s_acc[1][i] = 0.f; }
		__syncthreads();
		if (live) {
			// minx <= xi <= x1 <= maxx and miny <= yi <= y1 <= maxy: every local index is in [0, n)
			const int l[4] = { (o.yi - miny) * fw + (o.xi - minx), (o.yi - miny) * fw + (o.x1 - minx), (o.y1 - miny) * fw + (o.xi - minx),
				(o.y1 - miny) * fw + (o.x1 - minx) };
#pragma unroll
			for (int k = 0; k < 4; k++) {
				if (dL_dnbr_depth) atomicAdd(&s_acc[0][l[k]], (float)gDn[k]);
				if (dL_dnbr_opacity) atomicAdd(&s_acc[1][l[k]], (float)gOn[k]);
			}
		}
		__syncthreads();
		for (int i = tid; i < n; i += SLOT_THREADS) {
			const int ly = i / fw, lx = i - ly * fw;
			const size_t dst = (size_t)(miny + ly) * v.Wn + (minx + lx);
			const float d = s_acc[0][i], p = s_acc[1][i];
			if (dL_dnbr_depth && d != 0.f) atomicAdd(dL_dnbr_depth + dst, d);
			if (dL_dnbr_opacity && p != 0.f) atomicAdd(dL_dnbr_opacity + dst, p);
		}
		return;
	}
	if (!live) return;
	const size_t c[4] = { (size_t)o.yi * v.Wn + o.xi, (size_t)o.yi * v.Wn + o.x1, (size_t)o.y1 * v.Wn + o.xi, (size_t)o.y1 * v.Wn + o.x1 };
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (dL_dnbr_depth && gDn[k] != 0.0) atomicAdd(dL_dnbr_depth + c[k], (float)gDn[k]);
		if (dL_dnbr_opacity && gOn[k] != 0.0) atomicAdd(dL_dnbr_opacity + c[k], (float)gOn[k]);
	}
}

bool geo_positive(float x) { return std::isfinite(x) && x > 0.f; }

// 0: launch with `v`; 1: nothing to do; -1: refused
int geo_check(const char* who, const adgs_multiview_geo_desc* d, bool null_pointer, GeoView& v) {
	const std::string name(who);
	if (!d || null_pointer) { set_error(name + ": NULL pointer"); return -1; }
	if (d->struct_bytes < (int)sizeof(adgs_multiview_geo_desc)) { set_error(name + ": struct_bytes is smaller than adgs_multiview_geo_desc"); return -1; }
	if (d->H < 0 || d->W < 0 || d->Hn < 0 || d->Wn < 0) { set_error(name + ": negative H, W, Hn or Wn"); return -1; }
	if ((long long)d->H * d->W > (long long)INT_MAX || (long long)d->Hn * d->Wn > (long long)INT_MAX) { set_error(name + ": H * W or Hn * Wn exceeds INT_MAX"); return -1; }
	if (!geo_positive(d->tanfovx) || !geo_positive(d->tanfovy) || !geo_positive(d->tanfovx_n) || !geo_positive(d->tanfovy_n)) {
		set_error(name + ": the four tanfov values must be finite and > 0"); return -1;
	}
	if (!(geo_positive(d->min_opacity) && d->min_opacity <= 1.f)) { set_error(name + ": min_opacity must lie in (0, 1]"); return -1; }
	if (!geo_positive(d->max_pixel_error)) { set_error(name + ": max_pixel_error must be finite and > 0"); return -1; }
	for (int i = 0; i < 12; i++)
		if (!std::isfinite(d->pose[i])) { set_error(name + ": the pose must be finite"); return -1; }
	if (d->H == 0 || d->W == 0 || d->Hn == 0 || d->Wn == 0) return 1;
	v.H = d->H; v.W = d->W; v.Hn = d->Hn; v.Wn = d->Wn;
	v.inv_depth = d->inv_depth ? 1 : 0;
	v.tiles_x = (d->W + GEO_TX - 1) / GEO_TX;
	v.tx = (double)d->tanfovx; v.ty = (double)d->tanfovy;
	v.kx = (double)d->W / (2.0 * (double)d->tanfovx); v.ky = (double)d->H / (2.0 * (double)d->tanfovy);
	v.cx = 0.5 * (double)(d->W - 1); v.cy = 0.5 * (double)(d->H - 1);
	v.ku = (double)d->Wn / (2.0 * (double)d->tanfovx_n); v.kv = (double)d->Hn / (2.0 * (double)d->tanfovy_n);
	v.cu = 0.5 * (double)(d->Wn - 1); v.cv = 0.5 * (double)(d->Hn - 1);
	for (int i = 0; i < 9; i++) v.R[i] = (double)d->pose[i];
	for (int i = 0; i < 3; i++) v.t[i] = (double)d->pose[9 + i];
	v.max_err = (double)d->max_pixel_error;
	v.min_opacity = d->min_opacity;
	return 0;
}

// tiles of the reference image, a one-dimensional grid: ceil(W / 32) ceil(H / 8) <= H W <= INT_MAX
unsigned geo_tiles(const GeoView& v) { return (unsigned)((long long)v.tiles_x * ((v.H + GEO_TY - 1) / GEO_TY)); }

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_multiview_geo_forward(const adgs_multiview_geo_desc* desc, const float* depth, const float* opacity, const float* nbr_depth,
	const float* nbr_opacity, const float* weight, double* work, float* loss, float* err_out, float* weight_out, void* stream_) {
	GeoView v;
	const int c = geo_check("adgs_multiview_geo_forward", desc, !depth || !opacity || !nbr_depth || !nbr_opacity || !work || !loss, v);
	if (c) return c < 0 ? -1 : 0;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(multiview_geo_fwd_kernel, dim3(geo_tiles(v)), dim3(SLOT_THREADS), 0, stream, v, depth, opacity, nbr_depth, nbr_opacity, weight,
		work, err_out, weight_out);
	hipLaunchKernelGGL(multiview_geo_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_multiview_geo_backward(const adgs_multiview_geo_desc* desc, const float* depth, const float* opacity, const float* nbr_depth,
	const float* nbr_opacity, const float* weight, const double* work, const float* g_loss, float* dL_ddepth, float* dL_dopacity,
	float* dL_dnbr_depth, float* dL_dnbr_opacity, void* stream_) {
	GeoView v;
	const int c = geo_check("adgs_multiview_geo_backward", desc, !depth || !opacity || !nbr_depth || !nbr_opacity || !work || !g_loss, v);
	if (c) return c < 0 ? -1 : 0;
	if (!dL_ddepth && !dL_dopacity && !dL_dnbr_depth && !dL_dnbr_opacity) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const size_t plane_n = (size_t)v.Hn * v.Wn * sizeof(float);
	if (dL_dnbr_depth) ADGS_HIP_CHECK(hipMemsetAsync(dL_dnbr_depth, 0, plane_n, stream));
	if (dL_dnbr_opacity) ADGS_HIP_CHECK(hipMemsetAsync(dL_dnbr_opacity, 0, plane_n, stream));
	hipLaunchKernelGGL(multiview_geo_bwd_kernel, dim3(geo_tiles(v)), dim3(SLOT_THREADS), 0, stream, v, depth, opacity, nbr_depth, nbr_opacity,
		weight, work, g_loss, dL_ddepth, dL_dopacity, dL_dnbr_depth, dL_dnbr_opacity);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
