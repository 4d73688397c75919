// Bilateral-grid appearance compensation for gfx950 (include/adgs_bilagrid.h): slice + 3x4 affine, its backward, and the
// total-variation regulariser of the grids.
//
// A 64x4-pixel workgroup (one wave per image row, the tile of envmap.hip) touches only a few (x, y) columns of the grid: at
// 1920x1280 under the default 16x16 grid, 64 pixels span half a cell.  The forward stages those columns -- all L levels and the
// 12 channels -- in LDS once per workgroup and every pixel reads its 8 x 12 corners from there; the backward accumulates the
// workgroup's share of dL_dgrid in an LDS image of the same footprint and flushes each touched element with one global atomic.
// The footprint of a tile follows from the shape alone, so the host decides per call: a shape whose largest possible footprint
// does not fit the LDS budget (a small image under a large grid) runs the same kernels without LDS -- gathers from / atomics into
// global memory.  adgs_test_bilagrid_path (include/adgs_testing.h) reports that choice.
#include "common.h"
#include "slot_reduce.h"
#include "../../include/adgs_bilagrid.h"
#include "../../include/adgs_testing.h"
#include <algorithm>
#include <cmath>

namespace adgs {
namespace {

constexpr int TW = 64, TH = 4;               // pixel tile of a workgroup: wave w holds row w
constexpr int BG_LDS_FLOATS = 4096;          // budget of ONE footprint image (12 L levels x columns); the backward keeps two (32 KiB)

struct BgShape { int L, Hg, Wg, H, W; };
struct BgBox { int minx, miny, fw, fh; };    // the grid columns of a tile: [minx, minx + fw) x [miny, miny + fh)
// Where element (channel-level cz = c L + z, row y, column x) of a grid image lives: p[cz * zs + (y - oy) * rs + (x - ox)].
// Global block: zs = Hg Wg, rs = Wg, ox = oy = 0.  LDS footprint: zs = padded column count, rs = fw, (ox, oy) = the box origin.
struct BgView { int zs, rs, ox, oy; };
struct BgTaps { int x0, y0, z0; float fx, fy, fz, slope; };

// cell and fraction of pixel p of n along a grid axis of `cells` nodes; monotonic in p (every operation is), which is what lets a
// tile take its box from its first and last pixel.  (p + 0.5) / n (cells - 1) as (2 p + 1)(cells - 1) / (2 n): numerator and
// denominator are exact integers for every practical size, so the coordinate is rounded once.
__device__ __forceinline__ int bg_cell(int p, int n, int cells, float& f) {
	const float g = ((2.f * (float)p + 1.f) * (float)(cells - 1)) / (2.f * (float)n);
	const int c = min((int)g, cells - 2);
	f = g - (float)c;
	return c;
}
__device__ __forceinline__ BgTaps bg_taps(const BgShape& s, int px, int py, float r, float g, float b) {
	BgTaps t;
	t.x0 = bg_cell(px, s.W, s.Wg, t.fx);
	t.y0 = bg_cell(py, s.H, s.Hg, t.fy);
	const float top = (float)(s.L - 1), v = (0.299f * r + 0.587f * g + 0.114f * b) * top;
	t.slope = (v >= 0.f && v <= top) ? 1.f : 0.f;
	const float gz = fminf(fmaxf(v, 0.f), top);         // a NaN luma lands on level 0: no index leaves the grid
	t.z0 = min((int)gz, s.L - 2);
	t.fz = gz - (float)t.z0;
	return t;
}
__device__ __forceinline__ BgBox bg_box(const BgShape& s) {
	float f;
	const int px0 = blockIdx.x * TW, py0 = blockIdx.y * TH;
	BgBox b;
	b.minx = bg_cell(px0, s.W, s.Wg, f); b.miny = bg_cell(py0, s.H, s.Hg, f);
	b.fw = bg_cell(min(px0 + TW, s.W) - 1, s.W, s.Wg, f) + 2 - b.minx;
	b.fh = bg_cell(min(py0 + TH, s.H) - 1, s.H, s.Hg, f) + 2 - b.miny;
	return b;
}
__device__ __forceinline__ int bg_offset(const BgView& v, const BgTaps& t) { return t.z0 * v.zs + (t.y0 - v.oy) * v.rs + (t.x0 - v.ox); }

// A[c] and (WANT_D) dA[c]/dgz = upper level - lower level, for the 12 channels
template <bool WANT_D>
__device__ __forceinline__ void bg_affine(const float* __restrict__ g, const BgView& v, int L, const BgTaps& t, float* A, float* dA) {
	const float w00 = (1.f - t.fx) * (1.f - t.fy), w10 = t.fx * (1.f - t.fy), w01 = (1.f - t.fx) * t.fy, w11 = t.fx * t.fy;
	const int o = bg_offset(v, t);
#pragma unroll
	for (int c = 0; c < 12; c++) {
		const float* p = g + c * L * v.zs + o;
		const float lo = w00 * p[0] + w10 * p[1] + w01 * p[v.rs] + w11 * p[v.rs + 1];
		p += v.zs;
		const float hi = w00 * p[0] + w10 * p[1] + w01 * p[v.rs] + w11 * p[v.rs + 1];
		A[c] = lo + t.fz * (hi - lo);
		if (WANT_D) dA[c] = hi - lo;
	}
}

// copies the box's columns, every channel-level, into an LDS image [12 L][ncp]
__device__ __forceinline__ void bg_stage(float* dst, const float* __restrict__ grid, const BgShape& s, const BgBox& b, int ncp) {
	const int ncols = b.fw * b.fh, ncz = 12 * s.L, plane = s.Hg * s.Wg;
	for (int col = threadIdx.x & 15; col < ncols; col += 16) {
		const int ly = col / b.fw, lx = col - ly * b.fw;
		const float* src = grid + (b.miny + ly) * s.Wg + b.minx + lx;
		for (int cz = threadIdx.x >> 4; cz < ncz; cz += 16) dst[cz * ncp + col] = src[(size_t)cz * plane];
	}
}

__device__ __forceinline__ void bg_pixel_fwd(const float* __restrict__ g, const BgView& v, const BgShape& s, int px, int py,
	const float* __restrict__ image, float* __restrict__ out) {
	const size_t plane = (size_t)s.H * s.W, o = (size_t)py * s.W + px;
	const float r = image[o], gr = image[plane + o], b = image[2 * plane + o];
	const BgTaps t = bg_taps(s, px, py, r, gr, b);
	float A[12];
	bg_affine<false>(g, v, s.L, t, A, nullptr);
#pragma unroll
	for (int i = 0; i < 3; i++) out[i * plane + o] = A[4 * i] * r + A[4 * i + 1] * gr + A[4 * i + 2] * b + A[4 * i + 3];
}

template <bool LDS>
__global__ void __launch_bounds__(256) bg_slice_fwd_kernel(BgShape s, const float* __restrict__ grid, const float* __restrict__ image,
	float* __restrict__ out, int cap) {
	extern __shared__ float s_mem[];
	const int px = blockIdx.x * TW + (threadIdx.x & 63), py = blockIdx.y * TH + (threadIdx.x >> 6);
	const bool valid = px < s.W && py < s.H;
	if (LDS) {
		const BgBox b = bg_box(s);
		const int ncp = (b.fw * b.fh) | 1;             // odd: levels land on different banks
		if (12 * s.L * ncp <= cap) {                  // block-uniform; the host sized `cap` for the largest tile of this shape
			bg_stage(s_mem, grid, s, b, ncp);
			__syncthreads();
			if (valid) bg_pixel_fwd(s_mem, BgView{ncp, b.fw, b.minx, b.miny}, s, px, py, image, out);
			return;
		}
	}
	if (valid) bg_pixel_fwd(grid, BgView{s.Hg * s.Wg, s.Wg, 0, 0}, s, px, py, image, out);
}

// dL_dimage of one pixel: the affine part and the luma-slope part share A / dA and the six loads
__device__ __forceinline__ void bg_pixel_dimage(const float* __restrict__ g, const BgView& v, const BgShape& s, const BgTaps& t,
	float r, float gr, float b, const float* d, size_t o, float* __restrict__ dimage) {
	float A[12], dA[12];
	bg_affine<true>(g, v, s.L, t, A, dA);
	float slope = 0.f;
#pragma unroll
	for (int i = 0; i < 3; i++) slope += d[i] * (dA[4 * i] * r + dA[4 * i + 1] * gr + dA[4 * i + 2] * b + dA[4 * i + 3]);
	slope *= t.slope * (float)(s.L - 1);
	const size_t plane = (size_t)s.H * s.W;
	const float coef[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
	for (int k = 0; k < 3; k++) dimage[k * plane + o] = d[0] * A[k] + d[1] * A[4 + k] + d[2] * A[8 + k] + coef[k] * slope;
}

// The trilinear scatter of d[i] * (r, g, b, 1)[j] into an accumulator image.  MERGE (the LDS accumulator): aligned groups of 8
// lanes whose pixels share a cell -- neighbours in a row share (x0, y0), and z0 too wherever the image is smooth -- sum their
// products across the group and issue one atomic instead of eight: LDS float atomics retire about one lane per cycle and CU
// (envmap.hip), and 96 per pixel would cost several times the kernel's memory time.
template <bool MERGE>
__device__ __forceinline__ void bg_scatter(float* acc, const BgView& v, int L, const BgTaps& t, float r, float gr, float b, const float* d,
	bool valid, bool merged) {
	const float m[4] = {r, gr, b, 1.f};
	const float ux = 1.f - t.fx, uy = 1.f - t.fy, uz = 1.f - t.fz;
	const float w[8] = {ux * uy * uz, t.fx * uy * uz, ux * t.fy * uz, t.fx * t.fy * uz, ux * uy * t.fz, t.fx * uy * t.fz, ux * t.fy * t.fz, t.fx * t.fy * t.fz};
	const int off[8] = {0, 1, v.rs, v.rs + 1, v.zs, v.zs + 1, v.zs + v.rs, v.zs + v.rs + 1};
	const int o = bg_offset(v, t);
	const bool issue = MERGE && merged ? (threadIdx.x & 7) == 0 : valid;
#pragma unroll
	for (int c = 0; c < 12; c++) {
		const float val = d[c >> 2] * m[c & 3];
		float* p = acc + c * L * v.zs + o;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			float x = w[k] * val;
			if (MERGE) {
				float sum = x + __shfl_xor(x, 1, WAVE);
				sum += __shfl_xor(sum, 2, WAVE);
				sum += __shfl_xor(sum, 4, WAVE);
				x = merged ? sum : x;
			}
			if (issue) atomicAdd(p + off[k], x);
		}
	}
}

template <bool LDS>
__global__ void __launch_bounds__(256) bg_slice_bwd_kernel(BgShape s, const float* __restrict__ grid, const float* __restrict__ image,
	const float* __restrict__ dout, float* __restrict__ dgrid, float* __restrict__ dimage, int cap) {
	extern __shared__ float s_mem[];
	const int px = blockIdx.x * TW + (threadIdx.x & 63), py = blockIdx.y * TH + (threadIdx.x >> 6);
	const bool valid = px < s.W && py < s.H;
	const size_t plane = (size_t)s.H * s.W, o = valid ? (size_t)py * s.W + px : 0;
	const float r = valid ? image[o] : 0.f, gr = valid ? image[plane + o] : 0.f, b = valid ? image[2 * plane + o] : 0.f;
	const float d[3] = {valid ? dout[o] : 0.f, valid ? dout[plane + o] : 0.f, valid ? dout[2 * plane + o] : 0.f};
	const BgTaps t = bg_taps(s, px, py, r, gr, b);
	if (LDS) {
		const BgBox bx = bg_box(s);
		const int ncols = bx.fw * bx.fh, ncp = ncols | 1, n = 12 * s.L * ncp;
		if (n <= cap) {                               // block-uniform, as in the forward
			float* s_grid = s_mem;
			float* s_acc = s_mem + cap;
			const BgView lv{ncp, bx.fw, bx.minx, bx.miny};
			if (dimage) bg_stage(s_grid, grid, s, bx, ncp);
			if (dgrid) for (int i = threadIdx.x; i < n; i += 256) s_acc[i] = 0.f;
			__syncthreads();
			if (dimage && valid) bg_pixel_dimage(s_grid, lv, s, t, r, gr, b, d, o, dimage);
			if (!dgrid) return;
			{
				// a wave is one image row: y0 is wave-uniform and (z0, x0) names the cell.  An invalid pixel shares a key with nobody.
				const int lane = threadIdx.x & (WAVE - 1);
				const int key = valid ? t.z0 * s.Wg + t.x0 : -1 - lane;
				const int k1 = __shfl_xor(key, 1, WAVE), k2 = __shfl_xor(key, 2, WAVE), k4 = __shfl_xor(key, 4, WAVE);      // every lane takes part in all three
				const bool eq = key == k1 && key == k2 && key == k4;
				const unsigned long long all = __ballot(eq);
				const bool merged = ((all >> (lane & ~7)) & 0xffull) == 0xffull;
				if (__ballot(merged) != 0ull) bg_scatter<true>(s_acc, lv, s.L, t, r, gr, b, d, valid, merged);      // wave-uniform branch
				else bg_scatter<false>(s_acc, lv, s.L, t, r, gr, b, d, valid, false);
			}
			__syncthreads();
			const int ncz = 12 * s.L, gplane = s.Hg * s.Wg;
			for (int col = threadIdx.x & 15; col < ncols; col += 16) {
				const int ly = col / bx.fw, lx = col - ly * bx.fw;
				float* dst = dgrid + (bx.miny + ly) * s.Wg + bx.minx + lx;
				for (int cz = threadIdx.x >> 4; cz < ncz; cz += 16) {
					const float val = s_acc[cz * ncp + col];
					if (val != 0.f) atomicAdd(dst + (size_t)cz * gplane, val);
				}
			}
			return;
		}
	}
	if (!valid) return;
	const BgView gv{s.Hg * s.Wg, s.Wg, 0, 0};
	if (dimage) bg_pixel_dimage(grid, gv, s, t, r, gr, b, d, o, dimage);
	if (dgrid) bg_scatter<false>(dgrid, gv, s.L, t, r, gr, b, d, true, false);
}

// ---------------------------------------------------------------- total variation
struct TvShape { int L, Hg, Wg; long long total; float wz, wy, wx; };      // w_axis = 1 / (N 12 pairs along the axis per channel)
constexpr int TV_SLOTS = ADGS_BILAGRID_TV_WORK_DOUBLES;      // slot rows of one double (slot_reduce.h), nothing behind them

__global__ void __launch_bounds__(SLOT_THREADS) bg_tv_sum_kernel(TvShape s, const float* __restrict__ g, double* __restrict__ work) {
	const int plane = s.Hg * s.Wg;
	double sum[1] = { 0 };
	for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < s.total; e += (long long)gridDim.x * blockDim.x) {
		const long long row = e / s.Wg, lev = row / s.Hg;
		const int x = (int)(e - row * s.Wg), y = (int)(row - lev * s.Hg), z = (int)(lev % s.L);
		const float v = g[e];
		float acc = 0.f;
		if (x + 1 < s.Wg) { const float q = g[e + 1] - v; acc += s.wx * q * q; }
		if (y + 1 < s.Hg) { const float q = g[e + s.Wg] - v; acc += s.wy * q * q; }
		if (z + 1 < s.L) { const float q = g[e + plane] - v; acc += s.wz * q * q; }
		sum[0] += (double)acc;
	}
	slot_add_wave<TV_SLOTS, 1>(work, sum);
}
__global__ void __launch_bounds__(SLOT_THREADS) bg_tv_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double t[1];
	slot_finish<TV_SLOTS, 1>(work, t);
	if (threadIdx.x == 0) loss[0] = (float)t[0];
}
__global__ void __launch_bounds__(256) bg_tv_bwd_kernel(TvShape s, const float* __restrict__ g, const float* __restrict__ g_loss, float* __restrict__ dg) {
	const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= s.total) return;
	const int plane = s.Hg * s.Wg;
	const long long row = e / s.Wg, lev = row / s.Hg;
	const int x = (int)(e - row * s.Wg), y = (int)(row - lev * s.Hg), z = (int)(lev % s.L);
	const float v = g[e];
	float acc = 0.f;
	if (x > 0) acc += s.wx * (v - g[e - 1]);
	if (x + 1 < s.Wg) acc -= s.wx * (g[e + 1] - v);
	if (y > 0) acc += s.wy * (v - g[e - s.Wg]);
	if (y + 1 < s.Hg) acc -= s.wy * (g[e + s.Wg] - v);
	if (z > 0) acc += s.wz * (v - g[e - plane]);
	if (z + 1 < s.L) acc -= s.wz * (g[e + plane] - v);
	dg[e] = 2.f * g_loss[0] * acc;
}

// ---------------------------------------------------------------- host side
// The most grid nodes a tile of `tile` pixels (fewer when the image is smaller) can touch along an axis of `cells` nodes under n pixels:
// the first and the last pixel lie (tile - 1) / n (cells - 1) apart, so their cells differ by at most floor(that) + 1, and the last
// cell's upper node adds one.  The 1e-3 covers the rounding of the device's fp32 coordinates.
int bg_axis_nodes(int tile, int n, int cells) {
	const int m = std::min(tile, n);
	return std::min(cells, (int)std::floor((double)(m - 1) / (double)n * (double)(cells - 1) + 1e-3) + 3);
}
// floats of one LDS footprint image for this shape, 0: the shape runs without LDS
int bg_lds_floats(const BgShape& s) {
	const long long n = 12ll * s.L * ((bg_axis_nodes(TW, s.W, s.Wg) * bg_axis_nodes(TH, s.H, s.Hg)) | 1);
	return n <= BG_LDS_FLOATS ? (int)n : 0;
}
int bg_check_shape(BgShape& s, int L, int Hg, int Wg, int H, int W, const char* who) {
	if (L < 2 || Hg < 2 || Wg < 2) { set_error(std::string(who) + ": the grid needs L, Hg, Wg >= 2"); return -1; }
	if (H < 1 || W < 1) { set_error(std::string(who) + ": the image needs H, W >= 1"); return -1; }
	if (12ll * L * Hg * Wg > 0x7fffffffll || (H + TH - 1) / TH > 65535) { set_error(std::string(who) + ": grid or image too large (12 L Hg Wg < 2^31, H <= 262140)"); return -1; }
	s = BgShape{L, Hg, Wg, H, W};
	return 0;
}
int bg_check_tv(TvShape& s, int N, int L, int Hg, int Wg, const char* who) {
	if (N < 1) { set_error(std::string(who) + ": N must be >= 1"); return -1; }
	if (L < 2 || Hg < 2 || Wg < 2) { set_error(std::string(who) + ": the grid needs L, Hg, Wg >= 2"); return -1; }
	if (12ll * L * Hg * Wg > 0x7fffffffll || (double)N * 12.0 * L * Hg * Wg > 5e11) { set_error(std::string(who) + ": grids too large"); return -1; }
	const double n12 = 12.0 * (double)N;
	s = TvShape{L, Hg, Wg, 12ll * N * L * Hg * Wg, (float)(1.0 / (n12 * (L - 1) * (double)Hg * Wg)), (float)(1.0 / (n12 * (double)L * (Hg - 1) * Wg)),
		(float)(1.0 / (n12 * (double)L * Hg * (Wg - 1)))};
	return 0;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_bilagrid_slice_forward(int L, int Hg, int Wg, const float* grid, int H, int W, const float* image, float* out, void* stream) {
	BgShape s;
	if (bg_check_shape(s, L, Hg, Wg, H, W, "adgs_bilagrid_slice_forward") != 0) return -1;
	if (!grid || !image || !out) { set_error("adgs_bilagrid_slice_forward: NULL grid / image / out"); return -1; }
	const dim3 blocks((W + TW - 1) / TW, (H + TH - 1) / TH);
	const int cap = bg_lds_floats(s);
	if (cap) hipLaunchKernelGGL(bg_slice_fwd_kernel<true>, blocks, dim3(256), (size_t)cap * sizeof(float), (hipStream_t)stream, s, grid, image, out, cap);
	else hipLaunchKernelGGL(bg_slice_fwd_kernel<false>, blocks, dim3(256), 0, (hipStream_t)stream, s, grid, image, out, 0);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_bilagrid_slice_backward(int L, int Hg, int Wg, const float* grid, int H, int W, const float* image, const float* dL_dout,
	float* dL_dgrid, float* dL_dimage, void* stream) {
	BgShape s;
	if (bg_check_shape(s, L, Hg, Wg, H, W, "adgs_bilagrid_slice_backward") != 0) return -1;
	if (!grid || !image || !dL_dout) { set_error("adgs_bilagrid_slice_backward: NULL grid / image / dL_dout"); return -1; }
	if (!dL_dgrid && !dL_dimage) return 0;
	const dim3 blocks((W + TW - 1) / TW, (H + TH - 1) / TH);
	const int cap = bg_lds_floats(s);
	if (cap) hipLaunchKernelGGL(bg_slice_bwd_kernel<true>, blocks, dim3(256), 2 * (size_t)cap * sizeof(float), (hipStream_t)stream, s, grid, image, dL_dout,
		dL_dgrid, dL_dimage, cap);
	else hipLaunchKernelGGL(bg_slice_bwd_kernel<false>, blocks, dim3(256), 0, (hipStream_t)stream, s, grid, image, dL_dout, dL_dgrid, dL_dimage, 0);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_bilagrid_tv_forward(int N, int L, int Hg, int Wg, const float* grids, double* work, float* loss, void* stream_) {
	TvShape s;
	if (bg_check_tv(s, N, L, Hg, Wg, "adgs_bilagrid_tv_forward") != 0) return -1;
	if (!grids || !work || !loss) { set_error("adgs_bilagrid_tv_forward: NULL grids / work / loss"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(bg_tv_sum_kernel, dim3(reduce_blocks(s.total)), dim3(SLOT_THREADS), 0, stream, s, grids, work);
	hipLaunchKernelGGL(bg_tv_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_bilagrid_tv_backward(int N, int L, int Hg, int Wg, const float* grids, const float* g_loss, float* dL_dgrids, void* stream) {
	TvShape s;
	if (bg_check_tv(s, N, L, Hg, Wg, "adgs_bilagrid_tv_backward") != 0) return -1;
	if (!grids || !g_loss || !dL_dgrids) { set_error("adgs_bilagrid_tv_backward: NULL grids / g_loss / dL_dgrids"); return -1; }
	hipLaunchKernelGGL(bg_tv_bwd_kernel, dim3((unsigned)((s.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s, grids, g_loss, dL_dgrids);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_test_bilagrid_path(int L, int Hg, int Wg, int H, int W) {
	BgShape s;
	if (bg_check_shape(s, L, Hg, Wg, H, W, "adgs_test_bilagrid_path") != 0) return -1;
	return bg_lds_floats(s) ? 1 : 0;
}
