// Per-Gaussian camera-space normals and the depth-normal consistency loss, forward and backward, for gfx950 (wave64).
// The definitions are in include/adgs_normals.h.
//
// Gaussian normals: one thread per Gaussian, 256-thread blocks.  The rows of scales / means3D (12 bytes) and rotations (16 bytes) are read
// once per launch through the helpers of stream_access.h; the 16 floats of the view matrix are read at a uniform address.  The forward
// writes only the columns it owns of the [N, stride] rows (the rasterizer reads them next: plain stores); the backward recomputes k and the
// sign from the inputs and writes each dL/drotations row once.
//
// Consistency loss: one 32x16 tile per workgroup of 256 threads, two pixels per thread.  The expected depth z and the validity of a pixel
// (O >= min_opacity and D > 0) are staged ONCE per workgroup with their halo in LDS; z is formed and kept in double (its inputs are exact
// floats, so the central differences of z carry no rounding of z itself -- at 1920 columns the float32 evaluation is not good to 1e-4), and
// the per-pixel arithmetic behind it is double as well: the pass is bound by its six float reads per pixel, not by arithmetic.
// Forward: halo 1; the sums (sum v e, sum v) go in double per thread, then through the slot rows (slot_reduce.h); the finish kernel stores
// the totals and L behind the rows.
// Backward: a gather with halo 2.  Phase 1: every staged pixel p of the tile plus a halo of 1 that is valid forms its depth normal once,
// writes dL/dN(p) when it lies in the tile, and stores the gradients of its two tangents g_tx(p), g_ty(p) in LDS (float).  Phase 2: a tile
// pixel q collects  r(q) . (g_tx(q - e_x) - g_tx(q + e_x) + g_ty(q - e_y) - g_ty(q + e_y))  -- t_x(p) = z(p + e_x) r(p + e_x) - z(p - e_x) r(p - e_x) --
// and writes dL/dD(q), dL/dO(q) once: no atomics, no zero fill, no intermediate image.
//
// Byte model (HBM): forward reads (5 + [weight]) * 4 * H * W bytes and writes the slot rows; backward reads the same and writes up to 5 * 4 * H * W.
#include "common.h"
#include "stream_access.h"
#include "slot_reduce.h"
#include "../../include/adgs_loss.h"
#include "../../include/adgs_normals.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

// ------------------------------------------------------------------------------------------------ Gaussian normals
constexpr int GN_BLOCK = 256;

struct GnRow {
	float q[4];        // the normalised quaternion (w, x, y, z)
	float inv;         // 1 / |q|
	int k;             // the shortest axis
	float sign;        // +1: n_c faces the camera as it is
	float nc[3];       // the un-flipped camera-space normal
};

// column k of R(q), q = (w, x, y, z) normalised
__device__ __forceinline__ void gn_column(const float* q, int k, float* n) {
	const float w = q[0], x = q[1], y = q[2], z = q[3];
	if (k == 0) { n[0] = 1.f - 2.f * (y * y + z * z); n[1] = 2.f * (x * y + w * z); n[2] = 2.f * (x * z - w * y); }
	else if (k == 1) { n[0] = 2.f * (x * y - w * z); n[1] = 1.f - 2.f * (x * x + z * z); n[2] = 2.f * (y * z + w * x); }
	else { n[0] = 2.f * (x * z + w * y); n[1] = 2.f * (y * z - w * x); n[2] = 1.f - 2.f * (x * x + y * y); }
}

__device__ __forceinline__ GnRow gn_row(size_t i, const float* __restrict__ scales, const float* __restrict__ rotations, bool rot16,
	const float* __restrict__ means3D, const float* __restrict__ m) {
	GnRow r;
	const float s0 = ld_stream(scales + 3 * i), s1 = ld_stream(scales + 3 * i + 1), s2 = ld_stream(scales + 3 * i + 2);
	const float p0 = ld_stream(means3D + 3 * i), p1 = ld_stream(means3D + 3 * i + 1), p2 = ld_stream(means3D + 3 * i + 2);
	float4 q;
	if (rot16) q = ld_stream4(reinterpret_cast<const float4*>(rotations) + i);
	else q = make_float4(ld_stream(rotations + 4 * i), ld_stream(rotations + 4 * i + 1), ld_stream(rotations + 4 * i + 2), ld_stream(rotations + 4 * i + 3));
	r.inv = 1.f / fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);        // the deformation pass's normalisation
	r.q[0] = q.x * r.inv; r.q[1] = q.y * r.inv; r.q[2] = q.z * r.inv; r.q[3] = q.w * r.inv;
	float best = s0;
	r.k = 0;
	if (s1 < best) { best = s1; r.k = 1; }
	if (s2 < best) { r.k = 2; }
	float nw[3];
	gn_column(r.q, r.k, nw);
	float d = 0.f;
#pragma unroll
	for (int j = 0; j < 3; j++) {
		r.nc[j] = m[j] * nw[0] + m[4 + j] * nw[1] + m[8 + j] * nw[2];
		const float pc = m[j] * p0 + m[4 + j] * p1 + m[8 + j] * p2 + m[12 + j];
		d += r.nc[j] * pc;
	}
	r.sign = d <= 0.f ? 1.f : -1.f;
	return r;
}

__global__ void __launch_bounds__(GN_BLOCK) gaussian_normals_fwd_kernel(int N, const float* __restrict__ scales, const float* __restrict__ rotations, int rot16,
	const float* __restrict__ means3D, const float* __restrict__ viewmatrix, const float* __restrict__ mask, int stride, int c0, float* __restrict__ out) {
	const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
	if (i >= (size_t)N) return;
	const GnRow r = gn_row(i, scales, rotations, rot16 != 0, means3D, viewmatrix);
	float* row = out + i * (size_t)stride;
	if (mask) row[0] = ld_stream(mask + i);
	row[c0] = r.sign * r.nc[0]; row[c0 + 1] = r.sign * r.nc[1]; row[c0 + 2] = r.sign * r.nc[2];
}

__global__ void __launch_bounds__(GN_BLOCK) gaussian_normals_bwd_kernel(int N, const float* __restrict__ scales, const float* __restrict__ rotations, int rot16,
	const float* __restrict__ means3D, const float* __restrict__ viewmatrix, const float* __restrict__ g, int stride, int c0, float* __restrict__ dL_drot, int out16) {
	const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
	if (i >= (size_t)N) return;
	const float* m = viewmatrix;
	const GnRow r = gn_row(i, scales, rotations, rot16 != 0, means3D, m);
	const float* grow = g + i * (size_t)stride + c0;
	const float g0 = r.sign * ld_stream(grow), g1 = r.sign * ld_stream(grow + 1), g2 = r.sign * ld_stream(grow + 2);
	// through the view rotation: dL/dn_w[a] = sum_j m[4 a + j] dL/dn_c[j]
	const float a = m[0] * g0 + m[1] * g1 + m[2] * g2, b = m[4] * g0 + m[5] * g1 + m[6] * g2, c = m[8] * g0 + m[9] * g1 + m[10] * g2;
	const float w = r.q[0], x = r.q[1], y = r.q[2], z = r.q[3];
	float gq[4];        // dL/d(qh) through column k of R
	if (r.k == 0) {
		gq[0] = 2.f * (z * b - y * c);
		gq[1] = 2.f * (y * b + z * c);
		gq[2] = -4.f * y * a + 2.f * (x * b - w * c);
		gq[3] = -4.f * z * a + 2.f * (w * b + x * c);
	} else if (r.k == 1) {
		gq[0] = 2.f * (x * c - z * a);
		gq[1] = -4.f * x * b + 2.f * (y * a + w * c);
		gq[2] = 2.f * (x * a + z * c);
		gq[3] = -4.f * z * b + 2.f * (y * c - w * a);
	} else {
		gq[0] = 2.f * (y * a - x * b);
		gq[1] = -4.f * x * c + 2.f * (z * a - w * b);
		gq[2] = -4.f * y * c + 2.f * (w * a + z * b);
		gq[3] = 2.f * (x * a + y * b);
	}
	// the normalisation: d(q / |q|) / dq = (I - qh qh^T) / |q|
	const float along = w * gq[0] + x * gq[1] + y * gq[2] + z * gq[3];
	const float4 o = make_float4((gq[0] - w * along) * r.inv, (gq[1] - x * along) * r.inv, (gq[2] - y * along) * r.inv, (gq[3] - z * along) * r.inv);
	if (out16) st_stream4(reinterpret_cast<float4*>(dL_drot) + i, o);
	else { st_stream(dL_drot + 4 * i, o.x); st_stream(dL_drot + 4 * i + 1, o.y); st_stream(dL_drot + 4 * i + 2, o.z); st_stream(dL_drot + 4 * i + 3, o.w); }
}

int gn_check(const char* who, int N, int stride, int c0, bool mask, bool null_pointer) {
	const std::string name(who);
	if (null_pointer) { set_error(name + ": NULL pointer"); return -1; }
	if (N < 0) { set_error(name + ": negative N"); return -1; }
	if (stride < 3 || stride > 32) { set_error(name + ": stride must lie in [3, 32]"); return -1; }
	if (c0 < 0 || c0 + 3 > stride) { set_error(name + ": columns c0 .. c0 + 2 must lie in [0, stride)"); return -1; }
	if (mask && c0 == 0) { set_error(name + ": a mask goes to column 0 and needs c0 >= 1"); return -1; }
	return 0;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ------------------------------------------------------------------------------------------------ depth-normal consistency
constexpr int NC_TX = 32, NC_TY = 16, NC_LT = 256;
constexpr int NC_ROW = 2;                                       // doubles per slot row
constexpr int NC_MAX_TILES = (1 << 24) - 1;                     // tiles * 256 threads must stay below 2^32
static_assert(NC_LT == SLOT_THREADS && ADGS_NORMAL_WORK_DOUBLES >= ADGS_LOSS_SLOTS * NC_ROW + 3, "slot_add_wave's workgroup; three scalars behind the rows");
enum { NC_SVE = 0, NC_SV, NC_L };                              // the scalars behind the rows: sum v e, sum v, L

struct NcView {
	int H, W;
	double tx, ty;          // tanfovx, tanfovy
	double dx, dy;          // 2 tanfovx / W, 2 tanfovy / H: the ray step of one pixel
	float min_opacity;
	int inv_depth;
};

template <int HALO> struct NcRegion {
	static constexpr int RX = NC_TX + 2 * HALO, RY = NC_TY + 2 * HALO, RN = RX * RY;
};

// Stages z (double; 0 where invalid) and the validity O >= min_opacity && D > 0 (0 outside the image) of the region around tile (x0, y0).
// Ends with a barrier.
template <int HALO>
__device__ __forceinline__ void nc_stage(const NcView& v, const float* __restrict__ depth, const float* __restrict__ opacity, int x0, int y0, int tid,
	double* sz, unsigned char* sv) {
	using R = NcRegion<HALO>;
	constexpr int NI = (R::RN + NC_LT - 1) / NC_LT;
	float vd[NI], vo[NI];
	bool in[NI];
#pragma unroll
	for (int it = 0; it < NI; it++) {                           // every load in flight before the first division
		const int i = min(tid + it * NC_LT, R::RN - 1);
		const int ry = i / R::RX, rx = i - ry * R::RX;
		const int gy = y0 - HALO + ry, gx = x0 - HALO + rx;
		in[it] = gy >= 0 && gy < v.H && gx >= 0 && gx < v.W;
		const int off = min(max(gy, 0), v.H - 1) * v.W + min(max(gx, 0), v.W - 1);      // H * W <= INT_MAX
		vd[it] = depth[off];
		vo[it] = opacity[off];
	}
#pragma unroll
	for (int it = 0; it < NI; it++) {
		const int i = tid + it * NC_LT;
		if (i >= R::RN) continue;
		const bool ok = in[it] && vo[it] >= v.min_opacity && vd[it] > 0.f;
		sv[i] = ok ? 1 : 0;
		sz[i] = ok ? (v.inv_depth ? (double)vo[it] / (double)vd[it] : (double)vd[it] / (double)vo[it]) : 0.0;
	}
	__syncthreads();
}

// m of the pixel (gx, gy) staged at element i of a region RX wide
__device__ __forceinline__ bool nc_valid(const NcView& v, const unsigned char* sv, int i, int RX, int gx, int gy) {
	return gx >= 1 && gx <= v.W - 2 && gy >= 1 && gy <= v.H - 2 && sv[i] && sv[i - 1] && sv[i + 1] && sv[i - RX] && sv[i + RX];
}

__device__ __forceinline__ double nc_ray_x(const NcView& v, int gx) { return ((2.0 * (double)gx + 1.0) / (double)v.W - 1.0) * v.tx; }
__device__ __forceinline__ double nc_ray_y(const NcView& v, int gy) { return ((2.0 * (double)gy + 1.0) / (double)v.H - 1.0) * v.ty; }

// the two tangents, their cross product c = t_y x t_x and sigma = sqrt(c . c + 1e-30) at the pixel staged at element i
__device__ __forceinline__ void nc_depth_normal(const NcView& v, const double* sz, int i, int RX, int gx, int gy, double* t_x, double* t_y, double* c, double& sigma) {
	const double rx = nc_ray_x(v, gx), ry = nc_ray_y(v, gy);
	const double zxp = sz[i + 1], zxm = sz[i - 1], zyp = sz[i + RX], zym = sz[i - RX];
	const double ax = zxp - zxm, ay = zyp - zym;
	t_x[0] = ax * rx + (zxp + zxm) * v.dx; t_x[1] = ax * ry; t_x[2] = ax;
	t_y[0] = ay * rx; t_y[1] = ay * ry + (zyp + zym) * v.dy; t_y[2] = ay;
	c[0] = t_y[1] * t_x[2] - t_y[2] * t_x[1];
	c[1] = t_y[2] * t_x[0] - t_y[0] * t_x[2];
	c[2] = t_y[0] * t_x[1] - t_y[1] * t_x[0];
	sigma = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + 1e-30);
}

// LOSS: the two sums into the slot rows; otherwise m n_d into out [3, H, W]
template <bool LOSS>
__global__ void __launch_bounds__(NC_LT) normal_consistency_fwd_kernel(NcView v, int tiles_x, const float* __restrict__ normal, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ weight, double* __restrict__ work, float* __restrict__ out) {
	using R = NcRegion<1>;
	__shared__ double sz[R::RN];
	__shared__ unsigned char sv[R::RN];
	const int tid = threadIdx.x;
	const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
	const int x0 = bx * NC_TX, y0 = by * NC_TY;
	nc_stage<1>(v, depth, opacity, x0, y0, tid, sz, sv);
	const size_t plane = (size_t)v.H * v.W;
	const int lx = tid & (NC_TX - 1), gx = x0 + lx;
	double acc[NC_ROW] = { 0.0, 0.0 };                          // sum v e, sum v
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int ly = 2 * (tid >> 5) + o, gy = y0 + ly;
		if (gx >= v.W || gy >= v.H) continue;
		const int i = (ly + 1) * R::RX + lx + 1;
		const size_t p = (size_t)gy * v.W + gx;
		const bool m = nc_valid(v, sv, i, R::RX, gx, gy);
		double nd[3] = { 0.0, 0.0, 0.0 };
		if (m) {
			double t_x[3], t_y[3], c[3], sigma;
			nc_depth_normal(v, sz, i, R::RX, gx, gy, t_x, t_y, c, sigma);
			nd[0] = c[0] / sigma; nd[1] = c[1] / sigma; nd[2] = c[2] / sigma;
		}
		if constexpr (LOSS) {
			if (!m) continue;
			const double w = weight ? (double)weight[p] : 1.0;
			const double n0 = normal[p], n1 = normal[plane + p], n2 = normal[2 * plane + p];
			const double rho = sqrt(n0 * n0 + n1 * n1 + n2 * n2 + 1e-12);
			const double e = 1.0 - (n0 * nd[0] + n1 * nd[1] + n2 * nd[2]) / rho;
			acc[NC_SVE] += w * e; acc[NC_SV] += w;
		} else {
			out[p] = (float)nd[0]; out[plane + p] = (float)nd[1]; out[2 * plane + p] = (float)nd[2];
		}
	}
	if constexpr (LOSS) slot_add_wave<ADGS_LOSS_SLOTS, NC_ROW>(work, acc);
}

// one block: totals of the slot rows (left zero) -> the scalars behind them and the loss
__global__ void __launch_bounds__(SLOT_THREADS) normal_consistency_finish_kernel(double* __restrict__ work, float* __restrict__ loss) {
	double t[NC_ROW];
	slot_finish<ADGS_LOSS_SLOTS, NC_ROW>(work, t);
	if (threadIdx.x == 0) {
		double* tot = work + (size_t)ADGS_LOSS_SLOTS * NC_ROW;
		for (int q = 0; q < NC_ROW; q++) tot[q] = t[q];
		const double L = tot[NC_SV] > 0.0 ? tot[NC_SVE] / tot[NC_SV] : 0.0;
		tot[NC_L] = L;
		loss[0] = (float)L;
	}
}

__global__ void __launch_bounds__(NC_LT) normal_consistency_bwd_kernel(NcView v, int tiles_x, const float* __restrict__ normal, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ weight, const double* __restrict__ work, const float* __restrict__ g_loss,
	float* __restrict__ dL_dnormal, float* __restrict__ dL_ddepth, float* __restrict__ dL_dopacity) {
	using R = NcRegion<2>;
	constexpr int IX = NC_TX + 2, IY = NC_TY + 2, IN = IX * IY;        // the tile plus a halo of 1: the pixels whose depth normal the tile needs
	__shared__ double sz[R::RN];
	__shared__ unsigned char sv[R::RN];
	__shared__ float gtx[IN][3], gty[IN][3];
	const int tid = threadIdx.x;
	const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
	const int x0 = bx * NC_TX, y0 = by * NC_TY;
	nc_stage<2>(v, depth, opacity, x0, y0, tid, sz, sv);
	const size_t plane = (size_t)v.H * v.W;
	const double sum_v = work[(size_t)ADGS_LOSS_SLOTS * NC_ROW + NC_SV];
	const double gs = sum_v > 0.0 ? (double)g_loss[0] / sum_v : 0.0;
	const bool chain = dL_ddepth || dL_dopacity;
	// phase 1
	for (int j = tid; j < IN; j += NC_LT) {
		const int jy = j / IX, jx = j - jy * IX;
		const int gx = x0 - 1 + jx, gy = y0 - 1 + jy;
		const int i = (jy + 1) * R::RX + jx + 1;
		const bool in_tile = jx >= 1 && jx <= NC_TX && jy >= 1 && jy <= NC_TY && gx < v.W && gy < v.H;
		double dn[3] = { 0.0, 0.0, 0.0 }, a_x[3] = { 0.0, 0.0, 0.0 }, a_y[3] = { 0.0, 0.0, 0.0 };
		if ((in_tile || chain) && nc_valid(v, sv, i, R::RX, gx, gy)) {
			const size_t p = (size_t)gy * v.W + gx;
			const double a = gs * (weight ? (double)weight[p] : 1.0);          // dL/de(p)
			if (a != 0.0) {
				const double n0 = normal[p], n1 = normal[plane + p], n2 = normal[2 * plane + p];
				double t_x[3], t_y[3], c[3], sigma;
				nc_depth_normal(v, sz, i, R::RX, gx, gy, t_x, t_y, c, sigma);
				const double nd[3] = { c[0] / sigma, c[1] / sigma, c[2] / sigma };
				const double rho = sqrt(n0 * n0 + n1 * n1 + n2 * n2 + 1e-12);
				const double nh[3] = { n0 / rho, n1 / rho, n2 / rho };
				const double dot = nh[0] * nd[0] + nh[1] * nd[1] + nh[2] * nd[2];
				double gc[3];                                                 // dL/dc = -a (Nh - n_d (n_d . Nh)) / sigma
#pragma unroll
				for (int k = 0; k < 3; k++) {
					dn[k] = -a * (nd[k] - nh[k] * dot) / rho;
					gc[k] = -a * (nh[k] - nd[k] * dot) / sigma;
				}
				// c = t_y x t_x:  dL/dt_y = t_x x g_c,  dL/dt_x = g_c x t_y
				a_y[0] = t_x[1] * gc[2] - t_x[2] * gc[1]; a_y[1] = t_x[2] * gc[0] - t_x[0] * gc[2]; a_y[2] = t_x[0] * gc[1] - t_x[1] * gc[0];
				a_x[0] = gc[1] * t_y[2] - gc[2] * t_y[1]; a_x[1] = gc[2] * t_y[0] - gc[0] * t_y[2]; a_x[2] = gc[0] * t_y[1] - gc[1] * t_y[0];
			}
		}
#pragma unroll
		for (int k = 0; k < 3; k++) { gtx[j][k] = (float)a_x[k]; gty[j][k] = (float)a_y[k]; }
		if (in_tile && dL_dnormal) {
			const size_t p = (size_t)gy * v.W + gx;
			dL_dnormal[p] = (float)dn[0]; dL_dnormal[plane + p] = (float)dn[1]; dL_dnormal[2 * plane + p] = (float)dn[2];
		}
	}
	if (!chain) return;
	__syncthreads();
	// phase 2
	const int lx = tid & (NC_TX - 1), gx = x0 + lx;
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int ly = 2 * (tid >> 5) + o, gy = y0 + ly;
		if (gx >= v.W || gy >= v.H) continue;
		const size_t p = (size_t)gy * v.W + gx;
		const int j = (ly + 1) * IX + lx + 1;
		float gd = 0.f, go = 0.f;
		if (sv[(ly + 2) * R::RX + lx + 2]) {
			double G[3];
#pragma unroll
			for (int k = 0; k < 3; k++) G[k] = ((double)gtx[j - 1][k] - (double)gtx[j + 1][k]) + ((double)gty[j - IX][k] - (double)gty[j + IX][k]);
			const double gz = nc_ray_x(v, gx) * G[0] + nc_ray_y(v, gy) * G[1] + G[2];
			if (gz != 0.0) {
				const double D = depth[p], O = opacity[p];
				if (v.inv_depth) { gd = (float)(-gz * O / (D * D)); go = (float)(gz / D); }
				else { gd = (float)(gz / O); go = (float)(-gz * D / (O * O)); }
			}
		}
		if (dL_ddepth) dL_ddepth[p] = gd;
		if (dL_dopacity) dL_dopacity[p] = go;
	}
}

int nc_check(const char* who, int H, int W, float tanfovx, float tanfovy, float min_opacity, bool null_pointer, long long& tiles, NcView& v, int inv_depth) {
	const std::string name(who);
	if (null_pointer) { set_error(name + ": NULL pointer"); return -1; }
	if (H < 0 || W < 0) { set_error(name + ": negative H or W"); return -1; }
	if ((long long)H * W > (long long)INT_MAX) { set_error(name + ": H * W exceeds INT_MAX"); return -1; }
	if (!std::isfinite(tanfovx) || !std::isfinite(tanfovy) || !(tanfovx > 0.f) || !(tanfovy > 0.f)) { set_error(name + ": tanfovx and tanfovy must be finite and > 0"); return -1; }
	if (!std::isfinite(min_opacity) || !(min_opacity > 0.f) || !(min_opacity <= 1.f)) { set_error(name + ": min_opacity must lie in (0, 1]"); return -1; }
	tiles = (long long)((W + NC_TX - 1) / NC_TX) * ((H + NC_TY - 1) / NC_TY);
	if (tiles > NC_MAX_TILES) { set_error(name + ": more than 16777215 tiles of 32 x 16 pixels"); return -1; }
	v.H = H; v.W = W; v.tx = (double)tanfovx; v.ty = (double)tanfovy;
	v.dx = W ? 2.0 * v.tx / (double)W : 0.0; v.dy = H ? 2.0 * v.ty / (double)H : 0.0;
	v.min_opacity = min_opacity; v.inv_depth = inv_depth ? 1 : 0;
	return 0;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_gaussian_normals_forward(int N, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
	const float* mask, int stride, int c0, float* out, void* stream_) {
	if (gn_check("adgs_gaussian_normals_forward", N, stride, c0, mask != nullptr, !scales || !rotations || !means3D || !viewmatrix || !out)) return -1;
	if (N == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(gaussian_normals_fwd_kernel, dim3((unsigned)((N + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, stream, N, scales, rotations,
		aligned16(rotations) ? 1 : 0, means3D, viewmatrix, mask, stride, c0, out);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_gaussian_normals_backward(int N, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
	const float* g, int stride, int c0, float* dL_drotations, void* stream_) {
	if (gn_check("adgs_gaussian_normals_backward", N, stride, c0, false, !scales || !rotations || !means3D || !viewmatrix || !g || !dL_drotations)) return -1;
	if (N == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3((unsigned)((N + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, stream, N, scales, rotations,
		aligned16(rotations) ? 1 : 0, means3D, viewmatrix, g, stride, c0, dL_drotations, aligned16(dL_drotations) ? 1 : 0);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_normal_consistency_forward(int H, int W, const float* normal, const float* depth, const float* opacity, const float* weight,
	float tanfovx, float tanfovy, int inv_depth, float min_opacity, double* work, float* loss, void* stream_) {
	long long tiles = 0;
	NcView v;
	if (nc_check("adgs_normal_consistency_forward", H, W, tanfovx, tanfovy, min_opacity, !normal || !depth || !opacity || !work || !loss, tiles, v, inv_depth)) return -1;
	if (tiles == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const int tiles_x = (W + NC_TX - 1) / NC_TX;
	hipLaunchKernelGGL(normal_consistency_fwd_kernel<true>, dim3((unsigned)tiles), dim3(NC_LT), 0, stream, v, tiles_x, normal, depth, opacity, weight, work, (float*)nullptr);
	hipLaunchKernelGGL(normal_consistency_finish_kernel, dim3(1), dim3(SLOT_THREADS), 0, stream, work, loss);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_normal_consistency_backward(int H, int W, const float* normal, const float* depth, const float* opacity, const float* weight,
	float tanfovx, float tanfovy, int inv_depth, float min_opacity, const double* work, const float* g_loss,
	float* dL_dnormal, float* dL_ddepth, float* dL_dopacity, void* stream_) {
	long long tiles = 0;
	NcView v;
	if (nc_check("adgs_normal_consistency_backward", H, W, tanfovx, tanfovy, min_opacity, !normal || !depth || !opacity || !work || !g_loss, tiles, v, inv_depth)) return -1;
	if (tiles == 0 || (!dL_dnormal && !dL_ddepth && !dL_dopacity)) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const int tiles_x = (W + NC_TX - 1) / NC_TX;
	hipLaunchKernelGGL(normal_consistency_bwd_kernel, dim3((unsigned)tiles), dim3(NC_LT), 0, stream, v, tiles_x, normal, depth, opacity, weight, work, g_loss,
		dL_dnormal, dL_ddepth, dL_dopacity);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_depth_to_normal(int H, int W, const float* depth, const float* opacity, float tanfovx, float tanfovy, int inv_depth,
	float min_opacity, float* out, void* stream_) {
	long long tiles = 0;
	NcView v;
	if (nc_check("adgs_depth_to_normal", H, W, tanfovx, tanfovy, min_opacity, !depth || !opacity || !out, tiles, v, inv_depth)) return -1;
	if (tiles == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const int tiles_x = (W + NC_TX - 1) / NC_TX;
	hipLaunchKernelGGL(normal_consistency_fwd_kernel<false>, dim3((unsigned)tiles), dim3(NC_LT), 0, stream, v, tiles_x, (const float*)nullptr, depth, opacity,
		(const float*)nullptr, (double*)nullptr, out);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
