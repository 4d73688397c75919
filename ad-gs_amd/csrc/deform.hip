// Fused per-frame deformation for gfx950: B-spline / polynomial / Fourier trajectories,
// cumulative quaternion B-spline, scene||object concatenation and the activations
// (exp, sigmoid x time mask, normalize) in ONE streaming pass, with a hand-written backward.
//
// Reference semantics: utils/func_utils.py:121-173 (get_func_result) and
// scene/gaussian_model.py:88-231 (getters / get_deformed_pkg); the roma quaternion helpers
// (unitquat_to_rotvec / rotvec_to_unitquat / quat_product, XYZW) are restated from the
// library's published algorithm (see oracle/deform_oracle.py for the parity status).
//
// Roofline: HBM streaming.  Per Gaussian the forward reads the raw parameters once
// (59 floats + deformation rows) and writes the 59 activated floats the rasterizer reads;
// the backward reads the 59 upstream gradients and writes every parameter gradient.
//
// This file: the generic get_func_result kernels, the geometry kernels, their launch plan and the C entry points.  The quaternion
// spline is in quat_spline.h, the SH tensor / sh0 / parameter-gradient kernels in deform_sh.hip.
#include "common.h"
#include "kernels.h"
#include "quat_spline.h"
#include "../../include/adgs_testing.h"
#include <initializer_list>
#include <cstring>
#include <algorithm>

namespace adgs {
namespace {

// ------------------------------------------------------------------ generic get_func_result
template <int D, int NQ>
__global__ void __launch_bounds__(256) func_eval_fwd_kernel(int N, const float* __restrict__ param, adgs_func_eval f, float* __restrict__ out) {
	const int n = blockIdx.x * blockDim.x + threadIdx.x;
	if (n >= N) return;
	const float* p = param + (size_t)n * D * f.n_params;
	float res[D];
#pragma unroll
	for (int d = 0; d < D; d++) res[d] = lin_eval(p + d * f.n_params, f);
	if (D == 4 && NQ > 0) {
		const Q qv = quat_spline_eval<(NQ > 0 ? NQ : 1), false>(p, f, nullptr);
		res[0] = res[0] + qv.w; res[1] = res[1] + qv.x; res[2] = res[2] + qv.y; res[3 % D] = res[3 % D] + qv.z;
	}
#pragma unroll
	for (int d = 0; d < D; d++) out[(size_t)n * D + d] = res[d];
}
template <int D, int NQ>
__global__ void __launch_bounds__(256) func_eval_bwd_kernel(int N, const float* __restrict__ param, adgs_func_eval f,
	const float* __restrict__ dL_dout, float* __restrict__ dL_dparam) {
	const int n = blockIdx.x * blockDim.x + threadIdx.x;
	if (n >= N) return;
	const float* p = param + (size_t)n * D * f.n_params;
	float* gp = dL_dparam + (size_t)n * D * f.n_params;
	float g[D];
#pragma unroll
	for (int d = 0; d < D; d++) { g[d] = dL_dout[(size_t)n * D + d]; lin_bwd(gp + d * f.n_params, f, g[d]); }
	if (D == 4 && NQ > 0) {
		QuatSave<(NQ > 0 ? NQ : 1)> st;
		const Q out = quat_spline_eval<(NQ > 0 ? NQ : 1), true>(p, f, &st);
		quat_spline_bwd<(NQ > 0 ? NQ : 1)>(st, out, f, { g[0], g[1], g[2], g[3 % D] }, gp);
	}
}

// ------------------------------------------------------------------ fused get_deformed_pkg
// One thread per Gaussian of [n_begin, n_end).  The object Gaussians' deformation rows ([3][Cx] for xyz,
// [4][Cr] for the rotation) are staged through LDS with coalesced loads (func_eval.h: stage_rows), one
// parameter family after the other in the same buffer; the host launches the scene range without LDS.
// xyz is evaluated at the camera time and, when flow_xyz is given, at the flow time from the same staged
// rows (gaussian_renderer/__init__.py:57 calls get_deformed_xyz a second time for it).
struct DeformArgs {
	adgs_deform_params p; adgs_func_eval fx, fr, fb, fx2, fb2; adgs_deform_outputs o; float* flow_xyz;
	int stride_x, stride_r;
	int scene4;          // scene range as groups of four Gaussians with 16-byte accesses (every pointer 16-byte aligned)
	int xyz_rows;        // object xyz rows read directly (deform_fwd_xyz_rows) instead of staged through LDS
};

// ---- the elementwise steps every range shares, scalar and four wide
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 add3(float4 v, float a, float b, float c, float d) { return make_float4(v.x + a, v.y + b, v.z + c, v.w + d); }
__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float4 sigmoid(float4 x) { return make_float4(sigmoid(x.x), sigmoid(x.y), sigmoid(x.z), sigmoid(x.w)); }
__device__ __forceinline__ float sigmoid_bwd(float g, float mask, float sg) { return g * mask * sg * (1.f - sg); }      // sg = sigmoid(x); mask: the time mask (scene: 1)
__device__ __forceinline__ float4 exp4(float4 v) { return make_float4(expf(v.x), expf(v.y), expf(v.z), expf(v.w)); }
__device__ __forceinline__ float4 quat_normalize(float x, float y, float z, float w) {
	const float inv = 1.f / fmaxf(sqrtf(x * x + y * y + z * z + w * w), 1e-12f);
	return make_float4(x * inv, y * inv, z * inv, w * inv);
}
// gradient of quat_normalize at u = (q.x .. q.w) for the upstream gradient g
__device__ __forceinline__ float4 quat_normalize_bwd(float4 q, float4 g) {
	const float nr = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
	const float inv = 1.f / fmaxf(nr, 1e-12f);
	const float r0 = q.x * inv, r1 = q.y * inv, r2 = q.z * inv, r3 = q.w * inv;
	const float dot = ((r0 * g.x + r1 * g.y) + r2 * g.z) + r3 * g.w;
	if (nr > 1e-12f) return make_float4((g.x - r0 * dot) * inv, (g.y - r1 * dot) * inv, (g.z - r2 * dot) * inv, (g.w - r3 * dot) * inv);
	return make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
}
// the background row's offsets of the three components at the camera time (bg) and at the flow time (bg2); zero where that
// output or family is absent.  Compile-time row offsets: deform_fwd_xyz_rows picks its component from the results afterwards.
__device__ __forceinline__ void bg_offsets(const float* bgp, const adgs_func_eval& fb, const adgs_func_eval& fb2, bool want, bool want2,
	float (&bg)[3], float (&bg2)[3]) {
#pragma unroll
	for (int d = 0; d < 3; d++) bg[d] = bg2[d] = 0.f;
	if (!bgp) return;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		if (want && has_lin(fb)) bg[d] = lin_eval(bgp + d * fb.n_params, fb);
		if (want2 && has_lin(fb2)) bg2[d] = lin_eval(bgp + d * fb2.n_params, fb2);
	}
}

// ---- scene range, four Gaussians per thread: every tensor of the scene Gaussians is a plain elementwise map
// (copy + background offset, normalise, sigmoid, exp), and [N,3] rows read or written one Gaussian per thread are 12-byte
// strided accesses that reach ~1.9 TB/s (measured: 41.6 us for 800 k Gaussians, 80 MB).  Twelve floats = three float4:
// a thread that owns four consecutive Gaussians only ever issues aligned 16-byte loads and stores.
__device__ __forceinline__ void deform_fwd_scene_one(const DeformArgs& a, int n, const float* bg, const float* bg2) {
	// one scene Gaussian, scalar accesses (the < 4 Gaussians behind the last full group)
	for (int d = 0; d < 3; d++) {
		const float v = a.p.scene_xyz[3 * (size_t)n + d];
		if (a.o.xyz) a.o.xyz[3 * (size_t)n + d] = v + bg[d];
		if (a.flow_xyz) a.flow_xyz[3 * (size_t)n + d] = v + bg2[d];
	}
	if (a.o.rotation) {
		const float4 q = ld4(a.p.scene_rotation + 4 * (size_t)n);
		st4(a.o.rotation + 4 * (size_t)n, quat_normalize(q.x, q.y, q.z, q.w));
	}
	if (a.o.opacity) a.o.opacity[n] = sigmoid(a.p.scene_opacity[n]);
	if (a.o.scales) for (int d = 0; d < 3; d++) a.o.scales[3 * (size_t)n + d] = expf(a.p.scene_scaling[3 * (size_t)n + d]);
}
__device__ __forceinline__ void deform_fwd_scene4(const DeformArgs& a, int blk) {
	const int g = blk * blockDim.x + threadIdx.x;          // group of Gaussians 4g .. 4g+3
	const int Ns = a.p.Ns;
	if (4 * (size_t)g >= (size_t)Ns) return;
	float bg[3], bg2[3];
	bg_offsets(a.p.background_deform_param, a.fb, a.fb2, a.o.xyz != nullptr, a.flow_xyz != nullptr, bg, bg2);
	if (4 * g + 4 > Ns) { for (int n = 4 * g; n < Ns; n++) deform_fwd_scene_one(a, n, bg, bg2); return; }
	const size_t o3 = 12 * (size_t)g, o4 = 16 * (size_t)g;
	if (a.o.xyz || a.flow_xyz) {
		const float4 v0 = ld4(a.p.scene_xyz + o3), v1 = ld4(a.p.scene_xyz + o3 + 4), v2 = ld4(a.p.scene_xyz + o3 + 8);
		// component pattern of twelve consecutive floats: x y z x | y z x y | z x y z   (v + 0.0 keeps v bit for bit)
		if (a.o.xyz) {
			st4(a.o.xyz + o3, add3(v0, bg[0], bg[1], bg[2], bg[0])); st4(a.o.xyz + o3 + 4, add3(v1, bg[1], bg[2], bg[0], bg[1]));
			st4(a.o.xyz + o3 + 8, add3(v2, bg[2], bg[0], bg[1], bg[2]));
		}
		if (a.flow_xyz) {
			st4(a.flow_xyz + o3, add3(v0, bg2[0], bg2[1], bg2[2], bg2[0])); st4(a.flow_xyz + o3 + 4, add3(v1, bg2[1], bg2[2], bg2[0], bg2[1]));
			st4(a.flow_xyz + o3 + 8, add3(v2, bg2[2], bg2[0], bg2[1], bg2[2]));
		}
	}
	if (a.o.rotation) {
		float4 q[4];
#pragma unroll
		for (int k = 0; k < 4; k++) q[k] = ld4(a.p.scene_rotation + o4 + 4 * k);
#pragma unroll
		for (int k = 0; k < 4; k++) st4(a.o.rotation + o4 + 4 * k, quat_normalize(q[k].x, q[k].y, q[k].z, q[k].w));
	}
	if (a.o.opacity) st4(a.o.opacity + 4 * (size_t)g, sigmoid(ld4(a.p.scene_opacity + 4 * (size_t)g)));
	if (a.o.scales) {
#pragma unroll
		for (int k = 0; k < 3; k++) st4(a.o.scales + o3 + 4 * k, exp4(ld4(a.p.scene_scaling + o3 + 4 * k)));
	}
}

// PARTS: bit 0 = xyz / flow, bit 1 = rotation, bit 2 = opacity + scales (the object range is covered twice, by an xyz block set and a
// rotation block set, so that the two LDS-staged phases run side by side instead of one after the other in every block)
constexpr int DP_XYZ = 1, DP_ROT = 2, DP_REST = 4;
template <int PARTS, bool OBJ, int NQ>
__device__ __forceinline__ void deform_fwd_body(const DeformArgs& a, int blk, int n_begin, int n_end, float* __restrict__ s_rows) {
	const int tid = threadIdx.x, B = blockDim.x, base = n_begin + blk * B;
	const int Ns = a.p.Ns;
	const int count = min(B, n_end - base);
	const int n = base + tid;
	const bool valid = tid < count;
	const bool is_obj = OBJ && valid && n >= Ns;
	const int m = is_obj ? n - Ns : n;
	const bool blk_obj = OBJ && base + count > Ns;   // block-uniform: some member is an object Gaussian
	// ---- xyz (gaussian_model.py:173-185), at t and at the flow time
	if ((PARTS & DP_XYZ) && (a.o.xyz || a.flow_xyz)) {
		const int np = a.fx.n_params;
		const bool lin1 = a.o.xyz && a.p.xyz_deform_param && has_lin(a.fx);
		const bool lin2 = a.flow_xyz && a.p.xyz_deform_param && has_lin(a.fx2);
		const bool staged = blk_obj && (lin1 || lin2);
		if (staged) {
			stage_rows<true>(s_rows, a.stride_x, 3 * np, base, count, Ns, (const float*)nullptr, a.p.xyz_deform_param, tid, B);
			__syncthreads();
		}
		if (valid) {
			float bg[3], bg2[3];
			bg_offsets(a.p.background_deform_param, a.fb, a.fb2, a.o.xyz != nullptr, a.flow_xyz != nullptr, bg, bg2);
			const float* bp = is_obj ? a.p.obj_xyz + 3 * (size_t)m : a.p.scene_xyz + 3 * (size_t)m;
			const float* row = s_rows + tid * a.stride_x;
#pragma unroll
			for (int d = 0; d < 3; d++) {
				const float v = bp[d];
				if (a.o.xyz) {
					float v1 = v;
					if (is_obj && lin1) v1 = v1 + lin_eval(row + d * np, a.fx);
					a.o.xyz[3 * (size_t)n + d] = v1 + bg[d];
				}
				if (a.flow_xyz) {
					float v2 = v;
					if (is_obj && lin2) v2 = v2 + lin_eval(row + d * np, a.fx2);
					a.flow_xyz[3 * (size_t)n + d] = v2 + bg2[d];
				}
			}
		}
		if (staged) __syncthreads();                  // the buffer is reused below
	}
	// ---- rotation (gaussian_model.py:187-196): normalize(cat(scene_rot, obj_rot))
	if ((PARTS & DP_ROT) && a.o.rotation) {
		const int np = a.fr.n_params;
		const bool staged = blk_obj && a.p.rotation_deform_param != nullptr;
		if (staged) {
			stage_rows<true>(s_rows, a.stride_r, 4 * np, base, count, Ns, (const float*)nullptr, a.p.rotation_deform_param, tid, B);
			__syncthreads();
		}
		if (valid) {
			float u[4];
			if (!OBJ || !is_obj) {
				// four 4-byte loads: this body serves the scene range exactly when scene4_ok found a pointer that is not 16-byte aligned
				const float* q = a.p.scene_rotation + 4 * (size_t)m;
				u[0] = q[0]; u[1] = q[1]; u[2] = q[2]; u[3] = q[3];
			} else {
				const float* rp = a.p.rotation_deform_param ? s_rows + tid * a.stride_r : nullptr;
				float fv[4] = { 0.f, 0.f, 0.f, 0.f };
				if (rp) {
#pragma unroll
					for (int d = 0; d < 4; d++) fv[d] = lin_eval(rp + d * np, a.fr);
					if (NQ > 0) { const Q qv = quat_spline_eval<(NQ > 0 ? NQ : 1), false>(rp, a.fr, nullptr); fv[0] += qv.w; fv[1] += qv.x; fv[2] += qv.y; fv[3] += qv.z; }
				}
				if (a.fr.quat_start >= 0) {
#pragma unroll
					for (int d = 0; d < 4; d++) u[d] = fv[d];          // quaternion spline replaces _obj_rotation (:189-190)
				} else {
#pragma unroll
					for (int d = 0; d < 4; d++) u[d] = a.p.obj_rotation[4 * (size_t)m + d] + fv[d];
				}
			}
			st4(a.o.rotation + 4 * (size_t)n, quat_normalize(u[0], u[1], u[2], u[3]));
		}
	}
	if (!valid || !(PARTS & DP_REST)) return;
	// ---- opacity (gaussian_model.py:207-214)
	if (a.o.opacity) {
		float o = sigmoid(is_obj ? a.p.obj_opacity[m] : a.p.scene_opacity[m]);
		if (is_obj && (a.p.use_time_mask & ADGS_DEFORM_TIME_MASK)) {
			const float dt = a.p.t - a.p.gs_time[m];
			const float sig = expf(dt < 0.f ? a.p.gs_time_sigma[2 * (size_t)m] : a.p.gs_time_sigma[2 * (size_t)m + 1]);
			const float r = dt / sig;
			o = o * expf(-0.5f * (r * r));
		}
		a.o.opacity[n] = o;
	}
	// ---- scales (gaussian_model.py:89-91)
	if (a.o.scales) {
		const float* s = is_obj ? a.p.obj_scaling + 3 * (size_t)m : a.p.scene_scaling + 3 * (size_t)m;
#pragma unroll
		for (int d = 0; d < 3; d++) a.o.scales[3 * (size_t)n + d] = expf(s[d]);
	}
}


// Object xyz / flow rows without staging: one thread per (object Gaussian, component) ROW of xyz_deform_param, read as 8-byte
// words straight from global memory (consecutive threads own consecutive rows: every fetched line is fully used) and dotted
// with the dense basis vectors of the two time stamps; the [No,3] inputs and outputs are then plain coalesced 4-byte accesses.
__device__ __forceinline__ void deform_fwd_xyz_rows(const DeformArgs a, int blk, float* __restrict__ s_w) {   // by value: with a reference the compiler spills the whole argument struct to scratch (2.4 KB per lane)
	const int tid = threadIdx.x, B = blockDim.x, np = a.fx.n_params;
	const bool lin1 = a.o.xyz && has_lin(a.fx), lin2 = a.flow_xyz && has_lin(a.fx2);
	// uniform loop index: a per-lane index into the by-value argument struct would force the whole struct into scratch memory
	dense_basis_lds<true>(s_w, np, a.fx, lin1 ? lin_terms(a.fx) : 0, a.fx2, lin2 ? lin_terms(a.fx2) : 0, tid, B);
	const size_t r = (size_t)blk * B + tid;
	if (r >= 3 * (size_t)a.p.No) return;
	const int d = (int)(r % 3);
	const float2* row = reinterpret_cast<const float2*>(a.p.xyz_deform_param + r * np);
	float acc1 = 0.f, acc2 = 0.f;
#pragma unroll 3
	for (int k = 0; k < np / 2; k++) {
		const float2 v = row[k];
		// explicit fused multiply-adds in one fixed order: the camera-time and the flow-time sums must round identically, so that
		// evaluating a time stamp in either slot gives the same bits
		acc1 = fmaf(v.y, s_w[2 * k + 1], fmaf(v.x, s_w[2 * k], acc1));
		acc2 = fmaf(v.y, s_w[np + 2 * k + 1], fmaf(v.x, s_w[np + 2 * k], acc2));
	}
	// all three components with compile-time row offsets (as above: no per-lane struct access), then this thread's
	float b1[3], b2[3];
	bg_offsets(a.p.background_deform_param, a.fb, a.fb2, a.o.xyz != nullptr, a.flow_xyz != nullptr, b1, b2);
	const float bg = d == 0 ? b1[0] : (d == 1 ? b1[1] : b1[2]);
	const float bg2 = d == 0 ? b2[0] : (d == 1 ? b2[1] : b2[2]);
	const float v = a.p.obj_xyz[r];
	const size_t o = 3 * (size_t)a.p.Ns + r;
	if (a.o.xyz) a.o.xyz[o] = (lin1 ? v + acc1 : v) + bg;
	if (a.flow_xyz) a.flow_xyz[o] = (lin2 ? v + acc2 : v) + bg2;
}

struct DeformBwdArgs {
	adgs_deform_params p; adgs_func_eval fx, fr, fb, fx2, fb2;
	const float *g_xyz, *g_flow, *g_rot, *g_op, *g_sc;
	adgs_deform_grads g;
	int stride_x, stride_r;
	int scene4;          // as in DeformArgs
};

// the background row takes a gradient: its deformation is on at either time stamp
__device__ __forceinline__ bool wants_bg_grad(const DeformBwdArgs& a) { return a.g.background_deform_param && (has_lin(a.fb) || has_lin(a.fb2)); }

// Backward of deform_fwd_kernel.  The object Gaussians' parameter-gradient rows are assembled in LDS (every
// column written: zeros outside the active terms, so no caller zero-fill) and stored coalesced; the rotation
// rows need the parameters (staged in) and a second LDS region for the gradients.
// PARTS: bit 0 = xyz / background, bit 1 = rotation, bit 2 = opacity + scales.  OBJ = false is the scene
// range (no object member: none of the staging / spline code is instantiated, so the kernel stays light).
template <int PARTS, bool OBJ, int NQ>
__device__ __forceinline__ void deform_bwd_body(const DeformBwdArgs& a, int blk, int n_begin, int n_end, float* __restrict__ s_rows, float (*s_bg)[256 / WAVE]) {
	const int tid = threadIdx.x, B = blockDim.x, base = n_begin + blk * B;
	const int Ns = a.p.Ns;
	const int count = min(B, n_end - base);
	const int n = base + tid;
	const bool valid = tid < count;
	const bool is_obj = OBJ && valid && n >= Ns;
	const int m = is_obj ? n - Ns : n;
	const bool blk_obj = OBJ && base + count > Ns;
	// ---- xyz: upstream of the camera-time points and of the flow-time points
	if ((PARTS & DP_XYZ) && (a.g_xyz || a.g_flow)) {
		float gx[3] = { 0.f, 0.f, 0.f }, gf[3] = { 0.f, 0.f, 0.f };
		if (valid) {
#pragma unroll
			for (int d = 0; d < 3; d++) {
				if (a.g_xyz) gx[d] = a.g_xyz[3 * (size_t)n + d];
				if (a.g_flow) gf[d] = a.g_flow[3 * (size_t)n + d];
			}
			float* dst = is_obj ? (a.g.obj_xyz ? a.g.obj_xyz + 3 * (size_t)m : nullptr) : (a.g.scene_xyz ? a.g.scene_xyz + 3 * (size_t)m : nullptr);
			if (dst) { dst[0] = gx[0] + gf[0]; dst[1] = gx[1] + gf[1]; dst[2] = gx[2] + gf[2]; }
		}
		const int np = a.fx.n_params;
		if (blk_obj && a.g.xyz_deform_param) {
			// dense basis rows of the two time stamps behind the staging rows: d/dparam[n,d,k] = w1[k] g1[d] + w2[k] g2[d]
			float* s_w = s_rows + B * a.stride_x;
			dense_basis_lds(s_w, np, a.fx, a.g_xyz ? lin_terms(a.fx) : 0, a.fx2, a.g_flow ? lin_terms(a.fx2) : 0, tid, B);
			if (is_obj) {
				float* row = s_rows + tid * a.stride_x;
				for (int k = 0; k < np; k++) {
					const float w1 = s_w[k], w2 = s_w[np + k];
#pragma unroll
					for (int d = 0; d < 3; d++) row[d * np + k] = w1 * gx[d] + w2 * gf[d];
				}
			}
			__syncthreads();
			stage_rows<false>(s_rows, a.stride_x, 3 * np, base, count, Ns, (float*)nullptr, a.g.xyz_deform_param, tid, B);
			__syncthreads();
		}
		// background: the same [1,3,Cb] row is added to every Gaussian -> reduce g over all n
		// (restated in deform_bwd_scene4: as one shared helper, in any of five forms tried, it costs deform_bwd_kernel<0> two registers)
		if (wants_bg_grad(a)) {
#pragma unroll
			for (int d = 0; d < 6; d++) {
				float v = d < 3 ? gx[d % 3] : gf[d % 3];
#pragma unroll
				for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
				if ((tid & (WAVE - 1)) == 0) s_bg[d][tid / WAVE] = v;
			}
			__syncthreads();
			if (tid < 6) {
				float v = 0.f;
				for (int w = 0; w < (B + WAVE - 1) / WAVE; w++) v += s_bg[tid][w];
				const adgs_func_eval& f = tid < 3 ? a.fb : a.fb2;
				const bool on = tid < 3 ? (a.g_xyz != nullptr) : (a.g_flow != nullptr);
				const int total = f.n_terms[0] + f.n_terms[1] + f.n_terms[2];
				if (on) for (int i = 0; i < total; i++)
					atomicAdd(a.g.background_deform_param + (tid % 3) * f.n_params + f.index[i], f.weight[i] * v);
			}
			__syncthreads();
		}
	}
	// ---- rotation: r = u / |u|
	if ((PARTS & DP_ROT) && a.g_rot) {
		const int np = a.fr.n_params;
		const bool haver = a.p.rotation_deform_param != nullptr;
		const bool staged = blk_obj && haver;
		float* s_out = s_rows;           // gradient rows, in place: a thread is done with its parameter row (spline state saved in registers) before it writes its gradient row, and two sets of rows halved the waves a CU can hold
		if (staged) {
			stage_rows<true>(s_rows, a.stride_r, 4 * np, base, count, Ns, (const float*)nullptr, a.p.rotation_deform_param, tid, B);
			__syncthreads();
		}
		if (valid) {
			float u[4];
			const float* rp = (is_obj && haver) ? s_rows + tid * a.stride_r : nullptr;
			QuatSave<(NQ > 0 ? NQ : 1)> qs;
			Q qout = { 0.f, 0.f, 0.f, 0.f };
			if (!OBJ || !is_obj) {
				const float* q = a.p.scene_rotation + 4 * (size_t)m;      // 4-byte loads, as in the forward: the pointer may be misaligned
				u[0] = q[0]; u[1] = q[1]; u[2] = q[2]; u[3] = q[3];
			} else {
				float fv[4] = { 0.f, 0.f, 0.f, 0.f };
				if (rp) {
#pragma unroll
					for (int d = 0; d < 4; d++) fv[d] = lin_eval(rp + d * np, a.fr);
					if (NQ > 0) { qout = quat_spline_eval<(NQ > 0 ? NQ : 1), true>(rp, a.fr, &qs); fv[0] += qout.w; fv[1] += qout.x; fv[2] += qout.y; fv[3] += qout.z; }
				}
#pragma unroll
				for (int d = 0; d < 4; d++) u[d] = (a.fr.quat_start >= 0) ? fv[d] : a.p.obj_rotation[4 * (size_t)m + d] + fv[d];
			}
			// (quat_normalize_bwd restated: sharing it, in either form of the sum, costs deform_bwd_kernel<3> and <6> a register)
			const float nr = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
			const float inv = 1.f / fmaxf(nr, 1e-12f);
			float g[4], r[4], dot = 0.f;
			const float4 g4 = ld4(a.g_rot + 4 * (size_t)n);
			g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
#pragma unroll
			for (int d = 0; d < 4; d++) { r[d] = u[d] * inv; dot += r[d] * g[d]; }
			float gu[4];
#pragma unroll
			for (int d = 0; d < 4; d++) gu[d] = (nr > 1e-12f) ? (g[d] - r[d] * dot) * inv : g[d] * inv;
			if (!OBJ || !is_obj) {
				if (a.g.scene_rotation) st4(a.g.scene_rotation + 4 * (size_t)m, make_float4(gu[0], gu[1], gu[2], gu[3]));
			} else {
				if (a.g.obj_rotation) {
					const float k = (a.fr.quat_start >= 0) ? 0.f : 1.f;
					st4(a.g.obj_rotation + 4 * (size_t)m, make_float4(k * gu[0], k * gu[1], k * gu[2], k * gu[3]));
				}
				if (a.g.rotation_deform_param && rp) {
					float* gp = s_out + tid * a.stride_r;
					for (int k = 0; k < 4 * np; k++) gp[k] = 0.f;
#pragma unroll
					for (int d = 0; d < 4; d++) lin_bwd(gp + d * np, a.fr, gu[d]);
					if (NQ > 0) quat_spline_bwd<(NQ > 0 ? NQ : 1)>(qs, qout, a.fr, { gu[0], gu[1], gu[2], gu[3] }, gp);
				}
			}
		}
		if (staged && a.g.rotation_deform_param) {
			__syncthreads();
			stage_rows<false>(s_out, a.stride_r, 4 * np, base, count, Ns, (float*)nullptr, a.g.rotation_deform_param, tid, B);
		}
	}
	if (!valid || !(PARTS & DP_REST)) return;
	// ---- opacity
	if (a.g_op) {
		const float g = a.g_op[n];
		const float sg = sigmoid(is_obj ? a.p.obj_opacity[m] : a.p.scene_opacity[m]);
		float mask = 1.f;
		if (is_obj && (a.p.use_time_mask & ADGS_DEFORM_TIME_MASK)) {
			const float dt = a.p.t - a.p.gs_time[m];
			const bool neg = dt < 0.f;
			const float sig = expf(neg ? a.p.gs_time_sigma[2 * (size_t)m] : a.p.gs_time_sigma[2 * (size_t)m + 1]);
			const float r = dt / sig;
			mask = expf(-0.5f * (r * r));
			if (a.g.gs_time_sigma) {
				const float gsel = g * sg * mask * (r * r);      // d mask / d log-sigma = mask * (dt/sigma)^2
				a.g.gs_time_sigma[2 * (size_t)m] = neg ? gsel : 0.f;
				a.g.gs_time_sigma[2 * (size_t)m + 1] = neg ? 0.f : gsel;
			}
		} else if (is_obj && a.g.gs_time_sigma) {
			a.g.gs_time_sigma[2 * (size_t)m] = 0.f; a.g.gs_time_sigma[2 * (size_t)m + 1] = 0.f;
		}
		float* dst = is_obj ? a.g.obj_opacity : a.g.scene_opacity;
		if (dst) dst[m] = sigmoid_bwd(g, mask, sg);
	}
	// ---- scales
	if (a.g_sc) {
		const float* s = is_obj ? a.p.obj_scaling + 3 * (size_t)m : a.p.scene_scaling + 3 * (size_t)m;
		float* dst = is_obj ? (a.g.obj_scaling ? a.g.obj_scaling + 3 * (size_t)m : nullptr) : (a.g.scene_scaling ? a.g.scene_scaling + 3 * (size_t)m : nullptr);
		if (dst) {
#pragma unroll
			for (int d = 0; d < 3; d++) dst[d] = a.g_sc[3 * (size_t)n + d] * expf(s[d]);
		}
	}
}

// Backward of deform_fwd_scene4: four scene Gaussians per thread, 16-byte accesses only.
__device__ __forceinline__ void deform_bwd_scene4(const DeformBwdArgs& a, int blk, float (*s_bg)[256 / WAVE]) {
	const int tid = threadIdx.x, B = blockDim.x;
	const int g = blk * B + tid;
	const int Ns = a.p.Ns;
	const bool in_range = 4 * (size_t)g < (size_t)Ns;
	const bool full = in_range && 4 * g + 4 <= Ns;
	const int n0 = 4 * g, n1 = in_range ? min(Ns, n0 + 4) : n0;
	const size_t o3 = 12 * (size_t)g;
	float sx[3] = { 0.f, 0.f, 0.f }, sf[3] = { 0.f, 0.f, 0.f };      // per-component sums of the thread's upstream position gradients
	if (a.g_xyz || a.g_flow) {
		if (full) {
			const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
			const float4 x0 = a.g_xyz ? ld4(a.g_xyz + o3) : z, x1 = a.g_xyz ? ld4(a.g_xyz + o3 + 4) : z, x2 = a.g_xyz ? ld4(a.g_xyz + o3 + 8) : z;
			const float4 f0 = a.g_flow ? ld4(a.g_flow + o3) : z, f1 = a.g_flow ? ld4(a.g_flow + o3 + 4) : z, f2 = a.g_flow ? ld4(a.g_flow + o3 + 8) : z;
			if (a.g.scene_xyz) {
				st4(a.g.scene_xyz + o3, make_float4(x0.x + f0.x, x0.y + f0.y, x0.z + f0.z, x0.w + f0.w));
				st4(a.g.scene_xyz + o3 + 4, make_float4(x1.x + f1.x, x1.y + f1.y, x1.z + f1.z, x1.w + f1.w));
				st4(a.g.scene_xyz + o3 + 8, make_float4(x2.x + f2.x, x2.y + f2.y, x2.z + f2.z, x2.w + f2.w));
			}
			// x y z x | y z x y | z x y z
			sx[0] = ((x0.x + x0.w) + x1.z) + x2.y; sx[1] = ((x0.y + x1.x) + x1.w) + x2.z; sx[2] = ((x0.z + x1.y) + x2.x) + x2.w;
			sf[0] = ((f0.x + f0.w) + f1.z) + f2.y; sf[1] = ((f0.y + f1.x) + f1.w) + f2.z; sf[2] = ((f0.z + f1.y) + f2.x) + f2.w;
		} else {
			for (int n = n0; n < n1; n++)
				for (int d = 0; d < 3; d++) {
					const float gx = a.g_xyz ? a.g_xyz[3 * (size_t)n + d] : 0.f, gf = a.g_flow ? a.g_flow[3 * (size_t)n + d] : 0.f;
					if (a.g.scene_xyz) a.g.scene_xyz[3 * (size_t)n + d] = gx + gf;
					sx[d] += gx; sf[d] += gf;
				}
		}
		// background, as in deform_bwd_body, from the thread's sums
		if (wants_bg_grad(a)) {
#pragma unroll
			for (int d = 0; d < 6; d++) {
				float v = d < 3 ? sx[d % 3] : sf[d % 3];
#pragma unroll
				for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
				if ((tid & (WAVE - 1)) == 0) s_bg[d][tid / WAVE] = v;
			}
			__syncthreads();
			if (tid < 6) {
				float v = 0.f;
				for (int w = 0; w < (B + WAVE - 1) / WAVE; w++) v += s_bg[tid][w];
				const adgs_func_eval& f = tid < 3 ? a.fb : a.fb2;
				const bool on = tid < 3 ? (a.g_xyz != nullptr) : (a.g_flow != nullptr);
				const int total = f.n_terms[0] + f.n_terms[1] + f.n_terms[2];
				if (on) for (int i = 0; i < total; i++)
					atomicAdd(a.g.background_deform_param + (tid % 3) * f.n_params + f.index[i], f.weight[i] * v);
			}
		}
	}
	if (!in_range) return;
	if (a.g_rot && a.g.scene_rotation) {
		for (int n = n0; n < n1; n++)
			st4(a.g.scene_rotation + 4 * (size_t)n, quat_normalize_bwd(ld4(a.p.scene_rotation + 4 * (size_t)n), ld4(a.g_rot + 4 * (size_t)n)));
	}
	if (a.g_op && a.g.scene_opacity) {
		if (full) {
			const float4 gq = ld4(a.g_op + 4 * (size_t)g), sg = sigmoid(ld4(a.p.scene_opacity + 4 * (size_t)g));
			st4(a.g.scene_opacity + 4 * (size_t)g, make_float4(sigmoid_bwd(gq.x, 1.f, sg.x), sigmoid_bwd(gq.y, 1.f, sg.y), sigmoid_bwd(gq.z, 1.f, sg.z), sigmoid_bwd(gq.w, 1.f, sg.w)));
		} else for (int n = n0; n < n1; n++) a.g.scene_opacity[n] = sigmoid_bwd(a.g_op[n], 1.f, sigmoid(a.p.scene_opacity[n]));
	}
	if (a.g_sc && a.g.scene_scaling) {
		if (full) {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				const float4 gq = ld4(a.g_sc + o3 + 4 * k), e = exp4(ld4(a.p.scene_scaling + o3 + 4 * k));
				st4(a.g.scene_scaling + o3 + 4 * k, make_float4(gq.x * e.x, gq.y * e.y, gq.z * e.z, gq.w * e.w));
			}
		} else for (int n = n0; n < n1; n++) for (int d = 0; d < 3; d++) a.g.scene_scaling[3 * (size_t)n + d] = a.g_sc[3 * (size_t)n + d] * expf(a.p.scene_scaling[3 * (size_t)n + d]);
	}
}

// One launch per direction: the object Gaussians' blocks (splines: long dependent chains, few waves) come FIRST in the
// grid and the streaming scene blocks fill the rest of the chip around them -- separate launches would run the
// latency-bound object kernels on a mostly idle GPU.
template <int NQ>
__global__ void __launch_bounds__(256) deform_fwd_kernel(DeformArgs a, int nb_rot, int nb_xyz) {
	extern __shared__ float s_rows[];
	const int b = blockIdx.x;
	if (b < nb_rot) deform_fwd_body<DP_ROT | DP_REST, true, NQ>(a, b, a.p.Ns, a.p.Ns + a.p.No, s_rows);
	else if (b < nb_rot + nb_xyz) {
		if (a.xyz_rows) deform_fwd_xyz_rows(a, b - nb_rot, s_rows);
		else deform_fwd_body<DP_XYZ, true, 0>(a, b - nb_rot, a.p.Ns, a.p.Ns + a.p.No, s_rows);
	}
	else if (a.scene4) deform_fwd_scene4(a, b - nb_rot - nb_xyz);
	else deform_fwd_body<DP_XYZ | DP_ROT | DP_REST, false, 0>(a, b - nb_rot - nb_xyz, 0, a.p.Ns, s_rows);
}
template <int NQ>
__global__ void __launch_bounds__(256) deform_bwd_kernel(DeformBwdArgs a, int nb_rot, int nb_xyz) {
	extern __shared__ float s_rows[];
	__shared__ float s_bg[6][256 / WAVE];
	const int b = blockIdx.x;
	if (b < nb_rot) deform_bwd_body<DP_ROT, true, NQ>(a, b, a.p.Ns, a.p.Ns + a.p.No, s_rows, s_bg);
	else if (b < nb_rot + nb_xyz) deform_bwd_body<DP_XYZ | DP_REST, true, 0>(a, b - nb_rot, a.p.Ns, a.p.Ns + a.p.No, s_rows, s_bg);
	else if (a.scene4) deform_bwd_scene4(a, b - nb_rot - nb_xyz, s_bg);
	else deform_bwd_body<DP_XYZ | DP_ROT | DP_REST, false, 0>(a, b - nb_rot - nb_xyz, 0, a.p.Ns, s_rows, s_bg);
}

// ------------------------------------------------------------------ host: argument checks and the launch plan
static adgs_func_eval empty_func() { adgs_func_eval f; memset(&f, 0, sizeof(f)); f.quat_start = -1; return f; }
static int check_func(const adgs_func_eval* f, const char* what) {
	if (!f) return 0;
	const int total = f->n_terms[0] + f->n_terms[1] + f->n_terms[2];
	if (total < 0 || total > ADGS_FUNC_MAX_TERMS) { set_error(std::string(what) + ": too many basis terms"); return -1; }
	for (int i = 0; i < total; i++) if (f->index[i] < 0 || f->index[i] >= f->n_params) { set_error(std::string(what) + ": term index out of range"); return -1; }
	if (f->quat_start >= 0 && (f->quat_k + 1 > MAXQ || f->quat_k < 0 || f->quat_start + f->quat_k >= f->n_params)) {
		set_error(std::string(what) + ": quaternion spline window out of range"); return -1;
	}
	return 0;
}
// the evaluations an entry point was given, checked, and the absent ones replaced by the empty function
struct FuncArg { const adgs_func_eval* given; const char* what; adgs_func_eval* resolved; };
static int resolve_funcs(std::initializer_list<FuncArg> funcs) {
	for (const FuncArg& f : funcs) if (check_func(f.given, f.what) != 0) return -1;
	for (const FuncArg& f : funcs) *f.resolved = f.given ? *f.given : empty_func();
	return 0;
}

// the four-Gaussians-per-thread scene path needs every (non-NULL) scene pointer 16-byte aligned
static int scene4_ok(std::initializer_list<const void*> ptrs) {
	for (const void* q : ptrs) if (reinterpret_cast<uintptr_t>(q) & 15) return 0;
	return 1;
}

// The layout of one geometry launch (deform_fwd_kernel / deform_bwd_kernel), decided from the shapes and the pointer VALUES alone.
enum { PLAN_OK = 0, PLAN_REFUSED = 1, PLAN_REFUSED_FOR_BACKWARD = 2 };
struct DeformPlan {
	int B; size_t lds;                   // block size, dynamic LDS bytes
	int np_x, stride_x, stride_r;        // xyz row length (both time stamps read the same rows); LDS row strides (odd)
	int xyz_rows, scene4;                // DeformArgs::xyz_rows (forward only), ::scene4
	int nb_rot, nb_xyz, nb_scene;        // the three block sets, in grid order
	int refused;                         // PLAN_REFUSED: rows above MAX_STAGING_LDS; the forward also: PLAN_REFUSED_FOR_BACKWARD
};
static DeformPlan plan_rows(int np_xyz, int np_xyz_flow, int np_rotation) {
	DeformPlan pl = {};
	pl.B = 256;
	pl.np_x = std::max(np_xyz, np_xyz_flow);
	pl.stride_x = (3 * pl.np_x) | 1; pl.stride_r = (4 * np_rotation) | 1;
	return pl;
}
// the three block sets and the verdict, once B, lds, xyz_rows and scene4 are known
static void plan_blocks(DeformPlan& pl, const adgs_deform_params& p, bool rot_set, bool xyz_set) {
	const int nb_o = (p.No + pl.B - 1) / pl.B;
	pl.nb_rot = rot_set ? nb_o : 0;
	pl.nb_xyz = !xyz_set ? 0 : (pl.xyz_rows ? (int)((3 * (size_t)p.No + pl.B - 1) / pl.B) : nb_o);
	pl.nb_scene = (p.use_time_mask & ADGS_DEFORM_SKIP_SCENE) ? 0 : (pl.scene4 ? ((p.Ns + 3) / 4 + pl.B - 1) / pl.B : (p.Ns + pl.B - 1) / pl.B);
	pl.refused = pl.lds > MAX_STAGING_LDS ? PLAN_REFUSED : PLAN_OK;
}
// backward: rows of the longer family, and behind the xyz gradient rows the dense basis vectors of the two time stamps
static DeformPlan plan_bwd(const adgs_deform_params& p, int np_xyz, int np_xyz_flow, int np_rotation, const float* dL_dxyz, const float* dL_drotation,
	const float* dL_dopacity, const float* dL_dscales, const float* dL_dflow_xyz, const adgs_deform_grads& g) {
	DeformPlan pl = plan_rows(np_xyz, np_xyz_flow, np_rotation);
	if (p.No > 0) {
		pl.B = pick_block(std::max(pl.stride_x, pl.stride_r), &pl.lds);
		pl.lds = std::max(pl.lds, (size_t)pl.B * pl.stride_x * sizeof(float) + 2 * (size_t)pl.np_x * sizeof(float));
	}
	pl.scene4 = scene4_ok({ p.scene_xyz, p.scene_rotation, p.scene_opacity, p.scene_scaling, dL_dxyz, dL_dflow_xyz, dL_drotation, dL_dopacity, dL_dscales,
		g.scene_xyz, g.scene_rotation, g.scene_opacity, g.scene_scaling });
	plan_blocks(pl, p, dL_drotation != nullptr, dL_dxyz || dL_dflow_xyz || dL_dopacity || dL_dscales);
	return pl;
}
// forward; with ADGS_DEFORM_WILL_BACKWARD it also refuses what its backward could not stage
static DeformPlan plan_fwd(const adgs_deform_params& p, int np_xyz, int np_xyz_flow, int np_rotation, const adgs_deform_outputs& o, const float* flow_xyz) {
	DeformPlan pl = plan_rows(np_xyz, np_xyz_flow, np_rotation);
	// object xyz rows: direct 8-byte reads when the row length is even (rows are then 8-byte aligned), else staged through LDS
	pl.xyz_rows = p.No > 0 && pl.np_x > 0 && pl.np_x % 2 == 0 && p.xyz_deform_param && (reinterpret_cast<uintptr_t>(p.xyz_deform_param) & 7) == 0 && p.obj_xyz;
	if (p.No > 0) pl.B = pick_block(pl.xyz_rows ? pl.stride_r : std::max(pl.stride_x, pl.stride_r), &pl.lds);
	if (pl.xyz_rows) pl.lds = std::max(pl.lds, (size_t)2 * pl.np_x * sizeof(float));
	pl.scene4 = scene4_ok({ p.scene_xyz, p.scene_rotation, p.scene_opacity, p.scene_scaling, o.xyz, flow_xyz, o.rotation, o.opacity, o.scales });
	plan_blocks(pl, p, o.rotation || o.opacity || o.scales, o.xyz || flow_xyz);
	if (!pl.refused && (p.use_time_mask & ADGS_DEFORM_WILL_BACKWARD)) {
		const adgs_deform_grads none = {};
		if (plan_bwd(p, np_xyz, np_xyz_flow, np_rotation, nullptr, nullptr, nullptr, nullptr, nullptr, none).refused) pl.refused = PLAN_REFUSED_FOR_BACKWARD;
	}
	return pl;
}
// one geometry kernel over the plan's grid (a model without objects on the raw-scene path has nothing to deform)
template <typename Args>
static int launch_planned(const DeformPlan& pl, void (*kernel)(Args, int, int), const Args& a, hipStream_t stream) {
	const int blocks = pl.nb_rot + pl.nb_xyz + pl.nb_scene;
	if (blocks == 0) return 0;
	if (pl.lds > 48 * 1024) ADGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(pl.B), pl.lds, stream, a, pl.nb_rot, pl.nb_xyz);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

// the shared argument checks of adgs_func_eval_forward / _backward: 1 = launch, 0 = nothing to do, -1 = refused
static int func_eval_args(const char* who, int N, int D, bool pointers_ok, const adgs_func_eval* f) {
	if (N <= 0) return 0;
	if (!pointers_ok || !f || (D != 3 && D != 4)) { set_error(std::string(who) + ": bad arguments"); return -1; }
	return check_func(f, who) != 0 ? -1 : 1;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_func_eval_forward(int N, int D, const float* param, const adgs_func_eval* f, float* out, void* stream_) {
	const int go = func_eval_args("adgs_func_eval_forward", N, D, param && out, f);
	if (go <= 0) return go;
	if (D == 3 && f->quat_start >= 0) { set_error("quaternion spline needs D == 4"); return -1; }
	void (*kernel)(int, const float*, adgs_func_eval, float*) = func_eval_fwd_kernel<3, 0>;
#define ADGS_CALL(NQ) kernel = func_eval_fwd_kernel<4, NQ>
	if (D == 4) { ADGS_NQ_SWITCH(*f, ADGS_CALL) }
#undef ADGS_CALL
	hipLaunchKernelGGL(kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream_, N, param, *f, out);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_func_eval_backward(int N, int D, const float* param, const adgs_func_eval* f, const float* dL_dout, float* dL_dparam, void* stream_) {
	const int go = func_eval_args("adgs_func_eval_backward", N, D, param && dL_dout && dL_dparam, f);
	if (go <= 0) return go;
	void (*kernel)(int, const float*, adgs_func_eval, const float*, float*) = func_eval_bwd_kernel<3, 0>;
#define ADGS_CALL(NQ) kernel = func_eval_bwd_kernel<4, NQ>
	if (D == 4) { ADGS_NQ_SWITCH(*f, ADGS_CALL) }
#undef ADGS_CALL
	hipLaunchKernelGGL(kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream_, N, param, *f, dL_dout, dL_dparam);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_deform_forward_flow(const adgs_deform_params* p, const adgs_func_eval* f_xyz, const adgs_func_eval* f_rotation,
	const adgs_func_eval* f_shs, const adgs_func_eval* f_background, const adgs_func_eval* f_xyz_flow, const adgs_func_eval* f_background_flow,
	const adgs_deform_outputs* out, float* flow_xyz, void* stream_) {
	if (!p || !out) { set_error("adgs_deform_forward: NULL params/outputs"); return -1; }
	if (p->Ns + p->No <= 0) return 0;
	DeformArgs a;
	adgs_func_eval fs;
	if (resolve_funcs({ { f_xyz, "f_xyz", &a.fx }, { f_rotation, "f_rotation", &a.fr }, { f_shs, "f_shs", &fs }, { f_background, "f_background", &a.fb },
		{ f_xyz_flow, "f_xyz_flow", &a.fx2 }, { f_background_flow, "f_background_flow", &a.fb2 } }) != 0) return -1;
	a.p = *p; a.o = *out; a.flow_xyz = flow_xyz;
	if (flow_xyz && f_xyz && f_xyz_flow && f_xyz->n_params != f_xyz_flow->n_params) { set_error("f_xyz and f_xyz_flow describe different parameter tensors"); return -1; }
	if (flow_xyz && !f_xyz_flow) a.fx2.n_params = a.fx.n_params;
	hipStream_t stream = (hipStream_t)stream_;
	StageTimer timer(ST_DEFORM_FWD, stream);
	a.o.shs = nullptr;                       // SH rows go through the flat coalesced kernels of deform_sh.hip
	if (a.o.xyz || a.flow_xyz || a.o.rotation || a.o.opacity || a.o.scales) {
		const DeformPlan pl = plan_fwd(*p, a.fx.n_params, a.fx2.n_params, a.fr.n_params, a.o, flow_xyz);
		if (pl.refused == PLAN_REFUSED) { set_error("adgs_deform_forward: deformation rows too large for the LDS staging buffer"); return -1; }
		if (pl.refused) { set_error("adgs_deform_forward: deformation rows too large for the LDS staging buffer of the backward pass"); return -1; }
		a.fx.n_params = a.fx2.n_params = pl.np_x;
		a.stride_x = pl.stride_x; a.stride_r = pl.stride_r; a.xyz_rows = pl.xyz_rows; a.scene4 = pl.scene4;
		void (*kernel)(DeformArgs, int, int) = nullptr;
#define ADGS_CALL(NQ) kernel = deform_fwd_kernel<NQ>
		ADGS_NQ_SWITCH(a.fr, ADGS_CALL)
#undef ADGS_CALL
		if (launch_planned(pl, kernel, a, stream) != 0) return -1;
	}
	return out->shs ? launch_deform_shs_fwd(*p, fs, out->shs, stream) : 0;
}
extern "C" int adgs_deform_forward(const adgs_deform_params* p, const adgs_func_eval* f_xyz, const adgs_func_eval* f_rotation,
	const adgs_func_eval* f_shs, const adgs_func_eval* f_background, const adgs_deform_outputs* out, void* stream_) {
	return adgs_deform_forward_flow(p, f_xyz, f_rotation, f_shs, f_background, nullptr, nullptr, out, nullptr, stream_);
}

extern "C" int adgs_deform_backward_flow(const adgs_deform_params* p, const adgs_func_eval* f_xyz, const adgs_func_eval* f_rotation,
	const adgs_func_eval* f_shs, const adgs_func_eval* f_background, const adgs_func_eval* f_xyz_flow, const adgs_func_eval* f_background_flow,
	const float* dL_dxyz, const float* dL_drotation, const float* dL_dshs, const float* dL_dopacity, const float* dL_dscales, const float* dL_dflow_xyz,
	const adgs_deform_grads* grads, void* stream_) {
	if (!p || !grads) { set_error("adgs_deform_backward: NULL params/grads"); return -1; }
	if (p->Ns + p->No <= 0) return 0;
	DeformBwdArgs a;
	adgs_func_eval fs;
	if (resolve_funcs({ { f_xyz, "f_xyz", &a.fx }, { f_rotation, "f_rotation", &a.fr }, { f_shs, "f_shs", &fs }, { f_background, "f_background", &a.fb },
		{ f_xyz_flow, "f_xyz_flow", &a.fx2 }, { f_background_flow, "f_background_flow", &a.fb2 } }) != 0) return -1;
	a.p = *p; a.g = *grads;
	hipStream_t stream = (hipStream_t)stream_;
	StageTimer timer(ST_DEFORM_BWD, stream);
	a.g_xyz = dL_dxyz; a.g_flow = dL_dflow_xyz; a.g_rot = dL_drotation; a.g_op = dL_dopacity; a.g_sc = dL_dscales;
	if (dL_dxyz || dL_dflow_xyz || dL_drotation || dL_dopacity || dL_dscales) {
		const DeformPlan pl = plan_bwd(*p, a.fx.n_params, a.fx2.n_params, a.fr.n_params, dL_dxyz, dL_drotation, dL_dopacity, dL_dscales, dL_dflow_xyz, *grads);
		if (pl.refused) { set_error("adgs_deform_backward: deformation rows too large for the LDS staging buffer"); return -1; }
		a.fx.n_params = a.fx2.n_params = pl.np_x;
		a.stride_x = pl.stride_x; a.stride_r = pl.stride_r; a.scene4 = pl.scene4;
		void (*kernel)(DeformBwdArgs, int, int) = nullptr;
#define ADGS_CALL(NQ) kernel = deform_bwd_kernel<NQ>
		ADGS_NQ_SWITCH(a.fr, ADGS_CALL)
#undef ADGS_CALL
		if (launch_planned(pl, kernel, a, stream) != 0) return -1;
	}
	return dL_dshs ? launch_deform_shs_bwd(*p, fs, dL_dshs, *grads, stream) : 0;
}
extern "C" int adgs_deform_backward(const adgs_deform_params* p, const adgs_func_eval* f_xyz, const adgs_func_eval* f_rotation,
	const adgs_func_eval* f_shs, const adgs_func_eval* f_background,
	const float* dL_dxyz, const float* dL_drotation, const float* dL_dshs, const float* dL_dopacity, const float* dL_dscales,
	const adgs_deform_grads* grads, void* stream_) {
	return adgs_deform_backward_flow(p, f_xyz, f_rotation, f_shs, f_background, nullptr, nullptr,
		dL_dxyz, dL_drotation, dL_dshs, dL_dopacity, dL_dscales, nullptr, grads, stream_);
}

static void write_plan(const DeformPlan& pl, int32_t* out) {
	const int32_t v[ADGS_TEST_DEFORM_PLAN_FIELDS] = { pl.B, (int32_t)pl.lds, pl.np_x, pl.stride_x, pl.stride_r, pl.xyz_rows, pl.scene4, pl.nb_rot, pl.nb_xyz, pl.nb_scene, pl.refused };
	memcpy(out, v, sizeof(v));
}
extern "C" int adgs_test_deform_plan(const adgs_deform_params* p, int np_xyz, int np_xyz_flow, int np_rotation, const adgs_deform_outputs* out, const float* flow_xyz,
	const float* dL_dxyz, const float* dL_drotation, const float* dL_dopacity, const float* dL_dscales, const float* dL_dflow_xyz, const adgs_deform_grads* grads,
	int32_t* fwd, int32_t* bwd) {
	if (!p || !out || !grads || !fwd || !bwd) { set_error("adgs_test_deform_plan: NULL argument"); return -1; }
	write_plan(plan_fwd(*p, np_xyz, np_xyz_flow, np_rotation, *out, flow_xyz), fwd);
	write_plan(plan_bwd(*p, np_xyz, np_xyz_flow, np_rotation, dL_dxyz, dL_drotation, dL_dopacity, dL_dscales, dL_dflow_xyz, *grads), bwd);
	return 0;
}
