// The SH side of the per-frame deformation, and the two kernels other stages borrow from it: the [N, M, 3] SH tensor of
// adgs_deform_forward and its backward (flat coalesced copies), coefficient 0 of the raw-SH path (launch_sh0: the rasterizer's
// preprocess reads it), and the parameter-gradient rows of the linear families with the optional Adam step in their place
// (launch_lin_param_grad2: the preprocess backward and the optimizer launch it).  The geometry kernels are in deform.hip.
#include "common.h"
#include "kernels.h"
#include <cstring>

namespace adgs {
namespace {

// ---- SH coefficients as flat, fully coalesced streams (the per-Gaussian 192-byte rows are the
// bulk of the deformation traffic; one thread per Gaussian would touch 64 cache lines per access)
struct ShsFwdArgs {
	int Ns, N, M;
	const float *scene_dc, *obj_dc, *scene_rest, *obj_rest, *sp_scene, *sp_obj;
	adgs_func_eval fs;
	float* out;
};
__global__ void __launch_bounds__(256) deform_shs_fwd_kernel(ShsFwdArgs a) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 of the output
	const int row = a.M * 3;                                             // floats per Gaussian (multiple of 4 for M = 16; generic path below)
	const size_t total = (size_t)a.N * row;
	const size_t e0 = i * 4;
	if (e0 >= total) return;
	float v[4];
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const size_t e = e0 + k;
		if (e >= total) { v[k] = 0.f; continue; }
		const int n = (int)(e / row), c = (int)(e % row);
		const bool is_obj = n >= a.Ns;
		const int m = is_obj ? n - a.Ns : n;
		if (c < 3) {
			float x = (is_obj ? a.obj_dc : a.scene_dc)[3 * (size_t)m + c];
			const float* sp = is_obj ? a.sp_obj : a.sp_scene;
			if (sp && has_lin(a.fs)) x = x + lin_eval(sp + ((size_t)m * 3 + c) * a.fs.n_params, a.fs);
			v[k] = x;
		} else {
			v[k] = (is_obj ? a.obj_rest : a.scene_rest)[(size_t)m * (row - 3) + (c - 3)];
		}
	}
	if (e0 + 4 <= total && (row & 3) == 0) *reinterpret_cast<float4*>(a.out + e0) = make_float4(v[0], v[1], v[2], v[3]);
	else { for (int k = 0; k < 4; k++) if (e0 + k < total) a.out[e0 + k] = v[k]; }
}

// M = 16 (the reference's max_sh_degree 3): coefficient 0 is written by the sh0 kernel with a 48-float stride; this kernel moves the 45 floats of
// `rest` per Gaussian -- one thread per 16-byte word of the output, constant divisions, consecutive lanes on consecutive addresses on both
// sides.  (The generic kernel above computes e / row and e % row with run-time divisors per ELEMENT and evaluates f_shs in every 12th lane:
// 328 us at C3 for 372 MB.)
__global__ void __launch_bounds__(256) shs_rest_interleave_kernel(int Ns, int N, const float* __restrict__ scene_rest, const float* __restrict__ obj_rest, float* __restrict__ out) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)N * 12) return;
	const int n = (int)(i / 12), q = (int)(i - (size_t)n * 12);
	const bool is_obj = n >= Ns;
	const float* r = (is_obj ? obj_rest : scene_rest) + (size_t)(is_obj ? n - Ns : n) * 45;
	float* o = out + (size_t)n * 48 + 4 * q;
	if (q == 0) { o[3] = r[0]; return; }
	const float a = r[4 * q - 3], b = r[4 * q - 2], c = r[4 * q - 1], d = r[4 * q];
	*reinterpret_cast<float4*>(o) = make_float4(a, b, c, d);
}
// the inverse for the gradient [N,16,3] -> dc / rest gradients
__global__ void __launch_bounds__(256) shs_grad_split_kernel(int Ns, int N, const float* __restrict__ g, float* __restrict__ g_scene_dc, float* __restrict__ g_obj_dc,
	float* __restrict__ g_scene_rest, float* __restrict__ g_obj_rest) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)N * 12) return;
	const int n = (int)(i / 12), q = (int)(i - (size_t)n * 12);
	const bool is_obj = n >= Ns;
	const size_t m = is_obj ? n - Ns : n;
	const float4 v = *reinterpret_cast<const float4*>(g + (size_t)n * 48 + 4 * q);
	float* rest = is_obj ? g_obj_rest : g_scene_rest;
	if (q == 0) {
		float* dc = is_obj ? g_obj_dc : g_scene_dc;
		if (dc) { dc[3 * m] = v.x; dc[3 * m + 1] = v.y; dc[3 * m + 2] = v.z; }
		if (rest) rest[m * 45] = v.w;
		return;
	}
	if (rest) { float* r = rest + m * 45 + 4 * q - 3; r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
}

struct ShsBwdArgs {
	int Ns, N, M;
	const float* g;                                   // [N, M, 3]
	float *g_scene_dc, *g_obj_dc, *g_scene_rest, *g_obj_rest;
};
__global__ void __launch_bounds__(256) deform_shs_bwd_copy_kernel(ShsBwdArgs a) {
	const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int row = a.M * 3;
	if (e >= (size_t)a.N * row) return;
	const int n = (int)(e / row), c = (int)(e % row);
	const bool is_obj = n >= a.Ns;
	const int m = is_obj ? n - a.Ns : n;
	const float v = a.g[e];
	if (c < 3) { float* d = is_obj ? a.g_obj_dc : a.g_scene_dc; if (d) d[3 * (size_t)m + c] = v; }
	else { float* d = is_obj ? a.g_obj_rest : a.g_scene_rest; if (d) d[(size_t)m * (row - 3) + (c - 3)] = v; }
}
// d/d(param[n, c, k]) = w[k] * g[n, 0, c]: every column is written (zeros outside the active terms)
struct ParamGradArgs {
	int count, D, gstride;                            // `count` Gaussians of g; D rows per Gaussian
	const float* g;                                   // g[m * gstride + d]
	float* out;                                       // [count, D, n_params]
	adgs_func_eval f;
	// optional second segment in the same launch (blocks >= nb0): the object side after the scene side
	int nb0, count_b; const float* g_b; float* out_b;
	// ADAM instantiation: a segment whose slot is on (p != nullptr) applies the step to its parameter rows -- which have the layout
	// of `out` -- instead of storing the gradient (include/adgs_optim.h: adgs_sh_adam)
	AdamSlot adam = { nullptr, nullptr, nullptr, 0.f, 0.f }, adam_b = { nullptr, nullptr, nullptr, 0.f, 0.f };
	float beta1 = 0.f, beta2 = 0.f, eps = 0.f;
};
constexpr int PG_ITEMS = 8;                          // outputs per thread: two 16-byte stores, 256 float4 apart
// Every store instruction of a wave covers 1 KiB of consecutive bytes (lane i writes float4 number base + i; the thread's second
// float4 lies one block width further): 16 full 64-byte lines per instruction instead of 64 half-covered 32-byte pieces.
template <bool ADAM>
__global__ void __launch_bounds__(256) deform_lin_param_grad_kernel(ParamGradArgs a) {
	extern __shared__ float s_w[];
	const int np = a.f.n_params;
	// the segment's fields go into locals: writing to the by-value argument struct would move all of it into scratch memory
	const bool second = a.nb0 > 0 && (int)blockIdx.x >= a.nb0;
	const int seg_count = second ? a.count_b : a.count;
	const float* __restrict__ seg_g = second ? a.g_b : a.g;
	float* __restrict__ seg_out = second ? a.out_b : a.out;
	const size_t tot = (size_t)seg_count * a.D * np;
	const size_t blk0 = (size_t)(blockIdx.x - (second ? a.nb0 : 0)) * 256 * PG_ITEMS;
	// (Gaussian m, channel d, column k) of each half's first output and its upstream value: requested before the basis vector is
	// assembled in LDS, so that the load's round trip runs under the two barriers
	constexpr int HALVES = PG_ITEMS / 4;
	size_t e0[HALVES], m0[HALVES]; int k0[HALVES], d0[HALVES]; float gv0[HALVES];
#pragma unroll
	for (int half = 0; half < HALVES; half++) {
		e0[half] = blk0 + ((size_t)half * 256 + threadIdx.x) * 4;
		const size_t e = min(e0[half], tot - 1);
		size_t row;
		if (tot <= 0xffffffffull) { const uint32_t r32 = (uint32_t)e / (uint32_t)np; row = r32; k0[half] = (int)((uint32_t)e - r32 * (uint32_t)np); }
		else { row = e / np; k0[half] = (int)(e - row * np); }
		m0[half] = row / a.D; d0[half] = (int)(row - m0[half] * a.D);
		gv0[half] = seg_g[m0[half] * (size_t)a.gstride + d0[half]];
	}
	// ADAM: the parameter and its moments, requested in the same round trip (clamped quad index: unconditional loads)
	float* const ad_p = ADAM ? (second ? a.adam_b.p : a.adam.p) : nullptr;
	float* const ad_m = ADAM ? (second ? a.adam_b.m : a.adam.m) : nullptr;
	float* const ad_v = ADAM ? (second ? a.adam_b.v : a.adam.v) : nullptr;
	const float ad_step = ADAM ? (second ? a.adam_b.step_size : a.adam.step_size) : 0.f, ad_ibc2 = ADAM ? (second ? a.adam_b.inv_bc2_sqrt : a.adam.inv_bc2_sqrt) : 0.f;
	float4 p4[HALVES], m4[HALVES], v4[HALVES];
	if (ADAM && ad_p) {
		const size_t last4 = tot >= 4 ? (tot - 4) & ~(size_t)3 : 0;
#pragma unroll
		for (int half = 0; half < HALVES; half++) {
			const size_t e = tot >= 4 ? min(e0[half], last4) : 0;
			if (tot >= 4) { p4[half] = ld_stream4(reinterpret_cast<const float4*>(ad_p + e)); m4[half] = ld_stream4(reinterpret_cast<const float4*>(ad_m + e)); v4[half] = ld_stream4(reinterpret_cast<const float4*>(ad_v + e)); }
		}
	}
	for (int k = threadIdx.x; k < np; k += blockDim.x) s_w[k] = 0.f;
	__syncthreads();
	const int total = a.f.n_terms[0] + a.f.n_terms[1] + a.f.n_terms[2];
	for (int i = threadIdx.x; i < total; i += blockDim.x) s_w[a.f.index[i]] = a.f.weight[i];      // an int stride here: 98 VGPRs instead of 28
	__syncthreads();
#pragma unroll
	for (int half = 0; half < HALVES; half++) {
		if (e0[half] >= tot) return;
		size_t m = m0[half]; int k = k0[half], d = d0[half];
		float gv = gv0[half];
		float v[4];
#pragma unroll
		for (int it = 0; it < 4; it++) {
			v[it] = __fmul_rn(s_w[k], gv);       // rounded as the stored gradient is: the ADAM instantiation must not contract it into the update
			if (++k == np) {
				k = 0;
				if (++d == a.D) { d = 0; m++; }
				if (e0[half] + it + 1 < tot) gv = seg_g[m * (size_t)a.gstride + d];
			}
		}
		if (ADAM && ad_p) {
			if (e0[half] + 4 <= tot) {
				adam_update4(p4[half], m4[half], v4[half], make_float4(v[0], v[1], v[2], v[3]), a.beta1, a.beta2, a.eps, ad_step, ad_ibc2);
				st_stream4(reinterpret_cast<float4*>(ad_p + e0[half]), p4[half]); st_stream4(reinterpret_cast<float4*>(ad_m + e0[half]), m4[half]); st_stream4(reinterpret_cast<float4*>(ad_v + e0[half]), v4[half]);
			} else for (int it = 0; it < 4 && e0[half] + it < tot; it++) {
				const size_t e = e0[half] + it;
				float pp = ad_p[e], mm = ad_m[e], vv = ad_v[e];
				adam_update(pp, mm, vv, v[it], a.beta1, a.beta2, a.eps, ad_step, ad_ibc2);
				ad_p[e] = pp; ad_m[e] = mm; ad_v[e] = vv;
			}
			continue;
		}
		if (e0[half] + 4 <= tot) st_stream4(reinterpret_cast<float4*>(seg_out + e0[half]), make_float4(v[0], v[1], v[2], v[3]));
		else for (int it = 0; it < 4 && e0[half] + it < tot; it++) seg_out[e0[half] + it] = v[it];
	}
}

// The same rows for the raster backward of a prefilled frame (grad_prefill.h), by groups of 256 Gaussians of the frame under the published
// mask: in a SPARSE group the fill has stored the zero rows, and only the rows of the published Gaussians are written -- one row (D * n_params
// consecutive floats) per wave and store instruction; a DENSE group writes every row as the flat kernel does, 16-byte stores over the group's
// slab of each side.  Every element is __fmul_rn(w[k], g[m, d]), as there.
struct ParamGradRowsArgs {
	int Ns, P, D, gstride;                            // Gaussians [0, Ns): scene side, [Ns, P): object side
	const float *g_scene, *g_obj;                     // g[m * gstride + d], m counted from the side's first Gaussian
	float *out_scene, *out_obj;                       // [count, D, n_params] per side; nullptr: that side is not wanted
	const uint8_t* published;                         // [P]
	adgs_func_eval f;
};
__global__ void __launch_bounds__(PREFILL_GROUP) lin_param_grad_rows_kernel(ParamGradRowsArgs a) {
	extern __shared__ float s_w[];
	const int tid = threadIdx.x, base = blockIdx.x * PREFILL_GROUP;
	const bool pub = base + tid < a.P && a.published[base + tid] != 0;
	const int npub = __syncthreads_count(pub);
	const bool sparse = prefill_group_sparse(npub, min(PREFILL_GROUP, a.P - base));      // block-uniform: the rule the fill and the preprocess backward applied to these bytes
	if (sparse && npub == 0) return;
	const int np = a.f.n_params, L = a.D * np;
	for (int k = tid; k < np; k += PREFILL_GROUP) s_w[k] = 0.f;
	__syncthreads();
	const int total = a.f.n_terms[0] + a.f.n_terms[1] + a.f.n_terms[2];
	for (int i = tid; i < total; i += PREFILL_GROUP) s_w[a.f.index[i]] = a.f.weight[i];
	__syncthreads();
	if (sparse) {
		// the group's published Gaussians as a list in LDS (fewer than half of 256), their npub * L outputs dealt to all 256 threads:
		// consecutive threads on consecutive floats of a row
		__shared__ int s_list[PREFILL_GROUP];
		__shared__ int s_wave[PREFILL_GROUP / WAVE];
		const int lane = tid & (WAVE - 1), w = tid / WAVE;
		const uint64_t m = __builtin_amdgcn_ballot_w64(pub);
		if (lane == 0) s_wave[w] = __popcll(m);
		__syncthreads();
		int off = 0;
		for (int i = 0; i < w; i++) off += s_wave[i];
		if (pub) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = base + tid;
		__syncthreads();
		for (int e = tid; e < npub * L; e += PREFILL_GROUP) {
			const int j = e / L, c = e - j * L, d = c / np, gi = s_list[j];
			const bool ob = gi >= a.Ns;
			float* const out = ob ? a.out_obj : a.out_scene;
			if (!out) continue;
			const size_t r = ob ? gi - a.Ns : gi;
			st_stream(out + r * (size_t)L + c, __fmul_rn(s_w[c - d * np], (ob ? a.g_obj : a.g_scene)[r * (size_t)a.gstride + d]));
		}
		return;
	}
	const int end = min(base + PREFILL_GROUP, a.P);
#pragma unroll
	for (int side = 0; side < 2; side++) {
		const int first = side ? a.Ns : 0, lo = max(base, first), hi = side ? end : min(end, a.Ns);
		float* const out = side ? a.out_obj : a.out_scene;
		if (lo >= hi || !out) continue;
		float* const dst = out + (size_t)(lo - first) * L;
		const float* const g = (side ? a.g_obj : a.g_scene) + (size_t)(lo - first) * a.gstride;
		const int n = (hi - lo) * L;                   // <= 256 rows of the group
		auto elem = [&](int e) {
			const uint32_t row = (uint32_t)e / (uint32_t)np, m = row / (uint32_t)a.D;
			return __fmul_rn(s_w[(uint32_t)e - row * (uint32_t)np], g[(size_t)m * a.gstride + (row - m * (uint32_t)a.D)]);
		};
		const int head = min(n, (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
		if (tid < head) dst[tid] = elem(tid);
		const int n4 = (n - head) >> 2;
		for (int q = tid; q < n4; q += PREFILL_GROUP) {
			const int e = head + 4 * q;
			const uint32_t row0 = (uint32_t)e / (uint32_t)np;
			int k = (int)((uint32_t)e - row0 * (uint32_t)np);
			uint32_t m = row0 / (uint32_t)a.D; int d = (int)(row0 - m * (uint32_t)a.D);
			float gv = g[(size_t)m * a.gstride + d];
			float v[4];
#pragma unroll
			for (int it = 0; it < 4; it++) {
				v[it] = __fmul_rn(s_w[k], gv);
				if (++k == np) {
					k = 0;
					if (++d == a.D) { d = 0; m++; }
					if (e + it + 1 < n) gv = g[(size_t)m * a.gstride + d];
				}
			}
			st_stream4(reinterpret_cast<float4*>(dst + e), make_float4(v[0], v[1], v[2], v[3]));
		}
		const int tail0 = head + (n4 << 2);
		if (tail0 + tid < n) dst[tail0 + tid] = elem(tail0 + tid);
	}
}

// coefficient 0 of the raw-SH path: sh0[n, c] = dc[n, c] + f_shs(t)(shs_deform_param[n, c, :]).
// Fast kernel (n_params a multiple of 4, at most 32): one thread per (Gaussian, channel) ROW, which it reads as 16-byte
// words -- consecutive threads own consecutive rows, so the loads are perfectly coalesced without any staging -- and dots
// with the dense basis vector (zero where the family has no term).  General kernel: rows staged through LDS.
template <int NV4>
__global__ void __launch_bounds__(256) sh0_rows_kernel(int N, ShSource s, float* __restrict__ out, FramePrologue pro, int ostride) {
	__shared__ float s_w[NV4 * 4];
	run_frame_prologue(pro);      // counters the binning kernels accumulate into, the frame's snapshot of the slab bounds (saves a launch)
	__shared__ float s_part[256 * NV4 + 4];
	// The block owns 256 consecutive rows = 256 * NV4 consecutive 16-byte words of one segment (scene or object side).  Lane i of a
	// load instruction reads word base + i -- 1 KiB of consecutive bytes per wave and instruction instead of 64 words 16 * NV4 bytes
	// apart --, dots it with its quarter of the basis vector, and the NV4 partial sums of a row meet in LDS.  A block that straddles
	// the scene / object boundary takes the row-per-thread path.  The loads are issued BEFORE the basis vector is assembled in LDS
	// (two barriers): their round trip runs under that prologue.
	const int e0 = blockIdx.x * 256;                       // first row (row = n * 3 + c)
	const int rows = min(256, N * 3 - e0);
	const int split = 3 * s.Ns;                            // rows [0, split): scene side
	const bool one_side = (e0 >= split) || (e0 + rows <= split);
	const bool ob = e0 >= split;
	const float* sp = ob ? s.obj_sp : s.scene_sp;
	const bool fast = rows > 0 && one_side && sp != nullptr;            // block-uniform
	const size_t r0 = ob ? (size_t)e0 - split : (size_t)e0;
	float4 q[NV4];
	float dc = 0.f;
	if (fast) {
		const float4* src = reinterpret_cast<const float4*>(sp + r0 * (NV4 * 4));
		const int words = rows * NV4;
#pragma unroll
		for (int k = 0; k < NV4; k++) { const int wd = k * 256 + threadIdx.x; q[k] = ld_stream4(src + min(wd, words - 1)); }
		dc = (ob ? s.obj_dc : s.scene_dc)[r0 + min((int)threadIdx.x, rows - 1)];
	}
	for (int k = threadIdx.x; k < NV4 * 4; k += 256) s_w[k] = 0.f;
	__syncthreads();
	const int total = s.f.n_terms[0] + s.f.n_terms[1] + s.f.n_terms[2];
	for (int i = threadIdx.x; i < total; i += 256) s_w[s.f.index[i]] = s.f.weight[i];
	__syncthreads();
	if (rows <= 0) return;
	if (fast) {
#pragma unroll
		for (int k = 0; k < NV4; k++) {
			const int wd = k * 256 + threadIdx.x, part = wd % NV4;
			s_part[wd] = q[k].x * s_w[4 * part] + q[k].y * s_w[4 * part + 1] + q[k].z * s_w[4 * part + 2] + q[k].w * s_w[4 * part + 3];
		}
		__syncthreads();
		if ((int)threadIdx.x < rows) {
			float acc = 0.f;
#pragma unroll
			for (int k = 0; k < NV4; k++) acc += s_part[threadIdx.x * NV4 + k];
			const int e = e0 + threadIdx.x, n = e / 3;
			out[(size_t)n * ostride + (e - 3 * n)] = dc + acc;      // ostride = 3: the compact [N,3] array; 3 M: coefficient 0 inside [N,M,3]
		}
		return;
	}
	const int e = e0 + threadIdx.x;
	if (e >= N * 3) return;
	const int n = e / 3;
	const bool tob = n >= s.Ns;
	const size_t r = tob ? (size_t)e - 3 * (size_t)s.Ns : (size_t)e;
	float v = (tob ? s.obj_dc : s.scene_dc)[r];
	const float* tsp = tob ? s.obj_sp : s.scene_sp;
	if (tsp) {
		const float4* row = reinterpret_cast<const float4*>(tsp + r * (NV4 * 4));
		float4 q[NV4];
#pragma unroll
		for (int k = 0; k < NV4; k++) q[k] = row[k];
		float acc = 0.f;
#pragma unroll
		for (int k = 0; k < NV4; k++) acc += q[k].x * s_w[4 * k] + q[k].y * s_w[4 * k + 1] + q[k].z * s_w[4 * k + 2] + q[k].w * s_w[4 * k + 3];
		v = v + acc;
	}
	out[(size_t)n * ostride + (e - 3 * n)] = v;
}
__global__ void __launch_bounds__(256) sh0_kernel(int N, ShSource s, float* __restrict__ out, FramePrologue pro, int ostride) {
	extern __shared__ float s_rows[];
	run_frame_prologue(pro);
	const int tid = threadIdx.x, B = blockDim.x, base = blockIdx.x * B, count = min(B, N - base);
	const int np = s.f.n_params, L = 3 * np, stride = L | 1;
	const bool lin = (s.scene_sp || s.obj_sp) && has_lin(s.f);
	if (lin) {
		stage_rows<true>(s_rows, stride, L, base, count, s.Ns, s.scene_sp, s.obj_sp, tid, B);
		__syncthreads();
	}
	if (tid >= count) return;
	const int n = base + tid;
	const bool ob = n >= s.Ns;
	const size_t m = ob ? n - s.Ns : n;
	const float* dc = (ob ? s.obj_dc : s.scene_dc) + 3 * m;
	const bool has_row = lin && (ob ? s.obj_sp : s.scene_sp) != nullptr;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		float v = dc[c];
		if (has_row) v = v + lin_eval(s_rows + tid * stride + c * np, s.f);
		out[(size_t)ostride * n + c] = v;
	}
}
} // namespace

int launch_sh0(int N, const ShSource& s, float* out, hipStream_t stream, const FramePrologue* prologue, int ostride) {
	if (N <= 0) return 0;
	const FramePrologue pro = prologue ? *prologue : FramePrologue{ nullptr, 0, nullptr, nullptr, 0 };
	const int np = s.f.n_params;
	const bool lin = (s.scene_sp || s.obj_sp) && (s.f.n_terms[0] + s.f.n_terms[1] + s.f.n_terms[2]) > 0 && np > 0;
	const bool aligned = ((reinterpret_cast<uintptr_t>(s.scene_sp) | reinterpret_cast<uintptr_t>(s.obj_sp)) & 15) == 0;
	if (lin && np % 4 == 0 && np <= 32 && aligned) {
		using RowsKernel = void (*)(int, ShSource, float*, FramePrologue, int);
		static const RowsKernel rows[8] = { sh0_rows_kernel<1>, sh0_rows_kernel<2>, sh0_rows_kernel<3>, sh0_rows_kernel<4>,
			sh0_rows_kernel<5>, sh0_rows_kernel<6>, sh0_rows_kernel<7>, sh0_rows_kernel<8> };
		hipLaunchKernelGGL(rows[np / 4 - 1], dim3((unsigned)(((size_t)N * 3 + 255) / 256)), dim3(256), 0, stream, N, s, out, pro, ostride);
		ADGS_HIP_CHECK(hipGetLastError());
		return 0;
	}
	size_t lds = 0;
	const int B = pick_block((3 * np) | 1, &lds);
	if (lds > MAX_STAGING_LDS) { set_error("launch_sh0: SH deformation rows too large for the LDS staging buffer (more than 207 parameters per channel)"); return -1; }
	if (lds > 48 * 1024) ADGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sh0_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	hipLaunchKernelGGL(sh0_kernel, dim3((unsigned)((N + B - 1) / B)), dim3(B), lds, stream, N, s, out, pro, ostride);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
// two segments (scene side, object side) in ONE launch: a kernel boundary costs ~5 us, as much as a quarter of one side's work
int launch_lin_param_grad2(int count_a, const float* g_a, float* out_a, int count_b, const float* g_b, float* out_b, int D, int gstride,
	const adgs_func_eval& f, hipStream_t stream, const AdamSlot* adam_a, const AdamSlot* adam_b, float beta1, float beta2, float eps) {
	if (f.n_params <= 0) return 0;
	const AdamSlot off = { nullptr, nullptr, nullptr, 0.f, 0.f };
	const AdamSlot sa = adam_a ? *adam_a : off, sb = adam_b ? *adam_b : off;
	const bool on_a = (out_a || sa.p) && count_a > 0, on_b = (out_b || sb.p) && count_b > 0;
	if (!on_a && !on_b) return 0;
	if ((on_a && !g_a) || (on_b && !g_b)) { set_error("launch_lin_param_grad2: NULL gradient buffer"); return -1; }
	if ((on_a && out_a && sa.p) || (on_b && out_b && sb.p)) { set_error("launch_lin_param_grad2: a side takes the gradient store OR the Adam step"); return -1; }
	ParamGradArgs pg;
	pg.D = D; pg.gstride = gstride; pg.f = f; pg.beta1 = beta1; pg.beta2 = beta2; pg.eps = eps;
	const size_t per_block = (size_t)256 * PG_ITEMS;
	const size_t nb_a = on_a ? ((size_t)count_a * D * f.n_params + per_block - 1) / per_block : 0, nb_b = on_b ? ((size_t)count_b * D * f.n_params + per_block - 1) / per_block : 0;
	// a single active side travels as the first segment
	const bool two = on_a && on_b;
	pg.count = on_a ? count_a : count_b; pg.g = on_a ? g_a : g_b; pg.out = on_a ? out_a : out_b; pg.adam = on_a ? sa : sb;
	pg.nb0 = two ? (int)nb_a : 0; pg.count_b = two ? count_b : 0; pg.g_b = two ? g_b : nullptr; pg.out_b = two ? out_b : nullptr; pg.adam_b = two ? sb : off;
	if (sa.p || sb.p) hipLaunchKernelGGL(deform_lin_param_grad_kernel<true>, dim3((unsigned)(nb_a + nb_b)), dim3(256), f.n_params * sizeof(float), stream, pg);
	else hipLaunchKernelGGL(deform_lin_param_grad_kernel<false>, dim3((unsigned)(nb_a + nb_b)), dim3(256), f.n_params * sizeof(float), stream, pg);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
int launch_lin_param_grad_rows(int Ns, const float* g_scene, float* out_scene, int No, const float* g_obj, float* out_obj, int D, int gstride,
	const adgs_func_eval& f, const uint8_t* published, hipStream_t stream) {
	if (f.n_params <= 0) return 0;
	const bool on_a = out_scene && Ns > 0, on_b = out_obj && No > 0;
	if (!on_a && !on_b) return 0;
	if ((on_a && !g_scene) || (on_b && !g_obj) || !published) { set_error("launch_lin_param_grad_rows: NULL gradient buffer or mask"); return -1; }
	const ParamGradRowsArgs pg = { Ns, Ns + No, D, gstride, g_scene, g_obj, on_a ? out_scene : nullptr, on_b ? out_obj : nullptr, published, f };
	hipLaunchKernelGGL(lin_param_grad_rows_kernel, dim3((unsigned)((Ns + No + PREFILL_GROUP - 1) / PREFILL_GROUP)), dim3(PREFILL_GROUP), f.n_params * sizeof(float), stream, pg);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
int launch_lin_param_grad(int count, int D, const float* g, int gstride, float* out, const adgs_func_eval& f, hipStream_t stream) {
	if (count <= 0 || f.n_params <= 0) return 0;
	if (!g || !out) { set_error("launch_lin_param_grad: NULL gradient buffer"); return -1; }
	return launch_lin_param_grad2(count, g, out, 0, nullptr, nullptr, D, gstride, f, stream, nullptr, nullptr, 0.f, 0.f, 0.f);
}

int launch_deform_shs_fwd(const adgs_deform_params& p, const adgs_func_eval& fs, float* shs_out, hipStream_t stream) {
	const int N = p.Ns + p.No;
	if (p.sh_coeffs == 16 && (reinterpret_cast<uintptr_t>(shs_out) & 15) == 0 && (p.scene_shs_dc || p.obj_shs_dc)) {
		ShSource src;
		memset(&src, 0, sizeof(src));
		src.Ns = p.Ns; src.scene_dc = p.scene_shs_dc ? p.scene_shs_dc : p.obj_shs_dc; src.obj_dc = p.obj_shs_dc ? p.obj_shs_dc : p.scene_shs_dc;
		src.scene_sp = p.shs_deform_param_scene; src.obj_sp = p.shs_deform_param_obj; src.f = fs;
		if (launch_sh0(N, src, shs_out, stream, nullptr, 48) != 0) return -1;
		hipLaunchKernelGGL(shs_rest_interleave_kernel, dim3((unsigned)(((size_t)N * 12 + 255) / 256)), dim3(256), 0, stream, p.Ns, N, p.scene_shs_rest, p.obj_shs_rest, shs_out);
	} else {
		const ShsFwdArgs sa = { p.Ns, N, p.sh_coeffs, p.scene_shs_dc, p.obj_shs_dc, p.scene_shs_rest, p.obj_shs_rest, p.shs_deform_param_scene, p.shs_deform_param_obj, fs, shs_out };
		const size_t quads = ((size_t)N * p.sh_coeffs * 3 + 3) / 4;
		hipLaunchKernelGGL(deform_shs_fwd_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, sa);
	}
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
int launch_deform_shs_bwd(const adgs_deform_params& p, const adgs_func_eval& fs, const float* dL_dshs, const adgs_deform_grads& grads, hipStream_t stream) {
	const int N = p.Ns + p.No, M = p.sh_coeffs;
	const ShsBwdArgs sb = { p.Ns, N, M, dL_dshs, grads.scene_shs_dc, grads.obj_shs_dc, grads.scene_shs_rest, grads.obj_shs_rest };
	if (M == 16 && (reinterpret_cast<uintptr_t>(dL_dshs) & 15) == 0)
		hipLaunchKernelGGL(shs_grad_split_kernel, dim3((unsigned)(((size_t)N * 12 + 255) / 256)), dim3(256), 0, stream, sb.Ns, N, dL_dshs, sb.g_scene_dc, sb.g_obj_dc, sb.g_scene_rest, sb.g_obj_rest);
	else
		hipLaunchKernelGGL(deform_shs_bwd_copy_kernel, dim3((unsigned)(((size_t)N * M * 3 + 255) / 256)), dim3(256), 0, stream, sb);
	ADGS_HIP_CHECK(hipGetLastError());
	// the SH deformation rows: coefficient 0 of the upstream gradient times the basis vector, scene side and object side in one launch
	return launch_lin_param_grad2(p.Ns, dL_dshs, grads.shs_deform_param_scene, p.No, dL_dshs + (size_t)p.Ns * M * 3, grads.shs_deform_param_obj,
		3, M * 3, fs, stream);
}
} // namespace adgs
