// Cumulative quaternion B-spline of get_func_result (func_utils.py:156-171), forward and hand-written backward.  Device only.
#pragma once
#include "func_eval.h"

namespace adgs {

constexpr int MAXQ = ADGS_FUNC_MAX_QUAT;     // control quaternions per evaluation: quat_k + 1 <= MAXQ

struct Q { float w, x, y, z; };
__device__ __forceinline__ Q qmul(const Q& a, const Q& b) {
	Q c;
	c.x = a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y);
	c.y = a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z);
	c.z = a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x);
	c.w = a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z);
	return c;
}
__device__ __forceinline__ Q qconj(const Q& a) { return { a.w, -a.x, -a.y, -a.z }; }
__device__ __forceinline__ Q qadd(const Q& a, const Q& b) { return { a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z }; }
__device__ __forceinline__ float qdot(const Q& a, const Q& b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }

// ---- wxyz in / wxyz out ----
// param block of one Gaussian: [4][n_params]; control quaternion j = normalize(param[:, c0 + j] + (1,0,0,0)).
//   out = q_0 * prod_{j>=1} exp(B~_j * log(conj(q_{j-1}) q_j))
// log = roma.unitquat_to_rotvec (shortest arc: flip when w < 0; angle a = 2 atan2(|v|, w); factor a / sin(a/2),
// Taylor 2 + a^2/12 + 7a^4/2880 for a <= 1e-3), exp = roma.rotvec_to_unitquat (scale sin(n/2)/n, Taylor
// 0.5 - n^2/48 + n^4/3840 for n <= 1e-3).  Per segment this costs ONE atan2f and ONE sincosf: sin(a/2) and
// cos(a/2) of the log map are |v|/r and w/r with r = sqrt(|v|^2 + w^2) (the sine / cosine of atan2(|v|, w)), and
// the backward reuses the saved forward values instead of re-evaluating any transcendental.
// NQ = number of control quaternions used (quat_k + 1), a template parameter so that the per-segment state
// lives in registers sized for the actual spline order.
template <int NQ> struct QuatSave {
	Q q[NQ]; float inv_nrm[NQ];                 // normalised control quaternions, 1 / |ctrl|
	Q r[NQ];                                    // r[j] = exp(B~_j log(conj(q[j-1]) q[j])), j >= 1
	float vx[NQ], vy[NQ], vz[NQ], wq[NQ];       // delta_j = conj(q[j-1]) q[j] after the shortest-arc flip
	float a[NQ], n[NQ], she[NQ];                // log angle; |rotvec| of the exp and sin(n/2)
	bool flip[NQ];
};
__device__ __forceinline__ float log_factor(float a, float m, float rr) {
	if (a <= 1e-3f) { const float a2 = a * a; return 2.f + a2 / 12.f + 7.f * a2 * a2 / 2880.f; }
	return a * rr / m;                          // a / sin(a/2)
}
__device__ __forceinline__ float exp_scale(float n, float she) {
	if (n <= 1e-3f) { const float n2 = n * n; return 0.5f - n2 / 48.f + n2 * n2 / 3840.f; }
	return she / n;
}
template <int NQ, bool SAVE>
__device__ __forceinline__ Q quat_spline_eval(const float* __restrict__ p, const adgs_func_eval& f, QuatSave<NQ>* s) {
	const int np = f.n_params, c0 = f.quat_start;
	Q prev = { 1.f, 0.f, 0.f, 0.f }, acc = prev;
#pragma unroll
	for (int j = 0; j < NQ; j++) {
		const Q c = { p[0 * np + c0 + j] + 1.0f, p[1 * np + c0 + j], p[2 * np + c0 + j], p[3 * np + c0 + j] };
		const float inv = 1.f / fmaxf(sqrtf(qdot(c, c)), 1e-12f);
		const Q q = { c.w * inv, c.x * inv, c.y * inv, c.z * inv };
		if (SAVE) { s->q[j] = q; s->inv_nrm[j] = inv; }
		if (j == 0) acc = q;
		else {
			Q dq = qmul(qconj(prev), q);
			const bool flip = dq.w < 0.f;
			if (flip) { dq.w = -dq.w; dq.x = -dq.x; dq.y = -dq.y; dq.z = -dq.z; }
			const float m2 = dq.x * dq.x + dq.y * dq.y + dq.z * dq.z;
			const float m = sqrtf(m2);
			const float a = 2.f * atan2f(m, dq.w);
			const float fl = log_factor(a, m, sqrtf(m2 + dq.w * dq.w));
			const float B = f.quat_cum[j - 1];
			const float rv0 = fl * dq.x * B, rv1 = fl * dq.y * B, rv2 = fl * dq.z * B;
			const float n = sqrtf(rv0 * rv0 + rv1 * rv1 + rv2 * rv2);
			float she, che;
			sincosf(n * 0.5f, &she, &che);
			const float sc = exp_scale(n, she);
			const Q r = { che, sc * rv0, sc * rv1, sc * rv2 };
			acc = qmul(acc, r);
			if (SAVE) {
				s->r[j] = r; s->vx[j] = dq.x; s->vy[j] = dq.y; s->vz[j] = dq.z; s->wq[j] = dq.w;
				s->a[j] = a; s->n[j] = n; s->she[j] = she; s->flip[j] = flip;
			}
		}
		prev = q;
	}
	return acc;
}

// backward: writes d/dparam of (g_out . out) into gp [4][n_params] (columns c0..c0+NQ-1), ASSIGNING
template <int NQ>
__device__ __forceinline__ void quat_spline_bwd(const QuatSave<NQ>& s, const Q& out, const adgs_func_eval& f, const Q& g_out, float* __restrict__ gp) {
	const int np = f.n_params, c0 = f.quat_start;
	Q gq[NQ];
#pragma unroll
	for (int j = 0; j < NQ; j++) gq[j] = { 0.f, 0.f, 0.f, 0.f };
	Q G = g_out;                 // gradient w.r.t. part[j] = q0 r1 ... rj, starting at j = NQ-1
	Q P = out;                   // part[j], walked back with part[j-1] = part[j] conj(r_j)
#pragma unroll
	for (int j = NQ - 1; j >= 1; j--) {
		const Q rc = qconj(s.r[j]);
		const Q Pm = qmul(P, rc);
		const Q g_r = qmul(qconj(Pm), G);              // d(part[j-1] * r_j) / d r_j
		G = qmul(G, rc);                               // -> gradient w.r.t. part[j-1]
		P = Pm;
		// exp map backward
		const float vx = s.vx[j], vy = s.vy[j], vz = s.vz[j], w = s.wq[j], a = s.a[j];
		const float m2 = vx * vx + vy * vy + vz * vz, m = sqrtf(m2), rr2 = m2 + w * w, rr = sqrtf(rr2);
		const float fl = log_factor(a, m, rr);
		const float B = f.quat_cum[j - 1];
		const float rv0 = fl * vx * B, rv1 = fl * vy * B, rv2 = fl * vz * B;
		const float n = s.n[j], she = s.she[j], che = s.r[j].w;
		const float sc = exp_scale(n, she);
		float dsc_over_n, sinc;
		if (n <= 1e-3f) { dsc_over_n = -1.f / 24.f + n * n / 960.f; sinc = (n > 0.f) ? she / n : 0.5f; }
		else { dsc_over_n = ((0.5f * che * n - she) / (n * n)) / n; sinc = she / n; }
		const float t = rv0 * g_r.x + rv1 * g_r.y + rv2 * g_r.z;
		const float k = dsc_over_n * t - 0.5f * sinc * g_r.w;
		const float go0 = (sc * g_r.x + rv0 * k) * B, go1 = (sc * g_r.y + rv1 * k) * B, go2 = (sc * g_r.z + rv2 * k) * B;
		// log map backward: sin(a/2) = m / rr, cos(a/2) = w / rr
		float fp;
		if (a <= 1e-3f) fp = a / 6.f + 7.f * a * a * a / 720.f;
		else { const float sh = m / rr, ch = w / rr; fp = (sh - 0.5f * a * ch) / (sh * sh); }
		const float sdot = vx * go0 + vy * go1 + vz * go2;
		const float da_dm = 2.f * w / rr2, da_dw = -2.f * m / rr2;
		const float kv = (m > 0.f) ? fp * sdot * da_dm / m : 0.f;
		Q g_d = { fp * sdot * da_dw, fl * go0 + kv * vx, fl * go1 + kv * vy, fl * go2 + kv * vz };
		if (s.flip[j]) { g_d.w = -g_d.w; g_d.x = -g_d.x; g_d.y = -g_d.y; g_d.z = -g_d.z; }
		gq[j] = qadd(gq[j], qmul(s.q[j - 1], g_d));                       // L(conj(q_{j-1}))^T g = q_{j-1} * g
		gq[j - 1] = qadd(gq[j - 1], qconj(qmul(g_d, qconj(s.q[j]))));     // through the conjugation
	}
	gq[0] = qadd(gq[0], G);
#pragma unroll
	for (int j = 0; j < NQ; j++) {
		const float dd = qdot(s.q[j], gq[j]);
		const float inv = s.inv_nrm[j];
		gp[0 * np + c0 + j] = (gq[j].w - s.q[j].w * dd) * inv;
		gp[1 * np + c0 + j] = (gq[j].x - s.q[j].x * dd) * inv;
		gp[2 * np + c0 + j] = (gq[j].y - s.q[j].y * dd) * inv;
		gp[3 * np + c0 + j] = (gq[j].z - s.q[j].z * dd) * inv;
	}
}

// run CALL(NQ) with the compile-time number of control quaternions of `f` (0: no quaternion spline)
#define ADGS_NQ_SWITCH(f, CALL) \
	switch ((f).quat_start >= 0 ? (f).quat_k + 1 : 0) { \
		case 0: CALL(0); break; case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
		case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break; }

} // namespace adgs
