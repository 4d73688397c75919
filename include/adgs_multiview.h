/*
 * adgs_multiview.h -- C ABI of the multi-view photometric consistency loss (libadgs_hip.so): the plane-warped patch NCC of PGSR.
 *
 * The rendered depth and normal of a reference view describe a local plane at every pixel; that plane induces a homography into a
 * neighbouring training image; a small patch of the reference grey image is warped through it and compared with what the neighbour saw,
 * by normalised cross-correlation.  One render: the neighbour contributes its ground-truth grey image and its pose only.  The gradient
 * goes to the rendered depth, normal and opacity of the reference view.
 *
 * Conventions of include/adgs_loss.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched; the last parameter is the stream.
 *
 * Definition.  normal [3, H, W]: the blended, un-normalised normal map N; depth [H, W]: D; opacity [H, W]: O (as adgs_normals.h);
 * ref_gray [H, W]: I_r; nbr_gray [Hn, Wn]: I_n; weight [H, W] or NULL (= 1); samples: S int32 linear pixel indices y * W + x;
 * pose: R row-major then t, X_n = R X_r + t from the reference camera's frame to the neighbour's.  T = (2 radius + 1)^2 taps.
 *   r(x, y) = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)          the rasterizer's pixel centres (adgs_normals.h)
 *   u = (m.x / m.z) / tanfovx_n * Wn / 2 + (Wn - 1) / 2,  v = (m.y / m.z) / tanfovy_n * Hn / 2 + (Hn - 1) / 2      the neighbour's pixel of m
 * Per sample at p = (x0, y0):
 *   z  = O / D (inv_depth) or D / O,   Nh = N / sqrt(N . N + 1e-12),   r0 = r(p),   c0 = Nh . r0;   the plane is Nh . X = z c0
 *   tap k at q = p + (dx, dy), dx, dy in [-radius, radius], row-major over (dy, dx):
 *     s_k = (Nh . r(q)) / (z c0),   m_k = R r(q) + t s_k,   a_k = I_r(q)
 *     b_k = the bilinear sample of I_n at (u_k, v_k): xi = min(floor(u), Wn - 2), fx = u - xi (so u = Wn - 1 reads column Wn - 1 with
 *           fx = 1), the same in v; top = I[yi][xi] + fx (I[yi][xi + 1] - I[yi][xi]), bot the same of row yi + 1, b = top + fy (bot - top)
 *   Sa = sum a, Sb = sum b, C = sum a b - Sa Sb / T, Va = sum a^2 - Sa^2 / T, Vb = sum b^2 - Sb^2 / T,  e = 1 - C^2 / (Va Vb + eps)
 *   (PGSR's lncc: squared correlation, un-normalised sums).
 * A sample is valid (piecewise constant: no gradient goes through it) when 0 <= index < H W; radius <= x0 < W - radius and
 * radius <= y0 < H - radius; O >= min_opacity and D > 0; -c0 >= min_cos |r0|; every tap has m.z > 1e-6, 0 <= u <= Wn - 1 and
 * 0 <= v <= Hn - 1; and e < max_error.  An index outside the image is an invalid sample and is never dereferenced.
 *   L = sum_s w_s v_s e_s / sum_s w_s v_s,   w_s = weight[p_s];   L = 0 with all-zero gradients when the denominator is 0 (decided on the device).
 *
 * The inputs are float; the per-tap chain and the five sums are double (sum a^2 - Sa^2 / T cancels on low-texture patches: the float32
 * evaluation is off by up to 3e-3 of the largest gradient).  One wave per sample, lane k = tap k, no [S, T] tensor in memory.
 *
 * Forward: one launch plus a one-block finish kernel.  work: ADGS_MULTIVIEW_WORK_DOUBLES device doubles: ADGS_LOSS_SLOTS x 2 slot rows
 * (zero on entry and on return), then sum w v e, sum w v, L, which the backward reads -- keep the buffer until then.  loss: one device
 * float.  e_out: S floats or NULL: e_s where every gate before the last holds (e was formed), else 0.  valid_out: S bytes or NULL: v_s.
 *
 * Backward: the gradient maps that are given (dL_dnormal [3, H, W], dL_ddepth [H, W], dL_dopacity [H, W]; each may be NULL, all three
 * NULL: nothing is launched) are zero-filled on the stream, then ONE launch recomputes the taps, reduces
 * de/db_k grad I_n d(u, v)/dm t  to the sums for z and Nh, chains through the normalisation and z, and adds with float atomics at the
 * sampled pixels: a pixel listed once receives exactly one add (deterministic), a pixel listed twice the sum, every other pixel is 0.
 * g_loss: a DEVICE scalar.
 *
 * S = 0 or an empty image (H W = 0 or Hn Wn = 0) returns 0 and launches nothing.  Refused: a NULL desc / map / samples / work / loss /
 * g_loss, struct_bytes too small, negative sizes or S, H W or Hn Wn above INT_MAX, radius outside 1 .. 3, a tanfov that is not finite
 * and > 0, min_opacity or min_cos outside (0, 1], max_error outside (0, 1], eps not finite and > 0, a pose entry that is not finite.
 */
#ifndef ADGS_MULTIVIEW_H
#define ADGS_MULTIVIEW_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_MULTIVIEW_WORK_DOUBLES (256 * 2 + 4)
#define ADGS_MULTIVIEW_MAX_RADIUS 3

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_multiview_desc) of the caller */
	int H, W;                           /* the reference view */
	int Hn, Wn;                         /* the neighbour's grey image */
	int radius;                         /* 1 .. ADGS_MULTIVIEW_MAX_RADIUS */
	int inv_depth;
	float tanfovx, tanfovy;             /* the reference camera */
	float tanfovx_n, tanfovy_n;         /* the neighbour */
	float min_opacity, min_cos, max_error, eps;
	float pose[12];                     /* R row-major, then t */
} adgs_multiview_desc;

int adgs_multiview_ncc_forward(const adgs_multiview_desc* desc, const float* normal, const float* depth, const float* opacity,
	const float* ref_gray, const float* nbr_gray, const float* weight, const int32_t* samples, int S, double* work, float* loss,
	float* e_out, uint8_t* valid_out, void* stream);
int adgs_multiview_ncc_backward(const adgs_multiview_desc* desc, const float* normal, const float* depth, const float* opacity,
	const float* ref_gray, const float* nbr_gray, const float* weight, const int32_t* samples, int S, const double* work,
	const float* g_loss, float* dL_dnormal, float* dL_ddepth, float* dL_dopacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif
