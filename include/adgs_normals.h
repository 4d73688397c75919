/*
 * adgs_normals.h -- C ABI of the normal-map geometry prior (libadgs_hip.so): per-Gaussian camera-space normals for the rasterizer's
 * semantic channels, and the consistency loss between the blended normal map and the normals of the rendered depth (2DGS, GOF, PGSR).
 *
 * Conventions of include/adgs_loss.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched; the last parameter is the stream.
 */
#ifndef ADGS_NORMALS_H
#define ADGS_NORMALS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The normal of Gaussian i in camera space, oriented towards the camera.
 *   q   = rotations[i] (w, x, y, z), any non-zero length; qh = q / |q| (the deformation pass's normalisation), R = R(qh)
 *   k   = index of the smallest of scales[i][0..2], the lowest index on ties (strict <)
 *   n_w = R[:, k]
 *   n_c[j] = m[j] n_w.x + m[4 + j] n_w.y + m[8 + j] n_w.z      m: the transposed 4x4 view matrix the rasterizer receives (16 DEVICE floats)
 *   p_c[j] = the same product of means3D[i], plus m[12 + j]
 *   s   = +1 if n_c . p_c <= 0, else -1
 *   out[i][c0 .. c0 + 2] = s n_c
 * out: row-major [N, stride] floats, 3 <= stride <= 32, 0 <= c0, c0 + 3 <= stride.  With mask ([N] floats, needs c0 >= 1) column 0 of the
 * row receives mask[i]: the [N, D_S] `semantic` tensor of the rasterizer (object mask + normal) in one pass.  Every other column is left
 * untouched.  N = 0 returns 0 and launches nothing.
 */
int adgs_gaussian_normals_forward(int N, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
	const float* mask, int stride, int c0, float* out, void* stream);
/*
 * g: [N, stride] upstream gradient, read at columns c0 .. c0 + 2.  dL_drotations [N, 4]: every element is written once -- through the column
 * of R, the view rotation, the sign and the normalisation Jacobian (I - qh qh^T) / |q|.  k and s are piecewise constant: scales and means
 * receive no gradient.
 */
int adgs_gaussian_normals_backward(int N, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
	const float* g, int stride, int c0, float* dL_drotations, void* stream);

/*
 * Depth-normal consistency.  normal [3, H, W]: the blended, un-normalised normal map Nm; depth [H, W]: D as the rasterizer renders it
 * (sum alpha T / z under inv_depth, else sum alpha T z); opacity [H, W]: O; weight [H, W] or NULL (= 1).
 *   z   = O / D (inv_depth) or D / O                               expected depth
 *   r   = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)   the rasterizer's ndc2Pix pixel centres
 *   P   = z r
 *   t_x = P(x + 1, y) - P(x - 1, y),  t_y = P(x, y + 1) - P(x, y - 1),  evaluated as (z+ - z-) r + (z+ + z-) dr, dr = (2 tanfovx / W, 0, 0)
 *         (resp. (0, 2 tanfovy / H, 0)): no difference of two nearly equal products in the lateral coordinate
 *   c   = t_y x t_x            faces the camera: a fronto-parallel plane gives (0, 0, -1)
 *   n_d = c / sqrt(c . c + 1e-30),   Nh = Nm / sqrt(Nm . Nm + 1e-12),   e = 1 - Nh . n_d
 *   m   = 1 iff 1 <= x <= W - 2, 1 <= y <= H - 2, and O >= min_opacity and D > 0 at the pixel and its four neighbours
 *   v   = weight m,   L = sum v e / sum v   (sum v = 0: L = 0 and every gradient is zero, decided on the device)
 * One pass over 32 x 16 tiles (z and the validity staged in LDS with a halo of 1; the per-pixel arithmetic is double, the inputs float) and a
 * one-block finish kernel.  work: ADGS_NORMAL_WORK_DOUBLES device doubles: ADGS_LOSS_SLOTS x 2 slot rows (zero on entry and on return), then
 * sum v e, sum v, L, which the backward reads -- keep the buffer until then.  loss: one device float.
 *
 * Backward: one gather launch.  g_loss: a DEVICE scalar.  dL_dnormal [3, H, W], dL_ddepth [H, W], dL_dopacity [H, W]: each may be NULL
 * (then not computed); every element of a given output is written exactly once, exactly 0 wherever no valid term reaches.  No atomics, no
 * intermediate image: dL/dD and dL/dO at q collect from the depth normals of q +- 1 along both axes (staged halo 2) through
 * dz/dD = -O / D^2, dz/dO = 1 / D (inv_depth), or 1 / O, -D / O^2.
 *
 * adgs_depth_to_normal: forward only, writes m n_d into out [3, H, W] (visualisation, evaluation).
 * H * W = 0 returns 0 and launches nothing.  tanfovx, tanfovy: finite and > 0; min_opacity: in (0, 1].
 */
#define ADGS_NORMAL_WORK_DOUBLES (256 * 2 + 4)
int adgs_normal_consistency_forward(int H, int W, const float* normal, const float* depth, const float* opacity, const float* weight,
	float tanfovx, float tanfovy, int inv_depth, float min_opacity, double* work, float* loss, void* stream);
int adgs_normal_consistency_backward(int H, int W, const float* normal, const float* depth, const float* opacity, const float* weight,
	float tanfovx, float tanfovy, int inv_depth, float min_opacity, const double* work, const float* g_loss,
	float* dL_dnormal, float* dL_ddepth, float* dL_dopacity, void* stream);
int adgs_depth_to_normal(int H, int W, const float* depth, const float* opacity, float tanfovx, float tanfovy, int inv_depth,
	float min_opacity, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
