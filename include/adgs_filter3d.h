/*
 * adgs_filter3d.h -- C ABI of the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1) in libadgs_hip.so.
 *
 * Every Gaussian gets a low-pass filter whose size follows from the highest sampling rate any training camera has of it:
 *
 *   camera n:  p_cam = R_n p + t_n.  R_n | t_n are the first three COLUMNS of the project's (transposed, row-vector)
 *              world_view_transform V: R[i][j] = V[j][i], t[i] = V[3][i].  fx_n = W_n / (2 tan(FoVx_n / 2)), fy_n alike;
 *              the principal point is the image centre.
 *   camera n SEES p when z > 0.2 and, with zc = max(z, 0.001), u = x / zc fx_n + W_n / 2 and v = y / zc fy_n + H_n / 2 lie in
 *              [-0.15 W_n, 1.15 W_n] and [-0.15 H_n, 1.15 H_n].  (z > 0.2 makes zc = z; the kernel tests the equivalent
 *              |x fx_n| <= 0.65 W_n z and |y fy_n| <= 0.65 H_n z, which needs no division.)
 *   rate_k   = max over the cameras that see p_k of fx_n / z        (0: no camera sees it)
 *   filter_k = sqrt(0.2) / rate_k; a Gaussian with rate 0 gets the largest filter among the seen ones (the minimum positive
 *              rate); when nothing is seen every filter is 0.
 *
 * and the filter is applied to the activated scales s [P,3] and the activated opacity o [P,1] (time mask included):
 *
 *   S_i = sqrt(s_i^2 + f^2)         O = o sqrt(prod_i s_i^2 / (s_i^2 + f^2))         (the product of three ratios, each <= 1)
 *   dL/ds_i = gS_i s_i / S_i + gO O f^2 / (s_i (s_i^2 + f^2))        dL/do = gO sqrt(prod_i ...)        f receives no gradient
 *
 * The arithmetic of z and of fx_n / z is one rounding per operation in the order ((R20 x + R21 y) + R22 z) + t2 (no fused
 * multiply-add), and a maximum does not depend on the order of its operands: rates are bit-identical however the cameras are split
 * over calls, and data-parallel ranks that hold the same positions and cameras compute identical filters.
 *
 * All pointers are device fp32 unless said otherwise; nothing here synchronises, allocates or reads back to the host (every call
 * is legal under stream capture).  Negative return: adgs_last_error() has the reason (prefix "adgs_filter3d_") and nothing was
 * launched.  A size of 0 is a no-op.
 */
#ifndef ADGS_FILTER3D_H
#define ADGS_FILTER3D_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* one camera: 16 floats = 64 bytes.  [0..11] = R row-major then t (R00 R01 R02 R10 ... R22 t0 t1 t2), [12] fx, [13] fy, [14] W, [15] H */
#define ADGS_FILTER3D_CAMERA_FLOATS 16

/*
 * rate_inout[row] = max(init ? 0 : rate_inout[row], max over the `ncams` cameras that see xyz[row] of fx / z) for the rows
 * [row0, row0 + rows) of xyz [*,3] and rate_inout [*]; no other row is read or written.  cams: ncams records in device memory (16-byte aligned), read
 * wave-uniformly (there is no camera-table chunk: any count runs as one loop).  ncams may be 0 (with init: the rows become 0).
 */
int adgs_filter3d_accumulate(const float* xyz, int row0, int rows, const float* cams, int ncams, float* rate_inout, int init, void* stream);

/*
 * filter_out[k] = sqrt(0.2) / rate[k] for rate[k] > 0, sqrt(0.2) / (the minimum positive rate) for the other rows, 0 everywhere when
 * no rate is positive.  work: one device uint32 (contents on entry ignored, undefined on return).  A memset node, a reduction
 * (wave minimum of the bit patterns, one vector atomic per workgroup: the result does not depend on the launch order) and a
 * second kernel that writes filter_out.  rate and filter_out may be the same buffer.
 */
int adgs_filter3d_finalize(const float* rate, int P, float* filter_out, uint32_t* work, void* stream);

/* scales [P,3], opacity [P], filter [P] -> scales_out [P,3], opacity_out [P]: 20 bytes in and 16 out per Gaussian */
int adgs_filter3d_apply_forward(int P, const float* scales, const float* opacity, const float* filter, float* scales_out, float* opacity_out,
	void* stream);

/* the forward's inputs and the upstream gradients g_scales_out [P,3], g_opacity_out [P] -> g_scales [P,3], g_opacity [P], both fully
 * written: 36 bytes in and 16 out per Gaussian */
int adgs_filter3d_apply_backward(int P, const float* scales, const float* opacity, const float* filter, const float* g_scales_out,
	const float* g_opacity_out, float* g_scales, float* g_opacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif
