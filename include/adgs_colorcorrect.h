/*
 * adgs_colorcorrect.h -- C ABI of the colour fit behind the colour-corrected metrics (libadgs_hip.so).
 *
 * A model trained with a bilateral grid (adgs_bilagrid.h) absorbs per-camera exposure and white balance in the grid; evaluation views
 * have none, so their metrics count the rig's exposure mismatch as reconstruction error.  Trainers with such a grid therefore also
 * report colour-corrected metrics: a per-image colour transform of the render is fitted to the ground truth by least squares over the
 * unsaturated pixels, and the transformed render is measured.  This is that fit, iterated, on the device and in double precision.
 *
 * Definition.  x0 = clip(image, 0, 1) and y = clip(gt, 0, 1) in float32, converted to double; EVERYTHING after that is double, up to the
 * rounding of the output image to float32.  Feature vector of a colour x = (r, g, b), ADGS_CC_FEATURES wide:
 *   quadratic  phi(x) = [r, g, b, r^2, rg, rb, g^2, gb, b^2, 1]
 *   affine     phi(x) = [r, g, b, 0, 0, 0, 0, 0, 0, 1]              (the six quadratic entries are zero and skipped in the solve)
 * unclipped(z) = (z >= eps) && (z <= 1 - eps), eps converted from float to double once.  For k = 1 .. iters and each channel c:
 *   m_c   = weight * [unclipped(x0_c) && unclipped(x^{k-1}_c) && unclipped(y_c)]                         per pixel
 *   G_c   = sum m_c phi phi^T,   h_c = sum m_c phi y_c,   n_c = sum m_c,   phi = phi(x^{k-1})
 *   W^k_c solves (G_c + ridge I) W = h_c + ridge e_c      (e_c: the identity warp of channel c, 1 at linear feature c; always SPD)
 *   x^k_c = clip(phi(x^{k-1}) . W^k_c, 0, 1)
 * A channel with no usable pixel (n_c == 0) gets exactly e_c; one with few gets the fit nearest to it.  No intermediate image exists:
 * x^{k-1} of a pixel is recomputed from x0 by applying warps 1 .. k-1 in registers.
 *
 * The sums are double atomics into the work buffer: their order, and with it the last bits of the warps, differs from run to run (as
 * the sums of adgs_metrics.h do).  The warps are ill-conditioned by design (near-grey images); compare what they do to an image.
 */
#ifndef ADGS_COLORCORRECT_H
#define ADGS_COLORCORRECT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_CC_FEATURES 10     /* doubles per warp row */
#define ADGS_CC_MAX_ITERS 8
#define ADGS_CC_SLOTS 64        /* slot rows of the work buffer */
#define ADGS_CC_ROW 200         /* doubles per slot row: 3 x (55 unique Gram entries + 10), padded */
#define ADGS_CC_AFFINE 0
#define ADGS_CC_QUADRATIC 1

typedef struct {
	int struct_bytes;   /* sizeof(adgs_cc_desc) of the caller */
	int H, W;
	int model;          /* ADGS_CC_AFFINE | ADGS_CC_QUADRATIC */
	int iters;          /* 1 .. ADGS_CC_MAX_ITERS */
	float eps;          /* [0, 0.5) */
	double ridge;       /* > 0, finite */
} adgs_cc_desc;

/* doubles of `work`: ADGS_CC_SLOTS x ADGS_CC_ROW */
size_t adgs_cc_work_doubles(void);

/*
 * The fit.  image, gt: [3, H, W] fp32, unclipped; weight: [H, W] fp32 in [0, 1] or NULL (1 everywhere).
 * work: adgs_cc_work_doubles() device doubles under the convention of adgs_loss.h: zero on entry; workgroup b of an accumulate launch
 * adds its partial sums into slot row b % ADGS_CC_SLOTS, and the finishing launch of the same iteration adds the rows up, leaves them
 * zero and solves the three systems (Cholesky, double).
 * warps_out: [iters, 3, ADGS_CC_FEATURES] device doubles, support_out: [iters, 3] device doubles (n_c of every iteration).
 * Per iteration one accumulate and one finishing launch are enqueued on `stream`; the finishing launch of iteration k writes
 * warps_out[k], which the accumulate launch of iteration k + 1 reads.  Nothing is read back.
 * Returns 0, or a negative code with adgs_last_error() set and nothing launched: H or W < 1, iters outside 1..8, model outside 0..1,
 * eps outside [0, 0.5), ridge <= 0 or not finite, struct_bytes too small, a NULL desc / image / gt / work / warps_out / support_out.
 */
int adgs_cc_fit(const adgs_cc_desc* desc, const float* image, const float* gt, const float* weight, double* work, double* warps_out,
	double* support_out, void* stream);

/*
 * out = x^{n_warps} of `image` under warps[0 .. n_warps) ([n_warps, 3, ADGS_CC_FEATURES] device doubles), rounded to fp32, [3, H, W].
 * desc: H, W, model as in the fit (affine skips the quadratic entries); n_warps in 1 .. desc->iters.  Same refusals, and a NULL warps
 * / out or an n_warps outside that range.
 */
int adgs_cc_apply(const adgs_cc_desc* desc, const float* image, const double* warps, int n_warps, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
