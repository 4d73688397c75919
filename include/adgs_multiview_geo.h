/*
 * adgs_multiview_geo.h -- C ABI of the multi-view geometric consistency loss (libadgs_hip.so): the depth reprojection error of PGSR.
 *
 * A pixel of the reference view is lifted with the rendered depth and projected into a neighbouring view, re-lifted with the depth the
 * neighbour rendered there and projected back; the distance in pixels between where it started and where it lands is the error.  Two
 * renders: the gradient goes to the depth and opacity of the reference view and, at the four sampled corners, of the neighbour.  The
 * per-pixel exp(-error) of the valid pixels is also the weight upstream gives its photometric term (include/adgs_multiview.h: weight).
 *
 * Conventions of include/adgs_loss.h: an entry returns 0 on success, a negative code with adgs_last_error() = "<symbol>: ..." otherwise;
 * every refusal is decided on the host from the arguments alone, before anything is launched; the last parameter is the stream.
 *
 * Definition.  depth [H, W]: D; opacity [H, W]: O, as render() returns them; nbr_depth [Hn, Wn]: Dn; nbr_opacity [Hn, Wn]: On, from the
 * neighbour's own render (its own size and tanfov*_n); weight [H, W] or NULL (= 1); pose: R row-major then t, X_n = R X_r + t from the
 * reference camera's frame to the neighbour's.  Pixel centres and the pixel of a point are those of include/adgs_multiview.h:
 *   r(x, y) = (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)
 *   the pixel of m in a view of size (W, H): ((m.x / m.z) / tanfovx * W / 2 + (W - 1) / 2, (m.y / m.z) / tanfovy * H / 2 + (H - 1) / 2)
 * Per reference pixel p = (x, y):
 *   1. z = O / D (inv_depth) or D / O,  X = z r(p),  Y = R X + t,  (u, v) = the neighbour's pixel of Y
 *   2. the bilinear cell of include/adgs_multiview.h: xi = min(floor(u), Wn - 2), fx = u - xi (so u = Wn - 1 reads column Wn - 1 with
 *      fx = 1), the same in v; for its four corners c: z_c = On_c / Dn_c or Dn_c / On_c;
 *      top = z[yi][xi] + fx (z[yi][xi + 1] - z[yi][xi]), bot the same of row yi + 1, zh = top + fy (bot - top)
 *   3. Y' = Y / Y.z * zh
 *   4. X' = R^T (Y' - t), with R as given: it is not re-orthonormalised
 *   5. (x', y') = the reference view's pixel of X'
 *   6. err = sqrt((x' - x)^2 + (y' - y)^2); its derivative is (dx, dy) / err, and 0 when err == 0
 * Validity v_p (piecewise constant: no gradient goes through a gate) holds when all of: O >= min_opacity and D > 0; Y.z > 1e-6;
 * 0 <= u <= Wn - 1 and 0 <= v <= Hn - 1; all four corners have On_c >= min_opacity and Dn_c > 0; X'.z > 1e-6; err < max_pixel_error.
 * Nothing outside the two images is ever read.
 *   g_p = exp(-err_p), a constant of the differentiation;  L = sum_p w_p v_p g_p err_p / sum_p w_p v_p;
 *   L = 0 with all-zero gradients when the denominator is 0 (decided on the device).
 * Gradients: to D and O of the reference, through X and through the sampling position (u, v) of zh; to Dn and On at the four corners.
 *
 * The inputs are float; the chain is double: the round trip subtracts two nearly equal pixel coordinates, and its float32 evaluation at
 * 1280 x 1920 is off by up to 5.2e-4 px in err and by more than the largest gradient element in the gradients, whose direction
 * (dx, dy) / err is rounding noise in float32 once err is far below a pixel (tests/test_multiview_geo_ref.py).
 *
 * Forward: one pass over 32 x 8 tiles of the reference pixels plus a one-block finish kernel.  work: ADGS_MULTIVIEW_GEO_WORK_DOUBLES
 * device doubles: ADGS_LOSS_SLOTS x 2 slot rows (zero on entry and on return), then sum w v g err, sum w v, L, which the backward reads
 * -- keep the buffer until then.  loss: one device float.  err_out: H W floats or NULL: err where every gate before the last holds,
 * else 0.  weight_out: H W floats or NULL: v_p g_p.
 *
 * Backward: ONE launch recomputes the chain.  dL_ddepth and dL_dopacity [H, W] are written exactly once per element by plain stores,
 * zeros for invalid pixels included: no fill, no atomics, bit-reproducible.  dL_dnbr_depth and dL_dnbr_opacity [Hn, Wn] are zero-filled
 * on the stream and receive the corner contributions: a tile accumulates them in an LDS window over its footprint in the neighbour and
 * adds each touched pixel once with a float atomic; a tile whose footprint exceeds the window adds every corner directly.  The order of
 * those adds is not fixed.  Each of the four pointers may be NULL; with both neighbour pointers NULL no fill and no atomic is issued;
 * with all four NULL nothing is launched.  g_loss: a DEVICE scalar.
 *
 * An empty image (H W = 0 or Hn Wn = 0) returns 0 and launches nothing.  Refused: a NULL desc / map / work / loss / g_loss, struct_bytes
 * too small, negative sizes, H W or Hn Wn above INT_MAX, a tanfov that is not finite and > 0, min_opacity outside (0, 1],
 * max_pixel_error not finite and > 0, a pose entry that is not finite.
 */
#ifndef ADGS_MULTIVIEW_GEO_H
#define ADGS_MULTIVIEW_GEO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_MULTIVIEW_GEO_WORK_DOUBLES (256 * 2 + 4)

typedef struct {
	int struct_bytes;                   /* sizeof(adgs_multiview_geo_desc) of the caller */
	int H, W;                           /* the reference view */
	int Hn, Wn;                         /* the neighbour's render */
	int inv_depth;
	float tanfovx, tanfovy;             /* the reference camera */
	float tanfovx_n, tanfovy_n;         /* the neighbour */
	float min_opacity, max_pixel_error;
	float pose[12];                     /* R row-major, then t */
} adgs_multiview_geo_desc;

int adgs_multiview_geo_forward(const adgs_multiview_geo_desc* desc, const float* depth, const float* opacity, const float* nbr_depth,
	const float* nbr_opacity, const float* weight, double* work, float* loss, float* err_out, float* weight_out, void* stream);
int adgs_multiview_geo_backward(const adgs_multiview_geo_desc* desc, const float* depth, const float* opacity, const float* nbr_depth,
	const float* nbr_opacity, const float* weight, const double* work, const float* g_loss, float* dL_ddepth, float* dL_dopacity,
	float* dL_dnbr_depth, float* dL_dnbr_opacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif
