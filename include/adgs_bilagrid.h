/*
 * adgs_bilagrid.h -- C ABI of the bilateral-grid appearance compensation (libadgs_hip.so).
 *
 * Per training image n a grid G[n] of 3x4 affine colour transforms, [12, L, Hg, Wg] fp32 (channel 4 i + j = entry (i, j)),
 * is sliced at (pixel x, pixel y, luma of the pixel) and applied to the rendered colour -- per-image exposure / white-balance
 * compensation between render() and the losses.  For the image I [3, H, W] (planar, the rasterizer's layout) and pixel (px, py):
 *   gray = 0.299 r + 0.587 g + 0.114 b
 *   gx = (px + 0.5) / W * (Wg - 1),  gy = (py + 0.5) / H * (Hg - 1),  gz = clamp(gray * (L - 1), 0, L - 1)
 *   x0 = min(floor(gx), Wg - 2), fx = gx - x0   (the same for y and z)
 *   A[c]   = sum over the 8 corners of w_x w_y w_z G[c, z0 + dz, y0 + dy, x0 + dx]      (w = f upper, 1 - f lower)
 *   out[i] = A[4 i] r + A[4 i + 1] g + A[4 i + 2] b + A[4 i + 3]
 * i.e. grid_sample(bilinear, border padding, align_corners=True) of the grid at (x, y, gray) followed by the affine map.
 * The luma coordinate carries a gradient into the image: slope 1 for 0 <= gray (L - 1) <= L - 1, 0 outside, taken inside
 * the cell [z0, z0 + 1].
 *
 * All pointers are device fp32 unless said otherwise; upstream loss gradients are device scalars; nothing here synchronises
 * or allocates.  Negative return: adgs_last_error() has the reason and nothing was launched.  L, Hg, Wg >= 2; H, W >= 1; N >= 1.
 */
#ifndef ADGS_BILAGRID_H
#define ADGS_BILAGRID_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* grid: ONE image's [12, L, Hg, Wg] block; image [3, H, W] -> out [3, H, W] */
int adgs_bilagrid_slice_forward(int L, int Hg, int Wg, const float* grid, int H, int W, const float* image, float* out, void* stream);

/* dL_dgrid [12, L, Hg, Wg] is ACCUMULATED into (the caller provides zeros; float atomics: the last bits depend on arrival order),
 * dL_dimage [3, H, W] is fully written.  Either may be NULL: its work is skipped. */
int adgs_bilagrid_slice_backward(int L, int Hg, int Wg, const float* grid, int H, int W, const float* image, const float* dL_dout,
	float* dL_dgrid, float* dL_dimage, void* stream);

/*
 * Total variation of grids [N, 12, L, Hg, Wg]:
 *   TV = (1 / N) sum_n sum_{axis in L, Hg, Wg} mean over the 12 channels and all adjacent pairs along the axis of (difference)^2
 * work: ADGS_BILAGRID_TV_WORK_DOUBLES device doubles, zero on entry and zero again on return (the convention of adgs_loss.h: one
 * zero-initialised buffer serves every call).  loss: one device float.
 */
#define ADGS_BILAGRID_TV_WORK_DOUBLES 256
int adgs_bilagrid_tv_forward(int N, int L, int Hg, int Wg, const float* grids, double* work, float* loss, void* stream);
/* dL_dgrids = g_loss[0] * dTV/dgrids: every element is written, each by one thread from its neighbours (deterministic). */
int adgs_bilagrid_tv_backward(int N, int L, int Hg, int Wg, const float* grids, const float* g_loss, float* dL_dgrids, void* stream);

#ifdef __cplusplus
}
#endif
#endif
