/*
 * adgs_metrics.h -- C ABI of the fused evaluation pass (libadgs_hip.so).
 *
 * What the reference's evaluation loops do per view after the render, in one kernel and without a host synchronisation:
 *   render.py:54-62     clip(render, 0, 1), clip(gt, 0, 1), psnr(render[None], gt[None]), ssim(render[None], gt[None]), then
 *                       torchvision.utils.save_image (:64) and to8b (:39,68) for the PNG and the video
 *   train.py:204-258    training_report: clamp, mean |image - gt|, psnr(image, gt).mean() -- the mean of the per-channel PSNRs,
 *                       because utils/image_utils.py:17-19 reduces over shape[0]
 * and, for the metrics of a driving scene's dynamic objects (viewpoint.semantic > 0, viewpoint.sky: train.py:217,238), the same
 * sums weighted by up to ADGS_METRICS_MAX_REGIONS per-pixel masks.
 *
 * Per pixel and channel, with x = clip(image), y = clip(gt) (and, with `quantize`, x = floor(x * 255 + 0.5) / 255, the value a saved
 * PNG holds -- what upstream's metrics.py computes from the written files): |x - y|, (x - y)^2 and the SSIM map value (11x11 Gaussian
 * window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2: utils/loss_utils.py:36-66, the arithmetic of adgs_l1_ssim_forward).
 * Region 0 is the whole image (weight 1), region r >= 1 weighs a pixel by masks[r - 1][y][x] in [0, 1].  The row of (view, region) is
 *   [ sum w |x - y|,  sum w (x - y)^2 of channel 0, 1, 2,  sum w ssim_map,  sum w (once per pixel),  0,  0 ]
 * in double (channels 1 and 2 are 0 for a one-channel image).  The table holds RAW SUMS: PSNR and the means are formed by the caller
 * after one copy of the whole table:
 *   l1 = row[0] / (C row[5]);  mse = (row[1] + row[2] + row[3]) / (C row[5]);  ssim = row[4] / (C row[5])
 *   psnr (render.py:59)  = 10 log10(1 / mse);   psnr_channel_mean (train.py:258) = mean_c 10 log10(row[5] / row[1 + c])
 */
#ifndef ADGS_METRICS_H
#define ADGS_METRICS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADGS_METRICS_MAX_REGIONS 4
#define ADGS_METRICS_ROW 8      /* doubles per (view, region) row of the table */
#define ADGS_METRICS_SLOTS 256  /* slot rows of the work buffer */

typedef struct {
	int struct_bytes;   /* sizeof(adgs_metrics_desc) of the caller */
	int channels;       /* 1 or 3 */
	int H, W;
	int regions;        /* 0 .. ADGS_METRICS_MAX_REGIONS masks beside the whole image */
	int quantize;       /* 0 | 1: metrics of the 8-bit rounded image */
	int u8_mode;        /* out_u8: 0 none, 1 round (save_image: x * 255 + 0.5, clamped to [0, 255], truncated), 2 truncate (to8b: 255 clip(x), truncated) */
} adgs_metrics_desc;

/* doubles of `work` for a call with `regions` masks: ADGS_METRICS_SLOTS x (1 + regions) x ADGS_METRICS_ROW (0 for an invalid count) */
size_t adgs_metrics_work_doubles(int regions);

/*
 * One view.  image, gt: [channels, H, W] fp32, unclipped; masks: [regions, H, W] fp32 or NULL with regions == 0.
 * work: adgs_metrics_work_doubles(regions) device doubles under the convention of adgs_loss.h: zero on entry; workgroup b adds its
 * partial sums into slot row b % ADGS_METRICS_SLOTS, and the finishing kernel of the same call adds the rows up and leaves them zero.
 * table: the (1 + regions) rows from table[(view_index * (1 + regions)) * ADGS_METRICS_ROW] on are OVERWRITTEN with this view's sums
 * (the caller sizes the table; calls with one table use one `regions`).
 * out_u8: [H, W, channels] bytes (the order imageio and PNG writers take) of the CLIPPED, unquantised image under u8_mode, or NULL with
 * u8_mode 0; both modes equal the float32 two-step evaluation (multiply, then add / truncate) bit for bit.
 * Everything is enqueued on `stream`; nothing is read back.  Returns 0, or a negative code with adgs_last_error() set: channels not 1
 * or 3, H or W < 1, regions outside 0..4, regions > 0 with NULL masks, view_index < 0, u8_mode outside 0..2 or 1 / 2 with a NULL out_u8,
 * quantize not 0 or 1, struct_bytes too small, a NULL descriptor / image / gt / work / table.  Nothing is launched then.
 */
int adgs_metrics_accumulate(const adgs_metrics_desc* desc, const float* image, const float* gt, const float* masks, double* work, double* table,
	int view_index, uint8_t* out_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif
