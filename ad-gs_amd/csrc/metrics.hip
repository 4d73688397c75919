// Fused evaluation pass for gfx950 (include/adgs_metrics.h): per view ONE kernel clips the render and the ground truth as it stages them,
// forms |x - y|, (x - y)^2 and the SSIM map per pixel and channel, sums them for the whole image and for up to four weighted regions, and
// writes the 8-bit H x W x C image; a one-block-per-region finishing kernel moves the sums into the caller's table.  Reference:
// render.py:54-68 (clip, psnr, ssim, save_image, to8b) and train.py:204-258 (training_report).
// One 32x16 tile per workgroup FOR ALL CHANNELS (a channel loop over the staging / window passes of loss.hip's l1_ssim_fwd_kernel, whose
// helpers and per-pixel arithmetic -- tap order, expression -- this kernel shares: ssim_window.h): a pixel's mask weights are loaded once,
// and its channels meet in an LDS byte tile from which the 8-bit rows leave as 32-bit words.
#include "common.h"
#include "ssim_window.h"
#include "slot_reduce.h"
#include "../../include/adgs_metrics.h"

namespace adgs {
namespace {

using namespace ssimwin;
constexpr int MAXR = ADGS_METRICS_MAX_REGIONS, ROW = ADGS_METRICS_ROW, SLOTS = ADGS_METRICS_SLOTS;
constexpr int NQ = 6;                     // sums per region: |d|, d^2 of three channels, ssim, weight
constexpr int U8W = (TSX * 3 + 3) / 4 + 1;      // 32-bit words that a tile's 8-bit row can touch (96 bytes at any alignment)
static_assert(NQ <= ROW && SLOTS == LT, "one finishing thread per slot row");

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }      // torch.clip: a NaN passes

// What the staging does to an element: clip both images; of the render (a == 0) the tile's own pixels also leave as bytes, and with
// `quantize` the staged value becomes the one a saved PNG holds.  Every product and sum here is rounded on its own (no fused
// multiply-add): the bytes must equal float32 `x * 255 + 0.5` / `255 * x` evaluated in two steps, ties included.
struct StageEval {
	int quantize, u8_mode, C, c;
	unsigned char (*u8)[TSX * 3];
	__device__ __forceinline__ float operator()(int a, float v, int ly, int lx) const {
		const float x = clip01(v);
		if (a != 0) return x;
		const float t = __fmul_rn(x, 255.f), r = __fadd_rn(t, 0.5f);
		if (u8_mode && ly >= WR && ly < WR + TSY && lx >= WR && lx < WR + TSX)
			u8[ly - WR][(lx - WR) * C + c] = (unsigned char)(int)(u8_mode == 1 ? fminf(fmaxf(r, 0.f), 255.f) : t);
		return quantize ? __fdiv_rn(floorf(r), 255.f) : x;
	}
};

__global__ void __launch_bounds__(LT) metrics_kernel(int C, int H, int W, int regions, int quantize, int u8_mode,
	const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ masks, Window win, double* __restrict__ work,
	unsigned char* __restrict__ out_u8) {
	__shared__ __attribute__((aligned(16))) float s1[HSY][SSTR], s2[HSY][SSTR];
	__shared__ __attribute__((aligned(16))) float h[5][HSY][HSTR];      // horizontally filtered x1, x2, x1^2, x2^2, x1 x2
	__shared__ __attribute__((aligned(4))) unsigned char u8[TSY][TSX * 3];
	__shared__ double red[1 + MAXR][NQ][LT / WAVE];
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * TSX, y0 = blockIdx.y * TSY;
	const int tx = tid & (TSX - 1), g = tid >> 5;       // this thread's pixels: column tx, rows 2 g and 2 g + 1
	const size_t HW = (size_t)H * W;
	bool inside[2];
	float wt[MAXR][2];
#pragma unroll
	for (int o = 0; o < 2; o++) {
		const int gx = x0 + tx, gy = y0 + 2 * g + o;
		inside[o] = gx < W && gy < H;
#pragma unroll
		for (int r = 0; r < MAXR; r++) wt[r][o] = (r < regions && inside[o]) ? masks[(size_t)r * HW + (size_t)gy * W + gx] : 0.f;
	}
	double ad[2] = { 0.0, 0.0 }, sm[2] = { 0.0, 0.0 };
	float sq[3][2] = { { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f } };
	for (int c = 0; c < C; c++) {
		// the thread index through an opaque identity: everything the passes derive from it (clamped addresses, LDS offsets, inside-the-image
		// flags of five halo elements) would otherwise be hoisted out of the channel loop and kept in registers across it -- 174 VGPRs
		// (2 waves per SIMD) instead of 111 (4); recomputing them per channel is a few integer instructions
		int lt = tid;
		asm volatile("" : "+v"(lt));
		const int ltx = lt & (TSX - 1), lg = lt >> 5;
		{
			float (*const dst[2])[SSTR] = { s1, s2 };
			const float* const src[2] = { img, gt };
			stage_halos<2>(dst, src, (size_t)c * HW, x0, y0, H, W, lt, StageEval{ quantize, u8_mode, C, c, u8 });
		}
		__syncthreads();
		{	// horizontal pass: row r, outputs 4 sx .. 4 sx + 3
			const int r = lt >> 3, sx = lt & 7;
			if (r < HSY) {
				float u[16], v[16], t[16];
				load_run(&s1[r][4 * sx], u); load_run(&s2[r][4 * sx], v);
				*reinterpret_cast<float4*>(&h[0][r][4 * sx]) = window4(win, u);
				*reinterpret_cast<float4*>(&h[1][r][4 * sx]) = window4(win, v);
#pragma unroll
				for (int i = 0; i < 16; i++) t[i] = u[i] * u[i];
				*reinterpret_cast<float4*>(&h[2][r][4 * sx]) = window4(win, t);
#pragma unroll
				for (int i = 0; i < 16; i++) t[i] = v[i] * v[i];
				*reinterpret_cast<float4*>(&h[3][r][4 * sx]) = window4(win, t);
#pragma unroll
				for (int i = 0; i < 16; i++) t[i] = u[i] * v[i];
				*reinterpret_cast<float4*>(&h[4][r][4 * sx]) = window4(win, t);
			}
		}
		__syncthreads();
		// vertical pass: column tx, outputs rows 2 g and 2 g + 1
		float acc[5][2];
#pragma unroll
		for (int q = 0; q < 5; q++) {
			float col[NT + 1];
#pragma unroll
			for (int j = 0; j < NT + 1; j++) col[j] = h[q][2 * lg + j][ltx];
#pragma unroll
			for (int o = 0; o < 2; o++) {
				float a = 0.f;
#pragma unroll
				for (int k = 0; k < NT; k++) a += win.g[k] * col[o + k];
				acc[q][o] = a;
			}
		}
#pragma unroll
		for (int o = 0; o < 2; o++) {
			if (!inside[o]) continue;
			const int ty = 2 * lg + o;
			const float mu1 = acc[0][o], mu2 = acc[1][o], e11 = acc[2][o], e22 = acc[3][o], e12 = acc[4][o];
			const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
			const float sg1 = e11 - mu1_sq, sg2 = e22 - mu2_sq, sg12 = e12 - mu12;
			const float A1 = 2.f * mu12 + C1, A2 = 2.f * sg12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = sg1 + sg2 + C2;
			const float D = B1 * B2, inv = 1.f / D;
			sm[o] += (double)((A1 * A2) * inv);
			const float d = s1[ty + WR][ltx + WR] - s2[ty + WR][ltx + WR];
			ad[o] += (double)fabsf(d);
			const float d2 = __fmul_rn(d, d);
			if (c == 0) sq[0][o] = d2; else if (c == 1) sq[1][o] = d2; else sq[2][o] = d2;
		}
		__syncthreads();                  // s1 / s2 / h are restaged by the next channel; the last one publishes the byte tile
	}
	// region 0: the whole image; region r: mask r - 1
#pragma unroll
	for (int r = 0; r <= MAXR; r++) {
		if (r > regions) break;
		double v[NQ] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
		for (int o = 0; o < 2; o++) {
			const double w = r == 0 ? (inside[o] ? 1.0 : 0.0) : (double)wt[r > 0 ? r - 1 : 0][o];
			v[0] += w * ad[o]; v[1] += w * (double)sq[0][o]; v[2] += w * (double)sq[1][o]; v[3] += w * (double)sq[2][o]; v[4] += w * sm[o]; v[5] += w;
		}
#pragma unroll
		for (int q = 0; q < NQ; q++) {
			wave_sum(v[q]);
			if ((tid & (WAVE - 1)) == 0) red[r][q][tid / WAVE] = v[q];
		}
	}
	__syncthreads();
	const int nreg = 1 + regions;
	if (tid < nreg * NQ) {
		const int r = tid / NQ, q = tid - r * NQ;
		double t = 0.0;
		for (int w = 0; w < LT / WAVE; w++) t += red[r][q][w];
		const unsigned b = blockIdx.y * gridDim.x + blockIdx.x;
		if (t != 0.0) atomicAdd(work + ((size_t)(b % SLOTS) * nreg + r) * ROW + q, t);      // a region that has no weight in this tile adds nothing
	}
	if (u8_mode) {
		// the tile's rows of the H x W x C byte image: whole aligned 32-bit words where all four bytes belong to this tile's row, single bytes
		// at the two ends (3 W need not be a multiple of 4: a row starts at any alignment, and the word is shared with the neighbouring tile)
		const int rows = min(TSY, H - y0), len = min(TSX, W - x0) * C;
		for (int i = tid; i < TSY * U8W; i += LT) {
			const int row = i / U8W, k = i - row * U8W;
			if (row >= rows) continue;
			unsigned char* dst = out_u8 + ((size_t)(y0 + row) * W + x0) * C;
			const int b0 = 4 * k - (int)((uintptr_t)dst & 3);          // the word's first byte, as an index into the row
			if (b0 >= len) continue;
			if (b0 >= 0 && b0 + 4 <= len) {
				const unsigned v = (unsigned)u8[row][b0] | ((unsigned)u8[row][b0 + 1] << 8) | ((unsigned)u8[row][b0 + 2] << 16) | ((unsigned)u8[row][b0 + 3] << 24);
				*reinterpret_cast<unsigned*>(dst + b0) = v;
			} else {
#pragma unroll
				for (int j = 0; j < 4; j++) if (b0 + j >= 0 && b0 + j < len) dst[b0 + j] = u8[row][b0 + j];
			}
		}
	}
}

// one block per region: the slot rows' totals -> the table row of (view, region); the slot rows are consumed (zero afterwards)
__global__ void __launch_bounds__(LT) metrics_finish_kernel(int nreg, double* __restrict__ work, double* __restrict__ table_rows) {
	__shared__ double s[NQ][LT / WAVE];
	const int r = blockIdx.x;
	double* p = work + ((size_t)threadIdx.x * nreg + r) * ROW;
#pragma unroll
	for (int q = 0; q < NQ; q++) {
		double v = p[q];
		p[q] = 0.0;
		wave_sum(v);
		if ((threadIdx.x & (WAVE - 1)) == 0) s[q][threadIdx.x / WAVE] = v;
	}
	__syncthreads();
	if (threadIdx.x < ROW) {
		double t = 0.0;
		if (threadIdx.x < NQ) for (int w = 0; w < LT / WAVE; w++) t += s[threadIdx.x][w];
		table_rows[(size_t)r * ROW + threadIdx.x] = t;
	}
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_metrics_work_doubles(int regions) {
	if (regions < 0 || regions > MAXR) return 0;
	return (size_t)SLOTS * (size_t)(1 + regions) * ROW;
}

extern "C" int adgs_metrics_accumulate(const adgs_metrics_desc* desc, const float* image, const float* gt, const float* masks, double* work, double* table,
	int view_index, uint8_t* out_u8, void* stream_) {
	const char* who = "adgs_metrics_accumulate: ";
	if (!desc) { set_error(std::string(who) + "NULL descriptor"); return -1; }
	if (desc->struct_bytes < (int)sizeof(adgs_metrics_desc)) { set_error(std::string(who) + "struct_bytes is smaller than adgs_metrics_desc"); return -1; }
	if (desc->channels != 1 && desc->channels != 3) { set_error(std::string(who) + "channels must be 1 or 3"); return -1; }
	if (desc->H < 1 || desc->W < 1) { set_error(std::string(who) + "H and W must be at least 1"); return -1; }
	if (desc->regions < 0 || desc->regions > MAXR) { set_error(std::string(who) + "regions must be 0 .. " + std::to_string(MAXR)); return -1; }
	if (desc->regions > 0 && !masks) { set_error(std::string(who) + "regions > 0 with NULL masks"); return -1; }
	if (view_index < 0) { set_error(std::string(who) + "view_index must not be negative"); return -1; }
	if (desc->quantize != 0 && desc->quantize != 1) { set_error(std::string(who) + "quantize must be 0 or 1"); return -1; }
	if (desc->u8_mode < 0 || desc->u8_mode > 2) { set_error(std::string(who) + "u8_mode must be 0 (none), 1 (round) or 2 (truncate)"); return -1; }
	if (desc->u8_mode != 0 && !out_u8) { set_error(std::string(who) + "u8_mode without out_u8"); return -1; }
	if (!image || !gt || !work || !table) { set_error(std::string(who) + "NULL image / gt / work / table"); return -1; }
	const int gx = (desc->W + TSX - 1) / TSX, gy = (desc->H + TSY - 1) / TSY;
	if (gy > 65535) { set_error(std::string(who) + "image higher than 65535 tiles"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	static const Window win = make_window();
	const int nreg = 1 + desc->regions;
	hipLaunchKernelGGL(metrics_kernel, dim3(gx, gy), dim3(LT), 0, stream, desc->channels, desc->H, desc->W, desc->regions, desc->quantize, desc->u8_mode,
		image, gt, masks, win, work, out_u8);
	hipLaunchKernelGGL(metrics_finish_kernel, dim3(nreg), dim3(LT), 0, stream, nreg, work, table + (size_t)view_index * nreg * ROW);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}
