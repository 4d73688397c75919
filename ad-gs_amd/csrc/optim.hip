// Fused multi-tensor Adam for gfx950: every parameter group of the model in one launch, one pass
// over (p, g, m, v) -- 16 B read + 12 B written per parameter (+4 B when the gradient is zeroed),
// the HBM-streaming floor of the update.  Reference: torch.optim.Adam as configured at
// scene/gaussian_model.py:370 (eps = 1e-15, no weight decay), stepped at train.py:163-167.
#include "common.h"
#include "adam_update.h"
#include "kernels.h"
#include "../../include/adgs_optim.h"
#include <cmath>
#include <string>
#include <type_traits>

namespace adgs {
namespace {

constexpr int AB = 256;                 // threads per block
constexpr int AV = 4;                   // elements per thread per iteration (one 16-byte access per array)
constexpr int AI = 4;                   // iterations per thread
constexpr int ATILE = AB * AV * AI;     // elements per block
static_assert(WAVE * AV == ADGS_ADAM_TILE && ATILE % ADGS_ADAM_TILE == 0, "adgs_adam_group.tile_active: one byte per wave and iteration");

struct AdamTable {
	adgs_adam_group g[ADGS_ADAM_MAX_GROUPS];
	uint32_t first_block[ADGS_ADAM_MAX_GROUPS + 1];     // group i owns blocks [first_block[i], first_block[i+1])
	float step_size[ADGS_ADAM_MAX_GROUPS];               // lr / (1 - beta1^t)
	float inv_bc2_sqrt[ADGS_ADAM_MAX_GROUPS];            // 1 / sqrt(1 - beta2^t)
	int n;
	float beta1, beta2, eps;
	int zero_grad;
};

// Row visibility of the groups of a masked launch (adgs_adam_step_rows), parallel to AdamTable::g.  visible == nullptr: dense group.
struct AdamRows { const void* visible; uint32_t row_len; int32_t kind; };
struct AdamRowTable : AdamTable { AdamRows rows[ADGS_ADAM_MAX_GROUPS]; };
static_assert(sizeof(AdamRows) <= 24 && sizeof(AdamRowTable) <= 4096, "the launch arguments of the masked step: <= 24 B per group, < 4 KiB in all");

__device__ __forceinline__ bool row_visible(const void* visible, int kind, int64_t row) {
	return kind == ADGS_ADAM_ROWS_INT32 ? static_cast<const int32_t*>(visible)[row] > 0 : static_cast<const uint8_t*>(visible)[row] != 0;
}

// MASKED = false is the dense step.  MASKED = true (adgs_adam_step_rows): a group with a row visibility is viewed as [n_rows, row_len];
// rows that are not visible keep the bits of p / m / v and their gradient is not read.  Everything MASKED adds sits under
// `if constexpr`, so the dense instantiation is the code it was before the masked one existed.
template <bool MASKED>
__global__ void __launch_bounds__(AB) adam_kernel(const std::conditional_t<MASKED, AdamRowTable, AdamTable> t) {
	// which group does this block belong to (block-uniform binary search over <= 32 entries)
	int lo = 0, hi = t.n;
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (blockIdx.x >= t.first_block[mid]) lo = mid; else hi = mid; }
	const adgs_adam_group& G = t.g[lo];
	const float step_size = t.step_size[lo], ibc2 = t.inv_bc2_sqrt[lo];
	const int64_t base = (int64_t)(blockIdx.x - t.first_block[lo]) * ATILE;
	const bool zero_grad = t.zero_grad || (G.flags & ADGS_ADAM_ZERO_GRAD);
	const bool vec = ((reinterpret_cast<uintptr_t>(G.param) | reinterpret_cast<uintptr_t>(G.grad) | reinterpret_cast<uintptr_t>(G.exp_avg) |
	                   reinterpret_cast<uintptr_t>(G.exp_avg_sq)) & 15) == 0;
	// masked group: which of a thread's AV * AI elements sit in a visible row (bit 4 * it + k: element k of iteration `it` exists and is
	// visible), worked out BEFORE the loop: the visibility loads of all AI iterations are in flight together, and nothing of p / g / m / v
	// waits behind a division.  The block's first element is turned into (row, offset in the row) by the launch's one 64-bit division;
	// a thread's first element by a 32-bit one (it is < row_len + ATILE further on); later iterations advance by AB * AV with add / compare.
	[[maybe_unused]] const void* visible = nullptr;
	[[maybe_unused]] unsigned masks = 0;
	if constexpr (MASKED) {
		visible = t.rows[lo].visible;
		if (visible) {
			const uint32_t L = t.rows[lo].row_len;
			const int kind = t.rows[lo].kind;
			const int64_t row0 = base / (int64_t)L;
			const uint32_t e = (uint32_t)(base - row0 * (int64_t)L) + threadIdx.x * AV;
			uint32_t q = e / L, c = e - q * L;
			const uint32_t dq = (uint32_t)(AB * AV) / L, dr = (uint32_t)(AB * AV) - dq * L;
#pragma unroll
			for (int it = 0; it < AI; it++) {
				const int64_t i = base + ((int64_t)it * AB + threadIdx.x) * AV;
				const int64_t row = row0 + q;
				unsigned m4 = 0;
				if (L >= (uint32_t)AV) {
					// the quad touches at most two rows: its first `L - c` elements are in `row`, the others in `row + 1`
					if (i < G.numel) {
						const uint32_t head = L - c;                         // >= 1
						const bool on0 = row_visible(visible, kind, row);
						const bool on1 = (head < (uint32_t)AV && i + head < G.numel) ? row_visible(visible, kind, row + 1) : false;
#pragma unroll
						for (int k = 0; k < AV; k++) m4 |= ((i + k < G.numel) && ((uint32_t)k < head ? on0 : on1) ? 1u : 0u) << k;
					}
				} else {
					// rows of 1 - 3 elements: element k is (c + k) / L rows further on; four independent loads
#pragma unroll
					for (int k = 0; k < AV; k++) {
						const uint32_t ck = c + k, off = (ck >= L ? 1u : 0u) + (ck >= 2 * L ? 1u : 0u) + (ck >= 3 * L ? 1u : 0u);
						if (i + k < G.numel) m4 |= (row_visible(visible, kind, row + off) ? 1u : 0u) << k;
					}
				}
				masks |= m4 << (AV * it);
				q += dq; c += dr;
				if (c >= L) { c -= L; q++; }
			}
		}
	}
#pragma unroll
	for (int it = 0; it < AI; it++) {
		const int64_t i = base + ((int64_t)it * AB + threadIdx.x) * AV;
		// the 64 lanes of a wave cover one tile of ADGS_ADAM_TILE = 256 consecutive elements per iteration (i0 = its first element):
		// everything about the tile map is wave-uniform
		const int64_t i0 = base + ((int64_t)it * AB + (threadIdx.x & ~(WAVE - 1))) * AV;
		if (i0 >= G.numel) break;
		if (G.tile_active) {
			// a tile whose gradients and moments have been zero in every step so far: the update is the identity -- read the
			// gradient only (4 of the 28 bytes per element) and skip the tile while that is still all zero
			const int64_t tile = i0 / ADGS_ADAM_TILE;
			if (G.tile_active[tile] == 0) {
				if (G.flags & ADGS_ADAM_TILES_MARKED) continue;      // the gradient's producer marks the tiles it writes: nothing to look at
				bool nz = false;
				if (i < G.numel) {
					if (vec && i + AV <= G.numel) { const float4 g = *reinterpret_cast<const float4*>(G.grad + i); nz = g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f; }
					else for (int k = 0; k < AV && i + k < G.numel; k++) nz = nz || G.grad[i + k] != 0.f;
				}
				if (__ballot(nz) == 0ull) continue;
				if ((threadIdx.x & (WAVE - 1)) == 0) G.tile_active[tile] = 1;
			}
		}
		if constexpr (MASKED) {
			if (visible) {
				// bits k: element i + k exists and its row is visible
				const unsigned mask = (masks >> (AV * it)) & 15u;
				// every element of the tile visible (the usual case of a camera that sees most of the model): the dense code below
				if (__ballot(i + AV <= G.numel && mask != 15u) != 0ull || i0 + ADGS_ADAM_TILE > G.numel) {
					if (__ballot(mask != 0) == 0ull && !zero_grad) continue;          // no visible row in the tile: the wave touches nothing
					if (i >= G.numel) continue;
					const bool quad = vec && i + AV <= G.numel;
					if (mask == 0) {                                                  // no load, no store of p / m / v
						if (zero_grad) {
							if (quad) *reinterpret_cast<float4*>(G.grad + i) = make_float4(0.f, 0.f, 0.f, 0.f);
							else for (int k = 0; k < AV && i + k < G.numel; k++) G.grad[i + k] = 0.f;
						}
						continue;
					}
					if (quad) {
						const float4 p0 = ld_stream4(reinterpret_cast<const float4*>(G.param + i)), g = ld_stream4(reinterpret_cast<const float4*>(G.grad + i));
						const float4 m0 = ld_stream4(reinterpret_cast<const float4*>(G.exp_avg + i)), v0 = ld_stream4(reinterpret_cast<const float4*>(G.exp_avg_sq + i));
						float4 p = p0, m = m0, v = v0;
						adam_update(p.x, m.x, v.x, g.x, t.beta1, t.beta2, t.eps, step_size, ibc2);
						adam_update(p.y, m.y, v.y, g.y, t.beta1, t.beta2, t.eps, step_size, ibc2);
						adam_update(p.z, m.z, v.z, g.z, t.beta1, t.beta2, t.eps, step_size, ibc2);
						adam_update(p.w, m.w, v.w, g.w, t.beta1, t.beta2, t.eps, step_size, ibc2);
						if (mask != 15u) {
							// the quad straddles a visible and an invisible row: the invisible components go back with the bits they came with
							// (moves, no arithmetic: whatever their gradient held -- NaN, Inf -- does not reach them)
							if (!(mask & 1u)) { p.x = p0.x; m.x = m0.x; v.x = v0.x; }
							if (!(mask & 2u)) { p.y = p0.y; m.y = m0.y; v.y = v0.y; }
							if (!(mask & 4u)) { p.z = p0.z; m.z = m0.z; v.z = v0.z; }
							if (!(mask & 8u)) { p.w = p0.w; m.w = m0.w; v.w = v0.w; }
						}
						st_stream4(reinterpret_cast<float4*>(G.param + i), p);
						st_stream4(reinterpret_cast<float4*>(G.exp_avg + i), m);
						st_stream4(reinterpret_cast<float4*>(G.exp_avg_sq + i), v);
						if (zero_grad) *reinterpret_cast<float4*>(G.grad + i) = make_float4(0.f, 0.f, 0.f, 0.f);
					} else {
						for (int k = 0; k < AV && i + k < G.numel; k++) {
							if (mask & (1u << k)) {
								float p = G.param[i + k], m = G.exp_avg[i + k], v = G.exp_avg_sq[i + k];
								adam_update(p, m, v, G.grad[i + k], t.beta1, t.beta2, t.eps, step_size, ibc2);
								G.param[i + k] = p; G.exp_avg[i + k] = m; G.exp_avg_sq[i + k] = v;
							}
							if (zero_grad) G.grad[i + k] = 0.f;
						}
					}
					continue;
				}
			}
		}
		if (i >= G.numel) continue;
		if (vec && i + AV <= G.numel) {
			float4 p = ld_stream4(reinterpret_cast<const float4*>(G.param + i)), g = ld_stream4(reinterpret_cast<const float4*>(G.grad + i));
			float4 m = ld_stream4(reinterpret_cast<const float4*>(G.exp_avg + i)), v = ld_stream4(reinterpret_cast<const float4*>(G.exp_avg_sq + i));
			adam_update(p.x, m.x, v.x, g.x, t.beta1, t.beta2, t.eps, step_size, ibc2);
			adam_update(p.y, m.y, v.y, g.y, t.beta1, t.beta2, t.eps, step_size, ibc2);
			adam_update(p.z, m.z, v.z, g.z, t.beta1, t.beta2, t.eps, step_size, ibc2);
			adam_update(p.w, m.w, v.w, g.w, t.beta1, t.beta2, t.eps, step_size, ibc2);
			st_stream4(reinterpret_cast<float4*>(G.param + i), p);
			st_stream4(reinterpret_cast<float4*>(G.exp_avg + i), m);
			st_stream4(reinterpret_cast<float4*>(G.exp_avg_sq + i), v);
			if (zero_grad) *reinterpret_cast<float4*>(G.grad + i) = make_float4(0.f, 0.f, 0.f, 0.f);
		} else {
			for (int k = 0; k < AV && i + k < G.numel; k++) {
				float p = G.param[i + k], m = G.exp_avg[i + k], v = G.exp_avg_sq[i + k];
				adam_update(p, m, v, G.grad[i + k], t.beta1, t.beta2, t.eps, step_size, ibc2);
				G.param[i + k] = p; G.exp_avg[i + k] = m; G.exp_avg_sq[i + k] = v;
				if (zero_grad) G.grad[i + k] = 0.f;
			}
		}
	}
}

__global__ void __launch_bounds__(256) densification_stats_kernel(int N, const int32_t* __restrict__ radii, const float* __restrict__ g,
	float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_r) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= N) return;
	const int r = radii[i];
	if (r <= 0) return;                                   // visibility_filter = radii > 0 (gaussian_renderer/__init__.py:101)
	const float gx = g[3 * (size_t)i], gy = g[3 * (size_t)i + 1];
	accum[i] += sqrtf(gx * gx + gy * gy);                 // torch.norm(grad[:, :2], dim=-1)
	denom[i] += 1.f;
	if (max_r) max_r[i] = fmaxf(max_r[i], (float)r);
}

} // namespace

// the host forms the bias corrections in double like torch does (python floats), then rounds once
void adam_bias_terms(float lr, int step, float beta1, float beta2, float* step_size, float* inv_bc2_sqrt) {
	const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
	*step_size = (float)((double)lr / bc1);
	*inv_bc2_sqrt = (float)(1.0 / std::sqrt(bc2));
}
} // namespace adgs

using namespace adgs;

extern "C" int adgs_densification_stats(int N, const int32_t* radii, const float* viewspace_grad, float* xyz_gradient_accum, float* denom,
	float* max_radii2D, void* stream) {
	if (N <= 0) return 0;
	if (!radii || !viewspace_grad || !xyz_gradient_accum || !denom) { set_error("adgs_densification_stats: NULL pointer"); return -1; }
	hipLaunchKernelGGL(densification_stats_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, radii, viewspace_grad, xyz_gradient_accum, denom, max_radii2D);
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

// `who`: the entry the caller used, for adgs_last_error()
static int adam_step(const std::string& who, const adgs_adam_group* groups, const adgs_adam_rows* rows, int n_groups, float beta1, float beta2, float eps, int zero_grad,
	void* stream_) {
	if (n_groups <= 0) return 0;
	if (!groups || n_groups > ADGS_ADAM_MAX_GROUPS) { set_error(who + ": between 1 and 32 groups per call"); return -1; }
	AdamRowTable t;
	t.n = 0; t.beta1 = beta1; t.beta2 = beta2; t.eps = eps; t.zero_grad = zero_grad;
	uint64_t blocks = 0;
	bool masked = false;
	for (int i = 0; i < n_groups; i++) {
		const adgs_adam_group& g = groups[i];
		AdamRows r = {nullptr, 1u, ADGS_ADAM_ROWS_DENSE};
		if (rows && rows[i].kind != ADGS_ADAM_ROWS_DENSE) {
			const adgs_adam_rows& v = rows[i];
			if (v.kind != ADGS_ADAM_ROWS_INT32 && v.kind != ADGS_ADAM_ROWS_UINT8) { set_error("adgs_adam_step_rows: unknown kind of row visibility"); return -2; }
			if (v.row_len < 1 || v.n_rows < 0 || g.numel < 0 || v.n_rows != g.numel / v.row_len || g.numel % v.row_len != 0) {
				set_error("adgs_adam_step_rows: n_rows * row_len must be the group's numel, row_len >= 1"); return -2;
			}
			if (g.tile_active) { set_error("adgs_adam_step_rows: a group with a row visibility cannot have a tile_active map as well"); return -2; }
			if (!v.visible && v.n_rows > 0) { set_error("adgs_adam_step_rows: NULL row visibility"); return -2; }
			r.visible = v.visible; r.row_len = (uint32_t)v.row_len; r.kind = v.kind;
		}
		if (g.numel <= 0) continue;
		if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq || g.step < 1) { set_error(who + ": NULL pointer or step < 1 in a group"); return -1; }
		t.g[t.n] = g;
		t.rows[t.n] = r;
		masked = masked || r.visible != nullptr;
		t.first_block[t.n] = (uint32_t)blocks;
		adam_bias_terms(g.lr, g.step, beta1, beta2, &t.step_size[t.n], &t.inv_bc2_sqrt[t.n]);
		blocks += (uint64_t)((g.numel + ATILE - 1) / ATILE);
		t.n++;
	}
	if (t.n == 0) return 0;
	if (blocks > 0x7fffffffull) { set_error(who + ": too many elements for one launch"); return -1; }
	t.first_block[t.n] = (uint32_t)blocks;
	// no group with a visibility: the dense kernel, with the table it has always taken
	if (masked) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(AB), 0, (hipStream_t)stream_, t);
	else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(AB), 0, (hipStream_t)stream_, static_cast<const AdamTable&>(t));
	ADGS_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" int adgs_adam_step_rows(const adgs_adam_group* groups, const adgs_adam_rows* rows, int n_groups, float beta1, float beta2, float eps, int zero_grad,
	void* stream_) {
	return adam_step("adgs_adam_step_rows", groups, rows, n_groups, beta1, beta2, eps, zero_grad, stream_);
}

extern "C" int adgs_adam_step(const adgs_adam_group* groups, int n_groups, float beta1, float beta2, float eps, int zero_grad, void* stream_) {
	return adam_step("adgs_adam_step", groups, nullptr, n_groups, beta1, beta2, eps, zero_grad, stream_);
}
