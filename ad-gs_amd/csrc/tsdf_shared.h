// The device functions that the dense volume (tsdf.hip) and the block-sparse one (tsdf_sparse.hip) share: the per-point update chain of
// include/adgs_tsdf.h (steps 1-9) and the marching-tetrahedra pieces (the tables, classify, cell_faces, the faces of a cell).  Both files
// are built with the same flags and call the SAME functions, so a lattice point that both volumes hold and that saw the same views has
// the same bits in both.  The host code the two volumes' entry points share is here as well: the check of a view, the scratch of the extraction,
// the tail of extract_count and the argument checks of extract_emit, each with the entry's name for its messages.
#pragma once
#include "common.h"
#include "../../include/adgs_tsdf.h"
#include <climits>

namespace adgs {
namespace {

struct Lattice {
	int nx, ny, nz;
	unsigned n;             // nx ny nz < 2^31
	double vs, o[3];
};

struct TsdfView {
	int H, W, inv_depth;
	double kx, ky, cx, cy;  // W / (2 tanfovx), H / (2 tanfovy), (W - 1) / 2, (H - 1) / 2
	double R[9], t[3];
	double near, max_depth, trunc, max_weight;
	float min_opacity;
};

// What both volumes refuse of a view, in this order; then `v` is set.  -> 0 or -1
int check_view(const std::string& name, const adgs_tsdf_view* view, TsdfView& v) {
	if (view->struct_bytes < (int)sizeof(adgs_tsdf_view)) { set_error(name + ": struct_bytes is smaller than adgs_tsdf_view"); return -1; }
	if (view->H < 0 || view->W < 0) { set_error(name + ": negative H or W"); return -1; }
	if ((long long)view->H * view->W > (long long)INT_MAX) { set_error(name + ": H * W exceeds INT_MAX"); return -1; }
	if (!positive(view->tanfovx) || !positive(view->tanfovy)) { set_error(name + ": tanfovx and tanfovy must be finite and > 0"); return -1; }
	if (!positive(view->trunc)) { set_error(name + ": trunc must be finite and > 0"); return -1; }
	if (!(positive(view->min_opacity) && view->min_opacity <= 1.f)) { set_error(name + ": min_opacity must lie in (0, 1]"); return -1; }
	if (!(view->max_weight > 0.f)) { set_error(name + ": max_weight must be > 0"); return -1; }
	if (!(std::isfinite(view->near) && view->near >= 0.f)) { set_error(name + ": near must be finite and >= 0"); return -1; }
	for (int i = 0; i < 12; i++)
		if (!std::isfinite(view->pose[i])) { set_error(name + ": the pose must be finite"); return -1; }
	v.H = view->H; v.W = view->W; v.inv_depth = view->inv_depth ? 1 : 0;
	v.kx = (double)view->W / (2.0 * (double)view->tanfovx); v.ky = (double)view->H / (2.0 * (double)view->tanfovy);
	v.cx = 0.5 * (double)(view->W - 1); v.cy = 0.5 * (double)(view->H - 1);
	for (int i = 0; i < 9; i++) v.R[i] = view->pose[i];
	for (int i = 0; i < 3; i++) v.t[i] = view->pose[9 + i];
	v.near = (double)view->near; v.max_depth = (double)view->max_depth; v.trunc = (double)view->trunc; v.max_weight = (double)view->max_weight;
	v.min_opacity = view->min_opacity;
	return 0;
}

// Steps 1-9 for the lattice point (i, j, k) of the lattice at `L.o` with spacing `L.vs`; t, w: its tsdf and wsum; c: its first colour value (or
// NULL), the next channel `cstride` floats further.  A point that fails a gate returns before it reads or writes its values.
__device__ __forceinline__ void tsdf_update_point(const Lattice& L, const TsdfView& v, int i, int j, int k, const float* __restrict__ depth,
	const float* __restrict__ opacity, const float* __restrict__ image, const float* __restrict__ weight, float* __restrict__ t, float* __restrict__ wp,
	float* __restrict__ c, size_t cstride) {
	const double X0 = L.o[0] + L.vs * (double)i, X1 = L.o[1] + L.vs * (double)j, X2 = L.o[2] + L.vs * (double)k;
	const double z = v.R[6] * X0 + v.R[7] * X1 + v.R[8] * X2 + v.t[2];
	if (!(z > v.near)) return;
	const double x = v.R[0] * X0 + v.R[1] * X1 + v.R[2] * X2 + v.t[0];
	const double y = v.R[3] * X0 + v.R[4] * X1 + v.R[5] * X2 + v.t[1];
	// A cull in front of the exact test, to spare most of the lattice the two divisions: with z > 0, u + 0.5 < -1 and u + 0.5 > W + 1 are
	// x kx < -(cx + 1.5) z and x kx > (W + 0.5 - cx) z.  The margin of one pixel is far beyond any rounding of either form, so this never
	// drops a point the exact test keeps; false for NaN.  A wave whose 64 points all lie outside leaves here as a whole.
	const double xk = x * v.kx, yk = y * v.ky;
	if (xk < -(v.cx + 1.5) * z || xk > ((double)v.W + 0.5 - v.cx) * z || yk < -(v.cy + 1.5) * z || yk > ((double)v.H + 0.5 - v.cy) * z) return;
	const double uf =floor((x / z) * v.kx + v.cx + 0.5), vf = floor((y / z) * v.ky + v.cy + 0.5);
	if (!(uf >= 0.0 && uf < (double)v.W && vf >= 0.0 && vf < (double)v.H)) return;          // false for NaN
	// 0 <= xi < W and 0 <= yi < H: pix lies inside the images
	const size_t pix = (size_t)(int)vf * v.W + (int)uf;
	const float Of = opacity[pix], Df = depth[pix];
	if (!(Of >= v.min_opacity) || !(Df > 0.f)) return;
	const float wf = weight ? weight[pix] : 1.f;
	if (!(wf > 0.f)) return;
	const double zd = v.inv_depth ? (double)Of / (double)Df : (double)Df / (double)Of;
	if (!(zd <= v.max_depth)) return;
	const double sdf = zd - z;
	if (!(sdf >= -v.trunc)) return;
	const double d = fmin(1.0, sdf / v.trunc), w = (double)wf;
	const double W0 = (double)*wp, Wn = W0 + w;                 // > 0: w > 0 and the stored sum is never negative
	*t = (float)(((double)*t * W0 + d * w) / Wn);
	if (c) {
		const size_t plane = (size_t)v.H * v.W;
#pragma unroll
		for (int ch = 0; ch < 3; ch++) {
			float* dst = c + (size_t)ch * cstride;
			*dst = (float)(((double)*dst * W0 + (double)image[ch * plane + pix] * w) / Wn);
		}
	}
	*wp = (float)fmin(Wn, v.max_weight);
}

// ---- extraction ----

// the tet-vertex corner bits (x = 1, y = 2, z = 4) of the 6 Kuhn tets, 4 bits each from tet vertex 0 up; tets 0, 3, 4 have an even axis order
__device__ constexpr uint16_t TET_CORNERS[6] = { 0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640 };
// the slots +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z as corner bits, and the slot of a corner-bit difference d in nibble d
__device__ constexpr uint8_t BITS_OF_SLOT[7] = { 1, 2, 4, 3, 5, 6, 7 };
constexpr uint32_t SLOT_OF_BITS = 0x65423100u;
// the inside sets (bit m: tet vertex m is inside) whose triangles are reversed: even axis orders, then odd (the complement among the mixed sets);
// pinned by exact face equality against the geometric rule of tests/tsdf_ref.py
constexpr uint32_t REV_EVEN = 0x25A4, REV_ODD = 0x5A5A;

struct PointClass {
	uint32_t in8;           // bit b: corner p + b exists and is inside
	uint32_t vmask;         // the active slots of the 7 edges p owns
	bool cell;              // p's own cell is valid and has corners of both signs
};

// idx < L.n.  Reads tsdf at p + {0, 1}^3 and, when those differ in sign, wsum at p + {-1, 0, 1}^3, inside the lattice only.
__device__ __forceinline__ PointClass classify(const Lattice& L, const float* __restrict__ tsdf, const float* __restrict__ wsum, float min_weight,
	unsigned idx, int i, int j, int k) {
	PointClass pc; pc.in8 = 0; pc.vmask = 0; pc.cell = false;
	const size_t sx = 1, sy = (size_t)L.nx, sz = (size_t)L.nx * L.ny;
	uint32_t have = 0;
#pragma unroll
	for (int b = 0; b < 8; b++) {
		const int dx = b & 1, dy = (b >> 1) & 1, dz = b >> 2;
		if (i + dx < L.nx && j + dy < L.ny && k + dz < L.nz) {
			have |= 1u << b;
			if (tsdf[idx + dx * sx + dy * sy + dz * sz] < 0.f) pc.in8 |= 1u << b;
		}
	}
	if (pc.in8 == 0 || pc.in8 == have) return pc;              // one sign: no edge of p and no tet of its cell is cut
	uint32_t ok = 0;                                            // bit ((dz + 1) 3 + dy + 1) 3 + dx + 1: the corner exists and has wsum >= min_weight
#pragma unroll
	for (int dz = -1; dz <= 1; dz++)
#pragma unroll
		for (int dy = -1; dy <= 1; dy++)
#pragma unroll
			for (int dx = -1; dx <= 1; dx++) {
				const int a = i + dx, b = j + dy, c = k + dz;
				if (a >= 0 && a < L.nx && b >= 0 && b < L.ny && c >= 0 && c < L.nz && wsum[(size_t)c * sz + (size_t)b * sy + (size_t)a] >= min_weight)
					ok |= 1u << (((dz + 1) * 3 + dy + 1) * 3 + dx + 1);
			}
	// cell with lowest corner p + (a, b, c), a, b, c in {-1, 0}: valid when its 8 corners are
	uint32_t cells = 0;                                         // bit (c + 1) 4 + (b + 1) 2 + (a + 1)
#pragma unroll
	for (int q = 0; q < 8; q++) {
		const int a = (q & 1) - 1, b = ((q >> 1) & 1) - 1, c = (q >> 2) - 1;
		uint32_t need = 0;
#pragma unroll
		for (int e = 0; e < 8; e++) need |= 1u << (((c + (e >> 2) + 1) * 3 + b + ((e >> 1) & 1) + 1) * 3 + a + (e & 1) + 1);
		if ((ok & need) == need) cells |= 1u << q;
	}
	const bool in_p = pc.in8 & 1u;
#pragma unroll
	for (int s = 0; s < 7; s++) {
		const int ob = BITS_OF_SLOT[s];
		if (!((have >> ob) & 1u) || (((pc.in8 >> ob) & 1u) != 0) == in_p) continue;
		// the cells that contain the edge: along an axis the edge spans, the cell starts at p; along the others at p - 1 or p
		uint32_t with = 0;
#pragma unroll
		for (int q = 0; q < 8; q++) if ((q & ob) == ob) with |= 1u << q;      // q's bit of an axis set: the cell starts at p on that axis
		if (cells & with) pc.vmask |= 1u << s;
	}
	pc.cell = (cells >> 7) & 1u;                                // its corners are p + {0, 1}^3, of both signs here
	return pc;
}

// faces of the valid mixed cell with corner signs in8
__device__ __forceinline__ uint32_t cell_faces(uint32_t in8) {
	uint32_t f = 0;
#pragma unroll
	for (int t = 0; t < 6; t++) {
		const uint32_t c = TET_CORNERS[t];
		const int n = (int)((in8 >> (c & 15)) & 1u) + (int)((in8 >> ((c >> 4) & 15)) & 1u) + (int)((in8 >> ((c >> 8) & 15)) & 1u) + (int)((in8 >> (c >> 12)) & 1u);
		f += n == 2 ? 2u : (n == 1 || n == 3 ? 1u : 0u);
	}
	return f;
}

// Writes the triangles of the valid mixed cell with corner signs in8 from face `f` on (below n_faces only).  vid(lo, hi): the id of the vertex on
// the edge between the cell's corners lo < hi (corner bits, lo a subset of hi); it exists.
template <typename Vid>
__device__ __forceinline__ void cell_emit_faces(uint32_t in8, Vid vid, size_t f, size_t n_faces, int* __restrict__ faces) {
#pragma unroll
	for (int t = 0; t < 6; t++) {
		const uint32_t c = TET_CORNERS[t];
		uint32_t m = 0;                                         // bit q: tet vertex q is inside
#pragma unroll
		for (int q = 0; q < 4; q++) m |= ((in8 >> ((c >> (4 * q)) & 15u)) & 1u) << q;
		const int n = __popc(m);
		if (n == 0 || n == 4) continue;
		// the vertex on the edge between tet vertices a and b
		auto e = [&](int a, int b) -> int { return vid((int)((c >> (4 * min(a, b))) & 15u), (int)((c >> (4 * max(a, b))) & 15u)); };
		const bool rev = ((t == 0 || t == 3 || t == 4 ? REV_EVEN : REV_ODD) >> m) & 1u;
		auto put = [&](int p0, int p1, int p2) {
			if (f < n_faces) { faces[3 * f + 0] = rev ? p2 : p0; faces[3 * f + 1] = p1; faces[3 * f + 2] = rev ? p0 : p2; }
			f++;
		};
		if (n == 2) {
			const uint32_t out = ~m & 15u;
			const int a = __ffs((int)m) - 1, b = 31 - __clz((int)m), o0 = __ffs((int)out) - 1, o1 = 31 - __clz((int)out);
			const int q0 = e(a, o0), q1 = e(a, o1), q2 = e(b, o1), q3 = e(b, o0);
			put(q0, q1, q2);
			put(q0, q2, q3);
		} else {
			const uint32_t lone = n == 1 ? m : (~m & 15u);
			const int a = __ffs((int)lone) - 1;
			uint32_t rest = ~lone & 15u;
			const int r0 = __ffs((int)rest) - 1; rest &= rest - 1u;
			const int r1 = __ffs((int)rest) - 1; rest &= rest - 1u;
			const int r2 = __ffs((int)rest) - 1;
			if (n == 1) put(e(a, r0), e(a, r1), e(a, r2));
			else put(e(a, r2), e(a, r1), e(a, r0));
		}
	}
}

// exclusive prefix of v over the THREADS threads of the workgroup, in thread order; total: the sum.  Every thread calls it.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* s_wave /* [THREADS / WAVE] */, uint32_t& total) {
	const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
	uint32_t incl = v;
#pragma unroll
	for (int off = 1; off < WAVE; off <<= 1) {
		const uint32_t o = __shfl_up(incl, off, WAVE);
		if (lane >= off) incl += o;
	}
	__syncthreads();                                            // a previous use of s_wave is over
	if (lane == WAVE - 1) s_wave[wid] = incl;
	__syncthreads();
	uint32_t before = 0; total = 0;
#pragma unroll
	for (int w = 0; w < THREADS / WAVE; w++) { const uint32_t t = s_wave[w]; if (w < wid) before += t; total += t; }
	return before + incl - v;
}

// ---- extraction, host ----

// the scratch of the extraction: three uint32 per row (a chunk of the dense volume, a block of the sparse one: vertices, faces, has-vertices;
// scanned in place), the 64-bit totals, the scan's own scratch
struct ExtractTemp { uint32_t *cv, *cf, *ce; unsigned long long* totals; char* scan; size_t bytes; };
ExtractTemp carve_extract(char* base, size_t rows) {
	Carver c(base);
	ExtractTemp t;
	t.cv = c.take<uint32_t>(rows); t.cf = c.take<uint32_t>(rows); t.ce = c.take<uint32_t>(rows);
	t.totals = c.take<unsigned long long>(3 * SCAN_AUX_SLOTS);
	t.scan = c.take<char>(scan_temp_bytes(rows));
	t.bytes = c.size();
	return t;
}

// extract_count behind its count kernel, which wrote the three counts of every row: scans them in place, reads the totals back once, refuses a
// mesh beyond INT_MAX and writes `counts`.  -> 0 or -1
int extract_count_tail(const std::string& name, const ExtractTemp& t, size_t rows, hipStream_t stream, long long* counts) {
	ADGS_HIP_CHECK(hipMemsetAsync(t.totals, 0, 3 * SCAN_AUX_SLOTS * sizeof(unsigned long long), stream));
	uint32_t* row[3] = { t.cv, t.cf, t.ce };
	for (int r = 0; r < 3; r++)
		if (exclusive_scan_u32_sum(row[r], row[r], rows, t.scan, row[r], t.totals + r * SCAN_AUX_SLOTS, stream) != 0) return -1;
	unsigned long long sum[3];
	if (read_scan_totals<3, 0>(t.totals, stream, sum, nullptr) != 0) return -1;
	if (sum[0] > (unsigned long long)INT_MAX || sum[1] > (unsigned long long)INT_MAX) {
		set_error(name + ": the mesh has " + std::to_string(sum[0]) + " vertices and " + std::to_string(sum[1]) + " faces; more than INT_MAX of either is refused");
		return -1;
	}
	for (int r = 0; r < 3; r++) counts[r] = (long long)sum[r];
	return 0;
}

// What extract_emit refuses of `counts` and of its outputs.  max_V, max_F, max_E: what the volume can hold at most (beside INT_MAX vertices and
// faces, and an owner row per vertex at most); count_entry: the entry that returned the counts, for the message.  -> 0 or -1
int check_emit(const std::string& name, const char* count_entry, const long long* counts, long long max_V, long long max_F, long long max_E,
	const float* vertices, const int* faces, const void* owners, const float* color, const float* colors) {
	const long long V = counts[0], F = counts[1], E = counts[2];
	if (V < 0 || F < 0 || E < 0 || V > (long long)INT_MAX || F > (long long)INT_MAX || E > max_E || E > V || V > max_V || F > max_F) {
		set_error(name + ": counts are not what " + count_entry + " returned for this volume"); return -1;
	}
	if ((V > 0 && !vertices) || (F > 0 && !faces) || (E > 0 && !owners)) { set_error(name + ": NULL vertices, faces or owners"); return -1; }
	if ((color != nullptr) != (colors != nullptr)) { set_error(name + ": color and colors must be given together"); return -1; }
	return 0;
}

} // namespace
} // namespace adgs
