// The triangle-mesh z-buffer for gfx950 (wave64): nearest face and camera depth per pixel, normals, attribute interpolation and per-face
// visibility counts.  The definition is in include/adgs_zbuffer.h; this file is built with -ffp-contract=off (csrc/Makefile), so every
// double operation below rounds once, as the definition states it.
//
//   draw         fill (keys = all ones, counters = 0) -> setup (one lane per face; the wave expands its small faces) -> big (fixed grid over
//                the list of big faces, 8 x 8 tiles) -> resolve (one thread per pixel: face, depth, normal)
//   interpolate  one thread per pixel: the winner's setup again, by the same device functions
//   count_faces  pixel counts per face into scratch (one atomic per run of equal faces of a wave), then one thread per face folds
// A face is set up by face_setup() wherever it is needed, and its edge functions come from edge_setup() / edge_at(): one copy of the
// arithmetic the bit-equality rests on.  Every kernel that reads `faces` checks the three indices first (load_face, mesh_shared.h).
#include "common.h"
#include "mesh_shared.h"
#include "../../include/adgs_zbuffer.h"

namespace adgs {
namespace {

constexpr unsigned long long NO_KEY = ~0ull;
constexpr int HUGE_TILES = 256;            // a big face with more 8 x 8 tiles than this is shared by all workgroups of the big launch
constexpr int BIG_GROUPS = 1024;           // the fixed grid of the big launch: 4 workgroups per CU
constexpr int COUNT_ITERS = 16;            // groups of 64 pixels a wave of count_faces walks

enum FaceStatus { FACE_OK = 0, FACE_BAD_INDEX = 1, FACE_NEAR = 2, FACE_GUARD = 3, FACE_DEGENERATE = 4, FACE_CULLED = 5, FACE_NONE = 6 };

// the view as the kernels take it (by value)
struct ZView {
	int H, W, cull, small_max;
	double tanx, tany, near;
	float max_depth;
	double R[9], t[3];
};

struct ZFace {
	int U[3], V[3];                        // the snapped corners
	double q[3];                           // 1 / z
	long long A;                           // twice the signed area on the lattice
};

// the pixel centres in the bounding box of a face, clipped to the image: x0 .. x0 + bw - 1, y0 .. y0 + bh - 1 (bw or bh <= 0: none)
struct ZBox { int x0, y0, bw, bh; };

// the edge functions of a face at the origin of its box and their steps: E_k(x0 + i, y0 + j) = e[k] + 256 (dx[k] j - dy[k] i)
struct ZEdges { long long e[3]; int dx[3], dy[3]; };

__device__ __forceinline__ void to_camera(const ZView& vw, const double p[3], double c[3]) {
#pragma unroll
	for (int r = 0; r < 3; r++) c[r] = ((vw.R[3 * r + 0] * p[0] + vw.R[3 * r + 1] * p[1]) + vw.R[3 * r + 2] * p[2]) + vw.t[r];
}

// steps 1 to 7 of the definition
__device__ __forceinline__ int face_setup(const ZView& vw, const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t f, uint32_t V,
	ZFace& o) {
	uint32_t i[3];
	if (!load_face(faces, f, V, i)) return FACE_BAD_INDEX;
	double p[3][3], c[3][3];
	load_corners(vertices, i, p);
	bool near_ok = true;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		to_camera(vw, p[k], c[k]);
		near_ok = near_ok && isfinite(c[k][0]) && isfinite(c[k][1]) && isfinite(c[k][2]) && c[k][2] >= vw.near;
	}
	if (!near_ok) return FACE_NEAR;
	bool guard_ok = true;
	double u[3], v[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		u[k] = (c[k][0] / c[k][2]) / vw.tanx * ((double)vw.W * 0.5) + (double)(vw.W - 1) * 0.5;
		v[k] = (c[k][1] / c[k][2]) / vw.tany * ((double)vw.H * 0.5) + (double)(vw.H - 1) * 0.5;
		guard_ok = guard_ok && fabs(u[k]) <= (double)ADGS_ZBUFFER_GUARD && fabs(v[k]) <= (double)ADGS_ZBUFFER_GUARD;   // NaN fails
	}
	if (!guard_ok) return FACE_GUARD;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		o.U[k] = (int)rint((double)ADGS_ZBUFFER_SUBPIXEL * u[k]);
		o.V[k] = (int)rint((double)ADGS_ZBUFFER_SUBPIXEL * v[k]);
		o.q[k] = 1.0 / c[k][2];
	}
	o.A = (long long)(o.U[1] - o.U[0]) * (long long)(o.V[2] - o.V[0]) - (long long)(o.V[1] - o.V[0]) * (long long)(o.U[2] - o.U[0]);
	if (o.A == 0) return FACE_DEGENERATE;
	if (vw.cull && o.A > 0) return FACE_CULLED;
	return FACE_OK;
}

// floor(a / 256) for a of either sign is a >> 8; ceil(a / 256) = (a + 255) >> 8
__device__ __forceinline__ ZBox face_box(const ZView& vw, const ZFace& fc) {
	const int ulo = min(fc.U[0], min(fc.U[1], fc.U[2])), uhi = max(fc.U[0], max(fc.U[1], fc.U[2]));
	const int vlo = min(fc.V[0], min(fc.V[1], fc.V[2])), vhi = max(fc.V[0], max(fc.V[1], fc.V[2]));
	ZBox b;
	b.x0 = max((ulo + 255) >> 8, 0); b.y0 = max((vlo + 255) >> 8, 0);
	b.bw = min(uhi >> 8, vw.W - 1) - b.x0 + 1; b.bh = min(vhi >> 8, vw.H - 1) - b.y0 + 1;
	return b;
}

// the edges (a, b) = (1, 2), (2, 0), (0, 1), oriented by the sign of A, at the pixel (x0, y0); every factor fits in int32
__device__ __forceinline__ ZEdges edge_setup(const ZFace& fc, int x0, int y0) {
	ZEdges g;
	const int s = fc.A > 0 ? 1 : -1;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const int a = (k + 1) % 3, b = (k + 2) % 3;
		g.dx[k] = s * (fc.U[b] - fc.U[a]); g.dy[k] = s * (fc.V[b] - fc.V[a]);
		g.e[k] = (long long)g.dx[k] * (long long)(ADGS_ZBUFFER_SUBPIXEL * y0 - fc.V[a]) - (long long)g.dy[k] * (long long)(ADGS_ZBUFFER_SUBPIXEL * x0 - fc.U[a]);
	}
	return g;
}

// E at (x0 + i, y0 + j) from E at (x0, y0): two 32 x 32 -> 64 multiply-adds, no 64-bit product
__device__ __forceinline__ long long edge_at(long long e, int dx, int dy, int i, int j) {
	return e + (long long)ADGS_ZBUFFER_SUBPIXEL * ((long long)dx * (long long)j - (long long)dy * (long long)i);
}

// the smallest E that still covers: 0 on an edge that takes the centres on it (d.y > 0, or d.y = 0 and d.x > 0: a top or right edge), 1 elsewhere
__device__ __forceinline__ long long edge_threshold(int dx, int dy) { return (dy > 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

__device__ __forceinline__ double depth_sum(long long e0, long long e1, long long e2, double q0, double q1, double q2) {
	return ((double)e0 * q0 + (double)e1 * q1) + (double)e2 * q2;
}

// one covered sample: its key against the pixel's
__device__ __forceinline__ void put_sample(unsigned long long* __restrict__ keys, size_t pixel, long long e0, long long e1, long long e2, double q0, double q1,
	double q2, float max_depth, uint32_t f) {
	const float depth = (float)((double)(e0 + e1 + e2) / depth_sum(e0, e1, e2, q0, q1, q2));      // E0 + E1 + E2 = |A|
	if (!(depth <= max_depth)) return;
	const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)f;
	if (key < __hip_atomic_load(keys + pixel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
		__hip_atomic_fetch_min(keys + pixel, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- fill ----

// keys = NO_KEY; the five counters and the list's counters = 0
__global__ void __launch_bounds__(MESH_THREADS) zbuffer_fill_kernel(unsigned long long* __restrict__ keys, size_t n, unsigned long long* __restrict__ counts,
	uint32_t* __restrict__ lc) {
	const size_t p = (size_t)blockIdx.x * MESH_THREADS + threadIdx.x;
	if (p < n) keys[p] = NO_KEY;
	if (blockIdx.x == 0) {
		if (threadIdx.x < 5) counts[threadIdx.x] = 0ull;
		if (threadIdx.x < 4) lc[threadIdx.x] = 0u;
	}
}

// ---- setup and the small faces ----

// what a (face, pixel) pair needs from its face, in LDS: 88 bytes per lane
struct SmallFace { long long e[3]; double q[3]; int dx[3], dy[3]; int x0, y0, bw; uint32_t f; };

// lc[0]: the number of big faces, list[0 ..) from the front; lc[1]: the number of huge ones, list[F - 1 ..] from the back; lc[2]: the ticket
__global__ void __launch_bounds__(MESH_THREADS) zbuffer_setup_kernel(ZView vw, const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V,
	uint32_t F, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts, int* __restrict__ list, uint32_t* __restrict__ lc) {
	__shared__ SmallFace sf[MESH_THREADS];
	__shared__ uint32_t incl[MESH_THREADS];
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	const int lane = threadIdx.x & (WAVE - 1), wave0 = threadIdx.x & ~(WAVE - 1);
	ZFace fc;
	ZBox box = {0, 0, 0, 0};
	const int status = f < F ? face_setup(vw, vertices, faces, f, V, fc) : FACE_NONE;
	uint32_t n = 0;
	if (status == FACE_OK) {
		box = face_box(vw, fc);
		if (box.bw > 0 && box.bh > 0) n = (uint32_t)box.bw * (uint32_t)box.bh;        // <= H W < 2^31
	}
	// the five counters: one atomic per wave and counter that has something
#pragma unroll
	for (int k = FACE_BAD_INDEX; k <= FACE_CULLED; k++) {
		const unsigned long long m = __ballot(status == k);
		if (m && lane == 0) atomicAdd(counts + (k - 1), (unsigned long long)__popcll(m));
	}
	// big and huge faces: one atomic per wave and list
	const bool big = n > (uint32_t)vw.small_max;
	const bool huge_face = big && (size_t)((box.bw + 7) >> 3) * (size_t)((box.bh + 7) >> 3) > (size_t)HUGE_TILES;
	{
		const unsigned long long mb = __ballot(big && !huge_face), mh = __ballot(huge_face);
		const unsigned long long below = (1ull << lane) - 1ull;
		if (mb) {
			uint32_t base = 0;
			if (lane == 0) base = atomicAdd(lc + 0, (uint32_t)__popcll(mb));
			base = (uint32_t)__shfl((int)base, 0, WAVE);
			if (big && !huge_face) list[base + (uint32_t)__popcll(mb & below)] = (int)f;
		}
		if (mh) {
			uint32_t base = 0;
			if (lane == 0) base = atomicAdd(lc + 1, (uint32_t)__popcll(mh));
			base = (uint32_t)__shfl((int)base, 0, WAVE);
			if (huge_face) list[F - 1u - (base + (uint32_t)__popcll(mh & below))] = (int)f;      // big + huge <= F: the two ends never meet
		}
	}
	// small faces: the wave's prefix sum of n, then 64 (face, pixel) pairs at a time
	const bool small = n > 0 && !big;
	uint32_t sum = small ? n : 0u;
#pragma unroll
	for (int off = 1; off < WAVE; off <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)sum, off, WAVE);
		if (lane >= off) sum += up;
	}
	incl[threadIdx.x] = sum;
	if (small) {
		const ZEdges g = edge_setup(fc, box.x0, box.y0);
		SmallFace& s = sf[threadIdx.x];
#pragma unroll
		for (int k = 0; k < 3; k++) { s.e[k] = g.e[k]; s.q[k] = fc.q[k]; s.dx[k] = g.dx[k]; s.dy[k] = g.dy[k]; }
		s.x0 = box.x0; s.y0 = box.y0; s.bw = box.bw; s.f = f;
	}
	__syncthreads();                                            // every thread of the workgroup arrives: nothing above returns
	const uint32_t total = incl[wave0 + WAVE - 1];              // <= 64 small_max
	for (uint32_t base = 0; base < total; base += WAVE) {
		const uint32_t idx = base + (uint32_t)lane;
		if (idx >= total) continue;
		int lo = 0, hi = WAVE - 1;                              // the first lane whose inclusive sum exceeds idx
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			if (incl[wave0 + mid] > idx) hi = mid; else lo = mid + 1;
		}
		const SmallFace& s = sf[wave0 + lo];
		const uint32_t k = idx - (lo > 0 ? incl[wave0 + lo - 1] : 0u);
		const int j = (int)(k / (uint32_t)s.bw), i = (int)(k - (uint32_t)j * (uint32_t)s.bw);
		const long long e0 = edge_at(s.e[0], s.dx[0], s.dy[0], i, j), e1 = edge_at(s.e[1], s.dx[1], s.dy[1], i, j),
			e2 = edge_at(s.e[2], s.dx[2], s.dy[2], i, j);
		if (e0 < edge_threshold(s.dx[0], s.dy[0]) || e1 < edge_threshold(s.dx[1], s.dy[1]) || e2 < edge_threshold(s.dx[2], s.dy[2])) continue;
		put_sample(keys, (size_t)(s.y0 + j) * (size_t)vw.W + (size_t)(s.x0 + i), e0, e1, e2, s.q[0], s.q[1], s.q[2], vw.max_depth, s.f);
	}
}

// ---- the big faces ----

// the tiles first, first + stride, ... of face f, one 8 x 8 tile per wave at a time.  Everything up to the lane's own pixel is wave-uniform.
__device__ __forceinline__ void draw_tiles(const ZView& vw, const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V, uint32_t F, uint32_t f,
	unsigned long long* __restrict__ keys, size_t first, size_t stride) {
	ZFace fc;
	if (f >= F || face_setup(vw, vertices, faces, f, V, fc) != FACE_OK) return;      // not what the setup launch listed: cannot happen
	const ZBox box = face_box(vw, fc);
	if (box.bw <= 0 || box.bh <= 0) return;
	const ZEdges g = edge_setup(fc, box.x0, box.y0);
	long long thr[3], reach[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		thr[k] = edge_threshold(g.dx[k], g.dy[k]);
		// the most E_k grows from a tile's origin to any of its 64 pixels
		reach[k] = (long long)ADGS_ZBUFFER_SUBPIXEL * 7 * ((long long)max(g.dx[k], 0) + (long long)max(-g.dy[k], 0));
	}
	const size_t tw = (size_t)((box.bw + 7) >> 3), tiles = tw * (size_t)((box.bh + 7) >> 3);
	const int lane = threadIdx.x & (WAVE - 1), lx = lane & 7, ly = lane >> 3;
	for (size_t t = first; t < tiles; t += stride) {
		const int ty = (int)(t / tw), tx = (int)(t - (size_t)ty * tw);
		const long long o0 = edge_at(g.e[0], g.dx[0], g.dy[0], 8 * tx, 8 * ty), o1 = edge_at(g.e[1], g.dx[1], g.dy[1], 8 * tx, 8 * ty),
			o2 = edge_at(g.e[2], g.dx[2], g.dy[2], 8 * tx, 8 * ty);
		if (o0 + reach[0] < thr[0] || o1 + reach[1] < thr[1] || o2 + reach[2] < thr[2]) continue;      // an edge has the whole tile outside
		const int i = 8 * tx + lx, j = 8 * ty + ly;
		if (i >= box.bw || j >= box.bh) continue;
		const long long e0 = edge_at(g.e[0], g.dx[0], g.dy[0], i, j), e1 = edge_at(g.e[1], g.dx[1], g.dy[1], i, j),
			e2 = edge_at(g.e[2], g.dx[2], g.dy[2], i, j);
		if (e0 < thr[0] || e1 < thr[1] || e2 < thr[2]) continue;
		put_sample(keys, (size_t)(box.y0 + j) * (size_t)vw.W + (size_t)(box.x0 + i), e0, e1, e2, fc.q[0], fc.q[1], fc.q[2], vw.max_depth, f);
	}
}

// A fixed grid: a workgroup takes big faces by ticket and puts its waves on their tiles; the huge faces are walked by every workgroup, which
// strides over their tiles with the whole grid.  Nothing waits for another workgroup; with both lists empty it ends at once.
__global__ void __launch_bounds__(MESH_THREADS) zbuffer_big_kernel(ZView vw, const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V,
	uint32_t F, unsigned long long* __restrict__ keys, const int* __restrict__ list, uint32_t* __restrict__ lc) {
	__shared__ uint32_t ticket;
	const uint32_t nbig = min(lc[0], F), nhuge = min(lc[1], F);
	if (nbig == 0 && nhuge == 0) return;
	const size_t waves = MESH_THREADS / WAVE, wave = threadIdx.x / WAVE;
	if (nbig > 0) {
		for (;;) {                                              // at most nbig + 1 rounds: every round takes a ticket
			if (threadIdx.x == 0) ticket = atomicAdd(lc + 2, 1u);
			__syncthreads();
			const uint32_t t = ticket;
			__syncthreads();
			if (t >= nbig) break;                               // workgroup-uniform
			draw_tiles(vw, vertices, faces, V, F, (uint32_t)list[t], keys, wave, waves);
		}
	}
	for (uint32_t h = 0; h < nhuge; h++)
		draw_tiles(vw, vertices, faces, V, F, (uint32_t)list[F - 1u - h], keys, (size_t)blockIdx.x * waves + wave, (size_t)gridDim.x * waves);
}

// ---- resolve ----

__global__ void __launch_bounds__(MESH_THREADS) zbuffer_resolve_kernel(ZView vw, const unsigned long long* __restrict__ keys, size_t n,
	const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V, uint32_t F, int* __restrict__ face, float* __restrict__ depth,
	float* __restrict__ normal) {
	const size_t p = (size_t)blockIdx.x * MESH_THREADS + threadIdx.x;
	if (p >= n) return;
	const unsigned long long key = keys[p];
	const bool won = key != NO_KEY;
	const uint32_t f = (uint32_t)(key & 0xFFFFFFFFull);
	face[p] = won ? (int)f : -1;
	depth[p] = won ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
	if (!normal) return;
	double nx = 0.0, ny = 0.0, nz = 0.0;
	uint32_t i[3];
	if (won && f < F && load_face(faces, f, V, i)) {
		double q[3][3], c0[3], w[3], m[3];
		load_corners(vertices, i, q);
		const FaceEdges e = face_edges(q[0], q[1], q[2]);
		w[0] = e.cross_x(); w[1] = e.cross_y(); w[2] = e.cross_z();
#pragma unroll
		for (int r = 0; r < 3; r++) m[r] = (vw.R[3 * r + 0] * w[0] + vw.R[3 * r + 1] * w[1]) + vw.R[3 * r + 2] * w[2];
		to_camera(vw, q[0], c0);
		const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
		if (len > 0.0 && isfinite(len)) {
			const double s = ((m[0] * c0[0] + m[1] * c0[1]) + m[2] * c0[2]) > 0.0 ? -1.0 : 1.0;
			nx = s * m[0] / len; ny = s * m[1] / len; nz = s * m[2] / len;
		}
	}
	normal[p] = (float)nx; normal[n + p] = (float)ny; normal[2 * n + p] = (float)nz;
}

// ---- interpolate ----

__global__ void __launch_bounds__(MESH_THREADS) zbuffer_interpolate_kernel(ZView vw, const float* __restrict__ vertices, const int* __restrict__ faces, uint32_t V,
	uint32_t F, const int* __restrict__ face_map, size_t n, int C, const float* __restrict__ attributes, float background, float* __restrict__ out) {
	const size_t p = (size_t)blockIdx.x * MESH_THREADS + threadIdx.x;
	if (p >= n) return;
	const uint32_t f = (uint32_t)face_map[p];                   // -1 is >= F as unsigned
	ZFace fc;
	bool ok = f < F && face_setup(vw, vertices, faces, f, V, fc) == FACE_OK;
	double w0 = 0.0, w1 = 0.0, w2 = 0.0, S = 1.0;
	uint32_t i[3] = {0, 0, 0};
	const int py = (int)(p / (size_t)vw.W), px = (int)(p - (size_t)py * (size_t)vw.W);
	ok = ok && px <= ADGS_ZBUFFER_GUARD && py <= ADGS_ZBUFFER_GUARD;      // a drawn face's box ends there: further out the face did not win
	if (ok) {
		const ZEdges g = edge_setup(fc, px, py);
		ok = g.e[0] >= 0 && g.e[1] >= 0 && g.e[2] >= 0;
		if (ok) {
			S = depth_sum(g.e[0], g.e[1], g.e[2], fc.q[0], fc.q[1], fc.q[2]);
			w0 = (double)g.e[0] * fc.q[0]; w1 = (double)g.e[1] * fc.q[1]; w2 = (double)g.e[2] * fc.q[2];
			load_face(faces, f, V, i);                          // in range: face_setup accepted it
		}
	}
	for (int c = 0; c < C; c++) {
		float a = background;
		if (ok) {
			const double a0 = (double)attributes[(size_t)i[0] * (size_t)C + c], a1 = (double)attributes[(size_t)i[1] * (size_t)C + c],
				a2 = (double)attributes[(size_t)i[2] * (size_t)C + c];
			a = (float)(((w0 * a0 + w1 * a1) + w2 * a2) / S);
		}
		out[(size_t)c * n + p] = a;
	}
}

// ---- count_faces ----

// A wave walks COUNT_ITERS consecutive groups of 64 pixels and keeps a run (face, count).  Per group it takes the distinct faces of its lanes
// one at a time (the first remaining lane's, one ballot each): the run's face joins the run, any other is ONE atomic.  The run is flushed
// when a group no longer holds its face, and at the end: a face that fills the screen costs one atomic per 1024 pixels.
__global__ void __launch_bounds__(MESH_THREADS) zbuffer_count_pixels_kernel(const int* __restrict__ face_map, size_t n, uint32_t F, int* __restrict__ scratch) {
	const int lane = threadIdx.x & (WAVE - 1);
	const size_t base = ((size_t)blockIdx.x * (MESH_THREADS / WAVE) + threadIdx.x / WAVE) * (size_t)(WAVE * COUNT_ITERS) + lane;
	uint32_t run = 0xFFFFFFFFu; int run_n = 0;
	for (int it = 0; it < COUNT_ITERS; it++) {
		const size_t p = base + (size_t)it * WAVE;
		const uint32_t f = p < n ? (uint32_t)face_map[p] : 0xFFFFFFFFu;
		const bool has = f < F;
		unsigned long long rest = __ballot(has);
		if (rest == 0) continue;                                // wave-uniform
		if (__ballot(has && f == run) == 0) {
			if (run_n > 0 && lane == 0) atomicAdd(scratch + run, run_n);
			run = (uint32_t)__shfl((int)f, __ffsll((long long)rest) - 1, WAVE); run_n = 0;
		}
		while (rest) {                                          // one round per distinct face of the group: at most 64
			const uint32_t pick = (uint32_t)__shfl((int)f, __ffsll((long long)rest) - 1, WAVE);
			const unsigned long long same = __ballot(has && f == pick);
			if (pick == run) run_n += (int)__popcll(same);
			else if (lane == 0) atomicAdd(scratch + pick, (int)__popcll(same));
			rest &= ~same;
		}
	}
	if (run_n > 0 && lane == 0) atomicAdd(scratch + run, run_n);
}

__global__ void __launch_bounds__(MESH_THREADS) zbuffer_count_fold_kernel(uint32_t F, int* __restrict__ scratch, int* __restrict__ views,
	long long* __restrict__ pixels) {
	const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
	if (f >= F) return;
	const int c = scratch[f];
	if (c > 0) { views[f] += 1; pixels[f] += (long long)c; scratch[f] = 0; }
}

// ---- host ----

// the keys, the list of big faces (big from the front, huge from the back), its counters
struct DrawTemp { unsigned long long* keys; int* list; uint32_t* lc; size_t bytes; };
DrawTemp carve_draw(char* base, size_t pixels, size_t F) {
	Carver c(base);
	DrawTemp t;
	t.keys = c.take<unsigned long long>(pixels); t.list = c.take<int>(F); t.lc = c.take<uint32_t>(4);
	t.bytes = c.size();
	return t;
}

bool pixels_ok(long long H, long long W) { return count_ok(H) && count_ok(W) && (H == 0 || W <= (long long)INT_MAX / H); }

// the checks of a view that draw and interpolate share; "" when it is fine
std::string view_error(const adgs_zbuffer_view* view) {
	if (!view) return "NULL view";
	if (view->struct_bytes < (int)sizeof(adgs_zbuffer_view)) return "view.struct_bytes is smaller than adgs_zbuffer_view";
	if (view->H < 0 || view->W < 0) return "negative H or W";
	if (!pixels_ok(view->H, view->W)) return "H W must be below 2^31";
	if (!positive(view->tanfovx) || !positive(view->tanfovy)) return "tanfovx and tanfovy must be finite and > 0";
	if (!positive(view->near)) return "near must be finite and > 0";
	if (!(view->max_depth > 0.f)) return "max_depth must be > 0";
	for (int k = 0; k < 12; k++) if (!std::isfinite(view->pose[k])) return "pose must be finite";
	if (view->cull != 0 && view->cull != 1) return "cull must be 0 or 1";
	if (view->small_max < 0 || view->small_max > 4096) return "small_max must lie in [0, 4096]";
	if (view->stages < 0 || view->stages > 15) return "stages must lie in [0, 15]";
	return "";
}

ZView make_view(const adgs_zbuffer_view* view) {
	ZView v;
	v.H = view->H; v.W = view->W; v.cull = view->cull; v.small_max = view->small_max ? view->small_max : ADGS_ZBUFFER_SMALL_MAX;
	v.tanx = view->tanfovx; v.tany = view->tanfovy; v.near = view->near; v.max_depth = view->max_depth;
	for (int k = 0; k < 9; k++) v.R[k] = view->pose[k];
	for (int k = 0; k < 3; k++) v.t[k] = view->pose[9 + k];
	return v;
}

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" size_t adgs_zbuffer_temp_bytes(long long H, long long W, long long F) {
	return pixels_ok(H, W) && count_ok(F) ? carve_draw(nullptr, (size_t)(H * W), (size_t)F).bytes : 0;
}

extern "C" int adgs_zbuffer_draw(const adgs_zbuffer_view* view, int V, int F, const float* vertices, const int* faces, void* temp, int* face, float* depth,
	float* normal, long long* counts, void* stream_) {
	const std::string name("adgs_zbuffer_draw");
	const std::string bad = view_error(view);
	if (!bad.empty()) { set_error(name + ": " + bad); return -1; }
	if (V < 0 || F < 0) { set_error(name + ": negative V or F"); return -1; }
	if ((F > 0 && !faces) || (F > 0 && V > 0 && !vertices) || !temp || !face || !depth || !counts) { set_error(name + ": NULL pointer"); return -1; }
	const size_t n = (size_t)view->H * (size_t)view->W;
	if (n == 0) return 0;
	hipStream_t stream = (hipStream_t)stream_;
	const ZView vw = make_view(view);
	const int stages = view->stages ? view->stages : 15;
	const DrawTemp t = carve_draw((char*)temp, n, (size_t)F);
	unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
	if (stages & 1) ADGS_LAUNCH(zbuffer_fill_kernel, dim3(blocks_of(n)), dim3(MESH_THREADS), 0, stream, t.keys, n, cnt, t.lc);
	if (F > 0 && (stages & 2)) ADGS_LAUNCH(zbuffer_setup_kernel, dim3(blocks_of((size_t)F)), dim3(MESH_THREADS), 0, stream, vw, vertices, faces, (uint32_t)V,
		(uint32_t)F, t.keys, cnt, t.list, t.lc);
	if (F > 0 && (stages & 4)) ADGS_LAUNCH(zbuffer_big_kernel, dim3(BIG_GROUPS), dim3(MESH_THREADS), 0, stream, vw, vertices, faces, (uint32_t)V, (uint32_t)F,
		t.keys, (const int*)t.list, t.lc);
	if (stages & 8) ADGS_LAUNCH(zbuffer_resolve_kernel, dim3(blocks_of(n)), dim3(MESH_THREADS), 0, stream, vw, (const unsigned long long*)t.keys, n, vertices,
		faces, (uint32_t)V, (uint32_t)F, face, depth, normal);
	return 0;
}

extern "C" int adgs_zbuffer_interpolate(const adgs_zbuffer_view* view, int V, int F, const float* vertices, const int* faces, const int* face_map, int C,
	const float* attributes, float background, float* out, void* stream_) {
	const std::string name("adgs_zbuffer_interpolate");
	const std::string bad = view_error(view);
	if (!bad.empty()) { set_error(name + ": " + bad); return -1; }
	if (V < 0 || F < 0 || C < 0) { set_error(name + ": negative V, F or C"); return -1; }
	if (C > 0 && (!face_map || !out || (F > 0 && !faces) || (F > 0 && V > 0 && (!vertices || !attributes)))) { set_error(name + ": NULL pointer"); return -1; }
	const size_t n = (size_t)view->H * (size_t)view->W;
	if (n == 0 || C == 0) return 0;
	ADGS_LAUNCH(zbuffer_interpolate_kernel, dim3(blocks_of(n)), dim3(MESH_THREADS), 0, (hipStream_t)stream_, make_view(view), vertices, faces, (uint32_t)V,
		(uint32_t)F, face_map, n, C, attributes, background, out);
	return 0;
}

extern "C" int adgs_zbuffer_count_faces(int H, int W, int F, const int* face_map, int* scratch, int* views, long long* pixels, void* stream_) {
	const std::string name("adgs_zbuffer_count_faces");
	if (H < 0 || W < 0 || F < 0) { set_error(name + ": negative H, W or F"); return -1; }
	if (!pixels_ok(H, W)) { set_error(name + ": H W must be below 2^31"); return -1; }
	const size_t n = (size_t)H * (size_t)W;
	if (n == 0 || F == 0) return 0;
	if (!face_map || !scratch || !views || !pixels) { set_error(name + ": NULL pointer"); return -1; }
	hipStream_t stream = (hipStream_t)stream_;
	const size_t per_group = (size_t)MESH_THREADS * COUNT_ITERS;
	ADGS_LAUNCH(zbuffer_count_pixels_kernel, dim3((unsigned)((n + per_group - 1) / per_group)), dim3(MESH_THREADS), 0, stream, face_map, n, (uint32_t)F, scratch);
	ADGS_LAUNCH(zbuffer_count_fold_kernel, dim3(blocks_of((size_t)F)), dim3(MESH_THREADS), 0, stream, (uint32_t)F, scratch, views, pixels);
	return 0;
}
