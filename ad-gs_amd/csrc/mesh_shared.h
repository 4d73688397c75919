// What the three files that read an indexed triangle mesh share: mesh.hip (clean-up), simplify.hip (simplification) and geometry.hip
// (evaluation).  One copy of the face check that stands in front of every dereference, of a face's corners and cross product in double, of
// the search in sorted (key, corner) pairs with its scratch, and of the small host helpers.  The functions are inline, so each is compiled
// with the flags of the file that includes it: mesh.o is built with the default contraction, geometry.o and simplify.o with
// -ffp-contract=off, and the arithmetic of each file is what it was when it carried its own copy.
#pragma once
#include "common.h"
#include <climits>

namespace adgs {
namespace {

constexpr int MESH_THREADS = 256;                               // the workgroup of every kernel of the three files

// true and i[] set when the three indices of face f lie in [0, V): checked before every dereference
__device__ __forceinline__ bool load_face(const int* __restrict__ faces, uint32_t f, uint32_t V, uint32_t i[3]) {
	i[0] = (uint32_t)faces[3 * (size_t)f + 0]; i[1] = (uint32_t)faces[3 * (size_t)f + 1]; i[2] = (uint32_t)faces[3 * (size_t)f + 2];
	return i[0] < V && i[1] < V && i[2] < V;                    // a negative index is >= 2^31 > V as unsigned
}

// row v of a [., 3] float array as doubles; v is in range
__device__ __forceinline__ void load_point(const float* __restrict__ a, uint32_t v, double p[3]) {
#pragma unroll
	for (int d = 0; d < 3; d++) p[d] = (double)a[3 * (size_t)v + d];
}

// the corners of a face whose indices load_face accepted
__device__ __forceinline__ void load_corners(const float* __restrict__ vertices, const uint32_t i[3], double p[3][3]) {
#pragma unroll
	for (int k = 0; k < 3; k++) load_point(vertices, i[k], p[k]);
}

// the edges a = p1 - p0 and b = p2 - p0 of a face with the corners p, and the components of a x b: twice the face's area along its normal.
// One component per call, so that a caller that accumulates them keeps each product beside its sum, where mesh.o's contraction finds it.
struct FaceEdges {
	double ax, ay, az, bx, by, bz;
	__device__ __forceinline__ double cross_x() const { return ay * bz - az * by; }
	__device__ __forceinline__ double cross_y() const { return az * bx - ax * bz; }
	__device__ __forceinline__ double cross_z() const { return ax * by - ay * bx; }
};
__device__ __forceinline__ FaceEdges face_edges(const double p0[3], const double p1[3], const double p2[3]) {
	FaceEdges e;
	e.ax = p1[0] - p0[0]; e.ay = p1[1] - p0[1]; e.az = p1[2] - p0[2];
	e.bx = p2[0] - p0[0]; e.by = p2[1] - p0[1]; e.bz = p2[2] - p0[2];
	return e;
}

// the first position of the ascending keys[0, n) with keys[] >= v (n when there is none): at most 34 steps for n = 3 F.  The entries
// equal to v are the run that starts there.
__device__ __forceinline__ size_t first_at_least(const uint32_t* __restrict__ keys, size_t n, uint32_t v) {
	size_t lo = 0, hi = n;
	while (lo < hi) {
		const size_t mid = lo + (hi - lo) / 2;
		if (keys[mid] < v) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// ---- host ----

unsigned blocks_of(size_t n) { return (unsigned)((n + MESH_THREADS - 1) / MESH_THREADS); }
bool count_ok(long long n) { return n >= 0 && n <= (long long)INT_MAX; }
bool sizes_ok(long long V, long long F) { return count_ok(V) && count_ok(F); }

// the number of key bits a radix sort of the keys 0 .. top needs, at most `limit`
int bits_of(unsigned long long top, int limit = 32) {
	int bits = 1;
	while (bits < limit && (top >> bits) != 0) bits++;
	return bits;
}

// the scratch of a stable sort of the 3 F (key, corner id) pairs of a mesh: the ping-pong buffers and the sort's own scratch
struct CornerPairTemp { uint32_t *k0, *k1, *v0, *v1; char* sort; size_t bytes; };
CornerPairTemp carve_corner_pairs(char* base, size_t F) {
	Carver c(base);
	CornerPairTemp t;
	const size_t n = 3 * F;
	t.k0 = c.take<uint32_t>(n); t.k1 = c.take<uint32_t>(n); t.v0 = c.take<uint32_t>(n); t.v1 = c.take<uint32_t>(n);
	t.sort = c.take<char>(sort_temp_bytes(n));
	t.bytes = c.size();
	return t;
}

} // namespace
} // namespace adgs
