// TSDF fusion of rendered depth maps and marching tetrahedra on the fused volume, for gfx950 (wave64).
// The definition is in include/adgs_tsdf.h.
//
// Integration: one thread per lattice point over the linear index, 256 per workgroup, so a wave touches 64 consecutive floats (256
// contiguous bytes) of tsdf, wsum and each colour plane.  The position comes from (i, j, k) directly and the chain is double: the nearest
// pixel is a floor() of a projected coordinate and the update is a gate on z_d - z, so a float32 chain would decide differently from the
// definition at pixel boundaries and at the truncation band far more often than the handful of exact ties.  A point that fails a gate
// returns before it reads the volume: the traffic of a view is 8 (+ 12 with colour) bytes read and as many written per UPDATED point,
// plus the image pixels it gathers (neighbouring lattice points share them).
//
// Extraction: classify, scan, emit over chunks of 256 consecutive lattice points (one workgroup each), which gives the canonical order of
// the header for free.  A lattice point owns its 7 forward edges (the vertices) and the cell it is the lowest corner of (the faces).
//   count        per chunk: vertices, faces, "has a vertex"                            -> three uint32 per chunk
//   scan         exclusive_scan_u32_sum over each of the three; the totals travel as 64-bit sums and are read back once
//   emit points  recomputes the chunk; writes its vertices and, for chunks with vertices only, one word per owner:
//                (offset of the owner's first vertex within the chunk) << 8 | its 7 slot bits
//   emit faces   recomputes the chunk's cells; the id of a vertex on an edge is its owner's chunk base + the owner's offset + the
//                popcount of the lower slot bits
// A point whose 8 forward corners all have one sign owns no vertex and no face and costs 8 loads; otherwise the 27 wsum values around it
// decide which of the 7 cells that contain its edges are valid.
#include "common.h"
#include "tsdf_shared.h"
#include "../../include/adgs_tsdf.h"
#include <climits>
#include <cmath>

namespace adgs {
namespace {

constexpr int TSDF_THREADS = ADGS_TSDF_CHUNK;
static_assert(TSDF_THREADS == 256 && ADGS_TSDF_OWNER_BYTES_PER_CHUNK == TSDF_THREADS * sizeof(uint32_t), "one word per owner of a chunk");

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_integrate_kernel(Lattice L, TsdfView v, const float* __restrict__ depth, const float* __restrict__ opacity,
	const float* __restrict__ image, const float* __restrict__ weight, float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ color) {
	const unsigned idx = blockIdx.x * (unsigned)TSDF_THREADS + threadIdx.x;
	if (idx >= L.n) return;
	const unsigned row = idx / (unsigned)L.nx;
	const int i = (int)(idx - row * (unsigned)L.nx), k = (int)(row / (unsigned)L.ny), j = (int)(row - (unsigned)k * (unsigned)L.ny);
	tsdf_update_point(L, v, i, j, k, depth, opacity, image, weight, tsdf + idx, wsum + idx, color ? color + idx : nullptr, (size_t)L.n);
}

// ---- extraction ----

// the tables, classify, cell_faces and cell_emit_faces: tsdf_shared.h.  The orientation table is restated here, where tests/test_tsdf_ref.py pins it
// against the geometric rule; the two copies cannot drift apart.
namespace pinned { constexpr uint32_t REV_EVEN = 0x25A4, REV_ODD = 0x5A5A; }
static_assert(pinned::REV_EVEN == REV_EVEN && pinned::REV_ODD == REV_ODD, "tsdf_shared.h carries another orientation table");

__device__ __forceinline__ void split_index(const Lattice& L, unsigned idx, int& i, int& j, int& k) {
	const unsigned row = idx / (unsigned)L.nx;
	i = (int)(idx - row * (unsigned)L.nx); k = (int)(row / (unsigned)L.ny); j = (int)(row - (unsigned)k * (unsigned)L.ny);
}

// EMIT false: the three counts of the chunk.  EMIT true: the chunk's vertices and, when it has any, its owner words.
template <bool EMIT>
__global__ void __launch_bounds__(TSDF_THREADS) tsdf_points_kernel(Lattice L, const float* __restrict__ tsdf, const float* __restrict__ wsum,
	const float* __restrict__ color, float min_weight, uint32_t* __restrict__ cv, uint32_t* __restrict__ cf, uint32_t* __restrict__ ce,
	uint32_t* __restrict__ owners, unsigned n_owner_chunks, size_t n_vertices, float* __restrict__ vertices, float* __restrict__ colors) {
	__shared__ uint32_t s_wave[TSDF_THREADS / WAVE];
	const unsigned chunk = blockIdx.x, idx = chunk * (unsigned)TSDF_THREADS + threadIdx.x;
	PointClass pc; pc.in8 = 0; pc.vmask = 0; pc.cell = false;
	int i = 0, j = 0, k = 0;
	if (idx < L.n) { split_index(L, idx, i, j, k); pc = classify(L, tsdf, wsum, min_weight, idx, i, j, k); }
	uint32_t nv_chunk, nf_chunk;
	const uint32_t local = block_exclusive<TSDF_THREADS>((uint32_t)__popc(pc.vmask), s_wave, nv_chunk);
	if (!EMIT) {
		block_exclusive<TSDF_THREADS>(pc.cell ? cell_faces(pc.in8) : 0u, s_wave, nf_chunk);
		if (threadIdx.x == 0) { cv[chunk] = nv_chunk; cf[chunk] = nf_chunk; ce[chunk] = nv_chunk ? 1u : 0u; }
		return;
	}
	if (nv_chunk == 0) return;                                  // workgroup-uniform
	// cv, ce: scanned.  ce[chunk] < n_owner_chunks for a chunk with vertices
	owners[(size_t)min(ce[chunk], n_owner_chunks - 1u) * TSDF_THREADS + threadIdx.x] = (local << 8) | pc.vmask;
	if (!pc.vmask) return;
	const size_t sy = (size_t)L.nx, sz = (size_t)L.nx * L.ny;
	const double Tp = (double)tsdf[idx];
	size_t id = (size_t)cv[chunk] + local;
#pragma unroll
	for (int s = 0; s < 7; s++) {
		if (!((pc.vmask >> s) & 1u) || id >= n_vertices) continue;      // id < n_vertices for the volume that was counted
		const int ob = BITS_OF_SLOT[s], dx = ob & 1, dy = (ob >> 1) & 1, dz = ob >> 2;
		const size_t q = idx + dx + dy * sy + dz * sz;          // inside the lattice: the slot is active
		const double Tq = (double)tsdf[q], t = Tp / (Tp - Tq);  // the signs differ: Tp != Tq
		vertices[3 * id + 0] = (float)(L.o[0] + L.vs * ((double)i + t * (double)dx));
		vertices[3 * id + 1] = (float)(L.o[1] + L.vs * ((double)j + t * (double)dy));
		vertices[3 * id + 2] = (float)(L.o[2] + L.vs * ((double)k + t * (double)dz));
		if (colors) {
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const double Cp = (double)color[(size_t)c * L.n + idx], Cq = (double)color[(size_t)c * L.n + q];
				colors[3 * id + c] = (float)(Cp + t * (Cq - Cp));
			}
		}
		id++;
	}
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_faces_kernel(Lattice L, const float* __restrict__ tsdf, const float* __restrict__ wsum, float min_weight,
	const uint32_t* __restrict__ cv, const uint32_t* __restrict__ cf, const uint32_t* __restrict__ ce, const uint32_t* __restrict__ owners,
	unsigned n_owner_chunks, size_t n_faces, int* __restrict__ faces) {
	__shared__ uint32_t s_wave[TSDF_THREADS / WAVE];
	const unsigned chunk = blockIdx.x, idx = chunk * (unsigned)TSDF_THREADS + threadIdx.x;
	PointClass pc; pc.in8 = 0; pc.vmask = 0; pc.cell = false;
	if (idx < L.n) { int i, j, k; split_index(L, idx, i, j, k); pc = classify(L, tsdf, wsum, min_weight, idx, i, j, k); }
	uint32_t nf_chunk;
	const uint32_t local = block_exclusive<TSDF_THREADS>(pc.cell ? cell_faces(pc.in8) : 0u, s_wave, nf_chunk);
	if (!pc.cell) return;
	const unsigned sy = (unsigned)L.nx, sz = (unsigned)L.nx * (unsigned)L.ny;
	// the vertex on the edge between corners lo < hi (corner bits, lo a subset of hi) of this cell: it exists, so its owner's chunk has an owner word
	auto vid = [&](int lo, int hi) -> int {
		const unsigned owner = idx + (lo & 1) + ((lo >> 1) & 1) * sy + (lo >> 2) * sz;      // a corner of a valid cell: inside the lattice
		const unsigned oc = owner / (unsigned)TSDF_THREADS, ol = owner % (unsigned)TSDF_THREADS;
		const uint32_t word = owners[(size_t)min(ce[oc], n_owner_chunks - 1u) * TSDF_THREADS + ol];
		return (int)(cv[oc] + (word >> 8) + (uint32_t)__popc(word & ((1u << ((SLOT_OF_BITS >> (4 * (hi ^ lo))) & 15u)) - 1u)));
	};
	cell_emit_faces(pc.in8, vid, (size_t)cf[chunk] + local, n_faces, faces);
}

// 0: `L` is set; 1: an empty lattice; -1: refused
int check_volume(const std::string& name, const adgs_tsdf_volume* vol, Lattice& L) {
	if (vol->struct_bytes < (int)sizeof(adgs_tsdf_volume)) { set_error(name + ": struct_bytes is smaller than adgs_tsdf_volume"); return -1; }
	if (vol->nx < 0 || vol->ny < 0 || vol->nz < 0) { set_error(name + ": negative nx, ny or nz"); return -1; }
	const unsigned long long xy = (unsigned long long)vol->nx * (unsigned long long)vol->ny;
	if (xy > (unsigned long long)INT_MAX || xy * (unsigned long long)vol->nz > (unsigned long long)INT_MAX) {
		set_error(name + ": nx * ny * nz must be below 2^31"); return -1;
	}
	if (!positive(vol->voxel_size)) { set_error(name + ": voxel_size must be finite and > 0"); return -1; }
	for (int a = 0; a < 3; a++)
		if (!std::isfinite(vol->origin[a])) { set_error(name + ": the origin must be finite"); return -1; }
	L.nx = vol->nx; L.ny = vol->ny; L.nz = vol->nz;
	L.n = (unsigned)(xy * (unsigned long long)vol->nz);
	L.vs = (double)vol->voxel_size;
	for (int a = 0; a < 3; a++) L.o[a] = (double)vol->origin[a];
	return L.n == 0 ? 1 : 0;
}

// the rows of the extraction's scratch (ExtractTemp, tsdf_shared.h)
unsigned chunks_of(const Lattice& L) { return (L.n + (unsigned)TSDF_THREADS - 1u) / (unsigned)TSDF_THREADS; }

} // namespace
} // namespace adgs

using namespace adgs;

extern "C" int adgs_tsdf_integrate(const adgs_tsdf_volume* vol, const adgs_tsdf_view* view, const float* depth, const float* opacity, const float* image,
	const float* weight, float* tsdf, float* wsum, float* color, void* stream_) {
	const std::string name("adgs_tsdf_integrate");
	if (!vol || !view || !depth || !opacity || !tsdf || !wsum) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	const int c = check_volume(name, vol, L);
	if (c < 0) return -1;
	TsdfView v;
	if (check_view(name, view, v) < 0) return -1;
	if ((image != nullptr) != (color != nullptr)) { set_error(name + ": image and color must be given together"); return -1; }
	if (c == 1 || view->H == 0 || view->W == 0) return 0;
	ADGS_LAUNCH(tsdf_integrate_kernel, dim3(chunks_of(L)), dim3(TSDF_THREADS), 0, (hipStream_t)stream_, L, v, depth, opacity, image, weight, tsdf,
		wsum, color);
	return 0;
}

extern "C" size_t adgs_tsdf_extract_temp_bytes(const adgs_tsdf_volume* vol) {
	Lattice L;
	if (!vol || check_volume("adgs_tsdf_extract_temp_bytes", vol, L) < 0) return 0;
	return carve_extract(nullptr, chunks_of(L)).bytes;
}

extern "C" size_t adgs_tsdf_extract_owner_bytes(long long nonempty_chunks) {
	return nonempty_chunks > 0 ? (size_t)nonempty_chunks * ADGS_TSDF_OWNER_BYTES_PER_CHUNK : 0;
}

extern "C" int adgs_tsdf_extract_count(const adgs_tsdf_volume* vol, const float* tsdf, const float* wsum, float min_weight, void* temp, long long* counts,
	void* stream_) {
	const std::string name("adgs_tsdf_extract_count");
	if (!vol || !tsdf || !wsum || !temp || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	const int c = check_volume(name, vol, L);
	if (c < 0) return -1;
	counts[0] = counts[1] = counts[2] = 0;
	if (c == 1 || L.nx < 2 || L.ny < 2 || L.nz < 2) return 0;     // no cell, hence no vertex and no face
	hipStream_t stream = (hipStream_t)stream_;
	const unsigned chunks = chunks_of(L);
	const ExtractTemp t = carve_extract((char*)temp, chunks);
	ADGS_LAUNCH(tsdf_points_kernel<false>, dim3(chunks), dim3(TSDF_THREADS), 0, stream, L, tsdf, wsum, (const float*)nullptr, min_weight, t.cv, t.cf,
		t.ce, (uint32_t*)nullptr, 0u, (size_t)0, (float*)nullptr, (float*)nullptr);
	return extract_count_tail(name, t, chunks, stream, counts);
}

extern "C" int adgs_tsdf_extract_emit(const adgs_tsdf_volume* vol, const float* tsdf, const float* wsum, const float* color, float min_weight,
	const void* temp, void* owners, const long long* counts, float* vertices, int* faces, float* colors, void* stream_) {
	const std::string name("adgs_tsdf_extract_emit");
	if (!vol || !tsdf || !wsum || !temp || !counts) { set_error(name + ": NULL pointer"); return -1; }
	Lattice L;
	const int c = check_volume(name, vol, L);
	if (c < 0) return -1;
	const long long V = counts[0], F = counts[1], E = counts[2];
	const long long chunks = c == 1 ? 0 : (long long)chunks_of(L);
	if (check_emit(name, "adgs_tsdf_extract_count", counts, INT_MAX, INT_MAX, chunks, vertices, faces, owners, color, colors) < 0) return -1;
	if (V == 0 || E == 0) return 0;                              // no vertex, hence no face
	hipStream_t stream = (hipStream_t)stream_;
	const ExtractTemp t = carve_extract((char*)temp, (size_t)chunks);
	ADGS_LAUNCH(tsdf_points_kernel<true>, dim3((unsigned)chunks), dim3(TSDF_THREADS), 0, stream, L, tsdf, wsum, color, min_weight, t.cv, t.cf, t.ce,
		(uint32_t*)owners, (unsigned)E, (size_t)V, vertices, colors);
	if (F > 0) ADGS_LAUNCH(tsdf_faces_kernel, dim3((unsigned)chunks), dim3(TSDF_THREADS), 0, stream, L, tsdf, wsum, min_weight, (const uint32_t*)t.cv,
		(const uint32_t*)t.cf, (const uint32_t*)t.ce, (const uint32_t*)owners, (unsigned)E, (size_t)F, faces);
	return 0;
}
