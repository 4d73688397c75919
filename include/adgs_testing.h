/*
 * adgs_testing.h -- test-only entry points of libadgs_hip.so (device primitives that
 * the rasterizer and kNN paths are built from).  Not part of the drop-in boundary;
 * used by tests/ to check the hand-written scan / radix sort directly.
 */
#ifndef ADGS_TESTING_H
#define ADGS_TESTING_H
#include <stddef.h>
#include <stdint.h>
#include "adgs_deform.h"
#ifdef __cplusplus
extern "C" {
#endif
size_t adgs_test_scan_temp_bytes(size_t n);
/* out[i] = sum_{j<i} in[j]; in == out allowed */
int adgs_test_exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, char* temp, void* stream);
size_t adgs_test_sort_temp_bytes(size_t n);
/* stable LSD radix sort on key bits [0,end_bit); *_in are clobbered */
int adgs_test_sort_pairs_u64(uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n, int end_bit, char* temp, void* stream);
int adgs_test_sort_pairs_u32(uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n, int end_bit, char* temp, void* stream);
/* the scan above plus, when aux_in is given, sum(aux_in[0..n)) ADDED into the 32 counters aux_total[] (the caller adds them up);
 * in == out == aux_in allowed; aux_in == NULL leaves the counters alone */
int adgs_test_exclusive_scan_u32_sum(const uint32_t* in, uint32_t* out, size_t n, char* temp, const uint32_t* aux_in, unsigned long long* aux_total /* 32 slots */, void* stream);
/* the u64 sort with the count read on the device: sorts the first min(*d_n, n_cap) pairs; n_cap sizes the launch, the temporaries
 * (adgs_test_sort_temp_bytes(n_cap)) and all four arrays; out[min(*d_n, n_cap) .. n_cap) holds no result */
int adgs_test_sort_pairs_u64_dn(uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n_cap, const uint32_t* d_n, int end_bit, char* temp, void* stream);
/* Number of (tile, Gaussian) entries the default (v2) forward published for the backward replay of a frame: the sum of the
 * per-tile counts in the forward's image-state buffer.  Synchronises the stream; statistics only (bench.py). */
long long adgs_test_v2_published_entries(const char* img_buffer, int width, int height, void* stream);
/* Sum over the tiles of the candidates of the coarse cell's depth-sorted list each tile's walk went through before all of
 * its pixels were saturated (same buffer, same conditions). */
long long adgs_test_v2_scanned_candidates(const char* img_buffer, int width, int height, void* stream);
/* The two per-tile counters themselves (host arrays of `capacity` uint32 each, either may be NULL); returns the number of tiles. */
long long adgs_test_v2_tile_counters(const char* img_buffer, int width, int height, uint32_t* out_consumed, uint32_t* out_scanned, long long capacity, void* stream);
/* Batches of <= 64 tile-test survivors the forward handed to its blend loop, summed over the tiles (same buffer, same conditions). */
long long adgs_test_v2_blend_batches(const char* img_buffer, int width, int height, void* stream);
/* (start, end) of every coarse cell's depth-sorted candidate list (host array of 2 x `capacity` uint32); returns the number of cells. */
long long adgs_test_v2_cell_ranges(const char* img_buffer, int width, int height, uint32_t* out_ranges, long long capacity, void* stream);
/* The "published" mask of a default-pipeline training forward's geometry state (one byte per Gaussian: 1 when the blend handed the id to
 * the backward's replay lists, else 0) and the accumulator lines ([P][16] floats) as they stand -- after a backward: what the blend backward
 * summed.  out_bytes: host array of P bytes, out_lines: host array of 16 P floats; either may be NULL.  Returns P, -1 on an error.
 * Synchronises the stream. */
long long adgs_test_v2_published_mask(const char* geom_buffer, int P, uint8_t* out_bytes, float* out_lines, void* stream);
/* Byte offsets of the published mask (out2[0]) and of the accumulator lines (out2[1]) inside a default-pipeline geometry state of P
 * Gaussians: a test overwrites lines the backward must not read.  Host only.  Returns 0, -1 on a bad argument. */
int adgs_test_v2_geom_offsets(int P, long long* out2);

/* sizeof of the structs that cross the ABI by pointer (0 adgs_sh_source, 1 adgs_sh_grads, 2 adgs_frame_stats, 3 adgs_frame_status,
 * 4 adgs_func_eval, 5 adgs_adam_group, 6 adgs_sh_adam, 7 adgs_raster_options, 8 adgs_adam_rows, 9 adgs_raster_backward_options,
 * 10 adgs_metrics_desc, 11 adgs_cc_desc): a binding checks its mirror against it. */
size_t adgs_test_abi_sizeof(int which);

/* How many times the rasterizer has read an ADGS_* environment switch so far (process-wide).  The backward of a frame must not read any:
 * what the forward decided from the environment travels with the frame (api.hip: FrameCfg); a test reads this before and after. */
unsigned long long adgs_test_env_reads(void);

/* Overwrites the process-wide capacity hints the next default-pipeline forward is enqueued against (pairs, fine pairs; the
 * forward still uses at least P + 4096 / 8 P + 4096): lets a test force the "frame does not fit its capacity" path. */
void adgs_test_set_capacity_hints(long long pairs, long long fine_pairs);      /* also forgets the depth-slab bounds the bucket binning has learned */

/* Fills the calling thread's table of depth-slab bounds (bucket binning) with pseudo-random words: any contents must give the same
 * per-cell lists.  Returns 0, -1 when no bucket-binned frame has created the table yet. */
int adgs_test_scramble_slab_bounds(unsigned seed);

/* Which way adgs_bilagrid_slice_forward / _backward (include/adgs_bilagrid.h) run a call of this shape -- the choice depends on the shape
 * alone: 1 = grid columns staged / gradients accumulated in LDS, 0 = the footprint of a pixel tile can exceed the LDS budget (a small image
 * under a large grid): gathers from and atomics into global memory.  -1: a shape the entry points refuse. */
int adgs_test_bilagrid_path(int L, int Hg, int Wg, int H, int W);

/* The launch layout adgs_deform_forward_flow / adgs_deform_backward_flow (include/adgs_deform.h) would choose for their geometry kernel
 * on these arguments, from the same two plan functions the entry points call.  Host only: no HIP call, no device needed, and no tensor
 * pointer is dereferenced -- only the VALUES of the pointers in *p, *out, *grads and of the others are looked at (NULL or not,
 * alignment).  np_*: n_params of f_xyz, f_xyz_flow and f_rotation.  fwd / bwd each receive ADGS_TEST_DEFORM_PLAN_FIELDS words:
 * block size, dynamic LDS bytes, xyz row length, LDS stride of the xyz rows, of the rotation rows, xyz_rows (object xyz rows read
 * directly), scene4 (scene range four Gaussians per thread), blocks of the rotation set, of the xyz set, of the scene set, and
 * refused (0: no; 1: rows too large for the staging buffer; 2, forward with ADGS_DEFORM_WILL_BACKWARD: too large for the backward's). */
#define ADGS_TEST_DEFORM_PLAN_FIELDS 11
int adgs_test_deform_plan(const adgs_deform_params* p, int np_xyz, int np_xyz_flow, int np_rotation, const adgs_deform_outputs* out, const float* flow_xyz,
	const float* dL_dxyz, const float* dL_drotation, const float* dL_dopacity, const float* dL_dscales, const float* dL_dflow_xyz,
	const adgs_deform_grads* grads, int32_t* fwd, int32_t* bwd);

#ifdef __cplusplus
}
#endif
#endif
