/*
 * gngf_ext3.h — third additive extension of the C-ABI of libgngf_hip.so.
 *
 * include/gngf.h (GNGF_ABI_VERSION 15), include/gngf_ext.h (GNGF_EXT_VERSION 1) and include/gngf_ext2.h (GNGF_EXT2_VERSION 1) are
 * pinned by the test suite as they stand.  Entry points added after them live here, in the same library and under the same
 * conventions (device pointers, `stream` a hipStream_t as void*, the return value a hipError_t as int, hipErrorInvalidValue (1) =
 * rejected arguments, nothing throws), with a version of their own.  The binding keeps them in a fourth table
 * (_lib.EXT3_SIGNATURES / _lib.EXT3_VERSION / _lib.EXT3_WRITES_NOTHING).  THIS header is open: a later change adds its entry
 * points here and raises GNGF_EXT3_VERSION.  The tests hold header, library and binding to each other, not to a list of names, and
 * find the guard-band cases of an entry point by looking for a module-level ext3_entry_points() in the GPU test files — no
 * existing test file names them.
 */
#ifndef GNGF_EXT3_H_
#define GNGF_EXT3_H_

#include <stdint.h>
#include "gngf.h"      /* gngf_bin_job */

#ifdef __cplusplus
extern "C" {
#endif

#define GNGF_EXT3_VERSION 2

int gngf_ext3_version(void);

/*
 * A model evaluated at P given coordinates in one forward-only launch (csrc/render.inc: the query forms of render_kernel,
 * instantiated in csrc/render_query.hip).  No workspace, no atomics, nothing but the outputs is written.
 *   Model arguments: those of gngf_render (include/gngf.h), with the same meaning and the same limits — tables (L,T,F) fp32 | fp16
 *   (16-byte aligned), vert_idx / vert_w (NV,K) and vstride for GNGF_MODE_VERTEX_TABLE, n_ls (L) int32 on the device, the decoder
 *   L F -> 64 -> 64 -> out_dim, mode one of GNGF_MODE_HASH / GNGF_MODE_VERTEX_TABLE / GNGF_MODE_DENSE_HASH, leaky.
 *   xy (P,2) fp32, 8-byte aligned: point p has the coordinate (xy[2 p], xy[2 p + 1]) = (row coordinate, column coordinate) — the
 *   order of a training batch and of a lattice point ((r0 + r) / denom, (c0 + c) / denom).  Read once per point (one 8-byte load),
 *   never written.
 *   rgb (P,out_dim) fp32 and / or img (P,out_dim) int32, each 4-byte aligned; either may be NULL, not both.
 * Value: rgb[p] = y, the decoder's sigmoid output at point p; img[p] = (int32_t)(y * 255.0f) (the product rounded on its own,
 *   conversion toward zero).  Both are, bit for bit, what gngf_render computes for a lattice point whose coordinate has the same
 *   fp32 bits: the coordinate is the only difference between the two kernels — the same gather, the same interpolation, the same
 *   MFMA chains, the same rcp / exp2 sigmoid.  A point's value does not depend on P, on its position in xy or on the other points.
 * Coordinates outside [0, 1]^2 are not rejected and never read outside a buffer: GNGF_MODE_HASH returns the model's value there
 *   (the hash is taken mod T); GNGF_MODE_VERTEX_TABLE clamps the vertex to [0, NV) and GNGF_MODE_DENSE_HASH clamps a dense level's
 *   vertex to the level's grid, so both return an edge value that is not the model's.  Non-finite coordinates read no address
 *   outside a buffer either, and give unspecified values.
 * Offsets into xy, rgb and img are 64-bit.  The launch is persistent: min(ceil(P / 128), 256) workgroups.
 * P = 0: success, no launch, nothing read or written (xy, rgb, img are not looked at beyond the checks below).
 * Rejected (hipErrorInvalidValue, before any launch, outputs untouched): everything gngf_render rejects of the model arguments;
 *   P < 0; a NULL xy with P > 0; xy not 8-byte aligned; rgb and img both NULL; rgb or img not 4-byte aligned.
 */
int gngf_ext3_query(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                    const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                    int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky,
                    const float* xy, int64_t P, float* rgb, int32_t* img, void* stream);

/*
 * gngf_ext3_query from a baked vertex grid: the model arguments of gngf_render_grid (include/gngf.h) — grid (sum_l (N_l + 2)^2, F)
 * fp32 (16-byte aligned) in gngf_vertex_grid_fwd's layout with Ls = L, n_ls (L) int32 on the device and n_ls_host, the same L
 * values on the host, the decoder, leaky — and the tail, the values and the rejections of gngf_ext3_query.
 * Value: bit for bit what gngf_render_grid computes for a lattice point whose coordinate has the same fp32 bits.  A corner is
 * clamped to its level's (N_l + 2)^2 vertices: a coordinate outside [0, 1]^2 reads the edge of the grid, never past it, and the
 * value there is not the model's.
 * Rejected: everything gngf_render_grid rejects of the model arguments (a negative n_ls_host among them), and the tail's cases.
 */
int gngf_ext3_query_grid(const float* grid, const int32_t* n_ls, const int32_t* n_ls_host,
                         const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                         int L, int F, int out_dim, int leaky,
                         const float* xy, int64_t P, float* rgb, int32_t* img, void* stream);

/*
 * (version 2) The flat vertex backward that OWNS its rows (csrc/vertex_flat_owned.hip): the arguments, the list, the item values,
 * the checks and the launch shape (ceil(N / 1024) workgroups of 256 threads, 4 items each) of gngf_vertex_grid_bwd_flat
 * (include/gngf.h) — but dtables is WRITTEN and added to, not only accumulated into, so it need not be zero:
 *   a run of equal item_dest that lies wholly inside one workgroup's 1024 items: its row (F floats) is STORED, 0.f + sum — a zero
 *     sum too (the row may hold an older value), and a -0.0 sum as +0.0, which is what adding it to a zeroed row leaves;
 *   a run that enters or leaves a workgroup (the workgroup reads item_dest[first - 1] and item_dest[end] to tell): each part is
 *     ADDED with a float atomic, zero sums skipped — the caller zeroes these rows before the launch (at most one per boundary
 *     between two workgroups; gngf_ext3_encode_tiled_bwd_clear_rows does it inside the launch that precedes this one);
 *   a row no item names is neither read nor written.
 * With those rows zeroed the result equals gngf_vertex_grid_bwd_flat's on a zeroed buffer, bit for bit wherever a run has at most
 * two parts (same partial sums, combined in the same order; a two-term add commutes).  No workgroup waits for another.
 * Rejected: what gngf_vertex_grid_bwd_flat rejects; dtables not aligned to min(4 F, 16) bytes.
 */
int gngf_ext3_vertex_grid_bwd_flat_owned(const int32_t* item_gi, const float* item_w, const int32_t* item_dest, int64_t N,
                                         const float* dG, const void* dG64, int64_t vtot, float* dtables, int64_t rows, int F,
                                         void* stream);

/*
 * (version 2) gngf_encode_tiled_bwd (include/gngf.h: same arguments, same meaning, same launches) with a row-clear rider:
 * a few more workgroups of the level-interleaved kernel's launch (one row per thread) store zeros to the F floats at
 * clear_base + F * clear_rows[i], i < n_clear_rows (a negative row number is skipped; the caller checks the upper range).  The
 * launch reads and writes clear_base nowhere else; the rows are clear when the next launch on the stream starts.
 * n_clear_rows == 0: exactly gngf_encode_tiled_bwd (clear_base / clear_rows are not looked at).
 * Rejected: what gngf_encode_tiled_bwd rejects; n_clear_rows < 0 or > 2^24; with n_clear_rows > 0: a NULL clear_base or clear_rows,
 *   max_items == 0, or a shape the level-interleaved backward kernel does not take (gngf_tiled_interleaved_applies).
 */
int gngf_ext3_encode_tiled_bwd_clear_rows(const float* sorted, const int32_t* items, const int32_t* n_items, int max_items,
                          const int32_t* tile_item_base, const int32_t* tile_level_off, const int32_t* n_ls,
                          const int32_t* n_ls_host, const float* genc, const float* genc_absmax, int absmax_count,
                          int absmax_stride, float* dG, float* partials, int L, int Ls, int F, int tile_shift,
                          int lds_bytes, int chunk, const float* ride_slabs, float* ride_dW0, float* ride_db0,
                          float* ride_dW1, float* ride_db1, float* ride_dW2, float* ride_db2, int64_t ride_P,
                          int ride_in_dim, int ride_out_dim, const float* gloss_promised, const float* gloss_arrived,
                          const float* mse_pred, const float* mse_label,
                          float* mse_loss, float* mse_workspace, int64_t mse_n, float* hash_dtables, int64_t hash_T,
                          void* dG64, int log2_pixels, const gngf_bin_job* next_bin,
                          float* clear_base, const int32_t* clear_rows, int n_clear_rows, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNGF_EXT3_H_ */
