/*
 * gngf_ext2.h — second additive extension of the C-ABI of libgngf_hip.so.
 *
 * include/gngf.h is closed at GNGF_ABI_VERSION 15 and include/gngf_ext.h at GNGF_EXT_VERSION 1 with exactly two names: both are
 * pinned, name for name, by the test suite.  Entry points added after that live here, in the same library and under the same
 * conventions (device pointers, `stream` a hipStream_t as void*, the return value a hipError_t as int, hipErrorInvalidValue (1) =
 * rejected arguments, nothing throws), with a version of their own.  The binding keeps them in a third table
 * (_lib.EXT2_SIGNATURES / _lib.EXT2_VERSION).  THIS header stays open: a later change adds its entry points here and raises
 * GNGF_EXT2_VERSION; the tests hold header, library and binding to each other, not to a fixed list of names.
 */
#ifndef GNGF_EXT2_H_
#define GNGF_EXT2_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNGF_EXT2_VERSION 1

int gngf_ext2_version(void);

/* int64 words of gngf_ext2_render_score's workspace: two per persistent workgroup, for the largest grid (2 * 256). */
int gngf_ext2_render_score_workspace_words(void);

/*
 * A model scored against the uint8 image it was trained on, in one render launch that writes no picture (csrc/render.inc:
 * the scoring forms of render_kernel) and a one-workgroup launch behind it on the same stream.
 *   Model arguments: those of gngf_render (include/gngf.h), with the same meaning and the same limits — tables (L,T,F) fp32 | fp16
 *   (16-byte aligned), vert_idx / vert_w (NV,K) and vstride for GNGF_MODE_VERTEX_TABLE, n_ls (L) int32 on the device, the decoder
 *   L F -> 64 -> 64 -> out_dim, mode one of GNGF_MODE_HASH / GNGF_MODE_VERTEX_TABLE / GNGF_MODE_DENSE_HASH, leaky.
 *   image (h,w,C) uint8, any alignment;  step >= 1;  sums: 2 int64;  workspace: gngf_ext2_render_score_workspace_words() int64,
 *   written before it is read (nothing needs clearing; words past the size query are never touched).
 * Lattice: image pixels (i step, j step), i < ceil(h / step), j < ceil(w / step).  The coordinate of such a pixel is
 *   ((float)(i step) / denom, (float)(j step) / denom) — the integer is exact in fp32 (h, w <= 2^24), each division is correctly
 *   rounded: bit for bit what gngf_render gives lattice point (i step, j step) of a full render with the same denom, and what
 *   gngf_ext_sample_pixels gives the pixel centre.  A step past both sides scores pixel (0, 0) alone.
 * Value: v[c] = (int32_t)(y[c] * 255.0f), y the decoder's sigmoid output, by gngf_render's own operations (same gather, same MFMA
 *   chains, same rcp / exp2 sigmoid, the product rounded on its own, conversion toward zero): the integer gngf_render stores in img.
 * Result, exact in int64 (independent of the grid: integer sums):
 *   sums[0] = #{(i, j, c) : v == image[i step, j step, c]},   sums[1] = sum (v - image[i step, j step, c])^2
 *   — gngf_image_metrics' two sums, in its order, over n = ceil(h / step) ceil(w / step) C elements.  Texel offsets are 64-bit.
 * No atomics: lanes reduce across the wave, the waves through LDS, each of the at most 256 workgroups stores its pair, the
 * second launch adds the pairs.
 * Rejected (hipErrorInvalidValue, before any launch, sums untouched): everything gngf_render rejects of the model arguments
 * and of denom (not > 0); C != out_dim; h or w outside [1, 2^24]; step < 1; a NULL image, sums or workspace; sums or workspace
 * not 8-byte aligned.
 */
int gngf_ext2_render_score(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                           const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                           int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky,
                           const uint8_t* image, int64_t h, int64_t w, int C, float denom, int64_t step,
                           int64_t* sums, int64_t* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNGF_EXT2_H_ */
