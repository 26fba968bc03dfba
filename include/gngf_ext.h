/*
 * gngf_ext.h — additive extension of the C-ABI of libgngf_hip.so.
 *
 * include/gngf.h is closed at GNGF_ABI_VERSION 15: its set of entry points, their signatures and its version are pinned by the test
 * suite.  Entry points added after that live here, in the same library and under the same conventions (device pointers, `stream` a
 * hipStream_t as void*, the return value a hipError_t as int, hipErrorInvalidValue (1) = rejected arguments, nothing throws), with a
 * version of their own.  The binding keeps them in a table of their own as well (_lib.EXT_SIGNATURES / _lib.EXT_VERSION).
 */
#ifndef GNGF_EXT_H_
#define GNGF_EXT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNGF_EXT_VERSION 1

int gngf_ext_version(void);

/*
 * A training batch drawn straight from the uint8 image (csrc/sample.hip): P random positions and their targets.
 *   image (h,w,C) uint8;  xy (P,2) fp32 = (row, col) / denom, the layout of every encoder entry point;  target (P,C) fp32.
 *   draw: ONE device int64, the number of batches drawn so far.  The launch reads it as d; a one-lane launch behind it on the same
 *   stream stores d + 1 — a captured call draws a new batch on every replay.
 * Sample i of draw d, 64-bit wrapping arithmetic:
 *   s = seed + 0x9E3779B97F4A7C15 * (d * P + i + 1)
 *   z = s;  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *   u = z >> 40,  v = (z >> 16) & 0xFFFFFF                                  (24 bits each)
 * continuous == 0 — a random pixel centre, with replacement:
 *   r = (u * h) >> 24, c = (v * w) >> 24;  xy = ((float)r / denom, (float)c / denom);  target[k] = (float)image[r,c,k] / 255.0f
 * continuous == 1 — a random position, target looked up bilinearly (every fp32 operation rounded on its own):
 *   pr = ((float)u * 0x1p-24f) * (float)(h - 1),  pc = ((float)v * 0x1p-24f) * (float)(w - 1);  xy = (pr / denom, pc / denom)
 *   r0 = min((int)floorf(pr), h - 2), fr = pr - (float)r0;  c0, fc likewise
 *   t = (float)texel / 255.0f at t00 = (r0,c0), t01 = (r0,c0+1), t10 = (r0+1,c0), t11 = (r0+1,c0+1)
 *   target[k] = ((t00 (1-fr)(1-fc) + t01 (1-fr) fc) + t10 fr (1-fc)) + t11 fr fc
 * Both divisions are correctly rounded.  Texel offsets are 64-bit.
 * Rejected (hipErrorInvalidValue, before any launch): a NULL pointer with P > 0; C outside 1..4; denom not > 0; h or w outside
 * [1, 2^24]; continuous other than 0 or 1, or 1 with h < 2 or w < 2; P < 0; xy or target not 4-byte, draw not 8-byte aligned.
 * P == 0: success, no launch, draw unchanged.
 */
int gngf_ext_sample_pixels(const uint8_t* image, int64_t h, int64_t w, int C, float denom,
                           int64_t seed, int64_t* draw, int continuous,
                           float* xy, float* target, int64_t P, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GNGF_EXT_H_ */
