// Split-bf16 helpers of the decoder's hybrid backward and training kernels (included by decoder.hip inside namespace gngf).
//
// A product moves from v_mfma_f32_32x32x2_f32 to v_mfma_f32_32x32x16_bf16: each fp32 operand value is split EXACTLY into three
// bf16 terms by truncation, x = hi + mid + lo (8 + 8 + 8 significant bits: `hi` is the upper half of the fp32 word, the residuals are
// exact fp32 subtractions), and a product is the sum of six of the nine cross terms accumulated in fp32,
//     a b ~= hi lo + lo hi + mid mid + hi mid + mid hi + hi hi          (dropped: mid lo, lo mid, lo lo  <  2^-23 |a b|)
// i.e. at the accuracy of an fp32 fma chain (tests/test_gpu_dense.py compares the decoders with a float64 evaluation).
// Why: six bf16 MFMAs take 6 x 32 cycles for a 32x32x16 block that costs 8 x 64 cycles on the fp32 pipe, and — measured,
// tools/micro/gen_mfma_bf16_mix.py — VALU instructions issue underneath a bf16 MFMA (4 per MFMA for free), which they never
// do under an fp32 one: the splitting (5.5 VALU instructions per value) mostly disappears under the matrix pipe.
// The operand layouts keep the trick of the fp32 kernels: products are computed transposed (feature on the accumulator
// register, pixel on the lane), and since ANY permutation of the k axis is allowed as long as A and B agree on it, accumulator
// registers 8c .. 8c+7 of both lane halves ARE k-chunk c of the next layer's B operand — no LDS round trip between layers.
//   k-chunk (t, c) of a 64-wide activation, lane half h, element j  <->  feature 32 t + crow(8 c + j, h)
//   k-chunk c of the input row,            lane half h, element j  <->  input feature h KIN/2 + 8 c + j
// (An all-bf16 decoder pair built on the same split was measured and dropped: DESIGN.md §3.)

struct Planes { u32x4 hi, mid, lo; };

__device__ __forceinline__ unsigned pack_hi16(float b, float a) {      // (upper half of b) : (upper half of a)
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ float trunc_residual(float v) { return v - __uint_as_float(__float_as_uint(v) & 0xffff0000u); }   // exact

// exact three-way split of eight fp32 values = one B (or A) fragment of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ Planes split8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7) {
  const float x[8] = {x0, x1, x2, x3, x4, x5, x6, x7};
  unsigned hi[4], mid[4], lo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = x[2 * q], b = x[2 * q + 1];
    hi[q] = pack_hi16(b, a);
    const float ra = trunc_residual(a), rb = trunc_residual(b);
    mid[q] = pack_hi16(rb, ra);
    lo[q] = pack_hi16(trunc_residual(rb), trunc_residual(ra));
  }
  Planes p;
  p.hi = u32x4{hi[0], hi[1], hi[2], hi[3]}; p.mid = u32x4{mid[0], mid[1], mid[2], mid[3]}; p.lo = u32x4{lo[0], lo[1], lo[2], lo[3]};
  return p;
}

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
__device__ __forceinline__ f32x16 mfma_b(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// acc += A B over one k-chunk, six cross terms, smallest first, for two output tiles sharing the B operand, interleaved
// (independent accumulators back to back)
__device__ __forceinline__ void mfma_split2(const Planes& a0, const Planes& a1, const Planes& b, f32x16& c0, f32x16& c1) {
  c0 = mfma_b(a0.hi, b.lo, c0);  c1 = mfma_b(a1.hi, b.lo, c1);
  c0 = mfma_b(a0.lo, b.hi, c0);  c1 = mfma_b(a1.lo, b.hi, c1);
  c0 = mfma_b(a0.mid, b.mid, c0); c1 = mfma_b(a1.mid, b.mid, c1);
  c0 = mfma_b(a0.hi, b.mid, c0); c1 = mfma_b(a1.hi, b.mid, c1);
  c0 = mfma_b(a0.mid, b.hi, c0); c1 = mfma_b(a1.mid, b.hi, c1);
  c0 = mfma_b(a0.hi, b.hi, c0);  c1 = mfma_b(a1.hi, b.hi, c1);
}

// The same six cross terms one at a time (P = 0 .. 5, in mfma_split2's order), for the schedules that put a few VALU instructions
// behind every single MFMA (decoder.hip, "issue model": at most five hide under one bf16 MFMA) instead of a burst behind a pair.
template <int P> __device__ __forceinline__ void mfma_cross(const Planes& a, const Planes& b, f32x16& c) {
  static_assert(P >= 0 && P < 6, "six cross terms");
  if constexpr (P == 0) c = mfma_b(a.hi, b.lo, c);
  else if constexpr (P == 1) c = mfma_b(a.lo, b.hi, c);
  else if constexpr (P == 2) c = mfma_b(a.mid, b.mid, c);
  else if constexpr (P == 3) c = mfma_b(a.hi, b.mid, c);
  else if constexpr (P == 4) c = mfma_b(a.mid, b.hi, c);
  else c = mfma_b(a.hi, b.hi, c);
}
// One twelfth of split8: pair q = K / 3 of the eight values (a, b = values 2 q, 2 q + 1), phase K % 3 — the packed upper halves |
// the two first residuals and their upper halves | the two second residuals' upper halves: 1 + 5 + 5 VALU instructions, the same
// expressions as split8.  ra / rb carry the first residuals from phase 1 to phase 2.  The empty asm statement keeps a twelfth where
// it was written (a pure instruction may otherwise drift to its first use, past the scheduling barriers of the slots).
template <int K> __device__ __forceinline__ void split_twelfth(float a, float b, unsigned (&hi)[4], unsigned (&mid)[4], unsigned (&lo)[4],
                                                              float& ra, float& rb) {
  constexpr int q = K / 3, p = K % 3;
  static_assert(K >= 0 && K < 12, "twelve sub-steps");
  if constexpr (p == 0) { hi[q] = pack_hi16(b, a); asm volatile("" : "+v"(hi[q])); }
  else if constexpr (p == 1) { ra = trunc_residual(a); rb = trunc_residual(b); mid[q] = pack_hi16(rb, ra); asm volatile("" : "+v"(mid[q])); }
  else { lo[q] = pack_hi16(trunc_residual(rb), trunc_residual(ra)); asm volatile("" : "+v"(lo[q])); }
}

// k index of a 64-wide activation at chunk cc (= 2 t + c), lane half h, element j
__device__ __forceinline__ int kmapS(int cc, int h, int j) { return 32 * (cc >> 1) + crow(8 * (cc & 1) + j, h); }

// A fragments (weights) as bf16 planes in LDS, one 16-byte read per lane and fragment:  frag[(f * 3 + plane) * 64 + lane]
__device__ __forceinline__ void store_planes(u32x4* dst, const Planes& p) { dst[0] = p.hi; dst[64] = p.mid; dst[128] = p.lo; }
__device__ __forceinline__ Planes load_planes(const u32x4* src) { Planes p; p.hi = src[0]; p.mid = src[64]; p.lo = src[128]; return p; }
