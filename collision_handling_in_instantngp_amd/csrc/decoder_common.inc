// What the decoder kernels (decoder.hip) and the render kernels (render.inc) share, in a file of its own so that a second
// translation unit (render_score.hip) can include render.inc without decoder.hip: the accumulator vector types, the MFMA
// builtin, the lane -> row maps of the 32x32 products and the coalesced LDS copy of the raw weights.
#ifndef GNGF_DECODER_COMMON_INC_
#define GNGF_DECODER_COMMON_INC_

namespace gngf {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kH = 64;                 // hidden width (both hidden layers)
constexpr int kDecThreads = 256;

__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// k index (feature of a 64-wide activation held as two accumulator tiles) consumed at chained k-step s2 by lane half h
__device__ __forceinline__ int kmapC(int s2, int h) { return 32 * (s2 >> 4) + crow(s2 & 15, h); }

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// Coalesced copy of the raw weights into LDS with a +1 padded row stride (conflict-free strided reads afterwards):
//   W0s [64][in_dim+1] | W1s [64][65] | W2s [4][65] | b0 [64] | b1 [64] | b2 [4]
struct RawOff { int w0, w1, w2, b0, b1, b2, total; };
__host__ __device__ inline RawOff raw_offsets(int in_dim) {
  RawOff o;
  o.w0 = 0; o.w1 = o.w0 + kH * (in_dim + 1); o.w2 = o.w1 + kH * 65; o.b0 = o.w2 + 4 * 65; o.b1 = o.b0 + kH; o.b2 = o.b1 + kH;
  o.total = o.b2 + 4;
  return o;
}
__device__ __forceinline__ void stage_raw(float* raw, const float* __restrict__ W0, const float* __restrict__ b0,
                                          const float* __restrict__ W1, const float* __restrict__ b1,
                                          const float* __restrict__ W2, const float* __restrict__ b2, int in_dim, int out_dim) {
  const RawOff o = raw_offsets(in_dim);
  for (int e = threadIdx.x; e < kH * in_dim; e += kDecThreads) raw[o.w0 + (e / in_dim) * (in_dim + 1) + e % in_dim] = W0[e];
  for (int e = threadIdx.x; e < kH * kH; e += kDecThreads) raw[o.w1 + (e >> 6) * 65 + (e & 63)] = W1[e];
  for (int e = threadIdx.x; e < 4 * kH; e += kDecThreads) raw[o.w2 + (e >> 6) * 65 + (e & 63)] = (e >> 6) < out_dim ? W2[e] : 0.f;
  for (int e = threadIdx.x; e < kH; e += kDecThreads) { raw[o.b0 + e] = b0[e]; raw[o.b1 + e] = b1[e]; }
  if (threadIdx.x < 4) raw[o.b2 + threadIdx.x] = (b2 && (int)threadIdx.x < out_dim) ? b2[threadIdx.x] : 0.f;
  __syncthreads();
}

}  // namespace gngf

#endif  // GNGF_DECODER_COMMON_INC_
