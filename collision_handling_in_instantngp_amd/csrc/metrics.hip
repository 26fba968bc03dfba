// Epoch image and its two statistics (reference functions.py:308, 332-335, 690-692): the batches' decoder outputs become
// the (h,w,C) int32 image `(output * 255).int()` in image order, and train_accuracy / train_psnr need two INTEGER sums of
// it against the uint8 target — the number of equal elements and the sum of squared differences.  Both are produced
// exactly (int64 from the first addition), so 16 bytes cross to the host instead of the image.
#include "gngf_common.h"

namespace gngf {

constexpr int kMetricThreads = 256;
constexpr int kMetricElemsPerThread = 16;     // four 16-byte image loads per lane and trip
constexpr int kMetricMaxBlocks = 1024;        // partials the one-workgroup finish reads: 4 per lane
constexpr int kScatterMaxBlocks = 2048;       // 8 workgroups = 32 waves per CU; larger batches stride

// img[pix(i) * C + c] = (int32)(out[i * C + c] * 255.0f): one separately rounded fp32 product, conversion toward zero, no
// clamp — (output * 255).int() of torch.  Flat element index: a 12-byte row needs no alignment.
__global__ void __launch_bounds__(kMetricThreads)
image_scatter_kernel(const float* __restrict__ out, const int32_t* __restrict__ perm, int32_t* __restrict__ img, int64_t lo,
                     int64_t total /* n * C */, int C) {
  for (int64_t e = (int64_t)blockIdx.x * kMetricThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kMetricThreads) {
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const int64_t pix = perm ? (int64_t)perm[lo + i] : lo + i;
    img[pix * C + c] = (int32_t)(out[e] * 255.0f);
  }
}

__device__ __forceinline__ void metric_add(int32_t v, uint32_t t, int64_t& eq, int64_t& sse) {
  const int64_t d = (int64_t)v - (int64_t)t;              // |d| < 2^31 + 2^8: d * d < 2^63
  eq += d == 0;
  sse += d * d;
}

// partial[2 b], partial[2 b + 1] = the two sums over workgroup b's share.  Integer sums: the split over workgroups and lanes
// does not change the result.  vec: img 16-byte and target 4-byte aligned (four elements per load pair).
__global__ void __launch_bounds__(kMetricThreads)
image_metrics_partial_kernel(const int32_t* __restrict__ img, const uint8_t* __restrict__ target, int64_t* __restrict__ partial,
                             int64_t n, bool vec) {
  __shared__ int64_t red[2][kMetricThreads / 64];
  int64_t eq = 0, sse = 0;
  const int64_t tid = (int64_t)blockIdx.x * kMetricThreads + threadIdx.x, stride = (int64_t)gridDim.x * kMetricThreads;
  int64_t done = 0;                                       // elements [0, done) are covered by the vector loop
  if (vec) {
    const int64_t n4 = n >> 2;
    const int4* i4 = reinterpret_cast<const int4*>(img);
    const uint32_t* t4 = reinterpret_cast<const uint32_t*>(target);
    for (int64_t e = tid; e < n4; e += stride) {
      const int4 v = i4[e];
      const uint32_t t = t4[e];
      metric_add(v.x, t & 255u, eq, sse);
      metric_add(v.y, (t >> 8) & 255u, eq, sse);
      metric_add(v.z, (t >> 16) & 255u, eq, sse);
      metric_add(v.w, t >> 24, eq, sse);
    }
    done = n4 << 2;
  }
  for (int64_t e = done + tid; e < n; e += stride) metric_add(img[e], target[e], eq, sse);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { eq += __shfl_xor(eq, o, 64); sse += __shfl_xor(sse, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = eq; red[1][threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int64_t s = 0;
    for (int w = 0; w < kMetricThreads / 64; ++w) s += red[threadIdx.x][w];
    partial[2 * (int64_t)blockIdx.x + threadIdx.x] = s;
  }
}

// one workgroup: sums[k] = sum over b of partial[2 b + k]
__global__ void __launch_bounds__(kMetricThreads)
image_metrics_finish_kernel(const int64_t* __restrict__ partial, int64_t* __restrict__ sums, int nblocks) {
  __shared__ int64_t red[2][kMetricThreads / 64];
  int64_t eq = 0, sse = 0;
  for (int b = threadIdx.x; b < nblocks; b += kMetricThreads) { eq += partial[2 * b]; sse += partial[2 * b + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { eq += __shfl_xor(eq, o, 64); sse += __shfl_xor(sse, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = eq; red[1][threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int64_t s = 0;
    for (int w = 0; w < kMetricThreads / 64; ++w) s += red[threadIdx.x][w];
    sums[threadIdx.x] = s;
  }
}

}  // namespace gngf

using namespace gngf;

// img (P,C) int32, rows perm[lo + i] (perm == NULL: lo + i) for i in [0, n) = (int32)(out[i, :] * 255.0f), out (n,C) fp32
// contiguous.  perm (P) int32 with every value in [0, P): NOT checked here — the caller validates it once.
extern "C" int gngf_image_scatter(const float* out, const int32_t* perm, int32_t* img, int64_t lo, int64_t n, int64_t P, int C,
                                  void* stream) {
  GNGF_CHECK_ARG(out && img && C >= 1 && C <= 4 && n > 0 && lo >= 0 && P > 0 && lo <= P - n);
  const int64_t total = n * C;
  const int64_t want = ceil_div(total, kMetricThreads);
  image_scatter_kernel<<<dim3((unsigned)(want > kScatterMaxBlocks ? kScatterMaxBlocks : want)), dim3(kMetricThreads), 0,
                         as_stream(stream)>>>(out, perm, img, lo, total, C);
  GNGF_RETURN_LAUNCH();
}

extern "C" int gngf_image_metrics_blocks(int64_t n_elems) {
  const int64_t want = ceil_div(n_elems, (int64_t)kMetricThreads * kMetricElemsPerThread);
  return (int)(want < 1 ? 1 : (want > kMetricMaxBlocks ? kMetricMaxBlocks : want));
}
extern "C" int gngf_image_metrics_workspace_words(int64_t n_elems) { return 2 * gngf_image_metrics_blocks(n_elems); }

// sums[0] = #{e : img[e] == target[e]}, sums[1] = sum_e (img[e] - target[e])^2 over n_elems elements, exact in int64.
// workspace: gngf_image_metrics_workspace_words(n_elems) int64 words (written before they are read: no clearing needed).
extern "C" int gngf_image_metrics(const int32_t* img, const uint8_t* target, int64_t* sums, int64_t* workspace, int64_t n_elems,
                                  void* stream) {
  GNGF_CHECK_ARG(img && target && sums && workspace && n_elems > 0);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(img) & 3) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  const bool vec = (reinterpret_cast<uintptr_t>(img) & 15) == 0 && (reinterpret_cast<uintptr_t>(target) & 3) == 0;
  const int blocks = gngf_image_metrics_blocks(n_elems);
  hipStream_t s = as_stream(stream);
  image_metrics_partial_kernel<<<dim3((unsigned)blocks), dim3(kMetricThreads), 0, s>>>(img, target, workspace, n_elems, vec);
  image_metrics_finish_kernel<<<dim3(1), dim3(kMetricThreads), 0, s>>>(workspace, sums, blocks);
  GNGF_RETURN_LAUNCH();
}
