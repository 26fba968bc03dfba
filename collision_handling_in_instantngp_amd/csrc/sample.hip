// Training batches drawn on the device from the uint8 image itself (include/gngf_ext.h: gngf_ext_sample_pixels): per sample one
// 64-bit counter-based draw (splitmix64 finaliser of seed + golden-ratio * counter), split into two 24-bit numbers — a random pixel
// centre, or a random continuous position whose target is the bilinear lookup of the four surrounding texels (the image task of
// Instant-NGP).  Every fp32 operation is rounded on its own (-ffp-contract=off) and both divisions are correctly rounded, so that
// a numpy restatement (tests/sampler_reference.py) gives the same bits.  The only per-pixel storage is the image: 1 B per channel.
#include "gngf_common.h"
#include "../../include/gngf_ext.h"

namespace gngf {

constexpr int kSampleThreads = 256;
constexpr int kSampleMaxBlocks = 2048;        // 8 workgroups = 32 waves per CU; larger batches stride
constexpr int64_t kSampleMaxSide = (int64_t)1 << 24;

__device__ __forceinline__ uint64_t sample_bits(uint64_t seed, uint64_t counter) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ float texel(const uint8_t* __restrict__ image, int64_t r, int64_t c, int64_t w, int C, int k) {
  return (float)image[(r * w + c) * C + k] / 255.0f;
}

// One lane per sample.  C: 1..4 channels as a template parameter (the channel loops unroll).  xy2: xy is 8-byte aligned, the pair
// goes out as one float2; otherwise as two floats.
template <int C, bool CONTINUOUS>
__global__ void __launch_bounds__(kSampleThreads)
sample_pixels_kernel(const uint8_t* __restrict__ image, int64_t h, int64_t w, float denom, uint64_t seed,
                     const int64_t* __restrict__ draw, float* __restrict__ xy, float* __restrict__ target, int64_t P, bool xy2) {
  const uint64_t base = (uint64_t)*draw * (uint64_t)P + 1ull;
  for (int64_t i = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kSampleThreads) {
    const uint64_t z = sample_bits(seed, base + (uint64_t)i);
    const uint64_t u = z >> 40, v = (z >> 16) & 0xFFFFFFull;
    float x0, x1, t[C];
    if (!CONTINUOUS) {
      const int64_t r = (int64_t)((u * (uint64_t)h) >> 24), c = (int64_t)((v * (uint64_t)w) >> 24);
      x0 = (float)r / denom;
      x1 = (float)c / denom;
#pragma unroll
      for (int k = 0; k < C; ++k) t[k] = texel(image, r, c, w, C, k);
    } else {
      const float pr = ((float)u * 0x1p-24f) * (float)(h - 1), pc = ((float)v * 0x1p-24f) * (float)(w - 1);
      x0 = pr / denom;
      x1 = pc / denom;
      int64_t r0 = (int64_t)floorf(pr), c0 = (int64_t)floorf(pc);
      r0 = r0 < h - 2 ? r0 : h - 2;                       // pr < h - 1 for every u: never taken, kept as a belt
      c0 = c0 < w - 2 ? c0 : w - 2;
      const float fr = pr - (float)r0, fc = pc - (float)c0;
      const float gr = 1.0f - fr, gc = 1.0f - fc;
      const float w00 = gr * gc, w01 = gr * fc, w10 = fr * gc, w11 = fr * fc;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const float t00 = texel(image, r0, c0, w, C, k), t01 = texel(image, r0, c0 + 1, w, C, k);
        const float t10 = texel(image, r0 + 1, c0, w, C, k), t11 = texel(image, r0 + 1, c0 + 1, w, C, k);
        t[k] = ((t00 * w00 + t01 * w01) + t10 * w10) + t11 * w11;
      }
    }
    if (xy2) {
      reinterpret_cast<float2*>(xy)[i] = make_float2(x0, x1);
    } else {
      xy[2 * i] = x0;
      xy[2 * i + 1] = x1;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) target[i * C + k] = t[k];
  }
}

// one lane, behind the sampling launch on the same stream: the next call (or the next replay of a captured one) draws batch d + 1
__global__ void sample_advance_kernel(int64_t* __restrict__ draw) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *draw = *draw + 1;
}

template <int C>
static void sample_launch(bool continuous, dim3 grid, hipStream_t s, const uint8_t* image, int64_t h, int64_t w, float denom,
                          uint64_t seed, const int64_t* draw, float* xy, float* target, int64_t P, bool xy2) {
  if (continuous)
    sample_pixels_kernel<C, true><<<grid, dim3(kSampleThreads), 0, s>>>(image, h, w, denom, seed, draw, xy, target, P, xy2);
  else
    sample_pixels_kernel<C, false><<<grid, dim3(kSampleThreads), 0, s>>>(image, h, w, denom, seed, draw, xy, target, P, xy2);
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext_version(void) { return GNGF_EXT_VERSION; }

extern "C" int gngf_ext_sample_pixels(const uint8_t* image, int64_t h, int64_t w, int C, float denom, int64_t seed, int64_t* draw,
                                      int continuous, float* xy, float* target, int64_t P, void* stream) {
  GNGF_CHECK_ARG(P >= 0 && C >= 1 && C <= 4 && denom > 0.0f);          // (NaN is not > 0)
  GNGF_CHECK_ARG(h >= 1 && h <= kSampleMaxSide && w >= 1 && w <= kSampleMaxSide);
  GNGF_CHECK_ARG(continuous == 0 || continuous == 1);
  GNGF_CHECK_ARG(!continuous || (h >= 2 && w >= 2));
  if (P == 0) return (int)hipSuccess;
  GNGF_CHECK_ARG(image && draw && xy && target);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(xy) & 3) == 0 && (reinterpret_cast<uintptr_t>(target) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(draw) & 7) == 0);
  const bool xy2 = (reinterpret_cast<uintptr_t>(xy) & 7) == 0;
  const int64_t want = ceil_div(P, kSampleThreads);
  const dim3 grid((unsigned)(want > kSampleMaxBlocks ? kSampleMaxBlocks : want));
  hipStream_t s = as_stream(stream);
  const uint64_t useed = (uint64_t)seed;
  switch (C) {
    case 1: sample_launch<1>(continuous != 0, grid, s, image, h, w, denom, useed, draw, xy, target, P, xy2); break;
    case 2: sample_launch<2>(continuous != 0, grid, s, image, h, w, denom, useed, draw, xy, target, P, xy2); break;
    case 3: sample_launch<3>(continuous != 0, grid, s, image, h, w, denom, useed, draw, xy, target, P, xy2); break;
    default: sample_launch<4>(continuous != 0, grid, s, image, h, w, denom, useed, draw, xy, target, P, xy2); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  sample_advance_kernel<<<dim3(1), dim3(1), 0, s>>>(draw);
  GNGF_RETURN_LAUNCH();
}
