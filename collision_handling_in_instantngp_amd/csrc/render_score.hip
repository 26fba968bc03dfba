// The scoring forms of the render kernel (render.inc: the kSrc*Score sources, whose sink is RenderScore) and the entry points of
// include/gngf_ext2.h.  A translation unit of its own: the scoring forms double the render instantiations, and here they compile
// next to decoder.hip instead of behind it.  The model checks, the picker and the launch are render.inc's host section, shared with
// the other forms; this file holds what only a score has — the checks of the image, step, sums and workspace, and the finish kernel,
// whose block is the launch's largest grid (kRenderMaxGrid).  GNGF_RENDER_KERNELS_ONLY leaves out nothing but the definitions of
// gngf_render and gngf_render_grid, which belong to decoder.hip.
#include "gngf_common.h"
#include "../../include/gngf_ext2.h"
#include <type_traits>
#include "decoder_common.inc"
#define GNGF_RENDER_KERNELS_ONLY
#include "render.inc"

namespace gngf {

// one workgroup: sums[k] = sum over b of partial[2 b + k], b < nwg <= kRenderMaxGrid = blockDim
__global__ void __launch_bounds__(kRenderMaxGrid)
render_score_finish_kernel(const int64_t* __restrict__ partial, int64_t* __restrict__ sums, int nwg) {
  __shared__ int64_t red[2][kRenderMaxGrid / 64];
  int64_t eq = 0, sse = 0;
  if ((int)threadIdx.x < nwg) { eq = partial[2 * threadIdx.x]; sse = partial[2 * threadIdx.x + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { eq += __shfl_xor(eq, o, 64); sse += __shfl_xor(sse, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = eq; red[1][threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int64_t s = 0;
    for (int w = 0; w < kRenderMaxGrid / 64; ++w) s += red[threadIdx.x][w];
    sums[threadIdx.x] = s;
  }
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext2_version(void) { return GNGF_EXT2_VERSION; }

extern "C" int gngf_ext2_render_score_workspace_words(void) { return 2 * kRenderMaxGrid; }

// sums = (#equal elements, sum of squared differences) of the model's (int32_t)(y * 255.0f) against image at the pixels
// (i step, j step).  See include/gngf_ext2.h.
extern "C" int gngf_ext2_render_score(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                                      const int32_t* n_ls, const float* W0, const float* b0, const float* W1, const float* b1,
                                      const float* W2, const float* b2, int L, int F, int64_t T, int K, int mode, int vstride,
                                      int64_t NV, int out_dim, int leaky, const uint8_t* image, int64_t h, int64_t w, int C,
                                      float denom, int64_t step, int64_t* sums, int64_t* workspace, void* stream) {
  constexpr int64_t kExact = (int64_t)1 << 24;            // integers up to here are exact in fp32
  GNGF_CHECK_ARG(C == out_dim && h >= 1 && h <= kExact && w >= 1 && w <= kExact && step >= 1 && denom > 0.f);
  GNGF_CHECK_ARG(image && sums && workspace);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(sums) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  // a step past both sides selects pixel (0, 0) alone, whatever its value: the kernel's products (lattice index) * step stay small
  const int64_t st = step < kExact ? step : kExact;
  RenderArgs a;
  a.rgb = nullptr; a.img = nullptr;
  a.rows = (h + st - 1) / st; a.cols = (w + st - 1) / st; a.r0 = 0; a.c0 = 0; a.denom = denom;
  GNGF_CHECK_ARG(render_table_model(a, tables, feat_dtype, vert_idx, vert_w, n_ls, W0, b0, W1, b1, W2, b2, L, F, T, K, mode, vstride, NV, out_dim));
  RenderScore sink;
  sink.image = image; sink.w = w; sink.step = st; sink.partial = workspace;
  hipStream_t s = as_stream(stream);
  const int nwg = render_launch(render_pick_mode<kSrcScore>(mode, feat_dtype, L * F, leaky != 0), a, sink, render_blocks(a.rows, a.cols), s);
  render_score_finish_kernel<<<dim3(1), dim3(kRenderMaxGrid), 0, s>>>(workspace, sums, nwg);
  GNGF_RETURN_LAUNCH();
}
