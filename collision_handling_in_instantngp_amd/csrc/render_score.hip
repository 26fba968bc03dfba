// The scoring forms of the render kernel (render.inc: the kSrc*Score sources, whose sink is RenderScore) and the entry points of
// include/gngf_ext2.h.  A translation unit of its own: the scoring forms double the render instantiations, and here they compile
// next to decoder.hip instead of behind it.
#include "gngf_common.h"
#include "../../include/gngf_ext2.h"
#include <type_traits>
#include "decoder_common.inc"
#define GNGF_RENDER_KERNELS_ONLY
#include "render.inc"

namespace gngf {

constexpr int kScoreMaxGrid = 256;                        // one persistent workgroup per CU, as gngf_render

using ScoreKern = void (*)(const RenderArgs, const RenderScore);
template <int KIN, int SRC, typename TT> static ScoreKern score_pick(bool leaky, bool exact) {
  if (leaky) return exact ? render_kernel<KIN, true, true, SRC, TT> : render_kernel<KIN, true, false, SRC, TT>;
  return exact ? render_kernel<KIN, false, true, SRC, TT> : render_kernel<KIN, false, false, SRC, TT>;
}
template <int SRC, typename TT> static ScoreKern score_pick_width(int in_dim, bool leaky) {
  return in_dim <= 32 ? score_pick<32, SRC, TT>(leaky, in_dim == 32) : score_pick<64, SRC, TT>(leaky, in_dim == 64);
}
template <int SRC> static ScoreKern score_pick_dtype(bool f16, int in_dim, bool leaky) {
  return f16 ? score_pick_width<SRC, __half>(in_dim, leaky) : score_pick_width<SRC, float>(in_dim, leaky);
}

// one workgroup: sums[k] = sum over b of partial[2 b + k], b < nwg <= kScoreMaxGrid = blockDim
__global__ void __launch_bounds__(kScoreMaxGrid)
render_score_finish_kernel(const int64_t* __restrict__ partial, int64_t* __restrict__ sums, int nwg) {
  __shared__ int64_t red[2][kScoreMaxGrid / 64];
  int64_t eq = 0, sse = 0;
  if ((int)threadIdx.x < nwg) { eq = partial[2 * threadIdx.x]; sse = partial[2 * threadIdx.x + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { eq += __shfl_xor(eq, o, 64); sse += __shfl_xor(sse, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = eq; red[1][threadIdx.x >> 6] = sse; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int64_t s = 0;
    for (int w = 0; w < kScoreMaxGrid / 64; ++w) s += red[threadIdx.x][w];
    sums[threadIdx.x] = s;
  }
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext2_version(void) { return GNGF_EXT2_VERSION; }

extern "C" int gngf_ext2_render_score_workspace_words(void) { return 2 * kScoreMaxGrid; }

// sums = (#equal elements, sum of squared differences) of the model's (int32_t)(y * 255.0f) against image at the pixels
// (i step, j step).  See include/gngf_ext2.h.
extern "C" int gngf_ext2_render_score(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                                      const int32_t* n_ls, const float* W0, const float* b0, const float* W1, const float* b1,
                                      const float* W2, const float* b2, int L, int F, int64_t T, int K, int mode, int vstride,
                                      int64_t NV, int out_dim, int leaky, const uint8_t* image, int64_t h, int64_t w, int C,
                                      float denom, int64_t step, int64_t* sums, int64_t* workspace, void* stream) {
  constexpr int64_t kExact = (int64_t)1 << 24;            // integers up to here are exact in fp32
  GNGF_CHECK_ARG(L > 0 && L <= GNGF_MAX_LEVELS && (F == 1 || F == 2 || F == 4) && L * F <= 64 && T > 0);
  GNGF_CHECK_ARG(out_dim > 0 && out_dim <= 4 && C == out_dim);
  GNGF_CHECK_ARG(h >= 1 && h <= kExact && w >= 1 && w <= kExact && step >= 1 && denom > 0.f);
  GNGF_CHECK_ARG(mode == GNGF_MODE_HASH || mode == GNGF_MODE_VERTEX_TABLE || mode == GNGF_MODE_DENSE_HASH);
  GNGF_CHECK_ARG(feat_dtype == GNGF_FEAT_F32 || feat_dtype == GNGF_FEAT_F16);
  GNGF_CHECK_ARG(tables && n_ls && W0 && b0 && W1 && b1 && W2 && b2 && image && sums && workspace);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(tables) & 15) == 0);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(sums) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
  const bool vt = mode == GNGF_MODE_VERTEX_TABLE;
  if (vt) GNGF_CHECK_ARG(vert_idx && vert_w && K > 0 && K <= GNGF_MAX_TOPK_WIDE && vstride > 0 && NV > 0 && NV * K < ((int64_t)1 << 31));
  // a step past both sides selects pixel (0, 0) alone, whatever its value: the kernel's products (lattice index) * step stay small
  const int64_t st = step < kExact ? step : kExact;
  RenderArgs a;
  a.tables = tables; a.vert_idx = vert_idx; a.vert_w = vert_w; a.n_ls = n_ls;
  a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
  a.rgb = nullptr; a.img = nullptr;
  a.rows = (h + st - 1) / st; a.cols = (w + st - 1) / st; a.r0 = 0; a.c0 = 0; a.denom = denom;
  a.L = L; a.F = F; a.T = T; a.K = vt ? K : 0; a.vstride = vt ? vstride : 0; a.NV = vt ? NV : 0;
  a.out_dim = out_dim; a.pow2 = (T & (T - 1)) == 0;
  RenderScore sink;
  sink.image = image; sink.w = w; sink.step = st; sink.partial = workspace;
  const int in_dim = L * F;
  const int64_t nblocks = ((a.cols + kRenderCols - 1) / kRenderCols) * ((a.rows + kRenderRows - 1) / kRenderRows);
  const int nwg = (int)(nblocks < kScoreMaxGrid ? nblocks : kScoreMaxGrid);
  const size_t smem = sizeof(float) * (size_t)raw_offsets(in_dim).total;
  const bool f16 = feat_dtype == GNGF_FEAT_F16;
  const ScoreKern fn = mode == GNGF_MODE_DENSE_HASH ? score_pick_dtype<kSrcDenseHashScore>(f16, in_dim, leaky != 0)
                       : vt                         ? score_pick_dtype<kSrcTableScore>(f16, in_dim, leaky != 0)
                                                    : score_pick_dtype<kSrcHashScore>(f16, in_dim, leaky != 0);
  hipStream_t s = as_stream(stream);
  fn<<<dim3((unsigned)nwg), dim3(kDecThreads), smem, s>>>(a, sink);
  render_score_finish_kernel<<<dim3(1), dim3(kScoreMaxGrid), 0, s>>>(workspace, sums, nwg);
  GNGF_RETURN_LAUNCH();
}
