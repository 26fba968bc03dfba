// The query forms of the render kernel (render.inc: the kSrc*Query sources, whose coordinates are read from memory and whose sink
// is a row per point) and the entry points of include/gngf_ext3.h.  A translation unit of its own, as render_score.hip: the query
// forms add as many instantiations as the storing forms have, and here they compile next to decoder.hip instead of behind it.
#include "gngf_common.h"
#include "../../include/gngf_ext3.h"
#include <type_traits>
#include "decoder_common.inc"
#define GNGF_RENDER_KERNELS_ONLY
#include "render.inc"

namespace gngf {

constexpr int kQueryMaxGrid = 256;                        // one persistent workgroup per CU, as gngf_render

template <int KIN, int SRC, typename TT> static auto query_pick(bool leaky, bool exact) -> void (*)(const RenderArgs, const typename RenderSrcArgs<SRC>::type) {
  if (leaky) return exact ? render_kernel<KIN, true, true, SRC, TT> : render_kernel<KIN, true, false, SRC, TT>;
  return exact ? render_kernel<KIN, false, true, SRC, TT> : render_kernel<KIN, false, false, SRC, TT>;
}
template <int SRC, typename TT> static auto query_pick_width(int in_dim, bool leaky) {
  return in_dim <= 32 ? query_pick<32, SRC, TT>(leaky, in_dim == 32) : query_pick<64, SRC, TT>(leaky, in_dim == 64);
}
template <int SRC> static auto query_pick_dtype(bool f16, int in_dim, bool leaky) {
  return f16 ? query_pick_width<SRC, __half>(in_dim, leaky) : query_pick_width<SRC, float>(in_dim, leaky);
}

// the tail of both entry points: 0 = nothing to launch (P = 0), 1 = rejected, 2 = launch
static int query_tail(const float* xy, int64_t P, const float* rgb, const int32_t* img) {
  if (P < 0 || !(rgb || img) || (P > 0 && !xy)) return 1;
  if ((reinterpret_cast<uintptr_t>(xy) & 7) != 0) return 1;
  if ((reinterpret_cast<uintptr_t>(rgb) & 3) != 0 || (reinterpret_cast<uintptr_t>(img) & 3) != 0) return 1;
  return P == 0 ? 0 : 2;
}

// the walk of the lattice forms over ceil(P / 128) blocks: one row of blocks, block column = block (render.inc)
static void query_walk(RenderArgs& a, int64_t P, int64_t& nblocks) {
  nblocks = (P + kQueryBlock - 1) / kQueryBlock;
  a.rows = kRenderRows; a.cols = nblocks * kRenderCols; a.r0 = 0; a.c0 = 0; a.denom = 1.f;
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext3_version(void) { return GNGF_EXT3_VERSION; }

// rgb / img (P, out_dim) of the model at the coordinates xy (P, 2).  See include/gngf_ext3.h.
extern "C" int gngf_ext3_query(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                               const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                               int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky,
                               const float* xy, int64_t P, float* rgb, int32_t* img, void* stream) {
  GNGF_CHECK_ARG(L > 0 && L <= GNGF_MAX_LEVELS && (F == 1 || F == 2 || F == 4) && L * F <= 64 && T > 0);
  GNGF_CHECK_ARG(out_dim > 0 && out_dim <= 4);
  GNGF_CHECK_ARG(mode == GNGF_MODE_HASH || mode == GNGF_MODE_VERTEX_TABLE || mode == GNGF_MODE_DENSE_HASH);
  GNGF_CHECK_ARG(feat_dtype == GNGF_FEAT_F32 || feat_dtype == GNGF_FEAT_F16);
  GNGF_CHECK_ARG(tables && n_ls && W0 && b0 && W1 && b1 && W2 && b2);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(tables) & 15) == 0);
  const bool vt = mode == GNGF_MODE_VERTEX_TABLE;
  if (vt) GNGF_CHECK_ARG(vert_idx && vert_w && K > 0 && K <= GNGF_MAX_TOPK_WIDE && vstride > 0 && NV > 0 && NV * K < ((int64_t)1 << 31));
  const int tail = query_tail(xy, P, rgb, img);
  GNGF_CHECK_ARG(tail != 1);
  if (tail == 0) return (int)hipSuccess;
  RenderArgs a;
  a.tables = tables; a.vert_idx = vert_idx; a.vert_w = vert_w; a.n_ls = n_ls;
  a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
  a.rgb = rgb; a.img = img;
  int64_t nblocks;
  query_walk(a, P, nblocks);
  a.L = L; a.F = F; a.T = T; a.K = vt ? K : 0; a.vstride = vt ? vstride : 0; a.NV = vt ? NV : 0;
  a.out_dim = out_dim; a.pow2 = (T & (T - 1)) == 0;
  RenderQuery q;
  q.xy = xy; q.P = P;
  const int in_dim = L * F;
  const unsigned nwg = (unsigned)(nblocks < kQueryMaxGrid ? nblocks : kQueryMaxGrid);
  const size_t smem = sizeof(float) * (size_t)raw_offsets(in_dim).total;
  const bool f16 = feat_dtype == GNGF_FEAT_F16;
  const auto fn = mode == GNGF_MODE_DENSE_HASH ? query_pick_dtype<kSrcDenseHashQuery>(f16, in_dim, leaky != 0)
                  : vt                         ? query_pick_dtype<kSrcTableQuery>(f16, in_dim, leaky != 0)
                                               : query_pick_dtype<kSrcHashQuery>(f16, in_dim, leaky != 0);
  fn<<<dim3(nwg), dim3(kDecThreads), smem, as_stream(stream)>>>(a, q);
  GNGF_RETURN_LAUNCH();
}

// gngf_ext3_query from a baked vertex grid.  See include/gngf_ext3.h.
extern "C" int gngf_ext3_query_grid(const float* grid, const int32_t* n_ls, const int32_t* n_ls_host,
                                    const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                    int L, int F, int out_dim, int leaky,
                                    const float* xy, int64_t P, float* rgb, int32_t* img, void* stream) {
  GNGF_CHECK_ARG(L > 0 && L <= GNGF_MAX_LEVELS && (F == 1 || F == 2 || F == 4) && L * F <= 64);
  GNGF_CHECK_ARG(out_dim > 0 && out_dim <= 4);
  GNGF_CHECK_ARG(grid && n_ls && n_ls_host && W0 && b0 && W1 && b1 && W2 && b2);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(grid) & 15) == 0);
  const int tail = query_tail(xy, P, rgb, img);
  GNGF_CHECK_ARG(tail != 1);
  RenderQueryGrid q;
  q.xy = xy; q.P = P; q.grid = grid;
  int64_t vtot = 0;
  for (int l = 0; l < GNGF_MAX_LEVELS; ++l) {
    q.goff[l] = vtot;
    if (l < L) {
      GNGF_CHECK_ARG(n_ls_host[l] >= 0);
      vtot += (int64_t)(n_ls_host[l] + 2) * (n_ls_host[l] + 2);
    }
  }
  if (tail == 0) return (int)hipSuccess;
  RenderArgs a;
  a.tables = nullptr; a.vert_idx = nullptr; a.vert_w = nullptr; a.n_ls = n_ls;
  a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
  a.rgb = rgb; a.img = img;
  int64_t nblocks;
  query_walk(a, P, nblocks);
  a.L = L; a.F = F; a.T = 0; a.K = 0; a.vstride = 0; a.NV = 0;
  a.out_dim = out_dim; a.pow2 = false;
  const int in_dim = L * F;
  const unsigned nwg = (unsigned)(nblocks < kQueryMaxGrid ? nblocks : kQueryMaxGrid);
  const size_t smem = sizeof(float) * (size_t)raw_offsets(in_dim).total;
  const auto fn = query_pick_width<kSrcGridQuery, float>(in_dim, leaky != 0);
  fn<<<dim3(nwg), dim3(kDecThreads), smem, as_stream(stream)>>>(a, q);
  GNGF_RETURN_LAUNCH();
}
