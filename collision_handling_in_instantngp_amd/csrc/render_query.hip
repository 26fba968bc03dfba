// The query forms of the render kernel (render.inc: the kSrc*Query sources, whose coordinates are read from memory and whose sink
// is a row per point) and the entry points of include/gngf_ext3.h.  A translation unit of its own, as render_score.hip: the query
// forms add as many instantiations as the storing forms have, and here they compile next to decoder.hip instead of behind it.
// The model checks, the picker and the launch are render.inc's host section, shared with the other forms; this file holds what
// only a query has — the checks of xy, P and the outputs (query_tail) and the one-row walk (query_walk).  GNGF_RENDER_KERNELS_ONLY
// leaves out nothing but the definitions of gngf_render and gngf_render_grid, which belong to decoder.hip.
#include "gngf_common.h"
#include "../../include/gngf_ext3.h"
#include <type_traits>
#include "decoder_common.inc"
#define GNGF_RENDER_KERNELS_ONLY
#include "render.inc"

namespace gngf {

// the tail of both entry points: 0 = nothing to launch (P = 0), 1 = rejected, 2 = launch
static int query_tail(const float* xy, int64_t P, const float* rgb, const int32_t* img) {
  if (P < 0 || !(rgb || img) || (P > 0 && !xy)) return 1;
  if ((reinterpret_cast<uintptr_t>(xy) & 7) != 0) return 1;
  if ((reinterpret_cast<uintptr_t>(rgb) & 3) != 0 || (reinterpret_cast<uintptr_t>(img) & 3) != 0) return 1;
  return P == 0 ? 0 : 2;
}

// the sink, and the walk of the lattice forms over ceil(P / 128) blocks: one row of blocks, block column = block (render.inc).
// Returns the number of blocks
static int64_t query_walk(RenderArgs& a, float* rgb, int32_t* img, int64_t P) {
  const int64_t nblocks = (P + kQueryBlock - 1) / kQueryBlock;
  a.rgb = rgb; a.img = img;
  a.rows = kRenderRows; a.cols = nblocks * kRenderCols; a.r0 = 0; a.c0 = 0; a.denom = 1.f;
  return nblocks;
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext3_version(void) { return GNGF_EXT3_VERSION; }

// rgb / img (P, out_dim) of the model at the coordinates xy (P, 2).  See include/gngf_ext3.h.
extern "C" int gngf_ext3_query(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                               const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                               int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky,
                               const float* xy, int64_t P, float* rgb, int32_t* img, void* stream) {
  const int tail = query_tail(xy, P, rgb, img);
  GNGF_CHECK_ARG(tail != 1);
  RenderArgs a;
  GNGF_CHECK_ARG(render_table_model(a, tables, feat_dtype, vert_idx, vert_w, n_ls, W0, b0, W1, b1, W2, b2, L, F, T, K, mode, vstride, NV, out_dim));
  if (tail == 0) return (int)hipSuccess;                  // (the model is checked even for P = 0)
  RenderQuery q;
  q.xy = xy; q.P = P;
  const int64_t nblocks = query_walk(a, rgb, img, P);
  render_launch(render_pick_mode<kSrcQuery>(mode, feat_dtype, L * F, leaky != 0), a, q, nblocks, as_stream(stream));
  GNGF_RETURN_LAUNCH();
}

// gngf_ext3_query from a baked vertex grid.  See include/gngf_ext3.h.
extern "C" int gngf_ext3_query_grid(const float* grid, const int32_t* n_ls, const int32_t* n_ls_host,
                                    const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                    int L, int F, int out_dim, int leaky,
                                    const float* xy, int64_t P, float* rgb, int32_t* img, void* stream) {
  const int tail = query_tail(xy, P, rgb, img);
  GNGF_CHECK_ARG(tail != 1);
  RenderArgs a;
  RenderQueryGrid q;
  q.xy = xy; q.P = P; q.grid = grid;
  GNGF_CHECK_ARG(render_grid_model(a, q.goff, grid, n_ls, n_ls_host, W0, b0, W1, b1, W2, b2, L, F, out_dim));
  if (tail == 0) return (int)hipSuccess;                  // (the model, its host resolutions included, is checked even for P = 0)
  const int64_t nblocks = query_walk(a, rgb, img, P);
  render_launch(render_pick<kSrcGridQuery, float>(L * F, leaky != 0), a, q, nblocks, as_stream(stream));
  GNGF_RETURN_LAUNCH();
}
