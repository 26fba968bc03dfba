// Vertex stage backward over the static item list of a frozen vertex table, the form that OWNS its rows
// (include/gngf_ext3.h: gngf_ext3_vertex_grid_bwd_flat_owned).  A translation unit of its own: new instantiations emitted in
// front of the training step's kernels have cost that step 1 % before.
//
// With a frozen table the rows of the table gradient that can ever receive a value are the dest values of the list, the same
// every step.  vertex_bwd_flat_kernel adds every run to a row somebody zeroed — the whole (L, T, F) buffer, every step.  Here a
// run that lies wholly inside one workgroup's kFlatTB * kFlatIPT items is STORED: the row needs no clear, last step's value is
// overwritten (a zero sum too).  A run that enters or leaves the workgroup is still added with an atomic, to a row the caller
// zeroed: at most one row per boundary between two workgroups (ops.vertex_flat_list lists them; rider workgroups of the
// pixel-stage backward's launch clear them).  No workgroup waits for another.
#include "gngf_common.h"
#include "../../include/gngf_ext3.h"

namespace gngf {

#include "vertex_flat.inc"

template <int F>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float* s) {
  // 0.f + s: a -0.0 sum is stored as the +0.0 that adding it to a zeroed row leaves (not folded away: x + 0.0 is not x for -0.0)
  if constexpr (F == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(0.f + s[0], 0.f + s[1]);
  } else if constexpr (F % 4 == 0) {
#pragma unroll
    for (int f = 0; f < F; f += 4)
      *reinterpret_cast<float4*>(p + f) = make_float4(0.f + s[f], 0.f + s[f + 1], 0.f + s[f + 2], 0.f + s[f + 3]);
  } else {
#pragma unroll
    for (int f = 0; f < F; ++f) p[f] = 0.f + s[f];
  }
}

template <int F, bool FROM64>
__global__ void __launch_bounds__(kFlatTB)
vertex_bwd_flat_owned_kernel(const int32_t* __restrict__ item_gi, const float* __restrict__ item_w, const int32_t* __restrict__ item_dest,
                             int64_t N, const float* __restrict__ dG, const unsigned long long* __restrict__ dG64, int64_t vtot,
                             float* __restrict__ dtables, int64_t rows) {
  const int64_t first = (int64_t)blockIdx.x * kFlatTB * kFlatIPT;
  const int64_t end = first + kFlatTB * kFlatIPT;
  const int64_t i0 = first + (int64_t)threadIdx.x * kFlatIPT;
  int gi[kFlatIPT], d[kFlatIPT];
  float w[kFlatIPT];
  flat_load_items(item_gi, item_w, item_dest, N, i0, gi, w, d);
  // the dest just outside the workgroup's items on either side: a run with one of them crosses the boundary (-2: no such item)
  const int d_before = first > 0 ? item_dest[first - 1] : -2;
  const int d_after = end < N ? item_dest[end] : -2;
  float v[kFlatIPT][F];
  flat_item_values<F, FROM64>(gi, w, dG, dG64, vtot, v);
  flat_segmented_reduce<F>(d, v, [&](int dest, const float* s) {
    if ((uint64_t)(int64_t)dest < (uint64_t)rows) {          // (dest -1: items past the end of the list)
      float* p = dtables + (int64_t)dest * F;
      if (dest == d_before || dest == d_after) {             // shared with a neighbouring workgroup: added, to a row cleared before
#pragma unroll
        for (int f = 0; f < F; ++f)
          if (s[f] != 0.f) atomicAdd(p + f, s[f]);
      } else {
        store_row<F>(p, s);                                  // mine alone: written, whatever the row held
      }
    }
  });
}

}  // namespace gngf

using namespace gngf;

extern "C" int gngf_ext3_vertex_grid_bwd_flat_owned(const int32_t* item_gi, const float* item_w, const int32_t* item_dest, int64_t N,
                                                    const float* dG, const void* dG64, int64_t vtot, float* dtables, int64_t rows,
                                                    int F, void* stream) {
  GNGF_CHECK_ARG(item_gi && item_w && item_dest && N > 0 && N < (1ll << 31) && (dG || dG64) && vtot > 0 && dtables);
  GNGF_CHECK_ARG(rows > 0 && rows < (1ll << 31));
  GNGF_CHECK_ARG(((reinterpret_cast<uintptr_t>(item_gi) | reinterpret_cast<uintptr_t>(item_w) | reinterpret_cast<uintptr_t>(item_dest)) & 15) == 0);
  GNGF_CHECK_ARG(F == 1 || F == 2 || F == 4 || F == 8);
  GNGF_CHECK_ARG((reinterpret_cast<uintptr_t>(dtables) & (uintptr_t)((F >= 4 ? 16 : 4 * F) - 1)) == 0);
  const dim3 grid((unsigned)ceil_div(N, (int64_t)kFlatTB * kFlatIPT)), block(kFlatTB);
#define GNGF_OWNED_LAUNCH(kF, FROM64)                                                                     \
  vertex_bwd_flat_owned_kernel<kF, FROM64><<<grid, block, 0, as_stream(stream)>>>(                         \
      item_gi, item_w, item_dest, N, dG64 ? nullptr : dG, static_cast<const unsigned long long*>(dG64), vtot, dtables, rows)
  switch (F) {
    case 1: if (dG64) GNGF_OWNED_LAUNCH(1, true); else GNGF_OWNED_LAUNCH(1, false); break;
    case 2: if (dG64) GNGF_OWNED_LAUNCH(2, true); else GNGF_OWNED_LAUNCH(2, false); break;
    case 4: if (dG64) GNGF_OWNED_LAUNCH(4, true); else GNGF_OWNED_LAUNCH(4, false); break;
    default: if (dG64) GNGF_OWNED_LAUNCH(8, true); else GNGF_OWNED_LAUNCH(8, false); break;
  }
#undef GNGF_OWNED_LAUNCH
  GNGF_RETURN_LAUNCH();
}
