// The flat segmented reduction of the vertex stage backward over a STATIC item list (frozen vertex table, no d w), shared by the
// translation units that instantiate it: encode_tiled.hip (vertex_bwd_flat_kernel: every run is ADDED to its row) and
// vertex_flat_owned.hip (vertex_bwd_flat_owned_kernel: a run that lies inside one workgroup is STORED).  Included inside
// namespace gngf, after gngf_common.h.
//
// Everything vertex_bwd_sorted_kernel resolves per step — order -> (vert_idx, vert_w) -> levels -> grid position, and where the
// equal-slot runs lie — is fixed between two table builds, so ops.vertex_flat_list resolves it once: one item per (level, vertex,
// k) = (gi: index into the vertex grid, w, dest: l * T + slot), sorted by dest.  The kernel is one flat segmented reduction: no
// level loop, no per-level barrier, one gather per item with all of a thread's gathers in flight together.
//   thread     kFlatIPT consecutive items (wide loads of gi / w / dest); runs that lie wholly inside it: one emit each
//   workgroup  the threads' open head / tail partials meet in ONE segmented scan (wave shuffles, then LDS across waves);
//              one emit per run that ends in, or crosses, the workgroup — no address gets more than one emit per workgroup
// The value of an item is formed exactly as vertex_bwd_sorted_kernel forms it (poison flag included).
// measured at the headline shape (2.87 M items, us per launch): 256 threads x 4 items 16.2 | 512 x 4: 16.3 | 128 x 4: 19.9 |
// 256 x 8: 19.7 | 128 x 8: 19.1; gathering a vertex's two 64-bit words in one 16-byte load instead of two 8-byte ones: 16.2 vs 16.4
// (no gain: not kept)
constexpr int kFlatTB = 256;       // threads per workgroup
constexpr int kFlatIPT = 4;        // items per thread (one 16-byte load per static array)
static_assert(kFlatIPT % 4 == 0 && kFlatTB % 64 == 0, "whole 16-byte loads, whole waves");

// the thread's kFlatIPT items, starting at i0
__device__ __forceinline__ void flat_load_items(const int32_t* __restrict__ item_gi, const float* __restrict__ item_w,
                                                const int32_t* __restrict__ item_dest, int64_t N, int64_t i0, int (&gi)[kFlatIPT],
                                                float (&w)[kFlatIPT], int (&d)[kFlatIPT]) {
  if (i0 + kFlatIPT <= N) {
#pragma unroll
    for (int c = 0; c < kFlatIPT; c += 4) {
      const int4 g4 = *reinterpret_cast<const int4*>(item_gi + i0 + c);
      const float4 w4 = *reinterpret_cast<const float4*>(item_w + i0 + c);
      const int4 d4 = *reinterpret_cast<const int4*>(item_dest + i0 + c);
      gi[c] = g4.x; gi[c + 1] = g4.y; gi[c + 2] = g4.z; gi[c + 3] = g4.w;
      w[c] = w4.x; w[c + 1] = w4.y; w[c + 2] = w4.z; w[c + 3] = w4.w;
      d[c] = d4.x; d[c + 1] = d4.y; d[c + 2] = d4.z; d[c + 3] = d4.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kFlatIPT; ++i) {                     // the ragged end; items past it: dest -1, which is never emitted
      const bool on = i0 + i < N;
      gi[i] = on ? item_gi[i0 + i] : 0;
      w[i] = on ? item_w[i0 + i] : 0.f;
      d[i] = on ? item_dest[i0 + i] : -1;
    }
  }
}

// the items' values: every gather of the thread is issued before the first one is used.  (The list is checked on the host when
// it is built; the clamp keeps a list that was not from reading outside the grid.)
template <int F, bool FROM64>
__device__ __forceinline__ void flat_item_values(const int (&gi)[kFlatIPT], const float (&w)[kFlatIPT], const float* __restrict__ dG,
                                                 const unsigned long long* __restrict__ dG64, int64_t vtot, float (&v)[kFlatIPT][F]) {
  if constexpr (FROM64) {
    unsigned long long q[kFlatIPT][F];
#pragma unroll
    for (int i = 0; i < kFlatIPT; ++i) {
      const int64_t g = gi[i] < 0 ? 0 : (gi[i] < vtot ? gi[i] : vtot - 1);
#pragma unroll
      for (int f = 0; f < F; ++f) q[i][f] = dG64[g * F + f];
    }
    const double inv64 = ldexp(1.0, -(int)(long long)dG64[vtot * F]);
    const bool poisoned = dG64[vtot * F + 1] != 0ull;
#pragma unroll
    for (int i = 0; i < kFlatIPT; ++i)
#pragma unroll
      for (int f = 0; f < F; ++f)
        v[i][f] = (poisoned ? __int_as_float(0x7fc00000) : (float)((double)(long long)q[i][f] * inv64)) * w[i];   // as vertex_bwd_sorted_kernel
  } else {
    float q[kFlatIPT][F];
#pragma unroll
    for (int i = 0; i < kFlatIPT; ++i) {
      const int64_t g = gi[i] < 0 ? 0 : (gi[i] < vtot ? gi[i] : vtot - 1);
#pragma unroll
      for (int f = 0; f < F; ++f) q[i][f] = dG[g * F + f];
    }
#pragma unroll
    for (int i = 0; i < kFlatIPT; ++i)
#pragma unroll
      for (int f = 0; f < F; ++f) v[i][f] = q[i][f] * w[i];
  }
}

// The workgroup's segmented reduction of (d, v): emit(dest, sum) is called exactly once per run of equal dest that touches the
// workgroup, with the sum of the run's items inside it (always combined in the same order).
template <int F, class Emit>
__device__ __forceinline__ void flat_segmented_reduce(const int (&d)[kFlatIPT], const float (&v)[kFlatIPT][F], Emit emit) {
  constexpr int NW = kFlatTB / 64;
  __shared__ int s_firstd[kFlatTB], s_lastd[kFlatTB];
  __shared__ float s_y[kFlatTB][F];
  __shared__ float s_wtot[NW][F];
  __shared__ int s_wflag[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the thread's own runs: the first one (head) and the last one (tail, = the head when there is no boundary inside the
  // thread) stay open; the ones in between are complete
  float acc[F], head[F];
  int nb = 0;
#pragma unroll
  for (int f = 0; f < F; ++f) { acc[f] = v[0][f]; head[f] = 0.f; }
#pragma unroll
  for (int i = 1; i < kFlatIPT; ++i) {
    if (d[i] != d[i - 1]) {
      if (nb == 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) head[f] = acc[f];
      } else {
        emit(d[i - 1], acc);
      }
      ++nb;
#pragma unroll
      for (int f = 0; f < F; ++f) acc[f] = v[i][f];
    } else {
#pragma unroll
      for (int f = 0; f < F; ++f) acc[f] += v[i][f];
    }
  }
  s_firstd[tid] = d[0];
  s_lastd[tid] = d[kFlatIPT - 1];
  __syncthreads();
  const int prev_d = tid > 0 ? s_lastd[tid - 1] : -2;                   // (-2: equal to no dest, not even a dead item's)
  const int next_d = tid + 1 < kFlatTB ? s_firstd[tid + 1] : -2;
  // inclusive segmented scan of the tail partials over the workgroup's threads; a thread STARTS a segment when its tail run
  // begins inside it, or at its first item
  const int starts = (nb > 0 || prev_d != d[0]) ? 1 : 0;
  float y[F];
  int flag = starts;
#pragma unroll
  for (int f = 0; f < F; ++f) y[f] = acc[f];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int fu = __shfl_up(flag, o, 64);
    float yu[F];
#pragma unroll
    for (int f = 0; f < F; ++f) yu[f] = __shfl_up(y[f], o, 64);
    if (lane >= o) {
      if (!flag) {
#pragma unroll
        for (int f = 0; f < F; ++f) y[f] += yu[f];
      }
      flag |= fu;
    }
  }
  if (lane == 63) {                                                      // the wave's open tail, and whether a segment starts in it
#pragma unroll
    for (int f = 0; f < F; ++f) s_wtot[wave][f] = y[f];
    s_wflag[wave] = flag;
  }
  __syncthreads();
  if (!flag) {                                                           // no segment has started in this wave up to this lane: the
    for (int q = wave - 1; q >= 0; --q) {                                // run comes in from the waves below
#pragma unroll
      for (int f = 0; f < F; ++f) y[f] += s_wtot[q][f];
      if (s_wflag[q]) break;
    }
  }
#pragma unroll
  for (int f = 0; f < F; ++f) s_y[tid][f] = y[f];
  __syncthreads();
  if (nb > 0) {                                                          // my head run ends inside me
    if (tid > 0 && prev_d == d[0]) {
#pragma unroll
      for (int f = 0; f < F; ++f) head[f] += s_y[tid - 1][f];
    }
    emit(d[0], head);
  }
  if (next_d != d[kFlatIPT - 1]) emit(d[kFlatIPT - 1], y);               // my tail run ends with me (or leaves the workgroup)
}
