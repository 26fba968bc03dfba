// The wide-K path: K in (GNGF_MAX_TOPK, GNGF_MAX_TOPK_WIDE] = 33 .. 128.  hpd.hip's selection kernels keep a sorted K-list per
// thread in LDS (2 K 256 4 B: 64 KiB at K = 32, 256 KiB at K = 128 — a CU has 160 KiB) and its blend kernels hold K-sized arrays
// per thread; neither scales, so K > 32 runs the kernels of this file and every K <= 32 call runs what it ran before.
//
// Selection (one 256-thread block per row, 38,528 B of static LDS: 4 workgroups per CU):
//   * every value becomes an order-preserving 32-bit key (larger float <-> larger unsigned; NaN -> 0, below -inf; -0 -> +0);
//   * T <= 8192: the row's keys are staged in LDS and the K best are selected among them;
//   * larger T: the pass over the row (the ONLY read of the logits, whatever K is) leaves one key per 64-column block, its maximum;
//     the K largest of a row lie in the K blocks that come first by (maximum desc, block asc) [if a top-K element e sat in another
//     block b, K blocks would each hold an element that beats e: one above max(b) >= e, or one equal to max(b) at a lower index];
//     those K x 64 candidates (32 KiB at K = 128, re-read from L2) replace the maxima in LDS and the K best are selected among them;
//     rows longer than 8192 x 64 = 2^19 are walked in tiles of that length, each tile's winners merged into the running K;
//   * "select the Kt best of n keys in LDS" is a 4 x 8-bit radix select (LDS histogram, descending scan) that yields the Kt-th key
//     and how many of its equals belong to the winners, followed by an ORDERED compaction (ballot prefix sums, position order), so
//     that among equal keys the lower index wins;
//   * the <= 2 K winners are ranked by (key desc, index asc) — a total order: every index is a real column of the row, in [0, T).
#include "gngf_common.h"
#include <limits.h>

namespace gngf {

constexpr int kWideBlock = 256;
constexpr int kWideSlots = 8192;                                  // key slots in LDS
constexpr int64_t kWideTile = (int64_t)kWideSlots * 64;           // columns per tile of the block-maxima form

struct WideSmem {
  alignas(16) uint32_t keys[kWideSlots];     // the row's keys | block maxima, then the candidates
  uint32_t hist[256];
  uint32_t wkey[2][2 * GNGF_MAX_TOPK_WIDE];  // winners (running K, then this tile's), double-buffered for the rank merge
  int widx[2][2 * GNGF_MAX_TOPK_WIDE];
  int cand[GNGF_MAX_TOPK_WIDE];              // candidate blocks of the tile, ascending
  uint32_t wtot[4][2];
  uint32_t scanw[4];
  uint32_t sel[2];
  float red[8];
  int redi[8];
};

__device__ __forceinline__ uint32_t wide_key(float v) {
  if (v != v) return 0u;
  if (v == 0.f) v = 0.f;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wide_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wide_wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax32(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wide_wave_usum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ float wide_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wide_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The Kt best of sm.keys[0 .. n) by (key desc, position asc), 1 <= Kt <= n <= kWideSlots: out(j, position, key) is called once per
// winner, j = 0 .. Kt-1 in POSITION order.  Called by the whole block, uniformly; ends on a barrier.
template <class Out>
__device__ __forceinline__ void wide_select(WideSmem& sm, int n, int Kt, Out&& out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0u, mask = 0u, remaining = (uint32_t)Kt;
  for (int shift = 24; shift >= 0; shift -= 8) {
    sm.hist[tid] = 0u;
    __syncthreads();
    for (int e = tid; e < n; e += kWideBlock) {
      const uint32_t k = sm.keys[e];
      if ((k & mask) == prefix) atomicAdd(&sm.hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = sm.hist[255 - tid];                       // descending digits: thread 0 owns digit 255
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) sm.scanw[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += sm.scanw[w];
    const uint32_t excl = incl - c;
    if (excl < remaining && remaining <= incl) { sm.sel[0] = (uint32_t)(255 - tid); sm.sel[1] = remaining - excl; }
    __syncthreads();
    prefix |= sm.sel[0] << shift;
    mask |= 0xffu << shift;
    remaining = sm.sel[1];
  }
  const uint32_t thr = prefix, need = remaining;                  // the Kt-th key; `need` of its equals are winners (>= 1)
  // ordered compaction: a wave owns a contiguous range of positions
  const int seg = ((n + kWideBlock - 1) / kWideBlock) * 64;
  const int s0 = wave * seg < n ? wave * seg : n;
  const int s1 = s0 + seg < n ? s0 + seg : n;
  uint32_t cg = 0u, ce = 0u;
  for (int e = s0 + lane; e < s1; e += 64) { const uint32_t k = sm.keys[e]; cg += k > thr; ce += k == thr; }
  cg = wide_wave_usum(cg);
  ce = wide_wave_usum(ce);
  if (lane == 0) { sm.wtot[wave][0] = cg; sm.wtot[wave][1] = ce; }
  __syncthreads();
  uint32_t gt_before = 0u, eq_before = 0u;
  for (int w = 0; w < wave; ++w) { gt_before += sm.wtot[w][0]; eq_before += sm.wtot[w][1]; }
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int e0 = s0; e0 < s1; e0 += 64) {                          // (uniform per wave)
    const int e = e0 + lane;
    const bool valid = e < s1;
    const uint32_t k = valid ? sm.keys[e] : 0u;
    const bool g = valid && k > thr, q = valid && k == thr;
    const unsigned long long mg = __ballot(g), me = __ballot(q);
    const uint32_t eqb = eq_before + (uint32_t)__popcll(me & lt);
    if (g || (q && eqb < need)) out((int)(gt_before + (uint32_t)__popcll(mg & lt) + (eqb < need ? eqb : need)), e, k);
    gt_before += (uint32_t)__popcll(mg);
    eq_before += (uint32_t)__popcll(me);
  }
  __syncthreads();
}

enum { WIDE_SOFTMAX = 0, WIDE_LOGITS = 1, WIDE_RAW = 2 };

// WIDE_SOFTMAX: z logits in, probabilities out (in place); the max and sum passes are softmax_topk_kernel's, statement for
//               statement, so the probabilities do not depend on which of the two kernels K selects; top-K on the probabilities.
// WIDE_LOGITS:  z only read; online (max, sum) as logits_stats_topk_kernel; top-K on the logits, probabilities expf(z - M) / S.
// WIDE_RAW:     top-K of the rows as they are (DifferentiableTopk); z only read.
template <int MODE>
__global__ void __launch_bounds__(kWideBlock)
wide_topk_kernel(float* __restrict__ z, float* __restrict__ topv, int32_t* __restrict__ topi, float* __restrict__ rowstat, int64_t T,
                 int K) {
  __shared__ WideSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* p = z + (int64_t)blockIdx.x * T;
  const bool direct = T <= kWideSlots;
  float m = -INFINITY, s = (MODE == WIDE_LOGITS) ? 0.f : 1.f;
  bool row_nan = false, has_nan = false;
  if (MODE == WIDE_SOFTMAX) {
    for (int64_t t = tid; t < T; t += kWideBlock) { const float v = p[t]; has_nan |= (v != v); m = fmaxf(m, v); }
    m = wide_wave_max(m);
    const unsigned long long nanmask = __ballot(has_nan);
    if (lane == 0) { sm.red[wave] = m; sm.redi[wave] = nanmask != 0ull; }
    __syncthreads();
    m = fmaxf(fmaxf(sm.red[0], sm.red[1]), fmaxf(sm.red[2], sm.red[3]));
    row_nan = (sm.redi[0] | sm.redi[1] | sm.redi[2] | sm.redi[3]) != 0;
    __syncthreads();
    s = 0.f;
    for (int64_t t = tid; t < T; t += kWideBlock) s += expf(p[t] - m);
    s = wide_wave_sum(s);
    if (lane == 0) sm.red[wave] = s;
    __syncthreads();
    s = (sm.red[0] + sm.red[1]) + (sm.red[2] + sm.red[3]);
    __syncthreads();
    if (rowstat && tid == 0) {
      rowstat[2 * (int64_t)blockIdx.x] = m;
      rowstat[2 * (int64_t)blockIdx.x + 1] = row_nan ? __int_as_float(0x7fc00000) : s;
    }
  }
  constexpr float kLog2e = 1.4426950408889634f;
  const bool vec = (MODE == WIDE_LOGITS) && (T % 4 == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  int nrun = 0, cur = 0;
  const int64_t tile_len = direct ? T : kWideTile;
  for (int64_t tile0 = 0; tile0 < T; tile0 += tile_len) {
    const int64_t tend = tile0 + tile_len < T ? tile0 + tile_len : T;
    const int n = (int)(tend - tile0);
    const int nb = (n + 63) >> 6;
    // ---- the pass over the tile: keys (direct) or block maxima into LDS
    if (vec) {
      for (int64_t base = tile0; base < tend; base += (int64_t)kWideBlock * 8) {       // (uniform trip count: the shuffles below)
        const int64_t t0 = base + (int64_t)tid * 4, t1 = t0 + (int64_t)kWideBlock * 4;
        const bool ok0 = t0 < tend, ok1 = t1 < tend;
        const float4 ninf = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        const float4 a = ok0 ? *reinterpret_cast<const float4*>(p + t0) : ninf;
        const float4 b = ok1 ? *reinterpret_cast<const float4*>(p + t1) : ninf;
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float mx = m;
#pragma unroll
        for (int q = 0; q < 8; ++q) { has_nan |= (v[q] != v[q]); mx = fmaxf(mx, v[q]); }
        if (mx > m) { s = (m == -INFINITY) ? 0.f : s * __builtin_amdgcn_exp2f((m - mx) * kLog2e); m = mx; }
        if (m > -INFINITY) {
#pragma unroll
          for (int q = 0; q < 8; ++q) s += __builtin_amdgcn_exp2f((v[q] - m) * kLog2e);   // exp2(-inf) = 0 for the padding
        }
        uint32_t k[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) k[q] = wide_key(v[q]);
        if (direct) {
          if (ok0) *reinterpret_cast<uint4*>(&sm.keys[t0 - tile0]) = make_uint4(k[0], k[1], k[2], k[3]);
          if (ok1) *reinterpret_cast<uint4*>(&sm.keys[t1 - tile0]) = make_uint4(k[4], k[5], k[6], k[7]);
        } else {
          uint32_t ka = ok0 ? umax32(umax32(k[0], k[1]), umax32(k[2], k[3])) : 0u;
          uint32_t kb = ok1 ? umax32(umax32(k[4], k[5]), umax32(k[6], k[7])) : 0u;
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {                      // 16 lanes x 4 columns = one 64-column block
            ka = umax32(ka, (uint32_t)__shfl_xor((int)ka, o, 64));
            kb = umax32(kb, (uint32_t)__shfl_xor((int)kb, o, 64));
          }
          if ((lane & 15) == 0) {
            if (ok0) sm.keys[(t0 - tile0) >> 6] = ka;
            if (ok1) sm.keys[(t1 - tile0) >> 6] = kb;
          }
        }
      }
    } else {
      for (int b = wave; b < nb; b += 4) {                        // a wave per 64-column block (uniform per wave)
        const int64_t t = tile0 + (int64_t)b * 64 + lane;
        const bool valid = t < tend;
        float q = valid ? p[t] : 0.f;
        if (MODE == WIDE_SOFTMAX && valid) {
          q = expf(q - m) / s;
          if (row_nan || q != q) q = 0.f;                         // nan_to_num (models.py:111)
          else if (q > 3.4028234663852886e38f) q = 3.4028234663852886e38f;
          p[t] = q;
        }
        if (MODE == WIDE_LOGITS && valid) {
          has_nan |= (q != q);
          if (q > m) { s = s * expf(m - q) + 1.f; m = q; }        // first element: s = 0 * exp(-inf) + 1
          else if (q > -INFINITY) s += expf(q - m);               // (-inf before any finite value: exp(-inf + inf) is NaN)
        }
        uint32_t k = valid ? wide_key(q) : 0u;
        if (direct) {
          if (valid) sm.keys[b * 64 + lane] = k;
        } else {
          k = wide_wave_umax(k);
          if (lane == 0) sm.keys[b] = k;
        }
      }
    }
    __syncthreads();
    // ---- block maxima -> candidate blocks -> candidate keys
    int npos = n, nvalid = n;
    if (!direct) {
      const int Kb = K < nb ? K : nb;
      wide_select(sm, nb, Kb, [&](int j, int pos, uint32_t) { sm.cand[j] = pos; });
      npos = Kb * 64;
      nvalid = (sm.cand[Kb - 1] == nb - 1) ? npos - (nb * 64 - n) : npos;
      __syncthreads();                                            // (cand[] read above; keys[] is rewritten below)
      for (int e = tid; e < npos; e += kWideBlock) {
        const int64_t t = tile0 + (int64_t)sm.cand[e >> 6] * 64 + (e & 63);
        sm.keys[e] = t < tend ? wide_key(p[t]) : 0u;              // (WIDE_SOFTMAX: the probabilities this block has just written)
      }
      __syncthreads();
    }
    // ---- this tile's winners behind the running ones, then the rank merge
    const int Kt = K < nvalid ? K : nvalid;
    wide_select(sm, npos, Kt, [&](int j, int pos, uint32_t k) {
      sm.wkey[cur][nrun + j] = k;
      sm.widx[cur][nrun + j] = (int)(direct ? tile0 + pos : tile0 + (int64_t)sm.cand[pos >> 6] * 64 + (pos & 63));
    });
    const int total = nrun + Kt;                                  // <= 2 K <= 256
    if (tid < total) {
      const uint32_t mk = sm.wkey[cur][tid];
      const int mi = sm.widx[cur][tid];
      int rank = 0;
      for (int j = 0; j < total; ++j) {
        const uint32_t kj = sm.wkey[cur][j];
        rank += (kj > mk) || (kj == mk && sm.widx[cur][j] < mi);
      }
      if (rank < K) { sm.wkey[cur ^ 1][rank] = mk; sm.widx[cur ^ 1][rank] = mi; }
    }
    cur ^= 1;
    nrun = total < K ? total : K;
    __syncthreads();
  }
  // ---- the row's statistics (streaming form) and the K outputs
  float M = m, S = s;
  if (MODE == WIDE_LOGITS) {
    const float wm = wide_wave_max(m);
    const unsigned long long nanmask = __ballot(has_nan);
    if (lane == 0) { sm.red[wave] = wm; sm.redi[wave] = nanmask != 0ull; }
    __syncthreads();
    M = fmaxf(fmaxf(sm.red[0], sm.red[1]), fmaxf(sm.red[2], sm.red[3]));
    row_nan = (sm.redi[0] | sm.redi[1] | sm.redi[2] | sm.redi[3]) != 0;
    __syncthreads();
    float sc = (m == -INFINITY) ? 0.f : s * expf(m - M);
    sc = wide_wave_sum(sc);
    if (lane == 0) sm.red[wave] = sc;
    __syncthreads();
    S = (sm.red[0] + sm.red[1]) + (sm.red[2] + sm.red[3]);
    if (tid == 0) {
      rowstat[2 * (int64_t)blockIdx.x] = M;
      rowstat[2 * (int64_t)blockIdx.x + 1] = row_nan ? __int_as_float(0x7fc00000) : S;
    }
  }
  if (tid < K && tid < nrun) {
    float v = wide_unkey(sm.wkey[cur][tid]);
    int idx = sm.widx[cur][tid];
    if (MODE == WIDE_LOGITS) {
      v = expf(v - M) / S;
      if (row_nan || v != v) v = 0.f;                             // nan_to_num (models.py:111)
      else if (v > 3.4028234663852886e38f) v = 3.4028234663852886e38f;
      if (row_nan) idx = tid;                                     // a NaN row is all zeros after nan_to_num: slots 0..K-1
    }
    topv[(int64_t)blockIdx.x * K + tid] = v;
    topi[(int64_t)blockIdx.x * K + tid] = idx;
  }
}

// mode: 0 in-place softmax + top-K (gngf_softmax_topk), 1 streaming statistics + top-K (gngf_logits_topk_pbar), 2 raw rows (gngf_topk).
// The callers have checked the arguments; K in (GNGF_MAX_TOPK, GNGF_MAX_TOPK_WIDE], K <= T < INT_MAX.
int wide_topk_launch(int mode, float* z, float* topv, int32_t* topi, float* rowstat, int64_t U, int64_t T, int K, hipStream_t s) {
  GNGF_CHECK_ARG(K > GNGF_MAX_TOPK && K <= GNGF_MAX_TOPK_WIDE && K <= T && T < INT_MAX && U > 0 && mode >= 0 && mode <= 2);
  const dim3 grid((unsigned)U), block(kWideBlock);
  if (mode == WIDE_SOFTMAX) wide_topk_kernel<WIDE_SOFTMAX><<<grid, block, 0, s>>>(z, topv, topi, rowstat, T, K);
  else if (mode == WIDE_LOGITS) wide_topk_kernel<WIDE_LOGITS><<<grid, block, 0, s>>>(z, topv, topi, rowstat, T, K);
  else wide_topk_kernel<WIDE_RAW><<<grid, block, 0, s>>>(z, topv, topi, rowstat, T, K);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- blend, K > GNGF_MAX_TOPK
// One wave per vertex row, two values per lane (k = lane, lane + 64): blend_w's arithmetic (expf, division by the sum) without a
// per-thread K-array.  The sums are wave reductions, so their rounding order differs from blend_w's serial loop.
__device__ __forceinline__ void wide_blend_w(float q0, float q1, bool h0, bool h1, int blend, float& w0, float& w1) {
  if (blend == GNGF_BLEND_RAW) { w0 = q0; w1 = q1; return; }
  if (blend == GNGF_BLEND_SOFTMAX) {
    const float m = wide_wave_max(fmaxf(h0 ? q0 : -INFINITY, h1 ? q1 : -INFINITY));
    const float e0 = h0 ? expf(q0 - m) : 0.f, e1 = h1 ? expf(q1 - m) : 0.f;
    const float s = wide_wave_sum(e0 + e1);
    w0 = e0 / s; w1 = e1 / s;
    return;
  }
  const float s = wide_wave_sum((h0 ? q0 : 0.f) + (h1 ? q1 : 0.f));
  w0 = q0 / s; w1 = q1 / s;
}

__global__ void __launch_bounds__(256)
wide_blend_fwd_kernel(const float* __restrict__ q, float* __restrict__ w, int64_t U, int K, int blend) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= U) return;                                              // (uniform per wave)
  const bool h0 = lane < K, h1 = lane + 64 < K;
  const float q0 = h0 ? q[u * K + lane] : 0.f, q1 = h1 ? q[u * K + lane + 64] : 0.f;
  float w0, w1;
  wide_blend_w(q0, q1, h0, h1, blend, w0, w1);
  if (h0) w[u * K + lane] = w0;
  if (h1) w[u * K + lane + 64] = w1;
}

__global__ void __launch_bounds__(256)
wide_blend_bwd_kernel(const float* __restrict__ q, const float* __restrict__ dw, float* __restrict__ dq, int64_t U, int K, int blend) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= U) return;
  const bool h0 = lane < K, h1 = lane + 64 < K;
  const float q0 = h0 ? q[u * K + lane] : 0.f, q1 = h1 ? q[u * K + lane + 64] : 0.f;
  float d0 = h0 ? dw[u * K + lane] : 0.f, d1 = h1 ? dw[u * K + lane + 64] : 0.f;
  if (blend == GNGF_BLEND_SOFTMAX) {
    float w0, w1;
    wide_blend_w(q0, q1, h0, h1, blend, w0, w1);
    const float dot = wide_wave_sum(w0 * d0 + w1 * d1);
    d0 = w0 * (d0 - dot); d1 = w1 * (d1 - dot);
  } else if (blend == GNGF_BLEND_NORM) {
    const float s = wide_wave_sum(q0 + q1), dqs = wide_wave_sum(d0 * q0 + d1 * q1);
    const float inv = 1.0f / s;
    d0 = d0 * inv - dqs * inv * inv; d1 = d1 * inv - dqs * inv * inv;
  }
  if (h0) dq[u * K + lane] = d0;
  if (h1) dq[u * K + lane + 64] = d1;
}

int wide_blend_launch(bool bwd, const float* q, const float* dw, float* out, int64_t U, int K, int blend, hipStream_t s) {
  GNGF_CHECK_ARG(K > GNGF_MAX_TOPK && K <= GNGF_MAX_TOPK_WIDE && U > 0);
  const dim3 grid((unsigned)ceil_div(U, 4)), block(256);
  if (bwd) wide_blend_bwd_kernel<<<grid, block, 0, s>>>(q, dw, out, U, K, blend);
  else wide_blend_fwd_kernel<<<grid, block, 0, s>>>(q, out, U, K, blend);
  return (int)hipGetLastError();
}

}  // namespace gngf
