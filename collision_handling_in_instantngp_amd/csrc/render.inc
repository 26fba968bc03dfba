// Forward-only render of a pixel lattice in ONE launch (included at the end of decoder.hip, and by render_score.hip and
// render_query.hip for the scoring and query forms: it needs decoder_common.inc — stage_raw / raw_offsets, crow / kmapC, the MFMA
// macro — and repeats the 4x4x1 output layer of decoder_fwd_kernel with its sigmoid).  Below the kernel: the host side every
// entry point shares — the model checks, the picker, the launch — and decoder.hip's own two entry points.
//
// decoder_fwd_kernel with its input produced in place: a lane owns one pixel of the lattice (col = lane & 31 of the transposed
// products), computes the pixel's coordinate from its row and column — ((float)(r0 + r) / denom, (float)(c0 + c) / denom), one
// correctly rounded fp32 division per axis, no coordinate tensor — and gathers the features of ITS lane half (features
// h S0 .. h S0 + S0 - 1, feature k of level k / F) straight into xr[], the registers layer 0 reads as its B operands.  Nothing is
// binned (a lattice is in tile order already), no (P, L F) encoding is written or read, and the launch has no workspace.
//   workgroup = a 16-column x 8-row block of the lattice, wave = 8 x 4 of it (neighbouring lanes gather from neighbouring
//   vertices), blocks walked grid-stride by a persistent grid with one wave per SIMD; weights and biases live in registers.
// The interpolation is encode_fwd_kernel's, operation for operation: make_cell, spatial_hash | vert_idx / vert_w of vertex
// gy vstride + gx (clamped), the K rows of a vertex accumulated in ascending k, ((f0 c0 + f1 c1) + f2 c2) + f3 c3.
// Schedule of a block (16 features of the lane half = one gather group; 64-wide inputs have two):
//   layer 0 | issue group 0 of the NEXT block | layer 1 | combine group 0 -> xr, issue group 1 | layer 2 | combine group 1 | stores
// Hash source: the loads of a group are in flight under the 64 MFMAs that follow them.  Vertex-table source: the row index
// depends on a load, so a group's K rows are accumulated where the group is issued (levels in chunks of <= 8 corners, the
// next k's index / weight pairs requested while the rows of k arrive).
// Grid source (gngf_render_grid): a baked model — the vertex grid of every level as the vertex stage writes it (G of
// gngf_vertex_grid_fwd with Ls = L).  A corner is row goff_l + gy (N_l + 2) + gx of it, gx / gy clamped to the level's grid:
// four independent dense loads a level, issued where the hash source issues its rows — no hash, no table, no index loads.
// It holds fewer live values than the other sources: no scratch at 32 features, 8 / 72 spilled registers at 64 (exact / narrower).
// Registers: the 32-feature forms fit the 512-entry file; the 64-feature forms (64 more weight registers, two groups) spill
// 28 - 125 registers to scratch in the gather phases.
// Scoring forms (the kSrc*Score sources, instantiated in render_score.hip: gngf_ext2_render_score): the same pixels by the same
// operations, but the sink is a comparison — the integer (int32_t)(y * 255.0f) against the uint8 image the lattice was laid over
// (pixel (i step, j step) of it), accumulated per lane as two exact int64 sums, reduced across the wave, through LDS across the
// workgroup's waves, and stored as the workgroup's two partial sums.  Nothing of the picture is written.
// Query forms (the kSrc*Query sources, instantiated in render_query.hip: gngf_ext3_query / gngf_ext3_query_grid): the same
// values by the same operations at coordinates READ from xy (P, 2) fp32 — (row coordinate, column coordinate), one float2 load
// a point — instead of formed from a row and a column.  A block is 128 consecutive points, point wave 32 + (lane & 31) of it for
// both lane halves (neighbouring lanes load neighbouring float2s); the next block's coordinates are requested where the lattice
// forms compute them, a block ahead and outside every divergent branch (a lane past P reads xy[P - 1]); the sink is row p of
// rgb / img (P, out_dim).  The host hands the walk a one-block-high lattice of ceil(P / 128) blocks: block column = block.
namespace gngf {

constexpr int kRenderCols = 16, kRenderRows = 8;        // the workgroup's block; a wave renders 8 x 4 of it
constexpr int kSrcHash = 0, kSrcTable = 1, kSrcGrid = 2;  // where a corner's features come from
// GNGF_MODE_DENSE_HASH: the hash source's gather with DenseHashRows (gngf_common.h) for the row — in a dense level the pixels of a
// wave's 8 x 4 block read neighbouring rows of the level's first (N_l + 2)^2, as the grid source does; a finer level is hashed
constexpr int kSrcDenseHash = 3;
// The scoring forms: source kSrcScore + s gathers as source s (hash, vertex table, dense-where-it-fits; not the grid) and compares
// instead of storing.  A source of its own, not a further template parameter: the storing instantiations keep their names.
constexpr int kSrcScore = 4;
constexpr int kSrcHashScore = kSrcScore + kSrcHash, kSrcTableScore = kSrcScore + kSrcTable, kSrcDenseHashScore = kSrcScore + kSrcDenseHash;
// The query forms: source kSrcQuery + s gathers as source s (all four) at coordinates read from memory.  Sources of their own for
// the scoring forms' reason: the storing and scoring instantiations keep their names and their code.
constexpr int kSrcQuery = 8;
constexpr int kSrcHashQuery = kSrcQuery + kSrcHash, kSrcTableQuery = kSrcQuery + kSrcTable, kSrcGridQuery = kSrcQuery + kSrcGrid,
              kSrcDenseHashQuery = kSrcQuery + kSrcDenseHash;
constexpr int kQueryBlock = kRenderCols * kRenderRows;    // points of a query block: one per pixel of a lattice block

struct RenderArgs {
  const void* tables; const int32_t* vert_idx; const float* vert_w; const int32_t* n_ls;
  const float *W0, *b0, *W1, *b1, *W2, *b2;
  float* rgb; int32_t* img;
  int64_t rows, cols, r0, c0;
  float denom;
  int L, F;
  int64_t T;
  int K, vstride;
  int64_t NV;
  int out_dim;
  bool pow2;
};
// the grid source's own arguments (a second kernel argument: the other sources' launches carry an empty one)
struct RenderGridArgs { const float* grid; int64_t goff[GNGF_MAX_LEVELS]; };
struct RenderNoGrid {};
template <int SRC> struct RenderSrcArgs { using type = RenderNoGrid; };
template <> struct RenderSrcArgs<kSrcGrid> { using type = RenderGridArgs; };
// the scoring forms' second argument: `image` (h, w, C = out_dim) uint8 is compared at pixel (r step, c step) for the lattice point
// (r, c), w the image's width; partial[2 b], partial[2 b + 1] = (#equal elements, sum of squared differences) of workgroup b
// (written by every workgroup: nothing needs clearing)
struct RenderScore { const uint8_t* image; int64_t w, step; int64_t* partial; };
template <> struct RenderSrcArgs<kSrcHashScore> { using type = RenderScore; };
template <> struct RenderSrcArgs<kSrcTableScore> { using type = RenderScore; };
template <> struct RenderSrcArgs<kSrcDenseHashScore> { using type = RenderScore; };
// the query forms' second argument: xy (P, 2) fp32, 8-byte aligned, P >= 1 — and, for the baked form, the grid source's own
struct RenderQuery { const float* xy; int64_t P; };
struct RenderQueryGrid { const float* xy; int64_t P; const float* grid; int64_t goff[GNGF_MAX_LEVELS]; };
template <> struct RenderSrcArgs<kSrcHashQuery> { using type = RenderQuery; };
template <> struct RenderSrcArgs<kSrcTableQuery> { using type = RenderQuery; };
template <> struct RenderSrcArgs<kSrcDenseHashQuery> { using type = RenderQuery; };
template <> struct RenderSrcArgs<kSrcGridQuery> { using type = RenderQueryGrid; };

// one table row (F consecutive values, F sizeof(TT)-aligned: the table base is 16-byte aligned) as fp32 — tload's values
template <int F> __device__ __forceinline__ void row_load(const float* r, float (&o)[F]) {
  if constexpr (F == 4) { const float4 q = *reinterpret_cast<const float4*>(r); o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; }
  else if constexpr (F == 2) { const float2 q = *reinterpret_cast<const float2*>(r); o[0] = q.x; o[1] = q.y; }
  else o[0] = tload(r);
}
template <int F> __device__ __forceinline__ void row_load(const __half* r, float (&o)[F]) {
  if constexpr (F == 4) {
    const __half2 q0 = reinterpret_cast<const __half2*>(r)[0], q1 = reinterpret_cast<const __half2*>(r)[1];
    o[0] = __low2float(q0); o[1] = __high2float(q0); o[2] = __low2float(q1); o[3] = __high2float(q1);
  } else if constexpr (F == 2) {
    const __half2 q = *reinterpret_cast<const __half2*>(r); o[0] = __low2float(q); o[1] = __high2float(q);
  } else o[0] = tload(r);
}

// 16 features of one lane half: the four corner values of every feature and the scaled coordinate (x N_l, y N_l) of every
// level, from which the combine forms the four coefficients again (make_cell on a grid of 1: the same operations, the same
// bits) — two registers a level across the MFMA run instead of four
struct RenderGroup { float fv[4][16]; float sx[16], sy[16]; };
__device__ __forceinline__ Cell scaled_cell(float x, float y, int n, float& sx, float& sy) {
  const float fn = (float)n;
  sx = x * fn; sy = y * fn;
  return make_cell(sx, sy, 1);
}

// Levels lev0 .. lev0 + 16 / F - 1 at coordinate (x, y).  Levels >= L (the narrower forms) give zeros.
template <int F, int SRC, bool EXACT, typename TT, typename GA>
__device__ __forceinline__ void render_issue(RenderGroup& G, const RenderArgs& a, const GA& ga, int lev0, float x, float y) {
  constexpr int NLG = 16 / F;
  const TT* tables = static_cast<const TT*>(a.tables);
  if constexpr (SRC == kSrcGrid) {
#pragma unroll
    for (int lv = 0; lv < NLG; ++lv) {
      const int level = lev0 + lv;                        // (< 64 / F <= GNGF_MAX_LEVELS for every form: RENDER_F)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int f = 0; f < F; ++f) G.fv[v][lv * F + f] = 0.f;
      G.sx[lv] = G.sy[lv] = 0.f;
      if (EXACT || level < a.L) {
        const int n = a.n_ls[level];
        const Cell cell = scaled_cell(x, y, n, G.sx[lv], G.sy[lv]);
        const float* g = ga.grid + ga.goff[level] * F;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          // clamped to the level's (n + 2)^2 vertices: a coordinate outside [0, 1]^2 reads the edge, never past the grid
          const int gx = min(max(cell.gx + (v & 1), 0), n + 1), gy = min(max(cell.gy + (v >> 1), 0), n + 1);
          float o[F];
          row_load<F>(g + ((int64_t)gy * (n + 2) + gx) * F, o);
#pragma unroll
          for (int f = 0; f < F; ++f) G.fv[v][lv * F + f] = o[f];
        }
      }
    }
  } else if constexpr (SRC == kSrcHash || SRC == kSrcDenseHash) {
    using ROWS = typename std::conditional<SRC == kSrcDenseHash, DenseHashRows, HashRows>::type;
#pragma unroll
    for (int lv = 0; lv < NLG; ++lv) {
      const int level = lev0 + lv;
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int f = 0; f < F; ++f) G.fv[v][lv * F + f] = 0.f;
      G.sx[lv] = G.sy[lv] = 0.f;
      if (EXACT || level < a.L) {
        const int n = a.n_ls[level];
        const Cell cell = scaled_cell(x, y, n, G.sx[lv], G.sy[lv]);
        const TT* tab = tables + (int64_t)level * a.T * F;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int gx = cell.gx + (v & 1), gy = cell.gy + (v >> 1);
          float o[F];
          row_load<F>(tab + ROWS::row(gx, gy, n + 2, a.T, a.pow2) * F, o);
#pragma unroll
          for (int f = 0; f < F; ++f) G.fv[v][lv * F + f] = o[f];
        }
      }
    }
  } else {
    constexpr int CL = F == 4 ? 1 : 2;                    // levels per chunk: <= 8 corners (16 row values) in flight
#pragma unroll
    for (int ch = 0; ch < NLG / CL; ++ch) {
      const int levc = lev0 + ch * CL;
      if (!EXACT && levc >= a.L) {
#pragma unroll
        for (int j = 0; j < CL; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            G.sx[ch * CL + j] = G.sy[ch * CL + j] = 0.f;
#pragma unroll
            for (int f = 0; f < F; ++f) G.fv[v][(ch * CL + j) * F + f] = 0.f;
          }
        continue;
      }
      unsigned vk[CL][4];                                 // vid K (host: NV K < 2^31)
      const TT* tab[CL];
      bool on[CL];
#pragma unroll
      for (int j = 0; j < CL; ++j) {
        on[j] = EXACT || levc + j < a.L;
        const int level = on[j] ? levc + j : 0;           // a level past the end reads level 0 and is zeroed below
        const Cell cell = scaled_cell(x, y, a.n_ls[level], G.sx[ch * CL + j], G.sy[ch * CL + j]);
        tab[j] = tables + (int64_t)level * a.T * F;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int gx = cell.gx + (v & 1), gy = cell.gy + (v >> 1);
          int64_t vid = (int64_t)gy * a.vstride + gx;
          vid = vid < 0 ? 0 : (vid >= a.NV ? a.NV - 1 : vid);   // never fault on out-of-domain coordinates
          vk[j][v] = (unsigned)(vid * a.K);
        }
      }
      float acc[CL][4][F], wc[CL][4];
      int ic[CL][4];
#pragma unroll
      for (int j = 0; j < CL; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          wc[j][v] = a.vert_w[vk[j][v]];
          ic[j][v] = a.vert_idx[vk[j][v]];
#pragma unroll
          for (int f = 0; f < F; ++f) acc[j][v][f] = 0.f;
        }
      for (int k = 0; k < a.K; ++k) {
        float row[CL][4][F], wn[CL][4];
        int in[CL][4];
        const unsigned kn = k + 1 < a.K ? k + 1 : k;      // (the last trip asks for its own pair again: no branch)
#pragma unroll
        for (int j = 0; j < CL; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) row_load<F>(tab[j] + (int64_t)ic[j][v] * F, row[j][v]);
#pragma unroll
        for (int j = 0; j < CL; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) { wn[j][v] = a.vert_w[vk[j][v] + kn]; in[j][v] = a.vert_idx[vk[j][v] + kn]; }
#pragma unroll
        for (int j = 0; j < CL; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int f = 0; f < F; ++f) acc[j][v][f] += row[j][v][f] * wc[j][v];
            wc[j][v] = wn[j][v]; ic[j][v] = in[j][v];
          }
      }
#pragma unroll
      for (int j = 0; j < CL; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int f = 0; f < F; ++f) G.fv[v][(ch * CL + j) * F + f] = on[j] ? acc[j][v][f] : 0.f;
    }
  }
}

template <int F, int OFF, int S0>
__device__ __forceinline__ void render_combine(const RenderGroup& G, float (&xr)[S0]) {
#pragma unroll
  for (int lv = 0; lv < 16 / F; ++lv) {
    const Cell cell = make_cell(G.sx[lv], G.sy[lv], 1);
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const int s = lv * F + f;
      xr[OFF + s] = ((G.fv[0][s] * cell.c[0] + G.fv[1][s] * cell.c[1]) + G.fv[2][s] * cell.c[2]) + G.fv[3][s] * cell.c[3];
    }
  }
}

// hidden_act's values (max(z, 0) | max(z, 0.01 z)) as an expression the compiler schedules itself
template <bool LEAKY> __device__ __forceinline__ float render_act(float z) { return LEAKY ? fmaxf(z, 0.01f * z) : fmaxf(z, 0.f); }

// F is wave-uniform: one branch per gather phase picks the unrolled form
#define RENDER_F(...)                                                  \
  do {                                                                 \
    if (a.F == 2) { constexpr int kF = 2; __VA_ARGS__; }               \
    else if (a.F == 4) { constexpr int kF = 4; __VA_ARGS__; }          \
    else if constexpr (KIN == 32) { constexpr int kF = 1; __VA_ARGS__; } /* (F = 1 at 64 features would be 64 levels) */ \
  } while (0)

template <int KIN, bool LEAKY, bool EXACT, int SRC, typename TT>
__global__ void __launch_bounds__(kDecThreads, 1)
render_kernel(const RenderArgs a, const typename RenderSrcArgs<SRC>::type ga) {
  constexpr int S0 = KIN / 2, NG = S0 / 16;
  constexpr bool QUERY = SRC >= kSrcQuery;                 // ga holds xy and P; a.rows x a.cols = 8 x 16 ceil(P / 128): a row of blocks
  constexpr bool SCORE = SRC >= kSrcScore && !QUERY;       // ga is the RenderScore sink; a.rows x a.cols its lattice, a.r0 = a.c0 = 0
  constexpr int GSRC = QUERY ? SRC - kSrcQuery : SCORE ? SRC - kSrcScore : SRC;      // where the corners come from
  const int in_dim = EXACT ? KIN : a.L * a.F;
  const int out_dim = a.out_dim;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  // register-resident operands, gathered from a coalesced LDS copy of the raw weights (as decoder_fwd_kernel)
  extern __shared__ float raw[];
  stage_raw(raw, a.W0, a.b0, a.W1, a.b1, a.W2, a.b2, in_dim, out_dim);
  const RawOff o = raw_offsets(in_dim);
  float a0r[2][S0], a1r[2][32], w2a[32];
  f32x16 b0v[2], b1v[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s = 0; s < S0; ++s) { const int k = h * S0 + s; a0r[t][s] = k < in_dim ? raw[o.w0 + (32 * t + i) * (in_dim + 1) + k] : 0.f; }
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) a1r[t][s2] = raw[o.w1 + (32 * t + i) * 65 + kmapC(s2, h)];
#pragma unroll
    for (int r = 0; r < 16; ++r) { b0v[t][r] = raw[o.b0 + 32 * t + crow(r, h)]; b1v[t][r] = raw[o.b1 + 32 * t + crow(r, h)]; }
  }
  const int ch = lane & 3;
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) w2a[s2] = raw[o.w2 + ch * 65 + kmapC(s2, h)];
  float b2v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) b2v[c] = raw[o.b2 + c];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s = 0; s < S0; ++s) asm volatile("" : "+a"(a0r[t][s]));
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) asm volatile("" : "+a"(a1r[t][s2]));
  }
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) asm volatile("" : "+a"(w2a[s2]));

  // blocks of the lattice, row-major; the grid stride is applied to (block row, block column) without a division per block
  const int64_t nbx = (a.cols + kRenderCols - 1) / kRenderCols, nby = (a.rows + kRenderRows - 1) / kRenderRows;
  const int64_t nblocks = nbx * nby;
  const int64_t gq = (int64_t)gridDim.x / nbx, gr = (int64_t)gridDim.x % nbx;
  int64_t by = (int64_t)blockIdx.x / nbx, bx = (int64_t)blockIdx.x % nbx;
  const int lr = (wave >> 1) * 4 + (i >> 3), lc = (wave & 1) * 8 + (i & 7);      // this lane's pixel inside a block
  // (r0 + rows, c0 + cols <= 2^24: the integers are exact in fp32; lanes past the ragged edges store nothing — in the scoring
  // forms they compute the last row / column's pixel again and are masked out of the sums)
  [[maybe_unused]] const int lp = wave * 32 + i;            // (query forms) this lane's point inside a block
  auto coord = [&](int64_t brow, int64_t bcol, float& x, float& y) {
    if constexpr (QUERY) {
      // point bcol 128 + lp (brow is 0), one 8-byte load; a lane past the end takes the last point's coordinate — a valid
      // address, no branch — and stores nothing
      const int64_t p = bcol * kQueryBlock + lp;
      const float2 q = reinterpret_cast<const float2*>(ga.xy)[p < ga.P ? p : ga.P - 1];          // 64-bit offsets
      x = q.x; y = q.y;
    } else if constexpr (SCORE) {
      // image pixel (r step, c step) of lattice point (r, c) — an exact integer < 2^24 — over denom; a lane past a ragged edge
      // takes the last row / column's coordinate (inside the image, as every gather of the model expects) and adds nothing
      const int64_t r = brow * kRenderRows + lr, c = bcol * kRenderCols + lc;
      x = (float)(int)((r < a.rows ? r : a.rows - 1) * ga.step) / a.denom;
      y = (float)(int)((c < a.cols ? c : a.cols - 1) * ga.step) / a.denom;
    } else {
      x = (float)(int)(a.r0 + brow * kRenderRows + lr) / a.denom;
      y = (float)(int)(a.c0 + bcol * kRenderCols + lc) / a.denom;
    }
  };
  [[maybe_unused]] int64_t eq = 0, sse = 0;                 // (scoring forms only)
  float xr[S0], x, y;
  RenderGroup G;
  coord(by, bx, x, y);
  RENDER_F(render_issue<kF, GSRC, EXACT, TT>(G, a, ga, h * (S0 / kF), x, y); render_combine<kF, 0>(G, xr));
  if constexpr (NG == 2)
    RENDER_F(render_issue<kF, GSRC, EXACT, TT>(G, a, ga, h * (S0 / kF) + 16 / kF, x, y); render_combine<kF, 16>(G, xr));
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t pr = by * kRenderRows + lr, pc = bx * kRenderCols + lc;         // this block's pixel
    [[maybe_unused]] const int64_t pq = bx * kQueryBlock + lp;                    // (query forms) this block's point
    [[maybe_unused]] uint32_t tv[4] = {0u, 0u, 0u, 0u};      // scoring forms: the pixel's texels, requested ahead of the MFMA runs
    if constexpr (SCORE) {
      // no divergent branch: a lane past a ragged edge reads the last row / column's texel (a valid address) and is masked below
      const int64_t tr = pr < a.rows ? pr : a.rows - 1, tc = pc < a.cols ? pc : a.cols - 1;
      const uint8_t* t = ga.image + ((tr * ga.step) * ga.w + tc * ga.step) * (int64_t)out_dim;          // 64-bit offsets
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < out_dim) tv[c] = t[c];
    }
    int64_t nrow = by + gq, ncol = bx + gr;
    if (ncol >= nbx) { ncol -= nbx; ++nrow; }
    if (blk + gridDim.x >= nblocks) { nrow = by; ncol = bx; }                     // past the end: this block again, never used
    coord(nrow, ncol, x, y);
    by = nrow; bx = ncol;
    // MFMA runs and VALU bursts alternate as in decoder_fwd_kernel, but through the MFMA builtin and plain C++ activations: the
    // gather phases keep the register file full, hipcc moves values between VGPRs and AGPRs around them, and it pads the
    // hazards of instructions it knows — not those of hand-written MFMA statements (measured: wrong pixels in the narrow and
    // vertex-table forms with the asm chains of decoder_fwd_kernel)
    f32x16 acc1[2] = {b0v[0], b0v[1]}, acc2[2] = {b1v[0], b1v[1]};
#pragma unroll
    for (int sx = 0; sx < S0; ++sx) {
      acc1[0] = MFMA(a0r[0][sx], xr[sx], acc1[0]);
      acc1[1] = MFMA(a0r[1][sx], xr[sx], acc1[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    RENDER_F(render_issue<kF, GSRC, EXACT, TT>(G, a, ga, h * (S0 / kF), x, y));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[t][r] = render_act<LEAKY>(acc1[t][r]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) {
      const float b = acc1[s2 >> 4][s2 & 15];
      acc2[0] = MFMA(a1r[0][s2], b, acc2[0]);
      acc2[1] = MFMA(a1r[1][s2], b, acc2[1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    RENDER_F(render_combine<kF, 0>(G, xr));
    if constexpr (NG == 2) RENDER_F(render_issue<kF, GSRC, EXACT, TT>(G, a, ga, h * (S0 / kF) + 16 / kF, x, y));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[t][r] = render_act<LEAKY>(acc2[t][r]);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < 32; s2 += 2) {
      d0 = __builtin_amdgcn_mfma_f32_4x4x1f32(w2a[s2], acc2[s2 >> 4][s2 & 15], d0, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_4x4x1f32(w2a[s2 + 1], acc2[(s2 + 1) >> 4][(s2 + 1) & 15], d1, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NG == 2) RENDER_F(render_combine<kF, 16>(G, xr));
    {
      float yv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float dc = d0[c] + d1[c];
        const float z = dc + __shfl_xor(dc, 32, 64) + b2v[c];
        // Sigmoid on the hardware exp2 / rcp units, as decoder_fwd_kernel
        yv[c] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
      }
      if constexpr (SCORE) {
        const bool mine = h == 0 && pr < a.rows && pc < a.cols;       // the lane that would store this pixel
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < out_dim) {                                          // metric_add of csrc/metrics.hip on the integer a render stores
            const int64_t d = (int64_t)(int32_t)(yv[c] * 255.0f) - (int64_t)tv[c];
            eq += mine && d == 0;
            sse += mine ? d * d : 0;
          }
      } else if constexpr (QUERY) {
        if (h == 0 && pq < ga.P) {
          const int64_t e = pq * out_dim;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < out_dim) {
              if (a.rgb) a.rgb[e + c] = yv[c];
              if (a.img) a.img[e + c] = (int32_t)(yv[c] * 255.0f);
            }
        }
      } else if (h == 0 && pr < a.rows && pc < a.cols) {
        const int64_t e = (pr * a.cols + pc) * out_dim;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < out_dim) {
            if (a.rgb) a.rgb[e + c] = yv[c];
            if (a.img) a.img[e + c] = (int32_t)(yv[c] * 255.0f);      // (output * 255).int(): csrc/metrics.hip
          }
      }
    }
  }
  if constexpr (SCORE) {
    // lanes -> wave (shuffles), waves -> workgroup (LDS), one pair per workgroup: integer sums, any split gives the same result
    __shared__ int64_t red[2][kDecThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { eq += __shfl_xor(eq, o, 64); sse += __shfl_xor(sse, o, 64); }
    if (lane == 0) { red[0][wave] = eq; red[1][wave] = sse; }
    __syncthreads();
    if (threadIdx.x < 2) {
      int64_t s = 0;
#pragma unroll
      for (int wv = 0; wv < kDecThreads / 64; ++wv) s += red[threadIdx.x][wv];
      ga.partial[2 * (int64_t)blockIdx.x + threadIdx.x] = s;
    }
  }
}
#undef RENDER_F

// ---- Host side, shared by the entry points of decoder.hip (below), render_score.hip and render_query.hip.  An entry point reads:
// its own sink and walk checks | the model (render_table_model / render_grid_model) | the pick | the launch.  A unit emits
// the kernels of the sources it names in its picks, and no others.

constexpr int kRenderMaxGrid = 256;                       // one persistent workgroup per CU: the largest grid of every form

template <int SRC> using RenderKern = void (*)(const RenderArgs, const typename RenderSrcArgs<SRC>::type);
// leaky x (32 | 64 features wide) x (exactly that wide | narrower) of one source and table type
template <int SRC, typename TT> static RenderKern<SRC> render_pick(int in_dim, bool leaky) {
  if (in_dim == 32) return leaky ? render_kernel<32, true, true, SRC, TT> : render_kernel<32, false, true, SRC, TT>;
  if (in_dim < 32) return leaky ? render_kernel<32, true, false, SRC, TT> : render_kernel<32, false, false, SRC, TT>;
  if (in_dim == 64) return leaky ? render_kernel<64, true, true, SRC, TT> : render_kernel<64, false, true, SRC, TT>;
  return leaky ? render_kernel<64, true, false, SRC, TT> : render_kernel<64, false, false, SRC, TT>;
}
template <int SRC> static RenderKern<SRC> render_pick(bool f16, int in_dim, bool leaky) {
  return f16 ? render_pick<SRC, __half>(in_dim, leaky) : render_pick<SRC, float>(in_dim, leaky);
}
// the three table sources of one family (BASE = 0: storing, kSrcScore, kSrcQuery) by the model's mode and table type
template <int BASE> static RenderKern<BASE + kSrcHash> render_pick_mode(int mode, int feat_dtype, int in_dim, bool leaky) {
  const bool f16 = feat_dtype == GNGF_FEAT_F16;
  return mode == GNGF_MODE_DENSE_HASH     ? render_pick<BASE + kSrcDenseHash>(f16, in_dim, leaky)
         : mode == GNGF_MODE_VERTEX_TABLE ? render_pick<BASE + kSrcTable>(f16, in_dim, leaky)
                                          : render_pick<BASE + kSrcHash>(f16, in_dim, leaky);
}

// what both models share: the level resolutions, the decoder and the widths.  false: refused
static bool render_decoder(RenderArgs& a, const int32_t* n_ls, const float* W0, const float* b0, const float* W1, const float* b1,
                           const float* W2, const float* b2, int L, int F, int out_dim) {
  if (!(L > 0 && L <= GNGF_MAX_LEVELS && (F == 1 || F == 2 || F == 4) && L * F <= 64 && out_dim > 0 && out_dim <= 4)) return false;
  if (!(n_ls && W0 && b0 && W1 && b1 && W2 && b2)) return false;
  a.n_ls = n_ls; a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
  a.L = L; a.F = F; a.out_dim = out_dim;
  return true;
}

// The table-sourced model (hash, vertex table, dense-where-it-fits): checks it and fills the model part of `a` — everything
// but the sink (rgb, img) and the walk (rows, cols, r0, c0, denom).  false: refused
static bool render_table_model(RenderArgs& a, const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                               const int32_t* n_ls, const float* W0, const float* b0, const float* W1, const float* b1,
                               const float* W2, const float* b2, int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV,
                               int out_dim) {
  if (!render_decoder(a, n_ls, W0, b0, W1, b1, W2, b2, L, F, out_dim) || T <= 0) return false;
  if (mode != GNGF_MODE_HASH && mode != GNGF_MODE_VERTEX_TABLE && mode != GNGF_MODE_DENSE_HASH) return false;
  if (feat_dtype != GNGF_FEAT_F32 && feat_dtype != GNGF_FEAT_F16) return false;
  if (!tables || (reinterpret_cast<uintptr_t>(tables) & 15) != 0) return false;
  const bool vt = mode == GNGF_MODE_VERTEX_TABLE;
  if (vt && !(vert_idx && vert_w && K > 0 && K <= GNGF_MAX_TOPK_WIDE && vstride > 0 && NV > 0 && NV * K < ((int64_t)1 << 31))) return false;
  a.tables = tables; a.vert_idx = vert_idx; a.vert_w = vert_w;
  a.T = T; a.K = vt ? K : 0; a.vstride = vt ? vstride : 0; a.NV = vt ? NV : 0;
  a.pow2 = (T & (T - 1)) == 0;
  return true;
}

// The grid-sourced model (a baked vertex grid): as render_table_model, and goff[l] = the first row of level l's grid, from
// the host mirror of the resolutions.  false: refused
static bool render_grid_model(RenderArgs& a, int64_t (&goff)[GNGF_MAX_LEVELS], const float* grid, const int32_t* n_ls,
                              const int32_t* n_ls_host, const float* W0, const float* b0, const float* W1, const float* b1,
                              const float* W2, const float* b2, int L, int F, int out_dim) {
  if (!render_decoder(a, n_ls, W0, b0, W1, b1, W2, b2, L, F, out_dim)) return false;
  if (!grid || !n_ls_host || (reinterpret_cast<uintptr_t>(grid) & 15) != 0) return false;
  int64_t vtot = 0;
  for (int l = 0; l < GNGF_MAX_LEVELS; ++l) {
    goff[l] = vtot;
    if (l < L) {
      if (n_ls_host[l] < 0) return false;
      vtot += (int64_t)(n_ls_host[l] + 2) * (n_ls_host[l] + 2);
    }
  }
  a.tables = nullptr; a.vert_idx = nullptr; a.vert_w = nullptr;
  a.T = 0; a.K = 0; a.vstride = 0; a.NV = 0; a.pow2 = false;
  return true;
}

// the blocks the kernel walks on a rows x cols lattice
static int64_t render_blocks(int64_t rows, int64_t cols) {
  return ((cols + kRenderCols - 1) / kRenderCols) * ((rows + kRenderRows - 1) / kRenderRows);
}

// One launch over nblocks blocks; returns the number of workgroups (the scoring form's finish kernel sums that many partials)
template <typename GA>
static int render_launch(void (*fn)(const RenderArgs, const GA), const RenderArgs& a, const GA& ga, int64_t nblocks, hipStream_t s) {
  const int nwg = (int)(nblocks < kRenderMaxGrid ? nblocks : kRenderMaxGrid);
  const size_t smem = sizeof(float) * (size_t)raw_offsets(a.L * a.F).total;
  fn<<<dim3((unsigned)nwg), dim3(kDecThreads), smem, s>>>(a, ga);
  return nwg;
}

// the sink and the walk of the two lattice forms (gngf_render, gngf_render_grid).  false: refused
static bool render_lattice_walk(RenderArgs& a, float* rgb, int32_t* img, int64_t rows, int64_t cols, int64_t r0, int64_t c0,
                                float denom) {
  constexpr int64_t kExact = (int64_t)1 << 24;            // integers up to here are exact in fp32
  if (!(rows >= 1 && cols >= 1 && denom > 0.f && r0 >= -kExact && c0 >= -kExact && r0 + rows <= kExact && c0 + cols <= kExact)) return false;
  if (!(rgb || img)) return false;
  a.rgb = rgb; a.img = img; a.rows = rows; a.cols = cols; a.r0 = r0; a.c0 = c0; a.denom = denom;
  return true;
}

}  // namespace gngf

#ifndef GNGF_RENDER_KERNELS_ONLY        // (render_score.hip and render_query.hip bring their own entry points)
// rgb (rows cols, out_dim) fp32 and / or img (same shape) int32 = (int)(rgb * 255.0f) of the model on the lattice
// ((r0 + r) / denom, (c0 + c) / denom), r < rows, c < cols, row-major.  See include/gngf.h.
extern "C" int gngf_render(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                           const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                           float* rgb, int32_t* img, int64_t rows, int64_t cols, int64_t r0, int64_t c0, float denom,
                           int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky, void* stream) {
  RenderArgs a;
  GNGF_CHECK_ARG(render_lattice_walk(a, rgb, img, rows, cols, r0, c0, denom));
  GNGF_CHECK_ARG(render_table_model(a, tables, feat_dtype, vert_idx, vert_w, n_ls, W0, b0, W1, b1, W2, b2, L, F, T, K, mode, vstride, NV, out_dim));
  render_launch(render_pick_mode<0>(mode, feat_dtype, L * F, leaky != 0), a, RenderNoGrid{}, render_blocks(rows, cols), as_stream(stream));
  GNGF_RETURN_LAUNCH();
}

// gngf_render from a baked vertex grid (the grid source above).  See include/gngf.h.
extern "C" int gngf_render_grid(const float* grid, const int32_t* n_ls, const int32_t* n_ls_host,
                                const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                float* rgb, int32_t* img, int64_t rows, int64_t cols, int64_t r0, int64_t c0, float denom,
                                int L, int F, int out_dim, int leaky, void* stream) {
  RenderArgs a;
  RenderGridArgs ga;
  ga.grid = grid;
  GNGF_CHECK_ARG(render_lattice_walk(a, rgb, img, rows, cols, r0, c0, denom));
  GNGF_CHECK_ARG(render_grid_model(a, ga.goff, grid, n_ls, n_ls_host, W0, b0, W1, b1, W2, b2, L, F, out_dim));
  render_launch(render_pick<kSrcGrid, float>(L * F, leaky != 0), a, ga, render_blocks(rows, cols), as_stream(stream));
  GNGF_RETURN_LAUNCH();
}
#endif  // GNGF_RENDER_KERNELS_ONLY

