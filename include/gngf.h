/*
 * gngf.h — C-ABI of libgngf_hip.so: the MI355X (gfx950) hot path of the multi-resolution hash-grid encoder
 * with learned (GNGF) collision handling.
 *
 * The reference (FedeMont/collision_handling_in_instantNGP) has NO FFI/plugin boundary: its boundary is the
 * Python nn.Module API of models.py.  These entry points are therefore what a maintainer binds with ctypes
 * underneath that module API; each one names the reference code it replaces
 * (file:line relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns every buffer;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are asynchronous;
 *   - the return value is a hipError_t as int (0 = hipSuccess); nothing throws;
 *     hipErrorInvalidValue (1) = rejected arguments (null pointer, unsupported F/K, negative size);
 *   - fp32 everywhere unless stated (`tables` of the fused encoder may be fp16 storage: feat_dtype; table GRADIENTS are
 *     always accumulated in fp32); indices handed to / from the reference-shaped API are int64,
 *     internal per-vertex tables use int32;
 *   - layouts:  xy (P,2) = (row, col) in [0,1];  tables (L,T,F) contiguous, level-major;
 *               enc (P, L*F) level-major / feature-minor (models.py:651);
 *               corner order v = dx + 2*dy, dx on input dim 0 (models.py:322-331);
 *               vertex table id  vid = gy * vstride + gx  (gx = row-axis vertex, fast).
 */
#ifndef GNGF_H_
#define GNGF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNGF_ABI_VERSION 15
#define GNGF_MAX_LEVELS 32
#define GNGF_MAX_TOPK 32        /* the bound of the per-thread-list kernels; larger K takes the wide path */
#define GNGF_MAX_TOPK_WIDE 128  /* the largest K any entry point accepts (csrc/topk_wide.hip) */

/* blend of the K looked-up rows — models.py:212-217 (global should_softmax_topk_features) */
enum { GNGF_BLEND_SOFTMAX = 0 /* True */, GNGF_BLEND_RAW = 1 /* None */, GNGF_BLEND_NORM = 2 /* False */ };

/* storage type of the level tables: fp32 (the reference) or fp16 (BASELINE.json config 5); arithmetic and gradients are fp32 */
enum { GNGF_FEAT_F32 = 0, GNGF_FEAT_F16 = 1 };

/* index source of the fused encoder.
 * GNGF_MODE_DENSE_HASH (additive: no ABI version of its own) is the rule of the Instant-NGP paper: level l is DENSE when its whole
 * vertex grid fits the table, (N_l + 2)^2 <= T, and vertex (gx, gy) then uses row gy * (N_l + 2) + gx — the vertex-grid layout, so
 * G_l is the first (N_l + 2)^2 rows of the level's table and no two vertices share a row; gx and gy are clamped to [0, N_l + 1]
 * there, so a coordinate outside [0, 1]^2 never leaves those rows.  Any other level uses spatial_hash(gx, gy, T) as
 * GNGF_MODE_HASH does.  vert_idx / vert_w / K / vstride / NV are ignored, as for GNGF_MODE_HASH; feature types and F as the entry
 * point supports for GNGF_MODE_HASH.  Accepted by gngf_encode_fwd, gngf_encode_bwd, gngf_vertex_grid_fwd, gngf_vertex_grid_bwd,
 * gngf_encode_tiled_prepare (G required; clear_rows rejected) and gngf_render; REJECTED (hipErrorInvalidValue) by
 * gngf_encode_tiled_fwd_fused — the staged levels take gngf_encode_tiled_prepare + gngf_encode_tiled_fwd, and their backward
 * gngf_encode_tiled_bwd into dG (without hash_dtables) + gngf_vertex_grid_bwd.  The entry points without a mode argument
 * (gngf_encode_bwd_bucketed, gngf_clear_hashed_rows, gngf_mark_batch_slots, gngf_hash_indices) serve the spatial hash only. */
enum { GNGF_MODE_HASH = 0 /* models.py:412-414 */, GNGF_MODE_VERTEX_TABLE = 1 /* models.py:416-418, de-duplicated */,
       GNGF_MODE_DENSE_HASH = 2 /* dense where it fits, hashed elsewhere */ };

int gngf_abi_version(void);

/* ---- a5+a6: _scale_to_grid + _fast_hash (models.py:486-528) -> idx (P,L,4) int64, as the module returns it */
int gngf_hash_indices(const float* xy, const int32_t* n_ls, int64_t* idx, int64_t P, int L, int64_t T, void* stream);

/* ---- a10/a11: MultiResHashEncoding.forward (models.py:173-229).
 * idx (P,L,4) when K == 0 (hash branch) or (P,L,4,K) (GNGF branch); probs (P,L,4,K) or NULL; out (P,F,L,4). */
int gngf_mrhe_fwd(const void* tables, int feat_dtype, const int64_t* idx, const float* probs, float* out,
                  int64_t P, int L, int F, int64_t T, int K, int blend, void* stream);
/* a15 at the same boundary: dtables (L,T,F) is ACCUMULATED into (caller zero-fills), dprobs (P,L,4,K) is written. */
int gngf_mrhe_bwd(const void* tables, int feat_dtype, const int64_t* idx, const float* probs, const float* gout,
                  float* dtables, float* dprobs, int64_t P, int L, int F, int64_t T, int K, int blend, void* stream);

/* ---- a12: _bilinear_interpolate (models.py:621-655): feats (P,F,L,4) -> enc (P,L*F); bwd writes dfeats. */
int gngf_bilinear_fwd(const float* xy, const int32_t* n_ls, const float* feats, float* enc,
                      int64_t P, int L, int F, void* stream);
int gngf_bilinear_bwd(const float* xy, const int32_t* n_ls, const float* genc, float* dfeats,
                      int64_t P, int L, int F, void* stream);

/* ---- a5..a12 fused, "direct" form: one lane per (pixel, level); table rows gathered straight from HBM/L2.
 * Only levels [l0, l1) are produced / consumed (enc rows stay (P, L*F)); the tiled form below covers the others.
 * mode HASH, DENSE_HASH: vert_idx/vert_w NULL, K ignored (DENSE_HASH: the backward adds to the dense rows with atomics too).
 * mode VERTEX_TABLE: vert_idx (NV,K) int32 slots and vert_w (NV,K) blend weights per grid vertex
 *   (vid = gy*vstride + gx), i.e. HPD(top-K) evaluated once per DISTINCT vertex instead of per instance.
 * pixel_order (ABI 12, may be NULL): as in gngf_encode_bwd_bucketed — the pixels walked in the tiled form's binned order (the
 *   gathers of neighbouring lanes then fall into the same aligned blocks of table rows); enc is written by original index. */
int gngf_encode_fwd(const float* xy, const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                    const int32_t* n_ls, float* enc, int64_t P, int L, int F, int64_t T, int K,
                    int mode, int vstride, int64_t NV, int l0, int l1, const float* pixel_order, void* stream);
/* backward: dtables (L,T,F) accumulated (caller zero-fills); dvert_w (NV,K) accumulated (caller zero-fills),
 * = sum over instances of c_v * <g, E_l[idx_k]>  (gradient w.r.t. the blend WEIGHT, before the blend's own backward). */
int gngf_encode_bwd(const float* xy, const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                    const int32_t* n_ls, const float* genc, float* dtables, float* dvert_w,
                    int64_t P, int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int l0, int l1,
                    void* stream);

/* backward of levels [l0, l1), spatial-hash source, WITHOUT one memory-side atomic per contribution (csrc/encode_bucket.hip: the
 * chip retires 20.6 G atomic row updates per second wherever the rows lie): the contributions are counting-sorted by table slice
 * ("bucket" = slot >> bucket_shift) and one workgroup per (level, bucket) sums its slice in a 64-bit fixed-point LDS image — the
 * result is bitwise reproducible.  Replaces the same reference lines as gngf_encode_bwd (models.py:382-392 backward).
 * gngf_encode_bwd_bucketed_plan: 1 and plan[0..5] = bucket_shift, buckets per level, pixel blocks, matrix ints, base ints, bytes of
 *   the item buffer — or 0 when the shape is not served (F not in {1,2,4}, > 8192 buckets per level, >= 2^31 contributions);
 *   image_bytes: LDS bytes of a bucket's image (1 KiB .. 128 KiB).
 * gngf_encode_bwd_bucketed: accumulate = 1 adds to dtables (L,T,F) fp32; 0 WRITES every row of levels [l0, l1) (no clear needed).
 *   matrix / base / items: scratch of the sizes the plan names.
 *   pixel_order (ABI 12, may be NULL): the batch's pixels as P records {x, y, bits(original index), 0} in TILE order (the `sorted`
 *   output of gngf_bin_pixels / gngf_bin_pixels2 for the same xy): walked in that order, a workgroup's contributions fall into a few
 *   hundred buckets instead of all of them (the hash keeps the low bits of gx) and leave as whole lines.  Same result bit for bit. */
int gngf_encode_bwd_bucketed_plan(int64_t P, int F, int64_t T, int nl, int image_bytes, int64_t* plan);
int gngf_encode_bwd_bucketed(const float* xy, const int32_t* n_ls, const float* genc, float* dtables, int64_t P, int L, int F,
                             int64_t T, int l0, int l1, int image_bytes, int accumulate, int32_t* matrix, int32_t* base,
                             void* items, const float* pixel_order, void* stream);

/* zeroes, in dtables (L,T,F) fp32, row hash(gx, gy) of level l for every vertex of levels [0, Ls): all the rows the staged levels
 * of a hash-indexed encoder can touch, whatever the batch (a gradient buffer kept from step to step needs no dense clear).
 * vtot = sum over those levels of (N_l + 2)^2.  Serves the zero_grad of functions.py:199 for such a buffer. */
int gngf_clear_hashed_rows(float* dtables, const int32_t* n_ls, int Ls, int F, int64_t T, int64_t vtot, void* stream);

/* ---- a5..a12 fused, "tiled" form: vertex stage + spatially binned, LDS-privatised pixel stage.
 * gngf_bin_pixels: bins P pixels into 4^tile_shift tiles of [0,1]^2.  NB binning blocks (<= 512); `chunk` = max pixels
 *   per work item.  Outputs: sorted (P,4) fp32 = x, y, bits(original index), 0;  items (max_items,4) int32 = start, count,
 *   tile, items-of-tile with max_items >= ceil(P/chunk) + 4^tile_shift;  n_items (4 int32: [0] = number of items, [1..3] = work counters of the persistent pixel-stage kernels, zeroed here and put
 *   back to zero by those kernels when they finish);  tile_off and tile_item_base
 *   (4^tile_shift + 1 each: exclusive prefixes of pixels / items per tile);  blockhist: scratch of 4^tile_shift * (NB + 1)
 *   int32. */
int gngf_bin_pixels(const float* xy, int64_t P, int tile_shift, int NB, int chunk, int32_t* blockhist, int32_t* tile_off,
                    int32_t* tile_item_base, int32_t* items, int32_t* n_items, float* sorted, void* stream);
/* gngf_encode_tiled_prepare: everything in front of the pixel stage as ONE chain of launches — the binning of gngf_bin_pixels plus
 *   gngf_vertex_grid_fwd (levels [0, Ls)) riding on it as extra workgroups plus two buffer clears: dG_zero (same shape as G; NULL:
 *   none; cleared by the vertex riders) and zero_fill (zero_floats floats, a multiple of 4, 16-byte aligned — the table gradient
 *   buffer; NULL: none).  Without zero_fill the vertex riders sit on the count launch; with it, zero_fill is cleared by riders of the
 *   count launch and the vertex riders sit on the scatter launch (four launches).  Parallel branches of a replayed hipGraph cost
 *   ~10 us per cross-queue dependency on this stack; riders on one chain cost nothing.
 *   G may be NULL for the spatial-hash source (round 5): no vertex grid is built — the pixel stage gathers from the level tables
 *   itself (gngf_encode_tiled_fwd_fused) — and the riders only clear (dG_zero / clear_rows), or do not run at all. */
int gngf_encode_tiled_prepare(const float* xy, int64_t P, int tile_shift, int NB, int chunk, int32_t* blockhist,
                              int32_t* tile_off, int32_t* tile_item_base, int32_t* items, int32_t* n_items, float* sorted,
                              const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w,
                              const int32_t* n_ls, const int32_t* n_ls_host, float* G, float* dG_zero, int dG_zero_words, int Ls,
                              int F, int64_t T, int K, int mode, int vstride, int64_t NV, float* zero_fill, int64_t zero_floats,
                              int32_t* persistent_ws, float* clear_rows, void* stream);
/* persistent_ws (optional): (2 * 4^tile_shift + 1) int32 = [tile totals | tile cursors | ticket], ZERO before its first use and
 * owned by one stream — with it (and without zero_fill) the binning is TWO launches instead of four: the tile totals meet in
 * global atomics, every scatter workgroup scans them itself, and the last one out puts the workspace back to zero.  With zero_fill
 * it is not touched. */
/* clear_rows (optional, spatial-hash source only): an (L,T,F) fp32 table gradient kept from step to step — the vertex riders zero
 * row hash(gx, gy) of every staged vertex's level on the way (what gngf_clear_hashed_rows does, without a launch of its own). */
/* dG_zero_words: 1 = dG_zero is the fp32 vertex-grid gradient (vtot * F floats); 2 = it is the 64-bit fixed-point form of
 * gngf_encode_tiled_bwd's dG64 ((vtot * F + 2) 64-bit words, the two trailing words cleared as well). */
/* vertex stage: G[(goff_l + gy*(N_l+2) + gx)*F + f] for levels [0, Ls), goff_l = sum_{j<l} (N_j+2)^2.
 * n_ls_host mirrors n_ls on the host (grid sizing only). */
int gngf_vertex_grid_fwd(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                         const int32_t* n_ls_host, float* G, int Ls, int F, int64_t T, int K, int mode, int vstride,
                         int64_t NV, void* stream);
/* dG -> dtables (L,T,F) accumulated (caller zero-fills) and dvert_w (NV,K) accumulated (NULL when not needed).
 * GNGF_MODE_DENSE_HASH (both directions): a dense level is a copy / an add of its (N_l + 2)^2 F consecutive values, 16 bytes per
 * lane where the level's bases are 16-byte aligned (no atomics: launches that add to the same dtables rows must be ordered on
 * the stream); rows >= (N_l + 2)^2 of a dense level are not touched. */
int gngf_vertex_grid_bwd(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                         const int32_t* n_ls_host, const float* dG, float* dtables, float* dvert_w, int Ls, int F, int64_t T,
                         int K, int mode, int vstride, int64_t NV, void* stream);
/* pixel stage over the work items of gngf_bin_pixels: enc / genc rows are (P, L*F); levels [0, Ls) handled here.
 * lds_bytes: dynamic LDS for the per-tile sub-grids (a level that does not fit falls back to global memory).
 * bwd ACCUMULATES into dG (caller zero-fills) in two passes with no global float atomics: every work item stores its
 * privatised sub-grid image to partials (max_items * lds_bytes/4 floats), then a gather pass sums, per vertex, the
 * images of the items that cover it.  Inside a work item the sub-grids accumulate in 64-bit fixed point (LDS float
 * atomics are ~20x slower than 64-bit integer ones on gfx950); `chunk` = the binning chunk (bounds the term count).
 * genc_absmax (optional): absmax_count floats, absmax_stride apart, whose maximum is a bound >= max |genc| that fixes the
 * fixed-point scale (one value, or the per-slab maxima gngf_decoder_bwd leaves in its workspace); NULL: each work item
 * scans its own rows first.
 * tile_level_off (4^tile_shift * Ls int32, optional): float offset of level l's sub-grid inside tile t's image at
 * [t * Ls + l], -1 when the level does not fit (levels are laid out back to back in ascending order, a level that
 * would exceed lds_bytes is skipped); NULL: the gather pass re-derives it per vertex. */
/* One binning job (the arguments of gngf_bin_pixels as a host struct) for the RESERVING form of the binning: gngf_bin_pixels2, or the
 * binning of ANOTHER batch riding on the pixel-stage launches of the current one — binning depends on the coordinates only, and the
 * batches of an epoch are fixed slices of one permutation, known in advance (functions.py:186-194).  A count workgroup reserves its
 * places in every tile on running per-tile cursors, the last count workgroup out writes the tile tables and the work items, a scatter
 * workgroup moves its pixels.  P > 0.  persistent_ws (required): (2 * 4^tile_shift + 3) int32 = [tile cursors | their values at the
 * start of the current job | unused | task counter of the riding scatter | ticket of the count workgroups], ZERO before its first
 * use and never reset, owned by one sequence of steps and used by these entry points only (NOT shared with
 * gngf_encode_tiled_prepare's).  blockhist: scratch, used as [NB][4^tile_shift] int32 — each count workgroup's reserved offsets,
 * for the scatter workgroup of the same index. */
typedef struct gngf_bin_job {
  const float* xy;            /* (P, 2) coordinates of the batch to bin */
  int64_t P;
  int tile_shift, NB, chunk;
  int32_t* blockhist;         /* 4^tile_shift * (NB + 1) scratch (the size gngf_bin_pixels needs: one workspace serves both) */
  int32_t* persistent_ws;
  int32_t* tile_off;          /* outputs, as gngf_bin_pixels */
  int32_t* tile_item_base;
  int32_t* items;
  int32_t* n_items;
  float* sorted;
} gngf_bin_job;
/* the reserving form as two launches of its own (count + tile tables -> scatter); same outputs as gngf_bin_pixels, the order of
 * the pixels inside a tile aside.  zero_fill (optional, zero_floats a multiple of 4, 16-byte aligned) is cleared by rider
 * workgroups of the count launch */
int gngf_bin_pixels2(const gngf_bin_job* job, float* zero_fill, int64_t zero_floats, void* stream);
/* pixel stage forward with the vertex stage forward fused into its staging loop (bit-identical to gngf_vertex_grid_fwd +
 * gngf_encode_tiled_fwd).  Level-interleaved kernel (F = 2, fp32 tables — see gngf_tiled_interleaved_applies): both index sources;
 * generic kernel (any other shape; round 5): spatial-hash source, fp32 or fp16 tables, next_count must be NULL.  fp16 tables at a
 * shape the level-interleaved kernel takes (F = 2 and the image fits) are rejected (hipErrorInvalidValue): the caller runs
 * gngf_vertex_grid_fwd + gngf_encode_tiled_fwd.
 * next_count (optional): the count half of another batch's binning runs in extra workgroups at the end of the launch's grid; its
 * scatter half rides on gngf_encode_tiled_bwd(..., next_bin) of the same step. */
int gngf_encode_tiled_fwd_fused(const float* sorted, const int32_t* items, const int32_t* n_items, int max_items,
                                const int32_t* n_ls, const int32_t* n_ls_host, const void* tables, int feat_dtype,
                                const int32_t* vert_idx, const float* vert_w, float* enc, int L, int Ls, int F, int64_t T, int K,
                                int mode, int vstride, int64_t NV, int tile_shift, int lds_bytes, const gngf_bin_job* next_count,
                                void* stream);
int gngf_encode_tiled_fwd(const float* sorted, const int32_t* items, const int32_t* n_items, int max_items,
                          const int32_t* n_ls, const int32_t* n_ls_host, const float* G, float* enc, int L, int Ls, int F,
                          int tile_shift, int lds_bytes, void* stream);
/* n_ls_host (host copy of n_ls; may be NULL): lets the launcher size the LEVEL-INTERLEAVED LDS images (F = 2, <= 16 staged
 * levels: vertex i of level l in row i, column l of 8-byte slots, so that the 16 level-lanes of a pixel never share an LDS
 * column); NULL, or gngf_set_tiled_interleaved(0): the back-to-back layout.  Results do not depend on the layout. */
int gngf_set_tiled_interleaved(int on);       /* returns the previous setting (default 1) */
/* 1 when gngf_encode_tiled_fwd (backward = 0) / gngf_encode_tiled_bwd (backward = 1) will run the level-interleaved kernel for
 * this shape under the current setting, else 0 (host logic only, no launch).  Only the interleaved backward fills dG64: callers
 * ask here before handing one over (gngf_encode_tiled_bwd rejects a dG64 + bound for a shape the generic kernels take). */
int gngf_tiled_interleaved_applies(const int32_t* n_ls_host, int Ls, int F, int tile_shift, int lds_bytes, int backward);
/* diagnostic: per-phase cycle totals of workgroup 0 of the interleaved backward kernel since the last call (read and cleared;
 * synchronises): [0] tail wait, [1] setup, [2] clear + bound, [3] main loop, [4] wait for the other waves, [5] store pass,
 * [6] items, [7] pixels */
int gngf_debug_il_stamps(unsigned long long* host8);
int gngf_encode_tiled_bwd(const float* sorted, const int32_t* items, const int32_t* n_items, int max_items,
                          const int32_t* tile_item_base, const int32_t* tile_level_off, const int32_t* n_ls,
                          const int32_t* n_ls_host, const float* genc, const float* genc_absmax, int absmax_count,
                          int absmax_stride, float* dG, float* partials, int L, int Ls, int F, int tile_shift, int lds_bytes,
                          int chunk, const float* ride_slabs, float* ride_dW0, float* ride_db0, float* ride_dW1, float* ride_db1,
                          float* ride_dW2, float* ride_db2, int64_t ride_P, int ride_in_dim, int ride_out_dim,
                          const float* gloss_promised, const float* gloss_arrived,
                          const float* mse_pred, const float* mse_label, float* mse_loss, float* mse_workspace, int64_t mse_n,
                          float* hash_dtables, int64_t hash_T, void* dG64, int log2_pixels, const gngf_bin_job* next_bin,
                          void* stream);
/* next_bin (optional; level-interleaved kernel only): the SCATTER half of another batch's binning — whose count half ran on
 * gngf_encode_tiled_fwd_fused(..., next_count) of the same step — as tasks the persistent workgroups claim once their own work
 * items are done (they run in the tail of the launch, where two workgroups in five are idle at the headline shape). */
/* ride_* (optional, ride_slabs NULL = none): the slab reduction of a preceding gngf_decoder_bwd that was called without
 * gradient pointers (= gngf_decoder_reduce(ride_slabs, ride_dW0 .. ride_db2, NULL, ride_P, ride_in_dim, ride_out_dim)) runs in
 * extra workgroups of this launch instead of a launch of its own (one dependent launch less on the step's critical path).
 * gloss_promised / gloss_arrived (optional device scalars, both or neither): genc came out of gngf_decoder_train, which ran its
 * backward with *gloss_promised before autograd delivered *gloss_arrived; if the two differ (relative 1e-6) every gradient
 * this launch writes (the vertex-grid gradient and the ridden decoder gradients) is NaN — checked on the device, no sync.
 * hash_dtables (optional; (L, hash_T, F) fp32 gradient buffer): spatial-hash index source on a single rank — the gather pass
 * adds every vertex's gradient straight to row _fast_hash(gx, gy) of the level's table gradient (= gngf_vertex_grid_bwd in hash
 * mode for levels [0, Ls)) and leaves dG unwritten: one launch and one round trip of dG less.  dG is still READ there and must be
 * zero on entry like any dG handed to this call: a work item adds what falls outside its tile's sub-grids to dG itself, and the
 * gather pass adds dG's value to what it scatters (a dG that is not zero-filled ends up in the table rows).  With dG = dG64 = NULL
 * the work items add their sums to those rows themselves (no vertex grid, no gather pass).
 * dG64 (optional; (vtot * F + 2) 64-bit words, ZERO on entry — gngf_encode_tiled_prepare clears it with dG_zero_words = 2) with
 * log2_pixels >= ceil(log2(P)) and a bound on |genc| (genc_absmax): the work items add their exact 64-bit fixed-point sums
 * straight into this vertex grid with global integer atomics (no partial images, no gather pass; bitwise reproducible), and
 * the launch ends with the conversion to dG (fp32) or — with hash_dtables — with the conversion and the hash-source vertex
 * stage reading dG.
 * Used by the interleaved kernels (F = 2, <= 16 staged levels); ignored otherwise.
 * mse_* (optional, mse_pred NULL = none): likewise gngf_mse_fwd(mse_pred, mse_label, mse_loss, mse_workspace, mse_n) — the
 * VALUE of the pixel loss, which no kernel of the step reads. */
/* vertex stage backward for the vertex-table source in SLOT order (order (NV*K) int32 = argsort of vert_idx, flat):
 * contention-free for any slot distribution (wave-level segmented reduction, one atomic per (wave, slot run));
 * dtables accumulated, dvert_w (NV,K) written without atomics (NULL when not needed).
 * dG64 (optional, with vtot = sum_l (N_l+2)^2; dG may then be NULL): read the vertex-grid gradient from the 64-bit fixed-point grid
 * gngf_encode_tiled_bwd filled (called with dG = NULL, which skips its conversion to fp32) — one launch less. */
int gngf_vertex_grid_bwd_sorted(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* order,
                                const int32_t* n_ls, const float* dG, const void* dG64, int64_t vtot, float* dtables, float* dvert_w,
                                int Ls, int F, int64_t T, int K, int vstride, int64_t NV, void* stream);
/* the same stage over a STATIC item list, for a frozen vertex table without d w (additive: no ABI version of its own).  One item
 * per (level l < Ls, vertex (gx, gy) of that level's (N_l+2)^2 grid, k < K), N of them, stably sorted by dest:
 *   item_gi = goff[l] + gy * (N_l+2) + gx  (index into the vertex grid, 0 <= gi < vtot),  item_w = vert_w[vid, k],
 *   item_dest = l * T + vert_idx[vid, k]   (0 <= dest < rows = Ls * T),                   vid = gy * vstride + gx.
 * The three arrays are 16-byte aligned and stay valid and unchanged while launches that read them are in flight; the caller has
 * checked the ranges (the kernel gathers through item_gi).  One flat segmented reduction: no level loop, one atomic per run of
 * equal dest that ends in or crosses a workgroup.  The gradient is read from dG64 when given (as above), else from dG (fp32);
 * every value is formed as in gngf_vertex_grid_bwd_sorted, poison flag included.  dtables (rows, F) is accumulated into. */
int gngf_vertex_grid_bwd_flat(const int32_t* item_gi, const float* item_w, const int32_t* item_dest, int64_t N, const float* dG,
                              const void* dG64, int64_t vtot, float* dtables, int64_t rows, int F, void* stream);

/* gngf_decoder_bwd at in_dim == 32 with the saved hidden layers: 1 (default) = hybrid kernel — the two products with the pixel
 * on the lane (dh1 = W1^T dz2, d enc = W0^T dz1) on the bf16 pipe with the exact three-way split, the weight-gradient products
 * on the fp32 pipe; 0 = everything on the fp32 pipe.  Process-wide; returns the previous setting. */
int gngf_set_decoder_bwd_hybrid(int on);
/* Forward AND backward of the decoder in ONE launch for a training step whose loss is torch.nn.MSELoss()(rgb, target)
 * (utils.py:99) with a KNOWN upstream gradient *gloss (device scalar, e.g. the loss weight l_mse of functions.py:243): rgb
 * (P,out_dim) is written, d enc and the parameter gradients as by gngf_decoder_bwd(target, gloss).  The tile's hidden layers
 * stay in registers between its forward and backward part (no hidden-layer buffer, no separate forward launch).  in_dim == 32
 * only (hipErrorInvalidValue otherwise: use gngf_decoder_fwd + gngf_decoder_bwd).  Gradient pointers all NULL: the caller
 * runs gngf_decoder_reduce on the slabs (as with gngf_decoder_bwd). */
int gngf_decoder_train(const float* enc, const float* target, const float* gloss, const float* W0, const float* b0,
                       const float* W1, const float* b1, const float* W2, const float* b2, float* rgb, float* denc,
                       float* dW0, float* db0, float* dW1, float* db1, float* dW2, float* db2, float* slabs,
                       float* denc_absmax, float* zero_fill, int64_t zero_floats, int64_t P, int in_dim, int out_dim, int leaky,
                       void* stream);
/* zero_fill (optional): zero_floats floats (a multiple of 4, 16-byte aligned) cleared by this launch on the way — the table
 * gradient the encoder backward will accumulate into; the stores issue between the kernel's MFMAs (no issue time, idle HBM)
 * instead of in rider workgroups of gngf_encode_tiled_prepare. */
/* ---- dense layers on the matrix cores.  act: 0 none, 1 ReLU, 2 LeakyReLU(0.01), 3 Sigmoid.
 * nn.Linear + activation of HashProbDistribution (models.py:80-88,105-106) and of the decoder (models.py:382-392).
 * gemm (gngf_linear_fwd, gngf_linear_bwd_weight, gngf_gemm_acc): which kernel THIS call's product runs on, one of the GNGF_GEMM_*
 * codes (any other value: hipErrorInvalidValue).  The split codes split every fp32 operand exactly into three bf16 terms and
 * accumulate six of the nine cross products in fp32 on the bf16 matrix pipe (error <= ~2e-7 sum |a_k b_k|, at or below the rounding
 * of an fp32 fma chain; 2-2.7x the fp32-MFMA rate).  They apply to large aligned products only — whole 128 x 128 tiles, contraction
 * (and its slice per block) a multiple of 32, 16-byte aligned operands, no activation mask on an operand, leading dimensions below
 * 2^22; on any other shape a split code runs the exact-fp32 kernels, as GNGF_GEMM_FP32 does.  gngf_linear_bwd_input is always
 * exact fp32, gngf_linear_fwd_rowstats always GNGF_GEMM_PLANES. */
#define GNGF_GEMM_FP32 0         /* exact fp32 MFMA */
#define GNGF_GEMM_PLANES 1       /* operands split once on the way into LDS: three bf16 planes (round 5) */
#define GNGF_GEMM_PLANES_ACC2 2  /* as 1, but the entries that ACCUMULATE into their output (gngf_linear_bwd_weight, gngf_gemm_acc) use
                                  * two planes and three products: |error| <= 3 * 2^-18 |a b| per product (the HashProbDistribution's
                                  * dW / dh, contractions of >= 4096 terms).  gngf_linear_fwd treats it as 1. */
#define GNGF_GEMM_WAVE_SPLIT 17  /* the round-4 kernel: every wave splits the fragments it reads (kept for A/B; same numbers as 1) */
int gngf_linear_fwd(const float* X, const float* W, const float* b, float* Y, int64_t M, int N, int K, int act, int gemm,
                    void* stream);
/* dX[M,K] = (dY .* act'(Y)) W ;  Y = activated output of the layer (may be NULL when act == 0) */
int gngf_linear_bwd_input(const float* dY, const float* Y, const float* W, float* dX, int64_t M, int N, int K, int act,
                          void* stream);
/* dW[N,K] += (dY .* act'(Y))^T X ; db[N] += column sums.  Accumulates (float atomics): zero-fill for a fresh gradient. */
int gngf_linear_bwd_weight(const float* dY, const float* Y, const float* X, float* dW, float* db, int64_t M, int N, int K,
                           int act, int gemm, void* stream);
/* C[M,N] += opA(A) opB(B), contraction Kc split over blocks.  ta: A stored (Kc,M); tb: B stored (N,Kc). */
int gngf_gemm_acc(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t Kc, int ta, int tb, int gemm,
                  void* stream);

/* ---- a13: the decoder MLP fused (models.py:382-392,469-470): Linear(in,64)+act, Linear(64,64)+act, Linear(64,out)+Sigmoid,
 * act = ReLU (leaky = 0) or LeakyReLU(0.01) (leaky = 1); in_dim <= 64, out_dim <= 4.  W* are (out,in) like nn.Linear. */
/* hidden (optional): gngf_decoder_hidden_floats(P) floats that receive the two activated hidden layers (512 B / pixel) for
 * gngf_decoder_bwd — the stores ride under the forward kernel's MFMAs, and the backward kernel then reads them back
 * instead of recomputing them (96 of its 292 MFMAs per 32 pixels). */
int gngf_decoder_fwd(const float* enc, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                     const float* b2, float* rgb, float* hidden, int64_t P, int in_dim, int out_dim, int leaky, void* stream);
int64_t gngf_decoder_hidden_floats(int64_t P);
/* backward: denc (P,in_dim) and the six parameter gradients, each WRITTEN (not accumulated); rgb = the forward output.
 * slabs: workspace of gngf_decoder_bwd_slabs(P) * gngf_decoder_slab_floats(in_dim, out_dim) floats.
 * denc_absmax (1 float, optional): receives max |denc| (NaN if any element is NaN) — a bound the tiled encoder backward
 * can take instead of scanning its input once more.
 * hidden (optional): the buffer gngf_decoder_fwd filled for the same enc and weights; NULL: recompute. */
int gngf_decoder_bwd(const float* enc, const float* rgb, const float* drgb, const float* target, const float* gloss,
                     const float* W0, const float* b0, const float* W1,
                     const float* b1, const float* W2, float* denc, float* dW0, float* db0, float* dW1, float* db1, float* dW2,
                     float* db2, float* slabs, float* denc_absmax, const float* hidden, float* zero_fill, int64_t zero_floats,
                     int64_t P, int in_dim, int out_dim, int leaky, void* stream);
/* zero_fill (optional; zero_floats floats, a multiple of 4, 16-byte aligned): cleared by the kernel on the way, a few 16-byte
 * stores per lane and tile (as gngf_decoder_train's) — the table gradient the encoder backward is about to accumulate into, at
 * shapes that have no fused training kernel (64 input features: BASELINE config 5). */
/* target + gloss (1 float), optional, instead of drgb: the gradient of the fused pixel loss,
 * d rgb = gloss[0] * 2 / (P * out_dim) * (rgb - target) (MSELoss backward), is formed inside the kernel (drgb may be NULL). */
 /* The six gradient pointers may ALL be NULL: the kernel then stops at the slabs and gngf_decoder_reduce finishes (e.g. on a
  * second stream, beside the encoder backward — which only needs max |denc|: the last float of every slab is that slab's
  * maximum, i.e. genc_absmax = slabs + slab_floats - 1, absmax_count = gngf_decoder_bwd_slabs(P), absmax_stride = slab_floats). */
int gngf_decoder_reduce(const float* slabs, float* dW0, float* db0, float* dW1, float* db1, float* dW2, float* db2,
                        float* denc_absmax, const float* gloss_promised, const float* gloss_arrived, int64_t P, int in_dim,
                        int out_dim, void* stream);
/* gloss_promised / gloss_arrived: as for gngf_encode_tiled_bwd (NULL, NULL: nothing was promised). */
int gngf_decoder_bwd_slabs(int64_t P);
/* measurement: duration (ns, device 100 MHz clock; first workgroup start -> last workgroup end) of the most recent
 * gngf_decoder_bwd main kernel — usable when the call sits inside a replayed hipGraph, where events cannot be recorded.
 * Synchronises the device. */
int gngf_decoder_bwd_last_span_ns(double* ns);
int gngf_decoder_slab_floats(int in_dim, int out_dim);

/* ---- a7/a8 tail, per DISTINCT vertex: Softmax(dim=-1) + nan_to_num + top-K (models.py:85,111,116; 5-19).
 * logits_probs (U,T): logits in, probabilities out (in place).  topk_val (U,K) sorted descending, topk_idx (U,K) int32;
 * ties resolve to the LOWER slot index (torch.topk leaves tie order unspecified).  rowstat (U,2) = (row max, row sum of
 * exp(z - max); NaN marks a NaN-poisoned row), optional (NULL): lets the backward rebuild p from recomputed logits. */
int gngf_softmax_topk(float* logits_probs, float* topk_val, int32_t* topk_idx, float* rowstat, int64_t U, int64_t T, int K,
                      void* stream);
/* streaming form for the chunked per-vertex path: logits are only READ (the (rows,T) distribution is never written):
 * one pass gives the online row statistics and the top-K (selected on the logits; probabilities = exp(z_k - max)/sum),
 * a second pass accumulates pbar (L,T) += mw (U,L)^T softmax(logits) when mw is given (L = 0: skipped). */
int gngf_logits_topk_pbar(const float* logits, float* topk_val, int32_t* topk_idx, float* rowstat, const float* mw, int L,
                          float* pbar, int64_t U, int64_t T, int K, void* stream);
/* DifferentiableTopk.forward alone (models.py:11) on arbitrary rows x (U,T); same ordering rules. */
int gngf_topk(const float* x, float* topk_val, int32_t* topk_idx, int64_t U, int64_t T, int K, void* stream);
/* backward of the above without the dense zero-filled scatter of models.py:27-35:
 *   g = gdense (U,T, optional) + mw (U,L) * G (L,T) (optional low-rank term of the batch-mean loss) + dq at topk_idx
 *   dlogits = p .* (g - <p, g>)        dlogits may alias probs. */
int gngf_softmax_bwd(const float* probs, const float* dq, const int32_t* topk_idx, const float* gdense, const float* mw,
                     const float* G, int L, float* dlogits, int64_t U, int64_t T, int K, void* stream);

/* The logits product with ROW STATISTICS in its epilogue, and their consumers (round 4): gngf_linear_fwd_rowstats = gngf_linear_fwd
 * without activation + rowparts (M, N / 64) float pairs (max, sum exp(y - max)) per row and 64-column block (whole 128 x 128 tiles
 * only: M % 128 == 0, N % 128 == 0, K % 32 == 0, 16-byte aligned — else hipErrorInvalidValue and the caller takes gngf_linear_fwd +
 * gngf_logits_topk_pbar); gngf_rowstats_topk = the statistics / top-K half of gngf_logits_topk_pbar from those partials (it reads
 * K x 64 logits per row instead of all T: the K largest logits lie inside the K blocks with the largest maxima);
 * gngf_pbar_accumulate = its batch-mean half.  Same results as gngf_logits_topk_pbar (models.py:85,105-123; utils.py:138,159). */
int gngf_linear_fwd_rowstats(const float* X, const float* W, const float* b, float* Y, float* rowparts, int64_t M, int N, int K,
                             void* stream);
int gngf_rowstats_topk(const float* logits, const float* rowparts, float* topk_val, int32_t* topk_idx, float* rowstat, int64_t U,
                       int64_t T, int K, void* stream);
int gngf_pbar_accumulate(const float* logits, const float* rowstat, const float* mw, int L, float* pbar, int64_t U, int64_t T,
                         void* stream);
/* the same backward from RECOMPUTED LOGITS, in place (logits in, d logits out), for the chunked per-vertex path:
 * p = exp(z - rowstat.max) / rowstat.sum;  g = mw (U,L) * G (L,T) + dq at topk_idx;  dz = p .* (g - <p,g>);
 * db (T) += column sums of dz (NULL: skipped).  scratch: U + U*K floats.  L = 0 / K = 0 drop the respective term. */
int gngf_softmax_bwd_lowrank(float* logits_dz, const float* rowstat, const float* dq, const int32_t* topk_idx, const float* mw,
                             const float* G, int L, float* db, float* scratch, const float* topk_p, int64_t U, int64_t T, int K,
                             void* stream);
/* The same backward WITHOUT the d-logits matrix (round 5): gngf_hpd_bwd_dot leaves the row dots
 *   dot[r] = sum_k topk_p[r,k] dq[r,k] + sum_t p[r,t] (mw G)[r,t]
 * (one read of the logits), and gngf_hpd_bwd_fused forms dz = p .* (mw G - dot) (+ p_k dq_k at the K top-K slots of a row) inside
 * the operand loaders of the last layer's two backward GEMMs, which read the LOGITS:
 *   dW (T,hidden) += dz^T h,  db (T) += column sums of dz (NULL: skipped),  dH (U,hidden) += dz W        (all three accumulate)
 * — what gngf_softmax_bwd_lowrank + gngf_linear_bwd_weight + gngf_gemm_acc compute (the autograd backward of models.py:84-85,
 * 105-116 under the batch-mean loss utils.py:138,159), with two passes over the (U,T) matrix instead of five.
 * The small operands are split ONCE per backward pass into bf16 planes by gngf_hpd_bwd_prepare:
 *   h (rows,hidden) = the last hidden layer of ALL vertices -> hp (planes, rows, hidden);  mw (rows,L) -> mwp (3, rows, 16), zero-padded
 *   W (T,hidden) = the last layer's weight -> Wp (planes, T, hidden);                      G (L,T) -> Gtp (3, T, 16), transposed
 * (either half may be skipped: h == NULL / W == NULL; L = 0: mw / G may be NULL).  planes: 3 = every fp32 value split exactly into
 * three bf16 terms (six products, fp32 accumulation), 2 = two terms, three products (|error| <= 3 * 2^-18 |a b| per product); the
 * operands of the small product mw G always keep the exact three.  gngf_hpd_bwd_fused takes hp / mwp AT THE CHUNK'S FIRST ROW
 * (pointer + u0 * hidden resp. + u0 * 16 elements) and rows_total = the rows they were prepared with (the plane stride); h (U,hidden)
 * and W in fp32 serve the K top-K terms only (K = 0: unused).  Diagnostic: planes + 16 / + 32 / + 48 run the dW + db part / the dH
 * part / the top-K terms alone.
 * Shapes: gngf_hpd_bwd_fused_applies(U, T, L, K, hidden) != 0 (U % 128 == 0, T % 128 == 0, T < 2^22, hidden == 128, L <= 16);
 * anything else is rejected (hipErrorInvalidValue) — the caller then takes the three separate entry points. */
int gngf_hpd_bwd_dot(const float* logits, const float* rowstat, const float* dq, const float* topk_p, const float* mw,
                     const float* G, int L, float* dot, int64_t U, int64_t T, int K, void* stream);
int gngf_hpd_bwd_fused_applies(int64_t U, int64_t T, int L, int K, int hidden);
int gngf_hpd_bwd_prepare(const float* h, const float* mw, int64_t rows, void* hp, void* mwp, const float* W, const float* G, int64_t T,
                         void* Wp, void* Gtp, int L, int hidden, int planes, void* stream);
int gngf_hpd_bwd_fused(const float* logits, const float* rowstat, const float* dot, const float* dq, const float* topk_p,
                       const int32_t* topk_idx, const void* hp, const void* mwp, int64_t rows_total, const void* Wp, const void* Gtp,
                       const float* h, const float* W, float* dW, float* db, float* dH, int64_t U, int64_t T, int K, int hidden,
                       int planes, void* stream);
/* topk_p (optional; (U,K)): the top-K probabilities gngf_logits_topk_pbar / gngf_softmax_topk returned for these logits — the
 * backward then takes p at the top-K slots from them instead of reading the logits again at random. */

/* verts[i] = (gx, gy) fp32 of vertex id u0+i (vid = gy*vstride + gx): the raw-integer HPD input of models.py:416-418 */
int gngf_vertex_coords(float* verts, int64_t u0, int64_t count, int vstride, void* stream);
/* blend weights of the K rows (models.py:212-217) on the per-vertex table, and their backward (dw -> dq) */
int gngf_blend_fwd(const float* q, float* w, int64_t U, int K, int blend, void* stream);
int gngf_blend_bwd(const float* q, const float* dw, float* dq, int64_t U, int K, int blend, void* stream);
/* counts (L,NV) int32 += number of (pixel, corner) instances of each vertex per level (caller zero-fills);
 * mw (NV,L) = counts / denom : weights of the batch-mean distribution p-bar_l (utils.py:138,159). */
int gngf_vertex_multiplicity(const float* xy, const int32_t* n_ls, int32_t* counts, int64_t P, int L, int vstride, int64_t NV,
                             void* stream);
int gngf_multiplicity_weights(const int32_t* counts, float* mw, int64_t NV, int L, float denom, void* stream);
/* reference-shaped outputs rebuilt from the per-vertex table: vid_out (P,L,4) int64, out_idx (P,L,4,K) int64,
 * out_val (P,L,4,K) fp32 (any of the three may be NULL) — models.py:478-484 return contract. */
int gngf_expand_vertex_table(const float* xy, const int32_t* n_ls, const int32_t* src_idx, const float* src_val,
                             int64_t* vid_out, int64_t* out_idx, float* out_val, int64_t P, int L, int K, int vstride,
                             int64_t NV, void* stream);

/* ---- pixel loss (row f1 of the scope table: the caller of the path) -------------------------------------------------
 * torch.nn.MSELoss() of utils.py:99 on the (P,out_dim) outputs: loss[0] = mean((pred - label)^2) over n elements.
 * workspace: gngf_mse_workspace_floats() floats, 8-byte aligned, zero-filled once before the first call (the kernel
 * resets it).  One launch; workgroup partials meet in a double-precision atomic.
 * pred and label (and dpred of gngf_mse_bwd) are 16-byte aligned; anything else is rejected (hipErrorInvalidValue). */
int gngf_mse_workspace_floats(void);
int gngf_mse_blocks(int64_t n);      /* workgroups gngf_mse_fwd launches for n elements */
int gngf_mse_fwd(const float* pred, const float* label, float* loss, float* workspace, int64_t n, void* stream);
/* its backward: dpred (n) = gout[0] * 2 (pred - label) / n   (gout: device scalar, the gradient of the loss value) */
int gngf_mse_bwd(const float* pred, const float* label, const float* gout, float* dpred, int64_t n, void* stream);

/* the distribution term of the same Loss (utils.py:122-174) on the batch-mean distribution pbar (L,T):
 *   out[l] = -(gamma + eps) * JS(pbar_l, uniform) + eps * KL(uniform || pbar_l),
 * both built from torch.nn.KLDivLoss(reduction='batchmean') on 1-D rows, i.e. divided by T.
 * workspace: gngf_js_kl_workspace_doubles(L) doubles (8-byte aligned, no initialisation needed). */
int gngf_js_kl_workspace_doubles(int L);
int gngf_js_kl_fwd(const float* pbar, float* out, double* workspace, int L, int64_t T, float gamma, float eps, void* stream);
/* its backward: dpbar (L,T) = gout[l] * d out[l] / d pbar[l,t] */
int gngf_js_kl_bwd(const float* pbar, const float* gout, float* dpbar, int L, int64_t T, float gamma, float eps, void* stream);

/* ---- collision statistics (row f3) ----------------------------------------------------------------------------------
 * counts (K,L) int32 = number of distinct slots in [0,T) among indices[:, l, :, k], indices (P,L,V,K) int64 contiguous
 * (K = 1: the hash source's (P,L,V)) — the torch.unique(...).numel() of calc_hash_collisions, models.py:568-619.
 * bitmap: gngf_slot_bitmap_words(L, K, T) uint32 words of workspace (cleared by the call). */
int64_t gngf_slot_bitmap_words(int L, int K, int64_t T);
int gngf_distinct_slot_counts(const int64_t* indices, int64_t P, int L, int V, int K, int64_t T, uint32_t* bitmap,
                              int32_t* counts, void* stream);
/* The same statistic without the index tensor (2 GiB per step at the headline shape): both index sources depend on (level,
 * vertex) only, so a batch's distinct slots are the slots of its touched vertices.  Marks the slots batch `xy` uses into
 * `bitmap` (gngf_slot_bitmap_words(L, K, T) 32-bit words, ACCUMULATED over calls: the caller clears it once per epoch);
 * vert_idx (NV,K) int32 with vid = gy * vstride + gx, or NULL for the spatial hash (K = 1, vstride >= N_max + 2, NV = vstride^2);
 * touched: workspace of L * ceil(NV / 32) words.  gngf_count_slot_bits then gives counts (K,L) as gngf_distinct_slot_counts. */
int gngf_mark_batch_slots(const float* xy, const int32_t* n_ls, int64_t P, int L, const int32_t* vert_idx, int K, int64_t T,
                          int vstride, int64_t NV, uint32_t* touched, uint32_t* bitmap, void* stream);
int gngf_count_slot_bits(const uint32_t* bitmap, int L, int K, int64_t T, int32_t* counts, void* stream);
/* The rows a model can EVER address, whatever the batch (coordinates in [0,1]^2): for every level l and every vertex
 * 0 <= gx, gy <= N_l + 1 (the corners of weight 0 at N_l + 1 included) ORs into `rowmask` — gngf_slot_bitmap_words(L, 1, T)
 * words laid out (L, ceil(T / 32)), bit (slot & 31) of word (slot >> 5); never cleared by the call, the caller zero-fills it
 * once — row spatial_hash(gx, gy) when vert_idx == NULL (K = 1), else the K rows vert_idx[(gy * vstride + gx) * K + k]
 * (vertices with gx >= vstride or beyond NV are not in the table and are skipped).  n_ls: device, n_ls_host: the same L
 * values on the host.  A superset of the rows that can receive a non-zero gradient: what gngf_adam_step_masked may skip. */
int gngf_mark_reachable_rows(const int32_t* n_ls, const int32_t* n_ls_host, int L, const int32_t* vert_idx, int K, int64_t T,
                             int vstride, int64_t NV, uint32_t* rowmask, void* stream);

/* ---- optimizer (row f2: the caller of the path) ---------------------------------------------------------------------
 * torch.optim.Adam as get_optimizer builds it (functions.py:96-127: betas (0.9, 0.99), eps 1e-15, L2-style weight
 * decay, dense moments, per-group lr), every tensor of every group in ONE launch.
 * segments: device array of nseg 64-byte records
 *     { void* param; const void* grad; float* exp_avg; float* exp_avg_sq; float* master; int64_t n; int64_t first_block;
 *       int32_t group; int32_t flags; }
 * with first_block = running sum of ceil(n / gngf_adam_block_elems()) and total_blocks that sum over all segments.
 * flags bit 0: param and grad are fp16 (fp16 level tables, BASELINE.json config 5) and `master` is the fp32 master copy
 * the update is applied to (param = round(master)); moments are fp32 either way; bit 1 (only with bit 0): `grad` is fp32
 * all the same — the buffer the table gradient was accumulated in, no fp16 copy.  inv_grad_scale multiplies every gradient
 * before use (1 / loss scale of fp16 training; 1 = off).
 * step: device float holding the number of steps taken so far; the call increments it and uses the new value (bias
 * corrections in double precision), so a step is capturable in a hipGraph.  lr, weight_decay: HOST arrays of ngroups
 * (<= GNGF_ADAM_MAX_GROUPS) values, indexed by a segment's `group`. */
#define GNGF_ADAM_MAX_GROUPS 4
int gngf_adam_block_elems(void);
int gngf_adam_step(const void* segments, int nseg, int64_t total_blocks, float* step, const float* lr,
                   const float* weight_decay, int ngroups, float beta1, float beta2, float eps, float inv_grad_scale,
                   void* stream);
/* The same step over reachable table rows only.  seg_masks: device array of nseg 16-byte records
 *     { const uint32_t* mask; int32_t row_elems; int32_t reserved; }
 * element e of segment i belongs to row e / row_elems and is processed when bit (row & 31) of mask[row >> 5] is set
 * (gngf_mark_reachable_rows writes such maps); rows whose bit is clear are neither read nor written.  mask == NULL: the
 * segment is processed densely — as is every segment of a group with weight_decay != 0 (decided by the kernel: with decay
 * an unreachable row does change).  Equal to gngf_adam_step bit for bit provided the moments of every masked-out row are 0,
 * which holds for rows that never receive a gradient. */
int gngf_adam_step_masked(const void* segments, int nseg, int64_t total_blocks, float* step, const float* lr,
                          const float* weight_decay, int ngroups, float beta1, float beta2, float eps, float inv_grad_scale,
                          const void* seg_masks, void* stream);

/* ---- epoch image and its statistics (functions.py:308, 332-335, 690-692) --------------------------------------------
 * img (P,C) int32 in image order: row perm[lo + i] (perm == NULL: row lo + i), i in [0, n), = (int32)(out[i, :] * 255.0f)
 * for one batch's outputs out (n,C) fp32 contiguous — one fp32 product, conversion toward zero, no clamp: torch's
 * (output * 255).int().  C in 1..4, 0 <= lo, lo + n <= P, n > 0.  perm (P) int32: every value must lie in [0, P); the
 * kernel does not check it (the caller validates the permutation once). */
int gngf_image_scatter(const float* out, const int32_t* perm, int32_t* img, int64_t lo, int64_t n, int64_t P, int C, void* stream);
/* sums[0] = #{e : img[e] == target[e]}, sums[1] = sum_e (img[e] - target[e])^2 over n_elems elements: int64 from the first
 * addition, exact and independent of the launch geometry (per-workgroup partials, one finishing workgroup).
 * workspace: gngf_image_metrics_workspace_words(n_elems) int64 words, no clearing needed; the partial kernel runs
 * gngf_image_metrics_blocks(n_elems) workgroups. */
int gngf_image_metrics_blocks(int64_t n_elems);
int gngf_image_metrics_workspace_words(int64_t n_elems);
int gngf_image_metrics(const int32_t* img, const uint8_t* target, int64_t* sums, int64_t* workspace, int64_t n_elems, void* stream);

/* ---- render: the model on a pixel lattice, forward only, one launch (csrc/render.inc) --------------------------------
 * Pixel (r, c), r < rows, c < cols, has the coordinate ((float)(r0 + r) / denom, (float)(c0 + c) / denom) — one correctly
 * rounded fp32 division per axis; no coordinate tensor is read — and row r cols + c of the outputs:
 *   rgb (rows cols, out_dim) fp32 = decoder(encoding(coordinate)), the forward pass of gngf_encode_fwd + gngf_decoder_fwd
 *   without the (P, L F) encoding in memory; img (same shape) int32 = (int32)(rgb * 255.0f), gngf_image_scatter's
 *   quantisation.  Either may be NULL, not both.  No workspace, no synchronisation.
 * tables (L,T,F) of feat_dtype, 16-byte aligned; mode GNGF_MODE_HASH, GNGF_MODE_DENSE_HASH, or GNGF_MODE_VERTEX_TABLE with vert_idx / vert_w
 * (NV,K), vstride and NV as gngf_encode_fwd takes them (vertices outside the table are clamped; NV K < 2^31).
 * Decoder W0 (64, L F), W1 (64,64), W2 (out_dim,64) and biases, hidden activation ReLU or (leaky) LeakyReLU(0.01).
 * Requires F in {1,2,4}, L <= GNGF_MAX_LEVELS, L F <= 64, out_dim <= 4, rows, cols >= 1, denom > 0 and
 * -2^24 <= r0, c0, r0 + rows <= 2^24, c0 + cols <= 2^24 (the integers are exact in fp32); else hipErrorInvalidValue. */
int gngf_render(const void* tables, int feat_dtype, const int32_t* vert_idx, const float* vert_w, const int32_t* n_ls,
                const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                float* rgb, int32_t* img, int64_t rows, int64_t cols, int64_t r0, int64_t c0, float denom,
                int L, int F, int64_t T, int K, int mode, int vstride, int64_t NV, int out_dim, int leaky, void* stream);
/* gngf_render from a BAKED model: grid (sum_l (N_l+2)^2, F) fp32, 16-byte aligned, is the vertex grid of every level as
 * gngf_vertex_grid_fwd writes it with Ls = L — row goff_l + gy (N_l+2) + gx, goff_l = sum_{j<l} (N_j+2)^2 — for either index
 * source and table type.  Corner v of a level reads row (clamp(gx + (v & 1), 0, N_l+1), clamp(gy + (v >> 1), 0, N_l+1)): four
 * independent dense loads, no tables, no vert_idx / vert_w, no hash; a coordinate outside [0, 1]^2 never faults (it reads the
 * grid's edge, which is not the model's value there).  n_ls (L) int32 on the device, n_ls_host its host mirror (the level
 * offsets are formed from it and passed with the launch).  Coordinates, decoder, outputs and quantisation as gngf_render.
 * Requires what gngf_render requires of L, F, out_dim, rows, cols, r0, c0, denom; else hipErrorInvalidValue. */
int gngf_render_grid(const float* grid, const int32_t* n_ls, const int32_t* n_ls_host,
                     const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                     float* rgb, int32_t* img, int64_t rows, int64_t cols, int64_t r0, int64_t c0, float denom,
                     int L, int F, int out_dim, int leaky, void* stream);

/* ---- epoch loop (functions.py:639-814: early stopping, the zero-collision stop, keeping the best model) ---------------
 * gngf_epoch_tail: one launch per epoch, one workgroup; takes the epoch's decisions on the device, advances `state` and
 * writes row e (the epoch's index, kept in the state) of the two logs.  No host synchronisation.
 * state: gngf_epoch_state_bytes() (128) bytes, 8-byte aligned:
 *     { int32 take, last, finished, stop, reason, cause, zero_checks, zero_all;
 *       int64 epoch, counter, best_sse, best_epoch, last_epoch; double best_loss; int64 reserved[6]; }
 *   initialised by the host: zeros, zero_all = 1, best_sse = the largest sse whose PSNR is >= 0 (-1: none), best_epoch =
 *   last_epoch = -1, best_loss = +inf.  take / last: flags for gngf_snapshot_if; finished: set with the last epoch — from
 *   then on a call changes nothing but take = last = 0.  reason (valid once finished): 1 `epochs` reached, 2 the early
 *   stopper, 3 the zero-collision rule.
 * loss, mse (nb) and kls, colls (nb, L; both may be NULL) fp32: per-batch values; their means are sequential sums in batch
 * order in double, divided by nb (np.mean for nb < 8).  sums: int64[2] of gngf_image_metrics.  used (Kc, L) int32 distinct
 * slot counts (gngf_count_slot_bits / gngf_distinct_slot_counts) or NULL with Kc = 0: the zero-collision rule is off;
 * hash_source != 0 (Kc = 1): level l is free of collisions when nverts[l] - used[0,l] == 0, otherwise when
 * sum_k (nverts[l] - used[k,l]) <= 0 (mean over k, clamped at 0, compared with 0).  nverts (L) int64.
 * logf (epochs, 2 + 2 L) double: loss, mse, kls[L], colls[L] (NaN where NULL).
 * logi (epochs, gngf_epoch_log_int_columns(Kc, L) = 6 + Kc L) int64: equal elements, sse, the stopper's counter, saved,
 * stopper fired, zero-collision stop, used[Kc L].
 * Order within an epoch: zero-collision rule (epochs 1..10), save decision (sse <= best_sse), break if the stop flag is
 * set, else for e != 0 EarlyStopping.__call__ (utils.py:186-205). */
int gngf_epoch_state_bytes(void);
int gngf_epoch_log_int_columns(int Kc, int L);
int gngf_epoch_tail(void* state, double* logf, int64_t* logi, const float* loss, const float* mse, const float* kls,
                    const float* colls, int nb, int L, const int64_t* sums, const int32_t* used, int Kc, int hash_source,
                    const int64_t* nverts, double tolerance, double min_delta, int should_reset, int64_t epochs, void* stream);
/* Predicated multi-tensor copy: when *flag != 0, dst = src for every record of the device array
 *     { const void* src; void* dst; int64_t bytes; int64_t first_block; }   (32 bytes)
 * with first_block = running sum of ceil(bytes / gngf_snapshot_block_bytes()) and total_blocks that sum (records of 0 bytes
 * are left out by the packer).  Any dtype: sizes are bytes; 16-byte accesses where both pointers allow, 4-byte or single
 * bytes elsewhere.  When *flag == 0 every workgroup returns after reading it.  src and dst must not overlap. */
int gngf_snapshot_block_bytes(void);
int gngf_snapshot_if(const void* records, int nrec, int64_t total_blocks, const int32_t* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNGF_H_ */
