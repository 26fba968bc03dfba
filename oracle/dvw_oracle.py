"""Float64 oracle of d vert_w, the gradient of the encoder with respect to the per-vertex blend weights — TEST INFRASTRUCTURE ONLY.

    d vert_w[vid, k] = sum_l sum_f ( sum over the (pixel, corner) terms t of level l that reach vid of  g[t, l, f] c[t] )  E_l[idx[vid, k], f]

Pure numpy on top of c_oracle.encode_bwd_f64: per level, the exact per-vertex sums gv_l[vid, f] of g c (and gm_l of |g| c, c >= 0)
come from that call with the identity as the slot table and unit weights — the trick of _oracle_table_grad_f64 in
tests/test_gpu_step_config_matrix.py — and the dot products with the table rows are formed here in float64.  fp16 tables: E is the
stored value widened (exact)."""
import numpy as np

from . import c_oracle


def vertex_ids(x, n, vstride):
    """(4, P) int64: vid = gy * vstride + gx of the four corners of every pixel's cell at resolution n — the cell arithmetic of
    oracle/gngf_oracle_c.c make_cell and of term_counts (floor of the fp32 product x * n)"""
    ax = np.floor(x[:, 0] * np.float32(n)).astype(np.int64)
    ay = np.floor(x[:, 1] * np.float32(n)).astype(np.int64)
    return np.stack([(ay + (v >> 1)) * vstride + (ax + (v & 1)) for v in range(4)])


def iter_levels(x, n_ls, genc, tables, vidx, vstride, l0=0, l1=None):
    """Per level l in [l0, l1): (l, want_l, mass_l, n_l, absE_l) —
        want_l[vid, k] = sum_f gv_l[vid, f] E_l[idx[vid, k], f]          (NV, K) float64
        mass_l[vid, k] = sum_f gm_l[vid, f] |E_l[idx[vid, k], f]|        (NV, K) float64
        n_l[vid]       = the number of (pixel, corner) terms that reach vid at this level      (NV,) int64
        absE_l[vid, k] = sum_f |E_l[idx[vid, k], f]|                     (NV, K) float64
    x (P, 2) float32, genc (P, L F) float32, tables (L, T, F) float32 or float16, vidx (NV, K) integer."""
    x = np.ascontiguousarray(x, np.float32)
    n_ls = np.ascontiguousarray(n_ls, np.int32)
    L, T, F = tables.shape
    P = x.shape[0]
    NV, K = vidx.shape
    l1 = L if l1 is None else l1
    assert genc.shape == (P, L * F) and 0 <= l0 <= l1 <= L
    ident, ones = np.arange(NV, dtype=np.int32)[:, None].copy(), np.ones((NV, 1), np.float32)
    rows = vidx.astype(np.int64)
    for l in range(l0, l1):
        vid = vertex_ids(x, int(n_ls[l]), vstride)
        assert P == 0 or (int(vid.min()) >= 0 and int(vid.max()) < NV), "a pixel's cell leaves the vertex table"
        assert P == 0 or int(np.floor(x[:, 0].max() * np.float32(n_ls[l]))) + 1 < vstride, "a pixel's cell leaves the table's columns"
        n_l = np.bincount(vid.ravel(), minlength=NV)
        g_l = np.ascontiguousarray(genc.reshape(P, L, F)[:, l, :], np.float32)
        gv, gm = (c_oracle.encode_bwd_f64(x, (1, NV, F), n_ls[l:l + 1], g, ident, ones, vstride, exact_products=True)[0]
                  for g in (g_l, np.abs(g_l)))
        E = tables[l].astype(np.float64)[rows]                              # (NV, K, F)
        want_l = np.einsum("vf,vkf->vk", gv, E)
        mass_l = np.einsum("vf,vkf->vk", gm, np.abs(E))
        yield l, want_l, mass_l, n_l, np.abs(E).sum(-1)


def vertex_weight_grad_f64(x, n_ls, genc, tables, vidx, vstride, l0=0, l1=None):
    """(want, mass, n) of levels [l0, l1): want and mass (NV, K) float64 — the exact gradient of the fp32 inputs and its absolute
    mass sum |g c E| — and n (NV,) int64, the number of (pixel, corner) terms that reach each vertex over those levels."""
    NV, K = vidx.shape
    want, mass, n = np.zeros((NV, K)), np.zeros((NV, K)), np.zeros(NV, np.int64)
    for _l, w_l, m_l, n_l, _e in iter_levels(x, n_ls, genc, tables, vidx, vstride, l0, l1):
        want += w_l
        mass += m_l
        n += n_l
    return want, mass, n
