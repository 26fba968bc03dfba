"""CPU: the float64 oracle of d vert_w (oracle/dvw_oracle.py) and the ONE check every d vert_w of the GPU tests
(tests/test_gpu_encode_dw.py) goes through — check_vertex_weight_grad: EVERY entry of the (NV, K) gradient within a bound relative
to the entry's own absolute mass, entries no pixel reaches exactly zero.  Here the oracle is held to a brute-force float64
restatement, the check is shown to reject the faults a bound relative to the largest entry cannot see, and to accept an fp32
evaluation of the same sums in shuffled order at the very shapes the GPU tests use.

Error model of one entry (vid, k)  (u = 2^-24; terms t = the (pixel, corner) pairs that reach vid, n of them over all levels, n_l at
level l;  m_l = sum_f sum_t |g c| |E_l[row, f]| the level's part of the entry's mass M = sum_l m_l;  row = idx[vid, k]):

  per-term / per-level factors, read off the kernels
    direct levels, encode_bwd_kernel (csrc/encode_direct.hip): per (pixel, corner, k) one lane per feature forms g_f E_f (1 rounding),
        the F lanes meet through log2 F __shfl_xor additions (1 rounding each on the path of any one product), the sum is multiplied
        by c (1), then ONE float atomic:  1 + log2 F + 1 <= F + 1 roundings per term                             -> (F + 1) u m_l
    staged levels, vertex_bwd_kernel / vertex_bwd_sorted_kernel (csrc/encode_tiled.hip): the level's grid value g_l[f] = sum_t g c
        arrives with the error of its sink —
          "fp32_grid": tiled_bwd_kernel / tiled_bwd_il_kernel round each work item's exact fixed-point sum to fp32 once and the
              gather pass adds the (few) items of a vertex in fp32; pixels outside an item's sub-grids add g c with float atomics:
              in every case an fp32 sum of at most n_l terms in any order, the roundings of the products included: (n_l + 2) u
              (the bound tests/test_gpu_step_config_matrix.py holds the same grid to)
          "dG64": the exact 64-bit sum of the whole batch rounded to fp32 ONCE (dg64_to_float_kernel, or on the fly): 1 u
              (the int64 -> double conversion in front of it rounds at 2^-53: not counted)
        then  dot = sum_f g_l[f] E_f, sequentially from 0: F products and F - 1 additions, <= F roundings        -> (sink + F) u m_l
    fixed-point quantisation of the staged levels (both sinks; to_fixed_fma rounds each term g c 2^S to the nearest integer):
        <= 2^-(S+1) per term, n_l 2^-(S+1) on g_l[f], times |E_f|                                       -> n_l 2^-(S+1) sum_f |E_l[row, f]|
        S = 60 - max(10, ceil log2 max(P, chunk)) - e as in check_rows_against_oracle (e one above the exponent of the largest
        |d enc|); a launch without a bound on |d enc| scales each work item by its own rows, which can only be finer.
  additions that bring the per-term / per-level values together — one rounding each, relative to a partial sum <= M(1 + ...):
    B  sorted kernel alone: dw_acc += dot over the staged levels the batch reaches at vid (adding an exact 0 does not round)
    C  vertex_bwd_kernel: one float atomic per staged level into the zeroed buffer, the direct levels' atomics into the same one
    D  direct form alone: n atomics
    A  sorted kernel WRITES its sum to a buffer of its own, the direct levels' n_d atomics go to a zeroed one, torch adds the two (1)
    E, F  as A / B on the fp32 copy of the fixed-point grid
    in every case at most  (staged levels reached) + n_d + 1  additions                                -> (L_reached + n_d + 1) u M
  float atomics may flush a subnormal term or partial sum: an absolute floor of n 2^-120.

  bound = [ sum_{l staged} (sink_l + F) m_l + sum_{l direct} (F + 1) m_l + (L_reached + n_d + 1) M ] u / (1 - k u)  + quantisation + floor,
          k = n + L + F + 3 >= every count of roundings that meet in one entry (the usual gamma_k = k u / (1 - k u) of a first-order
          bound made rigorous),
  and never more than the ceiling (n + L F + 8) u M + quantisation + floor:  sink_l + F <= n_l + 2 + F and n >= max_l n_l(staged) + n_d
  give  bound <= (n + L + F + 3) u M / (1 - k u), and L F + 8 - (L + F + 3) = (L - 1)(F - 1) + 4 > 0: the derived bound lies under the
  ceiling while k^2 u stays below that slack (k up to a few thousand); the second batch of every case crowds up to 10^5 terms on
  one vertex, where the ceiling — first order in u, no allowance for k^2 u^2 — is the smaller one.  The minimum of the two is
  applied, so the ceiling holds everywhere."""
import numpy as np
import pytest

from conftest import PARITY
from oracle import c_oracle, dvw_oracle
from oracle import gngf_oracle as orc
from test_gpu_encode import _coords, _degenerate_tables

U = 2.0 ** -24
SUBNORMAL_FLOOR = 2.0 ** -120
STEP2_SIDE = 0.125                      # pass 2's pixels all lie in [0, STEP2_SIDE)^2
SUBRECT = (0.6, 0.3)                    # the sub-rectangular cases take their pixels from [0, 0.6] x [0, 0.3]

needs_oracle = pytest.mark.skipif(not c_oracle.available(), reason="oracle/libgngf_oracle_c.so not built (make -C oracle)")

# name: (L, n_min, n_max, F, T, K, P) — the shapes of tests/test_gpu_encode_dw.py, each chosen for one branch of EncodeFunction.backward
DW_SHAPES = {
    "direct_f1": (4, 8, 32, 1, 256, 4, 2049), "direct_f2": (4, 8, 32, 2, 256, 4, 2049), "direct_f4": (4, 8, 32, 4, 256, 4, 2049),
    "direct_k1": (4, 8, 32, 2, 256, 1, 2049), "direct_k7": (4, 8, 32, 2, 256, 7, 2049),
    "staged": (4, 8, 32, 2, 256, 4, 2 ** 14), "staged_k1": (4, 8, 32, 2, 256, 1, 2 ** 14), "staged_k7": (4, 8, 32, 2, 256, 7, 2 ** 14),
    "mixed": (16, 16, 512, 2, 2 ** 12, 4, 2 ** 14),
    "generic": (8, 16, 128, 4, 2 ** 12, 3, 2 ** 15),
}


def vertex_extent(mx, my, n_max):
    """(vstride, NV) as models.GeneralNeuralGaugeFields._vertex_extent sizes the table for a batch whose largest coordinates are mx, my"""
    gx_hi = int(np.floor(np.float32(mx) * np.float32(n_max))) + 1
    gy_hi = int(np.floor(np.float32(my) * np.float32(n_max))) + 1
    return gx_hi + 1, (gx_hi + 1) * (gy_hi + 1)


def make_case(name, kind="uniform", fp16=False, subrect=False, seed=0):
    """Inputs of one case, numpy: two batches of the same P (the second in the [0, 1/8)^2 corner), tables uniform in +-0.5, an
    injected vertex table (slots `kind`: "uniform" or one of test_gpu_encode._degenerate_tables), standard normal d enc."""
    L, n_min, n_max, F, T, K, P = DW_SHAPES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name + kind)), int(fp16), int(subrect)])
    n_ls = orc.level_resolutions(n_min, n_max, L)
    x1 = _coords(P, rng)
    x1[100:164] = x1[100]                                        # many pixels in one cell
    if subrect:
        x1 *= np.array(SUBRECT, np.float32)                      # (the edge coordinates too: (0.6, 0.3) is the far corner)
        vstride, NV = vertex_extent(x1[:, 0].max(), x1[:, 1].max(), n_max)
        assert vstride < n_max + 2 and NV // vstride < vstride
    else:
        vstride = n_max + 2
        NV = vstride * vstride
    x2 = (rng.random((P, 2), dtype=np.float32) * np.float32(STEP2_SIDE)).astype(np.float32)
    tables = (rng.random((L, T, F), dtype=np.float32) - 0.5).astype(np.float16 if fp16 else np.float32)
    vidx = (rng.integers(0, T, (NV, K)).astype(np.int32) if kind == "uniform" else _degenerate_tables(kind, NV, K, T, rng))
    vw = rng.random((NV, K), dtype=np.float32)
    g1 = rng.standard_normal((P, L * F)).astype(np.float32)
    g2 = rng.standard_normal((P, L * F)).astype(np.float32)
    return dict(name=name, L=L, F=F, T=T, K=K, P=P, n_ls=n_ls, n_host=[int(n) for n in n_ls], vstride=vstride, NV=NV, tables=tables,
                vidx=vidx, vw=vw, x=(x1, x2), genc=(g1, g2))


def fixed_point_scale(genc, P, chunk):
    """S of the module docstring, exactly as check_rows_against_oracle computes it"""
    import math
    gmax = float(np.abs(genc).max())
    e = math.frexp(gmax)[1] + 1 if gmax > 0 else 0
    return 60 - max(10, (max(P, chunk) - 1).bit_length()) - e


def dvw_error_model(x, n_ls, genc, tables, vidx, vstride, Ls, sink, S):
    """-> (want, mass, n, rel, quant): the oracle's three arrays and the two parts of the module docstring's bound —
    rel (NV, K): the rounding part, already in absolute units; quant (NV, K): the fixed-point quantisation of the staged levels.
    Ls: levels [0, Ls) are staged (sink "fp32_grid" | "dG64"), levels [Ls, L) take the direct form."""
    assert sink in ("fp32_grid", "dG64", "none") and (Ls == 0 or sink != "none")
    L, _T, F = tables.shape
    NV, K = vidx.shape
    want, mass, units, quant = (np.zeros((NV, K)) for _ in range(4))
    n, adds = np.zeros(NV, np.int64), np.ones(NV, np.int64)
    for l, w_l, m_l, n_l, absE in dvw_oracle.iter_levels(x, n_ls, genc, tables, vidx, vstride):
        want += w_l
        mass += m_l
        n += n_l
        if l < Ls:
            sink_units = (n_l + 2)[:, None] if sink == "fp32_grid" else 1
            units += (sink_units + F) * m_l
            quant += (n_l * 2.0 ** -(S + 1))[:, None] * absE
            adds += n_l > 0
        else:
            units += (F + 1) * m_l
            adds += n_l
    k = (n + L + F + 3).astype(np.float64)
    assert float(k.max()) * U < 2.0 ** -4, "the model wants k u well below 1"
    rel = (units + adds[:, None] * mass) * (U / (1.0 - k * U))[:, None]
    return want, mass, n, rel, quant


def check_vertex_weight_grad(tag, got, want, mass, n, rel, quant, L, F, path, record=True):
    """EVERY entry of the (NV, K) gradient `got` against the oracle's `want`: |got - want| <= bound where mass > 0, exactly zero
    where mass == 0 (no pixel reaches the vertex), finite everywhere.  bound = min(rel, ceiling) + quant + floor of the module
    docstring, ceiling = (n + L F + 8) u mass.  `path` names the branch of EncodeFunction.backward that produced `got`; the worst
    |err| / bound and |err| / mass are printed and recorded under it.  -> (worst |err| / bound, worst |err| / mass)"""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape == mass.shape == rel.shape == quant.shape and n.shape == want.shape[:1], (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag} [{path}]: {int((~np.isfinite(got)).sum())} non-finite entries of d vert_w"
    nn = n.astype(np.float64)[:, None]
    ceiling = (nn + L * F + 8) * U * mass
    bound = np.minimum(rel, ceiling) + quant + nn * SUBNORMAL_FLOOR
    err = np.abs(got - want)
    pos = mass > 0
    assert not (pos & (n[:, None] == 0)).any()
    empty_nonzero = ~pos & (got != 0)
    over = pos & (err > bound)
    worst_b = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    worst_m = float((err[pos] / mass[pos]).max()) if pos.any() else 0.0
    print(f"[{tag}] d vert_w [{path}] vs float64 oracle: worst |err|/bound {worst_b:.3f}, |err|/mass {worst_m:.2e} "
          f"({int(pos.sum())} entries with mass, {int((~pos).sum())} without; largest n {int(n.max())})")
    if record:
        PARITY.record(f"{tag}: d vert_w, path {path}: |err| / (bound of the error model), every entry with mass > 0",
                      np.array([worst_b]), np.zeros(1), 0, 1.0)
        PARITY.record(f"{tag}: d vert_w, path {path}: |err| / mass, every entry with mass > 0", np.array([worst_m]), np.zeros(1), 0,
                      float((bound[pos] / mass[pos]).max()) if pos.any() else 0.0)
    if over.any():
        v, k = (int(i) for i in np.argwhere(over)[0])
        raise AssertionError(f"{tag} [{path}]: {int(over.sum())} entries of d vert_w outside the bound; first: vertex {v} k {k}: got "
                             f"{got[v, k]!r} want {want[v, k]!r} mass {mass[v, k]!r} n {int(n[v])} bound {bound[v, k]!r}")
    assert not empty_nonzero.any(), (f"{tag} [{path}]: {int(empty_nonzero.sum())} entries no pixel reaches are not exactly zero; first: "
                                     f"{tuple(int(i) for i in np.argwhere(empty_nonzero)[0])}")
    return worst_b, worst_m


# ------------------------------------------------------------------------------------------------ the oracle against brute force
def _brute_force_f64(x, n_ls, genc, tables, vidx, vstride):
    """The per-instance restatement of tests/test_gpu_encode.py — orc.encoding_backward's `d` = sum_f E[idx] g c per (pixel, level,
    corner, k), gathered per vertex with np.add.at — with every product and sum in float64 (no rounding of g c or of d to fp32)."""
    L, _T, F = tables.shape
    NV, K = vidx.shape
    P = x.shape[0]
    scaled, grid = orc.scale_to_grid(x, n_ls)
    c = orc.bilinear_coeffs(scaled, grid).astype(np.float64)                 # (P, L, 4), the fp32 coefficients
    gi = grid.astype(np.int64)
    vid = gi[:, 1] * vstride + gi[:, 0]                                       # (P, L, 4)
    idx = vidx[vid].astype(np.int64)                                          # (P, L, 4, K)
    feats = tables.astype(np.float64)[np.arange(L)[None, :, None, None], idx]   # (P, L, 4, K, F)
    g = genc.reshape(P, L, 1, 1, F).astype(np.float64)
    terms = (feats * g).sum(-1) * c[..., None]                                # (P, L, 4, K)
    mterms = (np.abs(feats) * np.abs(g)).sum(-1) * c[..., None]
    dvw, mass = np.zeros((NV, K)), np.zeros((NV, K))
    np.add.at(dvw, vid.reshape(-1), terms.reshape(-1, K))
    np.add.at(mass, vid.reshape(-1), mterms.reshape(-1, K))
    return dvw, mass, np.bincount(vid.reshape(-1), minlength=NV)


@needs_oracle
@pytest.mark.parametrize("subrect", [False, True], ids=["full_square", "sub_rectangle"])
def test_oracle_equals_the_brute_force_restatement_in_float64(subrect):
    rng = np.random.default_rng(3 + subrect)
    L, n_min, n_max, F, K, T, P = 3, 4, 11, 2, 3, 8, 300
    n_ls = orc.level_resolutions(n_min, n_max, L)
    x = _coords(P, rng)
    if subrect:
        x *= np.array(SUBRECT, np.float32)
        vstride, NV = vertex_extent(x[:, 0].max(), x[:, 1].max(), n_max)
        assert vstride < n_max + 2 and NV // vstride < vstride, (vstride, NV)
    else:
        vstride, NV = n_max + 2, (n_max + 2) ** 2
    tables = rng.random((L, T, F), dtype=np.float32) - 0.5
    vidx = rng.integers(0, T, (NV, K)).astype(np.int32)
    genc = rng.standard_normal((P, L * F)).astype(np.float32)
    want, mass, n = dvw_oracle.vertex_weight_grad_f64(x, n_ls, genc, tables, vidx, vstride)
    bf, bf_mass, bf_n = _brute_force_f64(x, n_ls, genc, tables, vidx, vstride)
    assert np.array_equal(n, bf_n) and int(n.sum()) == 4 * P * L
    assert np.array_equal(mass > 0, bf_mass > 0) and (mass > 0).any() and (subrect or (mass == 0).any())
    assert np.all(np.abs(want - bf) <= 1e-12 * mass), float((np.abs(want - bf) / np.maximum(mass, 1e-300)).max())
    assert np.all(np.abs(mass - bf_mass) <= 1e-12 * mass)
    # level ranges add up: the staged and the direct contributions can be told apart
    a, ma, na = dvw_oracle.vertex_weight_grad_f64(x, n_ls, genc, tables, vidx, vstride, 0, 2)
    b, mb, nb = dvw_oracle.vertex_weight_grad_f64(x, n_ls, genc, tables, vidx, vstride, 2, L)
    assert np.array_equal(na + nb, n) and np.all(np.abs(a + b - want) <= 1e-14 * mass) and np.all(np.abs(ma + mb - mass) <= 1e-14 * mass)
    # fp16 tables: the stored values, widened
    t16 = tables.astype(np.float16)
    w16, m16, _n = dvw_oracle.vertex_weight_grad_f64(x, n_ls, genc, t16, vidx, vstride)
    bf16, _m, _n = _brute_force_f64(x, n_ls, genc, t16.astype(np.float32), vidx, vstride)
    assert np.all(np.abs(w16 - bf16) <= 1e-12 * m16) and float(np.abs(w16 - want).max()) > 1e-6


# ------------------------------------------------------------------------------------------------ the check against faults and fp32
def _plan(case):
    from collision_handling_in_instantngp_amd import ops
    return ops.EncodePlan(case["P"], case["n_host"], case["F"])


@needs_oracle
def test_the_shapes_select_the_branches_they_were_chosen_for():
    """EncodePlan with the default tuning: which levels each shape stages, and on which pixel-stage kernel"""
    from collision_handling_in_instantngp_amd import ops
    assert ops.TUNING.tiled_min_pixels == 2 ** 14 and ops.TUNING.tiled_cells_per_pixel == 4
    for name, (L, _a, _b, F, _T, _K, P) in DW_SHAPES.items():
        plan = ops.EncodePlan(P, [int(n) for n in orc.level_resolutions(_a, _b, L)], F)
        if name.startswith("direct"):
            assert plan.Ls == 0, name                                        # branch D
        elif name.startswith("staged"):
            assert plan.Ls == L and plan.interleaved(backward=True), name     # branches B, C
        elif name == "mixed":
            assert plan.Ls == 13 and plan.interleaved(backward=True), (name, plan.Ls)     # branch A: 13 staged + 3 direct levels
        else:
            assert plan.Ls == L and not plan.interleaved(backward=True), name     # generic kernels, sink fp32_grid


@pytest.fixture(scope="module")
def mixed_model():
    """the "mixed" shape (13 staged + 3 direct levels), batch 1, with the error model of branch A — shared, never modified"""
    case = make_case("mixed")
    plan = _plan(case)
    x, genc = case["x"][0], case["genc"][0]
    S = fixed_point_scale(genc, case["P"], plan.chunk)
    return case, plan, dvw_error_model(x, case["n_ls"], genc, case["tables"], case["vidx"], case["vstride"], plan.Ls, "fp32_grid", S)


@needs_oracle
def test_check_rejects_a_vertex_that_loses_the_finest_staged_level(mixed_model):
    case, plan, (want, mass, n, rel, quant) = mixed_model
    l = plan.Ls - 1
    w_l, _m, n_l = dvw_oracle.vertex_weight_grad_f64(case["x"][0], case["n_ls"], case["genc"][0], case["tables"], case["vidx"],
                                                     case["vstride"], l, l + 1)
    reached = np.flatnonzero(n_l > 0)
    # the vertex of that level with the MOST terms over all levels (where a bound relative to the largest entry is blind) and the
    # one with the fewest
    for vid in (reached[np.argmax(n[reached])], reached[np.argmin(n[reached])]):
        got = want.copy()
        got[vid] -= w_l[vid]
        with pytest.raises(AssertionError, match="outside the bound"):
            check_vertex_weight_grad("fault: level lost", got, want, mass, n, rel, quant, case["L"], case["F"], "A", record=False)
    check_vertex_weight_grad("no fault", want.copy(), want, mass, n, rel, quant, case["L"], case["F"], "A", record=False)


@needs_oracle
def test_check_rejects_a_single_lost_term_a_swapped_row_pair_and_a_stale_entry(mixed_model):
    case, plan, (want, mass, n, rel, quant) = mixed_model
    L, F, K = case["L"], case["F"], case["K"]
    x, genc, tables, vidx, vstride = case["x"][0], case["genc"][0], case["tables"], case["vidx"], case["vstride"]
    # one (pixel, corner) term: pixel 1000, corner 3, at the coarsest level (the vertex collects hundreds of terms) and at the finest
    scaled, grid = orc.scale_to_grid(x[1000:1001], case["n_ls"])
    c = orc.bilinear_coeffs(scaled, grid).astype(np.float64)[0]              # (L, 4)
    gi = grid.astype(np.int64)[0]                                            # (2, L, 4)
    for l in (0, L - 1):
        vid = int(gi[1, l, 3] * vstride + gi[0, l, 3])
        term = (tables[l].astype(np.float64)[vidx[vid]] * genc[1000].reshape(L, F)[l].astype(np.float64)).sum(-1) * c[l, 3]
        assert c[l, 3] > 0 and n[vid] > (100 if l == 0 else 0)
        got = want.copy()
        got[vid] -= term
        with pytest.raises(AssertionError, match="outside the bound"):
            check_vertex_weight_grad("fault: term lost", got, want, mass, n, rel, quant, L, F, "A", record=False)
    # rows idx[vid, k] and idx[vid, (k + 1) % K] swapped for one vertex
    vid = int(np.argmax(n))
    assert len(set(vidx[vid].tolist())) == K
    got = want.copy()
    got[vid] = np.roll(want[vid], -1)
    with pytest.raises(AssertionError, match="outside the bound"):
        check_vertex_weight_grad("fault: rows swapped", got, want, mass, n, rel, quant, L, F, "A", record=False)
    # a vertex no pixel reaches holds 1e-30
    vid = int(np.flatnonzero(n == 0)[0])
    assert (mass[vid] == 0).all()
    got = want.copy()
    got[vid, 0] = 1e-30
    with pytest.raises(AssertionError, match="not exactly zero"):
        check_vertex_weight_grad("fault: stale entry", got, want, mass, n, rel, quant, L, F, "A", record=False)
    got[vid, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_vertex_weight_grad("fault: NaN", got, want, mass, n, rel, quant, L, F, "A", record=False)


def _fp32_shuffled(case, x, genc, Ls, rng):
    """d vert_w as the kernels form it, in numpy float32 with the terms in shuffled order: levels [0, Ls) through an fp32 vertex
    grid (one fp32 product g c per term, added one by one), the sequential dot product per (vertex, k) and one addition per level;
    levels [Ls, L) one term per (pixel, corner, k) — the products g_f E_f added pairwise, times c — added one by one."""
    f32 = np.float32
    L, F, K, NV, vstride = case["L"], case["F"], case["K"], case["NV"], case["vstride"]
    tables, vidx = case["tables"].astype(f32), case["vidx"].astype(np.int64)
    P = x.shape[0]
    scaled, grid = orc.scale_to_grid(x, case["n_ls"])
    c = orc.bilinear_coeffs(scaled, grid)                                     # (P, L, 4) fp32
    gi = grid.astype(np.int64)
    vid = gi[:, 1] * vstride + gi[:, 0]                                       # (P, L, 4)
    g = genc.reshape(P, L, F)
    out = np.zeros((NV, K), f32)
    for l in range(Ls):
        perm = rng.permutation(P * 4)
        G = np.zeros((NV, F), f32)
        np.add.at(G, vid[:, l].reshape(-1)[perm], (g[:, l, None, :] * c[:, l, :, None]).astype(f32).reshape(-1, F)[perm])
        E = tables[l][vidx]                                                   # (NV, K, F)
        dot = np.zeros((NV, K), f32)
        for f in range(F):
            dot = (dot + (G[:, None, f] * E[:, :, f]).astype(f32)).astype(f32)
        out = (out + dot).astype(f32)
    if Ls < L:
        rows, vals = [], []
        for l in range(Ls, L):
            E = tables[l][vidx[vid[:, l]]]                                    # (P, 4, K, F)
            pr = (E * g[:, l, None, None, :]).astype(f32)
            while pr.shape[-1] > 1:                                           # the lanes' pairwise (butterfly) sum
                pr = (pr[..., 0::2] + pr[..., 1::2]).astype(f32)
            vals.append((pr[..., 0] * c[:, l, :, None]).astype(f32).reshape(-1, K))
            rows.append(vid[:, l].reshape(-1))
        rows, vals = np.concatenate(rows), np.concatenate(vals)
        perm = rng.permutation(rows.shape[0])
        direct = np.zeros((NV, K), f32)
        np.add.at(direct, rows[perm], vals[perm])
        out = (out + direct).astype(f32)
    return out


@needs_oracle
@pytest.mark.parametrize("name,fp16,subrect", [("direct_f1", False, False), ("direct_f2", False, False), ("direct_f4", False, False),
                                               ("direct_k7", False, False), ("staged", False, False), ("staged", False, True),
                                               ("staged_k7", False, False), ("mixed", False, False), ("mixed", False, True),
                                               ("generic", False, False), ("generic", True, False)])
def test_check_accepts_an_fp32_evaluation_in_shuffled_order_at_the_gpu_shapes(name, fp16, subrect):
    """the reference alone stays inside the bound: both batches of the case (the second crowds every pixel into one corner: the
    largest n), with the levels staged as the plan stages them"""
    case = make_case(name, fp16=fp16, subrect=subrect)
    plan = _plan(case)
    rng = np.random.default_rng(11)
    for b in (0, 1):
        x, genc = case["x"][b], case["genc"][b]
        S = fixed_point_scale(genc, case["P"], getattr(plan, "chunk", 0))
        for Ls in (plan.Ls,):
            got = _fp32_shuffled(case, x, genc, Ls, rng)
            want, mass, n, rel, quant = dvw_error_model(x, case["n_ls"], genc, case["tables"], case["vidx"], case["vstride"], Ls,
                                                        "fp32_grid" if Ls else "none", S)
            wb, _wm = check_vertex_weight_grad(f"{name} fp16={fp16} subrect={subrect} batch {b + 1} Ls={Ls}", got, want, mass, n, rel,
                                               quant, case["L"], case["F"], "numpy float32, shuffled", record=False)
            assert 0 < wb <= 1
            if b == 1:
                assert (n[:, None] * np.ones_like(mass))[mass > 0].max() >= case["P"] // 8       # a vertex with thousands of terms
