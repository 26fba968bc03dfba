"""GPU: every gradient path held to float64 while the gradient's exponent moves over E = (-90 ... +90) (tests/grad_scale_cases.py).

Every backward path that avoids float atomics picks a power-of-two fixed-point scale from the gradient's exponent at run time
(pixel stage: S = min(126, 60 - max(10, log2 terms) - eg); bucketed direct levels: S = min(50, 61 - ceil log2 n) - (e + 1)); the
vertex stage reads the grid back with 2^-S.  Scaling an fp32 gradient by 2^k is exact, so
  * on the paths that sum integers or have no atomics the result at scale 2^k is 2^k times the result at scale 1 BIT FOR BIT while
    S is not clamped (S_k == S_0 - k) and the entry has all its 24 bits at both scales (the exactness mask; its preconditions are
    checked from the oracle alone in tests/test_grad_scale_cpu.py);
  * on every path, every entry stays within the project's own float64 bound of that path — with the CLAMPED S in the quantisation
    term: below gmax = 2^-76 the scale stops at 126 and a sum of n terms is quantised to n 2^-127, absolute.
Groups: A pixel-stage backward, B head-room at its limit, C the vertex stage reading a grid whose scale word is not 0, D bucketed
direct levels, E the direct float-atomic form, F the decoder kernels, G Adam with 1 / loss scale, H one model-level step per form.
The worst |err| / bound per path and exponent is printed and recorded (conftest.PARITY)."""
import ctypes

import numpy as np
import pytest
import torch

import grad_scale_cases as gsc
from conftest import PARITY
from oracle import c_oracle
from test_gpu_step_config_matrix import STAGED_REL, U

pytestmark = pytest.mark.gpu
DEV = "cuda"
needs_oracle = pytest.mark.skipif(not c_oracle.available(), reason="oracle/libgngf_oracle_c.so not built (make -C oracle)")


def t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def held(tag, got, want, bound, mass=None):
    """every entry: |got - want| <= bound, finite, exactly zero where no term arrives (mass == 0); prints and records the worst
    |err| / bound -> that ratio"""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape == bound.shape, (tag, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} non-finite entries"
    err = np.abs(got - want)
    if mass is not None:
        assert not (got[mass == 0] != 0).any(), f"{tag}: entries no term reaches are not exactly zero"
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"[{tag}] worst |err| / bound {worst:.3f}")
    PARITY.record(f"{tag}: |err| / bound, every entry", np.array([worst]), np.zeros(1), 0, 1.0)
    over = err > bound
    if over.any():
        i = tuple(int(v) for v in np.argwhere(over)[0])
        raise AssertionError(f"{tag}: {int(over.sum())} entries outside the bound; first {i}: got {got[i]!r} want {want[i]!r} bound {bound[i]!r}")
    return worst


def bit_equal_scaled(tag, got_k, got_0, want_0, k):
    """got_k == got_0 2^k bit for bit, on the entries of the exactness mask (float32 numpy arrays; want_0 float64 at scale 1)"""
    m = gsc.exact_mask(want_0, k)
    a = got_k[m]
    b = np.ldexp(got_0[m].astype(np.float64), k).astype(np.float32)
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    assert bad.size == 0, (f"{tag}: {bad.size} of {int(m.sum())} entries differ from 2^{k} times the result at scale 1; first: "
                           f"{a[bad[0]]!r} vs {b[bad[0]]!r}")
    assert m.mean() > 0.5


# ================================================================================================ A. pixel-stage backward
class _Pixel:
    """one geometry x feature width: inputs on the GPU, ONE binning, the float64 expectations at scale 1"""

    def __init__(self, ops, geometry, F):
        case = gsc.pixel_case(geometry, F)
        self.ops, self.case, self.F = ops, case, F
        self.P, self.L, self.T = case["P"], case["L"], case["T"]
        self.n_host = [int(n) for n in case["n_ls"]]
        self.n_t = t(case["n_ls"], torch.int32)
        self.plan = ops.EncodePlan(self.P, self.n_host, F, "tiled")
        assert self.plan.Ls == self.L
        self.ws = ops.TiledWorkspace(self.plan, t(case["x"]))                    # binning only
        c, gx, gy = gsc.corner_terms(case["x"], case["n_ls"])
        vid, vtot = gsc.vertex_grid_index(gx, gy, case["n_ls"])
        assert vtot == self.plan.vtot
        self.grid = gsc.sums_f64(vid, vtot, c, case["g"], F)                    # (want, mass, n) at scale 1
        rows = gsc.hash_rows(gx, gy, self.T) + (np.arange(self.L) * self.T)[None, :, None]
        self.rows = gsc.sums_f64(rows, self.L * self.T, c, case["g"], F)
        self.gmax = float(np.abs(case["g"]).max())

    def genc(self, k):
        return t(gsc.scaled(self.case["g"], k))

    def bound_of(self, k):
        return (torch.full((1,), self.gmax * 2.0 ** k, device=DEV), 1, 0)

    def S(self, k, launch_scale):
        return gsc.pixel_scale(self.gmax * 2.0 ** k, gsc.pixel_log2_terms(self.P, self.plan.chunk, launch_scale))

    def expect(self, which, k, rel, S):
        """(want, bound, mass) at scale k: rel |mass| (rel None: (n + 2) u) + n 2^-(S + 1) + the final rounding"""
        want, mass, n = self.grid if which == "grid" else self.rows
        nn = n.astype(np.float64)[:, None]
        r = (nn + 2) * U if rel is None else rel
        return np.ldexp(want, k), r * np.ldexp(mass, k) + nn * 2.0 ** -(S + 1) + gsc.FINAL_ROUNDING, mass


@pytest.fixture(scope="module")
def ops():
    from collision_handling_in_instantngp_amd import ops as o
    return o


def _interleaving(on):
    from collision_handling_in_instantngp_amd import _lib
    return _lib.query("gngf_set_tiled_interleaved", 1 if on else 0)


PIXEL_KERNELS = [("interleaved", 2), ("generic", 1), ("generic", 2), ("generic", 4)]


@needs_oracle
@pytest.mark.parametrize("geometry", list(gsc.PIXEL_GEOMETRIES))
@pytest.mark.parametrize("kernel,F", PIXEL_KERNELS, ids=[f"{k}-F{f}" for k, f in PIXEL_KERNELS])
def test_a_pixel_stage_sinks_follow_the_gradient_exponent(ops, geometry, kernel, F):
    """tiled_bwd_il_kernel (F = 2) and tiled_bwd_kernel (F = 1, 2 with interleaving switched off, 4), driven as
    test_fixed_point_vertex_grid_is_exact_and_order_free drives them, at every k of E; sinks: the fixed-point grid with its fp32
    conversion (interleaved kernel, bound given), table rows added by the store pass, the fp32 grid through partial images — each
    with a bound on |d enc| and without.  Bounds: the error model of tests/test_gpu_step_config_matrix.py — STAGED_REL for the exact
    sums rounded once, (n + 2) u mass for the fp32 grid, n 2^-(S + 1) with the clamped S — plus 2^-150 for the final rounding."""
    px = _Pixel(ops, geometry, F)
    plan, ws, n_t, L, T = px.plan, px.ws, px.n_t, px.L, px.T
    prev = _interleaving(kernel == "interleaved")
    try:
        assert plan.interleaved(backward=True) == (kernel == "interleaved")
        tag0 = f"A {geometry} {kernel} F={F}"
        # the table gradient of the scaled d enc from the C oracle, once per k: the expectation of the rows sink
        shape = (L, T, F)
        base = {}
        for k in (0,) + tuple(k for k in gsc.E if k != 0):       # scale 1 first: the base of the bit-for-bit comparisons
            gk = gsc.scaled(px.case["g"], k)
            want_c = c_oracle.encode_bwd_f64(px.case["x"], shape, px.case["n_ls"], gk, exact_products=True).reshape(-1, F)
            want, bound, mass = px.expect("rows", k, STAGED_REL[("hash", "table_rows")], 126)
            assert np.all(np.abs(want_c - want) <= 1e-13 * np.ldexp(mass, k)), "numpy restatement vs c_oracle.encode_bwd_f64"
            genc = px.genc(k)
            for bounded in (True, False):
                am = px.bound_of(k) if bounded else None
                S = px.S(k, False)
                # --- table rows added by the store pass
                dt = torch.zeros((L, T, F), dtype=torch.float32, device=DEV)
                trace = []
                prev_trace, ops.PIXEL_BWD_TRACE = ops.PIXEL_BWD_TRACE, trace
                try:
                    ops._pixel_bwd(plan, ws, n_t, genc, None, L, F, am, None, (dt, T), None)
                finally:
                    ops.PIXEL_BWD_TRACE = prev_trace
                assert trace[0]["direct_hash"] and trace[0]["interleaved"] == (kernel == "interleaved")
                want, bound, mass = px.expect("rows", k, STAGED_REL[("hash", "table_rows")], S)
                held(f"{tag0} rows bound={bounded} k={k}", dt.cpu().numpy().reshape(-1, F), want_c, bound, mass)
                # --- the fp32 grid through partial images + gather
                dG = torch.zeros((plan.vtot, F), dtype=torch.float32, device=DEV)
                ops._pixel_bwd(plan, ws, n_t, genc, dG, L, F, am, None)
                want, bound, mass = px.expect("grid", k, None, S)
                got = dG.cpu().numpy()
                held(f"{tag0} fp32 grid bound={bounded} k={k}", got, want, bound, mass)
                if k == 0:
                    base["grid", bounded] = got
                elif k in gsc.pixel_unclamped_ks(2.0 ** gsc.G_LO, gsc.pixel_log2_terms(px.P, plan.chunk, False)):
                    # no atomics on this path for in-domain pixels (one thread per vertex adds its items in a fixed order)
                    bit_equal_scaled(f"{tag0} fp32 grid bound={bounded} k={k}", got, base["grid", bounded], px.grid[0], k)
            if kernel != "interleaved":
                continue
            # --- the fixed-point grid and its fp32 conversion (one scale for the launch)
            S = px.S(k, True)
            dG64 = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
            dG = torch.full((plan.vtot, F), float("nan"), dtype=torch.float32, device=DEV)
            ops._pixel_bwd(plan, ws, n_t, genc, dG, L, F, px.bound_of(k), None, None, dG64)
            q = dG64.cpu().numpy()
            assert int(q[-2]) == S and int(q[-1]) == 0, (k, int(q[-2]), S, int(q[-1]))
            want, bound, mass = px.expect("grid", k, STAGED_REL[("hash", "dG64")], S)
            got = dG.cpu().numpy()
            held(f"{tag0} dG64 -> fp32 k={k}", got, want, bound, mass)
            nn = px.grid[2].astype(np.float64)[:, None]           # the integers themselves: nothing but the quantisation of the terms
            held(f"{tag0} dG64 integers k={k}", q[:-2].reshape(-1, F).astype(np.float64) * 2.0 ** -S, want,
                 nn * 2.0 ** -(S + 1) + 1e-13 * np.ldexp(mass, k), mass)
            if k == 0:
                base["q"], base["dG"], S0 = q[:-2].copy(), got, S
            if k == -90:
                assert S == 126
        if kernel == "interleaved":
            unclamped = gsc.pixel_unclamped_ks(px.gmax, gsc.pixel_log2_terms(px.P, plan.chunk, True))
            assert unclamped == (-40, -12, 0, 12, 40, 90)
            for k in unclamped:              # (run again in this order: the base is the k = 0 launch above)
                dG64 = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
                dG = torch.full((plan.vtot, F), float("nan"), dtype=torch.float32, device=DEV)
                ops._pixel_bwd(plan, ws, n_t, px.genc(k), dG, L, F, px.bound_of(k), None, None, dG64)
                q = dG64.cpu().numpy()
                assert int(q[-2]) == S0 - k and int(q[-1]) == 0
                assert np.array_equal(q[:-2], base["q"]), f"{tag0}: the fixed-point integers at k={k} differ from those at k=0"
                bit_equal_scaled(f"{tag0} dG64 -> fp32 k={k}", dG.cpu().numpy(), base["dG"], px.grid[0], k)
    finally:
        _interleaving(prev)


@pytest.mark.parametrize("kernel,F", PIXEL_KERNELS, ids=[f"{k}-F{f}" for k, f in PIXEL_KERNELS])
def test_a_zero_gradient_with_bound_zero_and_non_finite_bounds(ops, kernel, F):
    """d enc == 0 with bound 0: every output exactly zero (the fp32 grid of the conversion starts as 0xFF bytes), the scale word the
    restated S, no poison; an infinite bound behaves as a NaN bound does: everything the batch reaches is NaN, the poison word set."""
    px = _Pixel(ops, "small", F)
    plan, ws, n_t, L, T = px.plan, px.ws, px.n_t, px.L, px.T
    prev = _interleaving(kernel == "interleaved")
    try:
        zero = torch.zeros((px.P, L * F), device=DEV)
        am0 = (torch.zeros((1,), device=DEV), 1, 0)
        dt = torch.zeros((L, T, F), device=DEV)
        ops._pixel_bwd(plan, ws, n_t, zero, None, L, F, am0, None, (dt, T), None)
        dG = torch.zeros((plan.vtot, F), device=DEV)
        ops._pixel_bwd(plan, ws, n_t, zero, dG, L, F, am0, None)
        assert bool((dt == 0).all()) and bool((dG == 0).all())
        reached_rows, reached_grid = t(px.rows[1] > 0).reshape(L, T, F), t(px.grid[1] > 0)
        for bad in (float("inf"), float("nan")):
            amb = (torch.full((1,), bad, device=DEV), 1, 0)
            dt = torch.zeros((L, T, F), device=DEV)
            ops._pixel_bwd(plan, ws, n_t, px.genc(0), None, L, F, amb, None, (dt, T), None)
            assert bool(torch.isnan(dt[reached_rows]).all()), f"a bound of {bad} poisons every row the batch reaches"
            dG = torch.zeros((plan.vtot, F), device=DEV)
            ops._pixel_bwd(plan, ws, n_t, px.genc(0), dG, L, F, amb, None)
            assert bool(torch.isnan(dG[reached_grid]).all()) and not bool(torch.isfinite(dG[reached_grid]).any())
        if kernel == "interleaved":
            dG64 = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
            dG = torch.empty((plan.vtot, F), dtype=torch.float32, device=DEV)
            dG.view(torch.uint8).fill_(0xFF)
            ops._pixel_bwd(plan, ws, n_t, zero, dG, L, F, am0, None, None, dG64)
            q = dG64.cpu().numpy()
            assert int(q[-2]) == gsc.pixel_scale(0.0, gsc.pixel_log2_terms(px.P, plan.chunk, True)) == 50 and int(q[-1]) == 0
            assert not q[:-2].any() and bool((dG == 0).all()) and not bool(torch.isnan(dG).any())
            for bad in (float("inf"), float("nan")):
                dG64 = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
                dG = torch.zeros((plan.vtot, F), dtype=torch.float32, device=DEV)
                ops._pixel_bwd(plan, ws, n_t, px.genc(0), dG, L, F, (torch.full((1,), bad, device=DEV), 1, 0), None, None, dG64)
                assert bool(torch.isnan(dG).all()) and int(dG64[-1]) != 0, bad
    finally:
        _interleaving(prev)


# ================================================================================================ B. head-room at its limit
def _bucketed(x, n_ls, g, L, T, F, image):
    from collision_handling_in_instantngp_amd import _lib
    P = x.shape[0]
    plan = (ctypes.c_int64 * 6)()
    assert _lib.query("gngf_encode_bwd_bucketed_plan", P, F, T, L, image, plan) == 1
    dt = torch.zeros((L, T, F), device=DEV)
    matrix = torch.empty((plan[3],), dtype=torch.int32, device=DEV)
    base = torch.empty((plan[4],), dtype=torch.int32, device=DEV)
    items = torch.empty((plan[5],), dtype=torch.uint8, device=DEV)
    _lib.call("gngf_encode_bwd_bucketed", _lib.ptr(x), _lib.ptr(n_ls), _lib.ptr(g), _lib.ptr(dt), P, L, F, T, 0, L, image, 1,
              _lib.ptr(matrix), _lib.ptr(base), _lib.ptr(items), _lib.ptr(None), _lib.stream_ptr())
    torch.cuda.synchronize()
    return dt


@pytest.mark.parametrize("P", gsc.HEADROOM_P)
def test_b_head_room_at_its_limit(ops, P):
    """All P pixels on one point that is a vertex of every level (weights 1, 0, 0, 0), every gradient +-(2 - 2^-23) 2^e, the bound
    equal to that value: the "overflow is impossible" sentence of the pixel stage (sum < 2^60) and of a bucket (sum < 2^61) at the
    tight end.  Expected float32(P g) EXACTLY — alternating signs: 0 (even P) or g (odd P) — in the fixed-point grid, in the table
    rows (exact while one work item holds the batch; several items' sums, each rounded once, meet in float adds: STAGED_REL) and in
    the bucketed form (one row receives the P terms)."""
    F, T = 2, 4096
    L = len(gsc.HEADROOM_N)
    n_host = list(gsc.HEADROOM_N)
    plan = ops.EncodePlan(P, n_host, F, "tiled")
    assert plan.Ls == L and plan.interleaved(backward=True)
    n_t = t(np.array(n_host, np.int32), torch.int32)
    x0 = np.full((P, 2), 0.5, np.float32)
    _c, gx, gy = gsc.corner_terms(x0[:1], np.array(n_host, np.int32))
    vid, vtot = gsc.vertex_grid_index(gx, gy, n_host)
    hit_v = vid[0, :, 0]                                                          # the corner of weight 1, per level
    rows4 = gsc.hash_rows(gx, gy, T)[0]                                           # (L, 4)
    hit_r = rows4[:, 0]
    x_t = t(x0)
    ws = ops.TiledWorkspace(plan, x_t)                                            # binning only
    n_items = int(ws.n_items[0].item())
    assert n_items == -(-P // plan.chunk)
    for e in gsc.HEADROOM_E:
        for signs in gsc.HEADROOM_SIGNS:
            _x, g, _n, v, want = gsc.headroom_case(P, e, signs, F)
            tag = f"B P={P} e={e} {signs}"
            genc, am = t(g), (torch.full((1,), float(v), device=DEV), 1, 0)
            S = gsc.pixel_scale(float(v), gsc.pixel_log2_terms(P, plan.chunk, True))
            # fixed-point grid
            dG64 = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
            dG = torch.full((plan.vtot, F), float("nan"), dtype=torch.float32, device=DEV)
            ops._pixel_bwd(plan, ws, n_t, genc, dG, L, F, am, None, None, dG64)
            q = dG64.cpu().numpy()
            total = int(round(float(g[:, 0].astype(np.float64).sum()) * 2.0 ** S))
            assert int(q[-2]) == S and int(q[-1]) == 0 and abs(total) < 2 ** 60
            qq = q[:-2].reshape(-1, F)
            assert np.all(qq[hit_v] == total), (tag, qq[hit_v].tolist(), total)
            rest = np.ones(vtot, bool)
            rest[hit_v] = False
            assert not qq[rest].any()
            got = dG.cpu().numpy()
            assert np.all(got[hit_v] == want) and not got[rest].any(), (tag, got[hit_v].tolist(), float(want))
            # table rows
            dt = torch.zeros((L, T, F), dtype=torch.float32, device=DEV)
            ops._pixel_bwd(plan, ws, n_t, genc, None, L, F, am, None, (dt, T), None)
            got = dt.cpu().numpy()
            at = got[np.arange(L), hit_r]                                          # (L, F)
            if n_items == 1:
                assert np.all(at == want), (tag, at.tolist(), float(want))
            else:
                assert np.all(np.abs(at.astype(np.float64) - float(want)) <= STAGED_REL[("hash", "table_rows")] * P * float(v)), (tag, at.tolist())
            got[np.arange(L), hit_r] = 0
            assert not got.any(), tag
            # bucketed form: one bucket per level (T = 300, the 64 KiB image)
            Tb = 300
            rb = gsc.hash_rows(gx, gy, Tb)[0]
            db = _bucketed(x_t, n_t, genc, L, Tb, F, 65536).cpu().numpy()
            assert np.all(db[np.arange(L), rb[:, 0]] == want), (tag, db[np.arange(L), rb[:, 0]].tolist(), float(want))
            db[np.arange(L), rb[:, 0]] = 0
            assert not db.any(), tag


# ================================================================================================ C. vertex stage, scale word != 0
VERTEX_S = (-70, -1, 0, 1, 50, 126)
VERTEX_SHAPES = [((16, 23, 33), 4), ((14, 30), 1)]


def _vertex_expect(gi, wk, dest, rows, q, S, Fd):
    terms = wk.astype(np.float64)[:, None] * (q.astype(np.float64) * 2.0 ** -S)[gi]
    want, mass = np.zeros((rows, Fd)), np.zeros((rows, Fd))
    np.add.at(want, dest, terms)
    np.add.at(mass, dest, np.abs(terms))
    n_run = np.bincount(dest, minlength=rows).astype(np.float64)
    return want, mass, (n_run[:, None] + 2) * U * mass


@pytest.mark.parametrize("n_ls,K", VERTEX_SHAPES, ids=["n16_23_33-K4", "n14_30-K1"])
@pytest.mark.parametrize("exact", [False, True], ids=["rounded", "exact"])
def test_c_vertex_stage_reads_the_scale_word(ops, n_ls, K, exact):
    """gngf_vertex_grid_bwd_flat and vertex_bwd_sorted (ops._vertex_bwd(..., order, dG64)) on a host-built fixed-point grid of random
    40-bit signed integers q with scale words S in (-70, -1, 0, 1, 50, 126): the float64 sum of w q 2^-S at the (n_run + 2) 2^-24
    mass bound of tests/test_gpu_vertex_bwd_flat.py ("rounded"); with w in {1, 2} the result at S is exactly 2^-S times the result
    at 0 (every product and the conversion scale exactly; the sums meet in the same order: no atomics between the items of a row
    — flat form — or float adds of exactly scaled values)."""
    from test_gpu_vertex_bwd_flat import F as Fd, _launch, _list, _table
    T = 2048
    lst, gi, wk, dest, vtot = _list(n_ls, K, T, "uniform", 51, exact=exact)
    vi_np, w_np, vstride = _table(n_ls, K, T, "uniform", 51, exact)
    rows = len(n_ls) * T
    rng = np.random.default_rng(52)
    q = rng.integers(-2 ** 40, 2 ** 40, size=(vtot, Fd)).astype(np.int64)
    n_host = list(n_ls)
    plan = ops.EncodePlan(4096, n_host, Fd, "tiled")
    assert plan.Ls == len(n_ls) and plan.vtot == vtot
    n_t = t(np.array(n_host, np.int32), torch.int32)
    vi, vw = t(vi_np, torch.int32), t(w_np)
    order = ops.slot_order(vi, n_host, vstride)
    tables = torch.zeros((len(n_ls), T, Fd), device=DEV)
    base = {}
    for S in (0,) + tuple(s for s in VERTEX_S if s != 0):
        dG64 = torch.as_tensor(np.concatenate([q.reshape(-1), [S, 0]])).to(DEV)
        want, mass, bound = _vertex_expect(gi, wk, dest, rows, q, S, Fd)
        dt_f = torch.zeros((rows, Fd), dtype=torch.float32, device=DEV)
        _launch(lst, None, dG64, dt_f, rows)
        dt_s = torch.zeros((len(n_ls), T, Fd), dtype=torch.float32, device=DEV)
        ops._vertex_bwd(plan, tables, vi, vw, n_t, vstride, None, dt_s, None, order, dG64)
        torch.cuda.synchronize()
        for path, got in (("flat", dt_f.cpu().numpy()), ("sorted", dt_s.cpu().numpy().reshape(rows, Fd))):
            held(f"C {path} n={n_ls} K={K} {'exact' if exact else 'rounded'} S={S}", got, want, bound + gsc.FINAL_ROUNDING, mass)
            if exact and path == "flat":
                if S == 0:
                    base[path] = got
                else:
                    b = np.ldexp(base[path].astype(np.float64), -S).astype(np.float32)
                    assert np.array_equal(got.view(np.uint32), b.view(np.uint32)), f"C {path} S={S}: not 2^-S times the result at S=0"


@pytest.mark.parametrize("S", VERTEX_S)
def test_c_hash_source_reads_the_scale_word(ops, S):
    """the spatial-hash vertex stage behind the interleaved pixel-stage launch (dg64_to_float + vertex_bwd_kernel): a zero d enc
    with a bound chosen so that the launch's scale is S leaves a pre-filled fixed-point grid as it is — the table rows are the
    float64 sums of q 2^-S over the vertices that hash to them, at the (n_run + 2) 2^-24 mass bound"""
    F, (P, n_min, n_max, L, T) = 2, gsc.PIXEL_GEOMETRIES["small"]
    px = _Pixel(ops, "small", F)
    plan = px.plan
    log2_terms = gsc.pixel_log2_terms(P, plan.chunk, True)
    bound_val = 2.0 ** (60 - max(10, log2_terms) - S - 1)                        # eg = 60 - 10 - S
    assert gsc.pixel_scale(bound_val, log2_terms) == S
    rng = np.random.default_rng([60, S + 100])
    q = rng.integers(-2 ** 40, 2 ** 40, size=(plan.vtot, F)).astype(np.int64)
    dG64 = torch.as_tensor(np.concatenate([q.reshape(-1), [0, 0]])).to(DEV)
    dG = torch.full((plan.vtot, F), float("nan"), dtype=torch.float32, device=DEV)
    dt = torch.zeros((L, T, F), dtype=torch.float32, device=DEV)
    prev = _interleaving(True)
    try:
        ops._pixel_bwd(plan, px.ws, px.n_t, torch.zeros((P, L * F), device=DEV), dG, L, F,
                       (torch.full((1,), bound_val, device=DEV), 1, 0), None, (dt, T), dG64)
    finally:
        _interleaving(prev)
    out = dG64.cpu().numpy()
    assert int(out[-2]) == S and int(out[-1]) == 0 and np.array_equal(out[:-2].reshape(-1, F), q)
    g64 = q.astype(np.float64) * 2.0 ** -S
    assert np.array_equal(dG.cpu().numpy(), g64.astype(np.float32))              # one rounding
    # every vertex of every level grid adds to row hash(gx, gy)
    dest, goff = [], 0
    for l, n in enumerate(px.n_host):
        gy, gx = np.divmod(np.arange((n + 2) ** 2, dtype=np.int64), n + 2)
        dest.append(l * T + gsc.hash_rows(gx[:, None, None], gy[:, None, None], T)[:, 0, 0])
    dest = np.concatenate(dest)
    want, mass, bound = _vertex_expect(np.arange(plan.vtot), np.ones(plan.vtot, np.float32), dest, L * T, q, S, F)
    held(f"C hash source S={S}", dt.cpu().numpy().reshape(-1, F), want, bound + gsc.FINAL_ROUNDING, mass)


# ================================================================================================ D. bucketed direct levels
@needs_oracle
@pytest.mark.parametrize("name", list(gsc.BUCKET_SHAPES))
def test_d_bucketed_direct_levels_follow_the_gradient_exponent(ops, name):
    """csrc/encode_bucket.hip through _bucketed of tests/test_gpu_bucket.py, at every k of E: its own bound (6.0e-8 |want| + the
    quantum per term, scaled) against the reference's fp32 terms summed in double, and — the bucket scale is never clamped — bit
    equality with k = 0 at every k (integer sums, one rounding)."""
    from collision_handling_in_instantngp_amd import _lib
    from test_gpu_bucket import _bucketed as bucketed
    case = gsc.bucket_case(name)
    P, L, T, F, l0, l1, image = (case[k] for k in ("P", "L", "T", "F", "l0", "l1", "image"))
    x, n_ls, g = case["x"], case["n_ls"], case["g"]
    tx, tn = t(x), t(n_ls, torch.int32)
    c, gx, gy = gsc.corner_terms(x, n_ls)
    rows = gsc.hash_rows(gx, gy, T) + (np.arange(L) * T)[None, :, None]
    count = np.bincount(rows.reshape(-1), minlength=L * T).reshape(L, T, 1).astype(np.float64)
    room = min(50, 61 - int(np.ceil(np.log2(max(1.0, count.max())))))
    want0 = c_oracle.encode_bwd_f64(x, (L, T, F), n_ls, g)
    base = None
    for k in (0,) + tuple(k for k in gsc.E if k != 0):
        gk = gsc.scaled(g, k)
        want = c_oracle.encode_bwd_f64(x, (L, T, F), n_ls, gk)
        got, _plan = bucketed(ops, _lib, tx, tn, t(gk), L, T, F, l0, l1, image, 1)
        got = got.cpu().numpy()
        quantum = count * (2.0 ** -room) * float(np.abs(gk).max())
        held(f"D bucketed {name} k={k}", got, want, 6.0e-8 * np.abs(want) + quantum + gsc.FINAL_ROUNDING, count * np.ones_like(want))
        if k == 0:
            base = got
        else:
            bit_equal_scaled(f"D bucketed {name} k={k}", got, base, want0, k)


# ================================================================================================ E. direct float-atomic form
@needs_oracle
@pytest.mark.parametrize("F", gsc.DIRECT_F)
@pytest.mark.parametrize("T", gsc.DIRECT_T)
def test_e_direct_float_atomic_form_follows_the_gradient_exponent(ops, T, F):
    """gngf_encode_bwd — one float atomic per (pixel, corner[, k]) — for the spatial hash, a vertex table and MODE_DENSE_HASH, at
    every k of E: (n + 2) u times the row's mass, finite everywhere.  The baseline the other forms are said to equal."""
    from collision_handling_in_instantngp_amd import _lib
    case = gsc.direct_case(T, F)
    P, L, x, n_ls, g = case["P"], case["L"], case["x"], case["n_ls"], case["g"]
    n_host = [int(n) for n in n_ls]
    tx, tn = t(x), t(n_ls, torch.int32)
    tables = torch.zeros((L, T, F), device=DEV)
    c, gx, gy = gsc.corner_terms(x, n_ls)
    lvl = (np.arange(L) * T)[None, :, None]
    vstride, K = max(n_host) + 2, 3
    NV = vstride * vstride
    rng = np.random.default_rng(T + F)
    vidx = rng.integers(0, T, (NV, K)).astype(np.int32)
    vw = (rng.integers(1, 256, (NV, K)) / 256.0).astype(np.float32)             # 8-bit weights: g c w is one more exact-ish product
    dense = ops.dense_level_mask(n_host, T)
    hashed = gsc.hash_rows(gx, gy, T)
    dense_rows = gy * (np.asarray(n_ls, np.int64) + 2)[None, :, None] + gx
    sources = {
        "hash": (ops.MODE_HASH, None, None, hashed + lvl),
        "dense_hash": (ops.MODE_DENSE_HASH, None, None, np.where(np.array(dense)[None, :, None], dense_rows, hashed) + lvl),
        "vertex_table": (ops.MODE_VERTEX_TABLE, vidx, vw, None),
    }
    assert any(dense) or T < (n_host[0] + 2) ** 2
    for source, (mode, vi, w, rows) in sources.items():
        if vi is None:
            want0, mass0, n = gsc.sums_f64(rows, L * T, c, g, F)
        else:
            want0 = c_oracle.encode_bwd_f64(x, (L, T, F), n_ls, g, vi, w, vstride, exact_products=True).reshape(-1, F)
            mass0 = c_oracle.encode_bwd_f64(x, (L, T, F), n_ls, np.abs(g), vi, w, vstride, exact_products=True).reshape(-1, F)
            vid = gy * vstride + gx                                                # (P, L, 4)
            n = np.bincount((vi[vid].astype(np.int64) + lvl[..., None]).reshape(-1), minlength=L * T)
        nn = n.astype(np.float64)[:, None]
        # (every device tensor the launch reads is held in a name until the launch has finished)
        vi_t = None if vi is None else t(vi, torch.int32)
        w_t = None if w is None else t(w)
        if vi is not None:
            assert int(vi_t.min()) >= 0 and int(vi_t.max()) < T and tuple(vi_t.shape) == (NV, K) == tuple(w_t.shape)
            assert int(gy.max()) * vstride + int(gx.max()) < NV
        for k in gsc.E:
            dt = torch.zeros((L, T, F), device=DEV)
            gk_t = t(gsc.scaled(g, k))
            _lib.call("gngf_encode_bwd", _lib.ptr(tx), *ops._tab(tables), _lib.ptr(vi_t), _lib.ptr(w_t), _lib.ptr(tn), _lib.ptr(gk_t),
                      _lib.ptr(dt), _lib.ptr(None), P, L, F, T, 0 if vi is None else K, mode, 0 if vi is None else vstride,
                      0 if vi is None else NV, 0, L, _lib.stream_ptr())
            torch.cuda.synchronize()
            held(f"E direct {source} T={T} F={F} k={k}", dt.cpu().numpy().reshape(-1, F), np.ldexp(want0, k),
                 (nn + 2) * U * np.ldexp(mass0, k) + gsc.FINAL_ROUNDING, mass0)


# ================================================================================================ G. Adam with 1 / loss scale
@pytest.mark.parametrize("wd", [0.0, 1e-6], ids=["no_decay", "decay"])
@pytest.mark.parametrize("flavour", ["fp32", "fp16_grad32"])
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
def test_g_adam_divides_the_loss_scale_out_exactly(flavour, wd, masked):
    """gngf_adam_step and gngf_adam_step_masked with gradients g 2^k and inv_grad_scale = 2^-k: parameters, moments and the fp32
    master after three steps are bit-equal to k = 0 (the product g 2^k 2^-k is exact)."""
    from test_gpu_adam_masked import adam_call, bits_equal, clone_state, make_state, mask_words
    T, F = 777, 2
    st0, flags = make_state(T, F, flavour, 0, seed=91)
    assert st0["g"].dtype == torch.float32 and (flags & 2) == (2 if flavour == "fp16_grad32" else 0)
    rows = np.random.default_rng(92).random(T) < 0.6
    mask = mask_words(rows) if masked else None
    grads = [torch.randn((T, F), generator=torch.Generator().manual_seed(93 + i)).mul(1e-2).to(DEV) for i in range(3)]

    def run(k):
        st = clone_state(st0)
        for i, g in enumerate(grads):
            st["g"].copy_(torch.ldexp(g, torch.tensor(k, device=DEV)))
            assert bool((torch.ldexp(st["g"], torch.tensor(-k, device=DEV)) == g).all())
            adam_call(st["p"], st["g"], st["m"], st["v"], st["master"], flags, mask=mask, row_elems=F if masked else 0, wd=wd,
                      steps_before=float(i), inv_grad_scale=2.0 ** -k)
        return st
    ref = run(0)
    assert not bits_equal(ref["p"], st0["p"])
    for k in (-40, -12, 12, 40):
        got = run(k)
        for name in ("p", "m", "v", "master"):
            if ref[name] is not None:
                assert bits_equal(got[name], ref[name]), (flavour, wd, masked, k, name)


# ================================================================================================ F. decoder kernels
DEC_P = (129, 128 * 256 + 1)
# (form, in_dim): the one-launch training kernel exists at 32 encoder features; the two-kernel backward runs the hybrid kernel on
# saved hidden layers at 32 (the fp32 one at 64 and 24) or recomputes them in fp32
DEC_FORMS = [("fused", 32), ("saved", 32), ("recompute", 32), ("saved", 64), ("recompute", 64), ("saved", 24), ("recompute", 24)]
# k of the bit-for-bit comparison.  -90 is left to the float64 bound: d enc of these cases is of the order 2 gloss / (3 P) — below
# 2^-7 at P = 129 and 2^-15 at P = 32769 — so at k = -90 more than 99 % of its entries (and of the slabs') lie under 2^-102, outside
# the exactness mask (measured: 0.3 % - 0.7 % of d enc inside it), where fp32 has no 24 bits left and the matrix pipe flushes partial
# products.  A comparison over the remainder would claim nothing; bit_equal_scaled insists on half the entries.
DEC_E_EXACT = tuple(k for k in gsc.E if k != -90)


def _dtd():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import decoder_train_digests as dtd
    return dtd


def _decoder_run(dtd, form, leaky, P, in_dim, inp, drgb=None, hybrid=1):
    from collision_handling_in_instantngp_amd import _lib
    if form == "fused":
        assert drgb is None and in_dim == 32
        return dtd.run_fused(leaky, P, inp, reduce=True)
    prev = _lib.query("gngf_set_decoder_bwd_hybrid", hybrid)
    try:
        return dtd.run_two_kernels(leaky, P, inp, in_dim=in_dim, save_hidden=form in ("saved", "fp32"), drgb=drgb, reduce=True)
    finally:
        _lib.query("gngf_set_decoder_bwd_hybrid", prev)


def _slab_views(dtd, out, P, in_dim):
    from collision_handling_in_instantngp_amd import _lib
    nslabs, n = _lib.query("gngf_decoder_bwd_slabs", P), _lib.query("gngf_decoder_slab_floats", in_dim, dtd.OUT_DIM)
    s = out["slabs"].reshape(nslabs, n)
    return s[:, :-1], s[:, -1], nslabs


def _slab_maxima(denc, P, nslabs):
    """max |d enc| over the pixels of each slab: workgroup b takes the 128-pixel tiles b, b + nslabs, ..."""
    tiles = -(-P // 128)
    a = np.zeros((tiles * 128,), np.float32)
    a[:P] = np.abs(denc).max(1)
    per_tile = a.reshape(tiles, 128).max(1)
    return np.array([per_tile[b::nslabs].max() for b in range(nslabs)], np.float32)


def _check_max_words(tag, dtd, out, P, in_dim):
    _sums, words, nslabs = _slab_views(dtd, out, P, in_dim)
    want = _slab_maxima(out["denc"], P, nslabs)
    assert np.array_equal(words.view(np.uint32), want.view(np.uint32)), (tag, "slab max words", words[:4], want[:4])
    assert out["denc_absmax"].view(np.uint32)[0] == want.max().view(np.uint32), (tag, out["denc_absmax"], want.max())


@pytest.mark.parametrize("leaky", [0, 1], ids=["relu", "leaky"])
@pytest.mark.parametrize("P", DEC_P)
@pytest.mark.parametrize("form,in_dim", DEC_FORMS, ids=[f"{f}-{d}" for f, d in DEC_FORMS])
def test_f_decoder_kernels_follow_the_loss_scale(form, in_dim, P, leaky):
    """gngf_decoder_train and both two-kernel backward forms with gloss (or d rgb) = base 2^k: rgb keeps its bytes; d enc, the slabs
    and the six reduced gradients are 2^k times their k = 0 values bit for bit under the mask (none of these kernels has an atomic);
    each slab's last word and denc_absmax are the maximum of the |d enc| the kernel wrote; all nine outputs against _decoder_float64
    at the criterion of test_training_decoder_kernels_against_float64 (at most twice the error of the all-fp32 kernels on the same
    inputs + its slack; every error but rgb's and the loss's is relative to the largest expected entry, so the criterion scales);
    gloss 0 gives exact zeros; a non-finite gloss never comes out finite."""
    from test_gpu_dense import _decoder_errors, _decoder_float64
    from conftest import parity_close
    dtd = _dtd()
    base_inp = dtd.inputs(leaky, P, in_dim)
    tag0 = f"F {form}-{in_dim} P={P} leaky={leaky}"
    names = ("rgb", "loss", "d enc", "dW0", "db0", "dW1", "db1", "dW2", "db2")

    def with_gloss(v):
        return dict(base_inp, gloss=np.array([v], np.float32))

    def as_list(out):
        rgb64 = out["rgb"].astype(np.float64)
        loss = ((rgb64 - base_inp["target"]) ** 2).mean()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        return [dev(out["rgb"]), torch.tensor(loss), dev(out["denc"])] + [dev(g) for g in out["grads"]]

    base = _decoder_run(dtd, form, leaky, P, in_dim, with_gloss(1.25))
    want0 = _decoder_float64(base_inp["enc"], base_inp["target"], base_inp["ws"], leaky, 1.25)
    w_denc = want0[2].cpu().numpy()
    for k in gsc.E:
        gl = float(np.float32(1.25) * np.float32(2.0) ** k)
        out = _decoder_run(dtd, form, leaky, P, in_dim, with_gloss(gl))
        tag = f"{tag0} k={k}"
        assert out["rgb"].tobytes() == base["rgb"].tobytes(), tag
        assert all(np.isfinite(out[n]).all() for n in ("denc", "slabs", "denc_absmax")), tag
        _check_max_words(tag, dtd, out, P, in_dim)
        # float64: the criterion of test_training_decoder_kernels_against_float64 against the all-fp32 kernels at the same scale
        want = _decoder_float64(base_inp["enc"], base_inp["target"], base_inp["ws"], leaky, gl)
        errs = _decoder_errors(as_list(out), want)
        ref = _decoder_errors(as_list(_decoder_run(dtd, "fp32", leaky, P, in_dim, with_gloss(gl), hybrid=0)), want)
        for i, nm in enumerate(names):
            slack = 1e-7 if i == 0 else (1e-6 if i == 1 else (1e-7 if i == 2 else 2e-4))
            parity_close(np.array([errs[i]]), np.array([0.0]), 0, 2 * ref[i] + slack, f"{tag}: {nm} vs float64 (all-fp32 kernels: {ref[i]:.2e})")
        if k in DEC_E_EXACT and k != 0:
            bit_equal_scaled(f"{tag} d enc", out["denc"], base["denc"], w_denc, k)
            s_k, _w, _n = _slab_views(dtd, out, P, in_dim)
            s_0, _w, _n = _slab_views(dtd, base, P, in_dim)
            bit_equal_scaled(f"{tag} slabs", s_k, s_0, s_0.astype(np.float64), k)
            for i, (g_k, g_0) in enumerate(zip(out["grads"], base["grads"])):
                bit_equal_scaled(f"{tag} {names[3 + i]}", g_k, g_0, want0[3 + i].cpu().numpy(), k)
    # d rgb handed over instead of target + gloss (two-kernel forms): the same equivariance
    if form != "fused":
        d0 = ((np.float32(2 * 1.25 / (3 * P)) * (base["rgb"] - base_inp["target"])).astype(np.float32))
        b = _decoder_run(dtd, form, leaky, P, in_dim, base_inp, drgb=d0)
        for k in DEC_E_EXACT:
            out = _decoder_run(dtd, form, leaky, P, in_dim, base_inp, drgb=gsc.scaled(d0, k))
            _check_max_words(f"{tag0} d rgb k={k}", dtd, out, P, in_dim)
            assert out["rgb"].tobytes() == base["rgb"].tobytes()
            if k != 0:
                bit_equal_scaled(f"{tag0} d rgb k={k} d enc", out["denc"], b["denc"], b["denc"].astype(np.float64), k)
                bit_equal_scaled(f"{tag0} d rgb k={k} slabs", _slab_views(dtd, out, P, in_dim)[0], _slab_views(dtd, b, P, in_dim)[0],
                                 _slab_views(dtd, b, P, in_dim)[0].astype(np.float64), k)
    # gloss 0: exact zeros
    out = _decoder_run(dtd, form, leaky, P, in_dim, with_gloss(0.0))
    sums, words, _n = _slab_views(dtd, out, P, in_dim)
    assert not out["denc"].any() and not sums.any() and not words.any() and not out["denc_absmax"].any(), f"{tag0} gloss 0"
    assert out["rgb"].tobytes() == base["rgb"].tobytes()
    # a non-finite gloss: d enc overflows everywhere a pixel has a gradient — the max words must not be finite
    for bad in (float("inf"), float("nan")):
        out = _decoder_run(dtd, form, leaky, P, in_dim, with_gloss(bad))
        _s, words, _n = _slab_views(dtd, out, P, in_dim)
        assert not np.isfinite(words).any() and not np.isfinite(out["denc_absmax"]).any(), (tag0, bad, words[:4])
        assert not np.isfinite(out["denc"][np.abs(base["denc"]) > 0]).any(), (tag0, bad, "a non-finite gradient came out finite")


def test_f_non_finite_decoder_max_words_poison_the_pixel_stage(ops):
    """the slab max words of a decoder launch whose gloss is infinite, handed to the pixel-stage launch as its bound on |d enc|
    (count = slabs, stride = slab floats, as the training step hands them): the grid is poisoned"""
    from collision_handling_in_instantngp_amd import _lib
    dtd = _dtd()
    P = 129
    out = dtd.run_fused(0, P, dict(dtd.inputs(0, P), gloss=np.array([np.inf], np.float32)))
    nslabs, n = _lib.query("gngf_decoder_bwd_slabs", P), _lib.query("gngf_decoder_slab_floats", 32, dtd.OUT_DIM)
    slabs = t(out["slabs"])
    assert not np.isfinite(out["slabs"].reshape(nslabs, n)[:, -1]).any()
    px = _Pixel(ops, "small", 2)
    plan = px.plan
    prev = _interleaving(True)
    try:
        dG64 = torch.zeros((plan.vtot * 2 + 2,), dtype=torch.int64, device=DEV)
        dG = torch.zeros((plan.vtot, 2), dtype=torch.float32, device=DEV)
        ops._pixel_bwd(plan, px.ws, px.n_t, px.genc(0), dG, px.L, 2, (slabs[n - 1:], nslabs, n), None, None, dG64)
        assert bool(torch.isnan(dG).all()) and int(dG64[-1]) != 0
    finally:
        _interleaving(prev)


# ================================================================================================ H. one model-level step per form
@needs_oracle
@pytest.mark.parametrize("name,fused", [("cfg1", True), ("partly_staged_fp16", False)], ids=["cfg1-fused_loss", "partly_staged_fp16-plain"])
def test_h_one_model_step_under_a_loss_scale(name, fused):
    """net.fused_mse(target, gloss=2^k) with (loss 2^k).backward() (cfg1, hash) and the plain (mse 2^k).backward()
    (partly_staged_fp16, hash, FP16_TABLE_GRAD_FP32), k in (-12, +12): the captured d enc and the table gradient through
    check_rows_against_oracle (its bounds are all relative to the captured gradient), the decoder gradients divided by 2^k
    through check_step_against_oracle; fused form: the six decoder gradients are also 2^k times the k = 0 run, bit for bit."""
    from collision_handling_in_instantngp_amd import models, ops
    from test_gpu_bench_chain import _poison_allocator
    from test_gpu_step_config_matrix import (DECODER_GRADS, _build, _table_grad, check_rows_against_oracle, check_step_against_oracle,
                                             staged_sink)
    prev_tuning = ops.TUNING
    try:
        net, (L, F, T, P, fp32) = _build(models, ops, name, "hash")
        ops.FP16_TABLE_GRAD_FP32 = not fp32
        gen = torch.Generator(device=DEV).manual_seed(29)
        xy = torch.rand((P, 2), device=DEV, generator=gen)
        target = torch.rand((P, 3), device=DEV, generator=gen)
        n_ls = np.array(net._n_ls_host, np.int32)
        chunk = getattr(ops.EncodePlan(P, [int(n) for n in n_ls], F), "chunk", 0)
        _poison_allocator()
        base = None
        for k in (0, -12, 12):
            scale = 2.0 ** k
            for p in net.parameters():
                p.grad = None
                if getattr(p, "grad_fp32", None) is not None:
                    p.grad_fp32 = None
            captured, trace = [], []
            real = ops.decoder_apply

            def spy(enc, *a, **kw):
                enc.register_hook(lambda g: captured.append(g.detach().clone()))
                return real(enc, *a, **kw)
            prev_trace, ops.PIXEL_BWD_TRACE = ops.PIXEL_BWD_TRACE, trace
            ops.decoder_apply = spy
            try:
                if fused:
                    with net.fused_mse(target, gloss=scale):
                        rgb, _p, _i, _c = net(xy, 1.0)
                    loss = ops.mse_loss(rgb, target)
                else:
                    rgb, _p, _i, _c = net(xy, 1.0)
                    loss = torch.nn.functional.mse_loss(rgb, target)
                (loss * scale).backward()
                torch.cuda.synchronize()
            finally:
                ops.decoder_apply = real
                ops.PIXEL_BWD_TRACE = prev_trace
            assert len(captured) == 1
            genc = np.ascontiguousarray(captured[0].float().cpu().numpy())
            tag = f"H {name} {'fused_loss' if fused else 'plain'} k={k}"
            got = _table_grad(net, L)
            Ls = trace[0]["Ls"] if trace else 0
            sink = staged_sink(trace, "hash") if trace else "none"
            check_rows_against_oracle(tag, got, xy, genc, n_ls, T, F, Ls, sink, "hash", chunk)
            params = dict(net.named_parameters())
            raw = {nm: params[nm].grad.detach().clone() for nm in DECODER_GRADS}
            for nm in DECODER_GRADS:
                params[nm].grad.mul_(2.0 ** -k)                       # exact: the oracle's gradients are those of the unscaled loss
            check_step_against_oracle(tag, net, L, xy, target, rgb.detach(), float(loss.detach()))
            if k == 0:
                base = raw
            elif fused:
                for nm in DECODER_GRADS:
                    b = torch.ldexp(base[nm], torch.tensor(k, device=DEV))
                    m = t(gsc.exact_mask(base[nm].double().cpu().numpy(), k))
                    assert torch.equal(raw[nm][m].view(torch.int32), b[m].view(torch.int32)), f"{tag}: {nm} is not 2^{k} times the k = 0 run"
    finally:
        ops.TUNING = prev_tuning
        models.should_use_hash_function = False
