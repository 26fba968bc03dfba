"""CPU: what the gradient-magnitude tests (tests/test_gpu_grad_scale.py) rest on, checked from the oracle alone —
  * the float64 oracle is itself equivariant: encode_bwd_f64(g 2^k) == 2^k encode_bwd_f64(g), exactly;
  * the restated scales (tests/grad_scale_cases.py) against hand-computed values: at the clamp, at gmax = 0, at P = 2^n and 2^n + 1;
  * the head-room arithmetic of the tight cases: the fixed-point sum stays below 2^60 (pixel stage) and 2^61 (a bucket);
  * the preconditions of the bit-for-bit claims, for every case and every exponent: no fp32 product g c is subnormal or overflows,
    and at most 1 % of the non-zero expected entries fall outside the exactness mask."""
import math

import numpy as np
import pytest

import grad_scale_cases as gsc
from oracle import c_oracle
from test_encode_dw_cpu import fixed_point_scale

needs_oracle = pytest.mark.skipif(not c_oracle.available(), reason="oracle/libgngf_oracle_c.so not built (make -C oracle)")


def _all_cases():
    out = []
    for geo in gsc.PIXEL_GEOMETRIES:
        for F in gsc.PIXEL_F:
            out.append((f"pixel/{geo}/F{F}", gsc.pixel_case(geo, F)))
    for name in gsc.BUCKET_SHAPES:
        out.append((f"bucket/{name}", gsc.bucket_case(name)))
    for T in gsc.DIRECT_T:
        for F in gsc.DIRECT_F:
            out.append((f"direct/T{T}/F{F}", gsc.direct_case(T, F)))
    return out


CASES = _all_cases()


def test_exponent_set_and_base_gradient():
    assert gsc.E == (-90, -40, -12, 0, 12, 40, 90)
    g = gsc.base_gradient((400, 8), np.random.default_rng(1))
    a = np.abs(g)
    assert a.min() == 2.0 ** -20 and 2.0 ** 2 < a.max() < 2.0 ** 3 and (g > 0).any() and (g < 0).any()
    assert np.all(a[::3] == a.max())                                      # many terms at the bound itself
    for k in gsc.E:                                                       # scaling is exact and stays normal
        s = gsc.scaled(g, k)
        assert np.all(np.abs(s) >= 2.0 ** -126) and np.isfinite(s).all()


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_no_term_leaves_the_normal_range_and_the_mask_covers_99_percent(name, case):
    """the two preconditions of every bit-for-bit assertion of the GPU module, for the sinks it compares: the table rows and (pixel
    stage) the vertex grid"""
    c, gx, gy = gsc.corner_terms(case["x"], case["n_ls"])
    F, T, L = case["F"], case["T"], case["L"]
    assert np.all(np.ldexp(c.astype(np.float64), 16) == np.round(np.ldexp(c.astype(np.float64), 16))), "c is a multiple of 2^-16"
    assert gsc.terms_stay_normal(c, case["g"], F), name
    rows = gsc.hash_rows(gx, gy, T) + (np.arange(L) * T)[None, :, None]
    sinks = {"table rows": gsc.sums_f64(rows, L * T, c, case["g"], F)[0]}
    if name.startswith("pixel"):
        vid, vtot = gsc.vertex_grid_index(gx, gy, case["n_ls"])
        sinks["vertex grid"] = gsc.sums_f64(vid, vtot, c, case["g"], F)[0]
    for sink, want in sinks.items():
        assert np.count_nonzero(want) > 0
        for k in gsc.E:
            frac = gsc.outside_mask_fraction(want, k)
            assert frac <= gsc.MAX_OUTSIDE_MASK, (name, sink, k, frac)
        assert np.abs(want).max() * 2.0 ** max(gsc.E) < 2.0 ** 127          # no sum overflows either


def test_exact_mask_definition():
    w = np.array([0.0, 2.0 ** -102, 2.0 ** -103, 1.0, 2.0 ** 36, 2.0 ** 37, -2.0 ** -12, -2.0 ** -13])
    assert gsc.exact_mask(w, 0).tolist() == [True, True, False, True, True, True, True, True]
    assert gsc.exact_mask(w, 90).tolist() == [True, True, False, True, True, False, True, True]
    assert gsc.exact_mask(w, -90).tolist() == [True, False, False, True, True, True, True, False]


@needs_oracle
@pytest.mark.parametrize("F", gsc.PIXEL_F)
def test_oracle_is_equivariant_under_powers_of_two(F):
    """encode_bwd_f64(g 2^k) == 2^k encode_bwd_f64(g) exactly — with exact products and with the reference's fp32 products (no
    product is subnormal: the precondition above)"""
    case = gsc.pixel_case("small", F)
    shape = (case["L"], case["T"], F)
    # The oracle adds its terms with double-precision atomics from several threads, in any order: two calls agree exactly only where
    # every partial sum is exact.  Gradients with exponents in [0, 3) make them so — the products are multiples of 2^-39 (24-bit
    # mantissas from 2^-23, coefficients multiples of 2^-16) and a row of fewer than 2^11 terms stays below 2^14: 53 bits.
    g = np.where(np.abs(case["g"]) < 1, np.ldexp(np.frexp(case["g"])[0], 1), case["g"]).astype(np.float32)
    assert np.abs(g).min() >= 1 and np.abs(g).max() < 8 and (g < 0).any()
    for exact in (True, False):
        base = c_oracle.encode_bwd_f64(case["x"], shape, case["n_ls"], g, exact_products=exact)
        assert np.count_nonzero(base) > 0
        assert np.array_equal(base, np.round(np.ldexp(base, 39)) * 2.0 ** -39) and np.abs(base).max() < 2.0 ** 14
        for k in gsc.E:
            got = c_oracle.encode_bwd_f64(case["x"], shape, case["n_ls"], gsc.scaled(g, k), exact_products=exact)
            assert np.array_equal(got, np.ldexp(base, k)), (F, k, exact)
    # ... and it is the sum the helper forms with numpy
    c, gx, gy = gsc.corner_terms(case["x"], case["n_ls"])
    rows = gsc.hash_rows(gx, gy, case["T"]) + (np.arange(case["L"]) * case["T"])[None, :, None]
    want, mass, _n = gsc.sums_f64(rows, case["L"] * case["T"], c, case["g"], F)
    base = c_oracle.encode_bwd_f64(case["x"], shape, case["n_ls"], case["g"], exact_products=True).reshape(-1, F)
    assert np.all(np.abs(want - base) <= 1e-13 * mass)


def test_pixel_stage_scale_against_hand_computed_values():
    S = gsc.pixel_scale
    # gmax in [4, 8): frexp exponent 3.  400 pixels count as 2^10 terms
    assert gsc.pixel_log2_terms(400, 1024, True) == 9 and S(7.5, 9) == 60 - 10 - 3 == 47
    # P = 2^n and 2^n + 1: the bit length of P - 1
    assert gsc.pixel_log2_terms(2 ** 15, 4096, True) == 15 and gsc.pixel_log2_terms(2 ** 15 + 1, 4096, True) == 16
    assert S(7.5, 15) == 42 and S(7.5, 16) == 41
    assert gsc.pixel_log2_terms(2 ** 15 + 1, 4096, False) == 12 and gsc.pixel_log2_terms(5, 1024, False) == 10
    assert gsc.pixel_log2_terms(1, 1024, True) == 1 and gsc.pixel_log2_terms(2, 1024, True) == 1
    # an exact power of two is NOT below itself: gmax = 4 -> eg = 3, gmax just below -> eg = 2
    assert S(4.0, 10) == 47 and S(float(np.nextafter(np.float32(4), np.float32(0))), 10) == 48
    # gmax = 0, inf, nan: eg = 0
    assert S(0.0, 10) == 50 and S(float("inf"), 16) == 44 and S(float("nan"), 16) == 44
    # the clamp: gmax = 7.5 2^-90 -> eg = -87, 60 - 10 + 87 = 137 -> 126; first clamped at eg = -77, i.e. gmax < 2^-77
    assert gsc.pixel_scale_unclamped(7.5 * 2.0 ** -90, 9) == 137 and S(7.5 * 2.0 ** -90, 9) == 126
    assert S(2.0 ** -77, 10) == 126 and gsc.pixel_scale_unclamped(2.0 ** -77, 10) == 126 and gsc.pixel_scale_unclamped(2.0 ** -78, 10) == 127
    # large gradients: S goes negative, never clamped from below
    assert S(7.5 * 2.0 ** 90, 16) == 41 - 90 == -49
    # which exponents move S by exactly k
    assert gsc.pixel_unclamped_ks(7.5, 9) == (-40, -12, 0, 12, 40, 90)
    assert gsc.pixel_unclamped_ks(2.0 ** -20, 10) == (-40, -12, 0, 12, 40, 90)       # an item that only sees the smallest gradient: S_0 = 69
    assert gsc.pixel_unclamped_ks(2.0 ** -20, 10, ks=(-58, -57)) == (-57,)


def test_clamped_restatement_leaves_the_existing_callers_values_unchanged():
    rng = np.random.default_rng(0)
    for P, chunk in ((400, 1024), (2 ** 14, 2048), (2 ** 15 + 1, 4096)):
        g = rng.standard_normal((64, 8)).astype(np.float32)
        assert gsc.fixed_point_scale_clamped(g, P, chunk) == fixed_point_scale(g, P, chunk)          # O(1) gradients: no clamp
        tiny = gsc.scaled(g, -90)
        assert fixed_point_scale(tiny, P, chunk) > 126 and gsc.fixed_point_scale_clamped(tiny, P, chunk) == 126
    assert fixed_point_scale(np.zeros((4, 4), np.float32), 400, 1024) == 50 == gsc.fixed_point_scale_clamped(np.zeros((4, 4)), 400, 1024)
    # the conservative S never exceeds the launch's own
    g = gsc.base_gradient((400, 8), rng)
    for k in gsc.E:
        gk = gsc.scaled(g, k)
        assert gsc.fixed_point_scale_clamped(gk, 400, 1024) <= gsc.pixel_scale(float(np.abs(gk).max()), gsc.pixel_log2_terms(400, 1024, True))


def test_bucket_scale_against_hand_computed_values():
    B = gsc.bucket_scale
    assert B(1.0, 5, 100) == 50 - 1                    # few items: rows not counted, 2048 assumed -> room 50; 1.0 < 2^1
    assert B(1.5, 2048, 4096) == 50 - 1 and B(1.5, 2049, 4096) == 49 - 1         # ceil log2: 11 -> room 50, 12 -> room 49
    assert B(1.5, 2 ** 15, 2 ** 17) == 46 - 1 and B(1.5, 2 ** 15 + 1, 2 ** 17) == 45 - 1
    assert B(1.5 * 2.0 ** 90, 100, 100) == 50 - 91 and B(1.5 * 2.0 ** -90, 100, 100) == 50 + 89       # never clamped
    for k in gsc.E:
        assert B(3.0 * 2.0 ** k, 3000, 5000) == B(3.0, 3000, 5000) - k


@pytest.mark.parametrize("P", gsc.HEADROOM_P)
@pytest.mark.parametrize("e", gsc.HEADROOM_E)
def test_head_room_at_its_limit(P, e):
    """P terms of (2 - 2^-23) 2^e, the bound equal to that value: the fixed-point sum is an integer below 2^60 (pixel stage, one scale
    for the launch) / 2^61 (a bucket whose fullest row holds the P terms), and above a quarter of it — the tight end"""
    x, g, n_ls, v, want = gsc.headroom_case(P, e, "positive")
    assert float(want) == float(np.float32(P * float(v))) and np.all(g == v)
    S = gsc.pixel_scale(float(v), gsc.pixel_log2_terms(P, 4096, True))
    term = float(v) * 2.0 ** S
    assert term == int(term) and term < 2.0 ** 51                          # an exact integer that the fma form can hold
    total = int(term) * P
    assert total < 2 ** 60, (P, e, math.log2(total))
    if P >= 2 ** 10 and P & (P - 1) == 0:
        assert total > 2 ** 59                                             # a power of two of pixels fills the room to the last bit
    Sb = gsc.bucket_scale(float(v), P, 4 * P)
    tb = float(v) * 2.0 ** Sb
    assert tb == int(tb) and int(tb) * P < 2 ** 61, (P, e)
    if P > 2048 and P & (P - 1) == 0:
        assert int(tb) * P > 2 ** 60
    for signs, n in (("negative", -P), ("alternating", P % 2)):
        _x, g2, _n, _v, w2 = gsc.headroom_case(P, e, signs)
        assert float(w2) == float(np.float32(n * float(v)))
        assert float(g2[:, 0].astype(np.float64).sum()) == n * float(v)
    c, gx, gy = gsc.corner_terms(x[:1], n_ls)
    assert np.array_equal(c[0], np.tile(np.array([1, 0, 0, 0], np.float32), (len(n_ls), 1)))
