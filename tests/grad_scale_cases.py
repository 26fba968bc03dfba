"""Inputs, restated fixed-point scales and the exactness mask of the gradient-magnitude tests (tests/test_grad_scale_cpu.py,
tests/test_gpu_grad_scale.py).  numpy only.

Every backward path that avoids float atomics takes a power-of-two fixed-point scale from the gradient's exponent at run time.
Scaling an fp32 gradient by 2^k is exact, so on those paths the result at scale 2^k is the result at scale 1 times 2^k BIT FOR
BIT while the scale is not clamped and nothing leaves the normal range; the tests move the exponent over E and assert that.

  pixel stage (csrc/encode_tiled.hip, tiled_bwd_kernel / tiled_bwd_il_kernel):
      S = min(126, 60 - max(10, log2_terms) - eg),  gmax < 2^eg (frexp), eg = 0 for gmax == 0 or a non-finite gmax;
      log2_terms = max(1, bit_length(P - 1)) when one scale serves the launch (a bound on |d enc| AND the fixed-point grid dG64),
      ceil log2 chunk otherwise (per work item).  Every term |g c 2^S| < 2^(60 - log2_terms), so a sum of 2^log2_terms terms stays
      below 2^60.
  bucketed direct levels (csrc/encode_bucket.hip): S = min(50, 61 - ceil log2 n) - (e + 1),  |term| < 2^(e + 1) the bucket's largest
      fp32 term g c, n the terms of the bucket's fullest row (counted only in buckets of more than 2048 items, 2048 otherwise):
      the sum of n terms stays below 2^61.  Never clamped.

The coordinates lie on the lattice j / 256: x N is exact for every N < 2^16, the bilinear weights are multiples of 1 / 256 and every
coefficient c is an exact multiple of 2^-16 (24 bits at most) — the smallest non-zero c is 2^-16, so with |g| >= 2^-20 no product
g c 2^k is subnormal for k >= -90 (2^-126 is the smallest normal fp32 number) and none overflows for k <= 90."""
import math

import numpy as np

E = (-90, -40, -12, 0, 12, 40, 90)
U = 2.0 ** -24
G_LO, G_HI = -20, 3                  # the base gradient: 2^G_LO <= |g| < 2^G_HI
LATTICE = 256
FINAL_ROUNDING = 2.0 ** -150         # one rounding to fp32 at the bottom of the range (half the smallest subnormal)
MASK_LO, MASK_HI = 2.0 ** -102, 2.0 ** 127
MAX_OUTSIDE_MASK = 0.01

# name: (P, n_min, n_max, L, T) — the two geometries of test_fixed_point_vertex_grid_is_exact_and_order_free (tests/test_gpu_encode.py)
PIXEL_GEOMETRIES = {"small": (400, 8, 24, 4, 4096), "big": (2 ** 15 + 1, 16, 256, 16, 4096)}
PIXEL_F = (1, 2, 4)
# bucketed direct levels: two shapes of tests/test_gpu_bucket.py, (P, n_min, n_max, L, T, F, l0, l1, image bytes)
BUCKET_SHAPES = {"f1_t1000": (70001, 16, 512, 6, 1000, 1, 0, 6, 1024), "one_bucket": (5000, 16, 256, 2, 300, 2, 0, 2, 65536)}
# direct float-atomic form: P, n_min, n_max, L
DIRECT_SHAPE = (4099, 8, 32, 4)
DIRECT_T, DIRECT_F = (483, 512), (1, 2, 4)
# head-room at its limit
HEADROOM_P = (1024, 1025, 4096, 2 ** 15, 2 ** 15 + 1)
HEADROOM_E = (-12, 0, 40)
HEADROOM_N = (8, 16, 32)             # even N: the point (0.5, 0.5) is a vertex of every level
HEADROOM_SIGNS = ("positive", "negative", "alternating")


def level_resolutions(n_min, n_max, L):
    from oracle import gngf_oracle as orc
    return np.ascontiguousarray(orc.level_resolutions(n_min, n_max, L), np.int32)


# ------------------------------------------------------------------------------------------------ the restated scales
def exponent_above(gmax):
    """eg of the pixel stage: gmax < 2^eg as frexpf gives it; 0 for gmax == 0 and for a non-finite gmax"""
    gmax = float(gmax)
    return math.frexp(gmax)[1] if (gmax > 0 and math.isfinite(gmax)) else 0


def pixel_log2_terms(P, chunk, launch_scale):
    """launch_scale: a bound on |d enc| and the fixed-point grid are given (one scale for the launch, sized for the P pixels a
    vertex can receive); else the scale of one work item (chunk pixels at most)"""
    return max(1, int(P - 1).bit_length()) if launch_scale else int(chunk - 1).bit_length()


def pixel_scale_unclamped(gmax, log2_terms):
    return 60 - max(10, int(log2_terms)) - exponent_above(gmax)


def pixel_scale(gmax, log2_terms):
    """S of the pixel-stage backward, with the clamp"""
    return min(126, pixel_scale_unclamped(gmax, log2_terms))


def fixed_point_scale_clamped(genc, P, chunk):
    """fixed_point_scale of tests/test_encode_dw_cpu.py (the conservative S of check_rows_against_oracle: one exponent lower than the
    largest |d enc| gives, terms counted as max(P, chunk)) with the kernel's clamp"""
    gmax = float(np.abs(genc).max())
    e = math.frexp(gmax)[1] + 1 if gmax > 0 else 0
    return min(126, 60 - max(10, (max(int(P), int(chunk)) - 1).bit_length()) - e)


def bucket_scale(max_term, fullest_row, items):
    """S of one bucket: max_term the largest |fp32 term| in it (> 0, finite), fullest_row the terms of its fullest row, items the
    (pixel, corner) contributions in the bucket (rows are counted only above 2048 of them)"""
    e = math.frexp(float(max_term))[1] - 1                        # 2^e <= max_term < 2^(e + 1)
    e = max(e, -127)                                              # (subnormal terms read as exponent -127)
    n = int(fullest_row) if items > 2048 else 2048
    lg = 0 if n <= 1 else (n - 1).bit_length()
    return min(50, 61 - lg) - (e + 1)


def pixel_unclamped_ks(gmax_smallest, log2_terms, ks=E):
    """the k of `ks` at which S_k == S_0 - k for EVERY scale the launch can take: the largest S_0 is that of the smallest maximum
    an item (or the launch) can see, gmax_smallest"""
    s0 = pixel_scale_unclamped(gmax_smallest, log2_terms)
    return tuple(k for k in ks if s0 - k <= 126)


# ------------------------------------------------------------------------------------------------ inputs
def lattice_coords(P, rng):
    """(P, 2) float32 on the lattice j / 256, the corners and the centre among them, 64 pixels on one point"""
    x = (rng.integers(0, LATTICE + 1, (P, 2)) / float(LATTICE)).astype(np.float32)
    edge = np.array([[0, 0], [1, 1], [0, 1], [1, 0], [0.5, 0.5], [1 / 32, 31 / 32]], np.float32)
    x[:len(edge)] = edge[:P]
    if P > 200:
        x[100:164] = x[100]
    return x


def base_gradient(shape, rng):
    """float32, mixed signs, 2^-20 <= |g| < 2^3: 24-bit mantissas, most exponents in [0, 3) and one value in forty anywhere down to
    -20 (so that few sums fall below 2^-12: the exactness mask at k = -90); every third row sits at the maximum itself, as in
    test_fixed_point_vertex_grid_is_exact_and_order_free"""
    mant = 1.0 + rng.integers(0, 2 ** 23, shape) * 2.0 ** -23
    expo = np.where(rng.random(shape) < 0.025, rng.integers(G_LO, G_HI, shape), rng.integers(0, G_HI, shape))
    g = (mant * 2.0 ** expo * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    g[::3] = np.float32((2.0 - 2.0 ** -23) * 2.0 ** (G_HI - 1))
    g[1].reshape(-1)[0] = np.float32(2.0 ** G_LO)                   # both ends of the range are present
    assert float(np.abs(g).min()) >= 2.0 ** G_LO and float(np.abs(g).max()) < 2.0 ** G_HI
    return g


def scaled(g, k):
    """g 2^k in float32 — exact (asserted)"""
    out = np.ldexp(g, k).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.ldexp(g.astype(np.float64), k)), k
    return out


def pixel_case(geometry, F, seed=0):
    P, n_min, n_max, L, T = PIXEL_GEOMETRIES[geometry]
    rng = np.random.default_rng([seed, P, F])
    return dict(P=P, L=L, F=F, T=T, n_ls=level_resolutions(n_min, n_max, L), x=lattice_coords(P, rng), g=base_gradient((P, L * F), rng))


def bucket_case(name, seed=0):
    P, n_min, n_max, L, T, F, l0, l1, image = BUCKET_SHAPES[name]
    rng = np.random.default_rng([seed, P, F, T])
    x = lattice_coords(P, rng)
    x[7:2007] = x[7]                                              # 2000 pixels on one cell, as tests/test_gpu_bucket.py _case
    return dict(P=P, L=L, F=F, T=T, l0=l0, l1=l1, image=image, n_ls=level_resolutions(n_min, n_max, L), x=x,
                g=base_gradient((P, L * F), rng))


def direct_case(T, F, seed=0):
    P, n_min, n_max, L = DIRECT_SHAPE
    rng = np.random.default_rng([seed, P, F, T])
    return dict(P=P, L=L, F=F, T=T, n_ls=level_resolutions(n_min, n_max, L), x=lattice_coords(P, rng), g=base_gradient((P, L * F), rng))


def headroom_case(P, e, signs, F=2):
    """all P pixels on (0.5, 0.5) — a vertex of every level of HEADROOM_N, weights (1, 0, 0, 0) — and every gradient
    +-(2 - 2^-23) 2^e: -> (x, g, n_ls, value, expected sum as float32)"""
    assert signs in HEADROOM_SIGNS
    v = np.float32((2.0 - 2.0 ** -23) * 2.0 ** e)
    sign = {"positive": np.ones(P), "negative": -np.ones(P), "alternating": np.where(np.arange(P) % 2 == 0, 1.0, -1.0)}[signs]
    g = np.ascontiguousarray(np.repeat((sign * float(v)).astype(np.float32)[:, None], len(HEADROOM_N) * F, 1))
    x = np.full((P, 2), 0.5, np.float32)
    want = np.float32(float(sign.sum()) * float(v))               # P v needs 40 bits: exact in double, rounded to fp32 once
    return x, g, np.array(HEADROOM_N, np.int32), v, want


# ------------------------------------------------------------------------------------------------ geometry of the terms
def corner_terms(x, n_ls):
    """(c (P, L, 4) float32 coefficients as the kernels form them, gx, gy (P, L, 4) int64 vertex coordinates)"""
    from oracle import gngf_oracle as orc
    scaled_, grid = orc.scale_to_grid(x, n_ls)
    c = orc.bilinear_coeffs(scaled_, grid).astype(np.float32)
    gi = grid.astype(np.int64)
    return c, gi[:, 0], gi[:, 1]


def hash_rows(gx, gy, T):
    from oracle import gngf_oracle as orc
    return orc.spatial_hash(np.stack([gx, gy], 1).astype(np.int32), T).astype(np.int64)            # (P, L, 4)


def vertex_grid_index(gx, gy, n_ls):
    """(P, L, 4) index into the level grids laid back to back, (n + 2)^2 vertices each, and their total"""
    goff = np.concatenate([[0], np.cumsum([(int(n) + 2) ** 2 for n in n_ls])])
    gw = (np.asarray(n_ls, np.int64) + 2)[None, :, None]
    return goff[:-1][None, :, None] + gy * gw + gx, int(goff[-1])


def sums_f64(index, size, c, g, F):
    """float64 sums of the exact products g c per (index, f): (want, mass, n) of shapes (size, F), (size, F), (size,)"""
    P, L, _ = c.shape
    terms = g.reshape(P, L, 1, F).astype(np.float64) * c.astype(np.float64)[..., None]            # (P, L, 4, F)
    want, mass = np.zeros((size, F)), np.zeros((size, F))
    flat = index.reshape(-1)
    for f in range(F):
        want[:, f] = np.bincount(flat, weights=terms[..., f].reshape(-1), minlength=size)
        mass[:, f] = np.bincount(flat, weights=np.abs(terms[..., f]).reshape(-1), minlength=size)
    return want, mass, np.bincount(flat, minlength=size)


# ------------------------------------------------------------------------------------------------ the exactness mask
def exact_mask(want, k):
    """entries compared bit for bit at scale k: the float64 expected value w (at scale 1) is 0, or 2^-102 <= |w 2^k| < 2^127 — all 24
    bits exist at both scales"""
    a = np.abs(np.asarray(want, np.float64))
    a0, ak = a, np.ldexp(a, k)
    ok = lambda v: (v >= MASK_LO) & (v < MASK_HI)       # noqa: E731
    return (a == 0) | (ok(a0) & ok(ak))


def outside_mask_fraction(want, k):
    nz = np.asarray(want) != 0
    return float((~exact_mask(want, k) & nz).sum()) / max(1, int(nz.sum()))


def terms_stay_normal(c, g, F, ks=E):
    """no fp32 product g c 2^k is subnormal or overflows for any k of ks (zero products aside)"""
    P, L, _ = c.shape
    t = np.abs(g.reshape(P, L, 1, F).astype(np.float64) * c.astype(np.float64)[..., None])
    t = t[t > 0]
    return bool(t.min() * 2.0 ** min(ks) >= 2.0 ** -126) and bool(t.max() * 2.0 ** max(ks) < 2.0 ** 128 * (1 - 2.0 ** -25))
