"""numpy restatement of gngf_ext_sample_pixels (include/gngf_ext.h, csrc/sample.hip): the generator in uint64 with wrapping
arithmetic, every fp32 operation of the kernel as one numpy float32 operation in the stated order (numpy rounds each on its own, and
its float32 division is IEEE: correctly rounded), and — for the continuous mode — the bilinear value once more in float64 from the
fp32 positions.  Texels come from a callable texel(r, c, k) -> uint8 values, so that an image given by a formula needs no array."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
F32 = np.float32
TWO_M24 = F32(2.0 ** -24)


def bits(seed, draw, P, i=None):
    """z of samples i (default: all P) of draw `draw`"""
    i = np.arange(P, dtype=np.uint64) if i is None else np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        counter = np.uint64(draw % (1 << 64)) * np.uint64(P) + i + np.uint64(1)
        z = np.uint64(seed % (1 << 64)) + GOLDEN * counter
        z = z ^ (z >> np.uint64(30))
        z = z * M1
        z = z ^ (z >> np.uint64(27))
        z = z * M2
        z = z ^ (z >> np.uint64(31))
    return z


def uv(seed, draw, P, i=None):
    z = bits(seed, draw, P, i)
    return z >> np.uint64(40), (z >> np.uint64(16)) & np.uint64(0xFFFFFF)


def pixel_indices(u, v, h, w):
    """continuous == 0: (r, c) as int64"""
    return ((u * np.uint64(h)) >> np.uint64(24)).astype(np.int64), ((v * np.uint64(w)) >> np.uint64(24)).astype(np.int64)


def positions(u, v, h, w):
    """continuous == 1: fp32 (pr, pc)"""
    pr = (u.astype(F32) * TWO_M24) * F32(h - 1)
    pc = (v.astype(F32) * TWO_M24) * F32(w - 1)
    return pr, pc


def cells(pr, pc, h, w):
    """(r0, fr, c0, fc) of the bilinear lookup"""
    r0 = np.minimum(np.floor(pr).astype(np.int64), h - 2)
    c0 = np.minimum(np.floor(pc).astype(np.int64), w - 2)
    return r0, pr - r0.astype(F32), c0, pc - c0.astype(F32)


def array_texel(image):
    image = np.asarray(image)
    image = image[:, :, None] if image.ndim == 2 else image
    return lambda r, c, k: image[r, c, k]


def sample(texel, h, w, C, denom, seed, draw, P, continuous, i=None):
    """dict(xy (n,2) fp32, target (n,C) fp32, and — continuous — target64 (n,C) float64, r0, c0) of samples i of one draw.
    texel: array_texel(image) or any callable (r, c, k) -> uint8 on int64 index arrays."""
    u, v = uv(seed, draw, P, i)
    denom = F32(denom)
    out = {}
    if not continuous:
        r, c = pixel_indices(u, v, h, w)
        out["r"], out["c"] = r, c
        out["xy"] = np.stack([r.astype(F32) / denom, c.astype(F32) / denom], axis=1)
        out["target"] = np.stack([texel(r, c, k).astype(F32) / F32(255.0) for k in range(C)], axis=1)
        return out
    pr, pc = positions(u, v, h, w)
    out["pr"], out["pc"] = pr, pc
    out["xy"] = np.stack([pr / denom, pc / denom], axis=1)
    r0, fr, c0, fc = cells(pr, pc, h, w)
    out["r0"], out["c0"] = r0, c0
    one = F32(1.0)
    gr, gc = one - fr, one - fc
    w00, w01, w10, w11 = gr * gc, gr * fc, fr * gc, fr * fc
    fr64, fc64 = pr.astype(np.float64) - r0, pc.astype(np.float64) - c0
    t32, t64 = [], []
    for k in range(C):
        q = [texel(r0 + dr, c0 + dc, k) for dr, dc in ((0, 0), (0, 1), (1, 0), (1, 1))]
        t00, t01, t10, t11 = (x.astype(F32) / F32(255.0) for x in q)
        t32.append(((t00 * w00 + t01 * w01) + t10 * w10) + t11 * w11)
        d00, d01, d10, d11 = (x.astype(np.float64) / 255.0 for x in q)
        t64.append(d00 * (1 - fr64) * (1 - fc64) + d01 * (1 - fr64) * fc64 + d10 * fr64 * (1 - fc64) + d11 * fr64 * fc64)
    out["target"] = np.stack(t32, axis=1).astype(F32)
    out["target64"] = np.stack(t64, axis=1)
    return out
