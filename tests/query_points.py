"""Shared by tests/test_query_cpu.py and tests/test_gpu_query.py: the coordinates the query tests evaluate a model at off the
lattice, and the oracle's values there.  No test lives here.

off_lattice(P, n_ls, seed): P - len(tail) seeded uniform coordinates in [0, 1)^2 and a tail of exact values — 0.0 and 1.0 on
either axis, and k / N_l for several levels, the cell boundaries of level l, where floor() changes and a corner weight is 0.
The seeds below were chosen on the CPU: for each (model, seed) fewer than 5 % of the oracle's elements lie in the rounding zone
of test_gpu_render.check_render (tests/test_query_cpu.py asserts it for the models whose oracle is cheap)."""
import numpy as np

P_HASH, P_GNGF, P_OUTSIDE = 4099, 1031, 1031
SEED = 11
SEED_OUTSIDE = 12

HASH_MODELS = ("hash-L16F2", "hash-L4F2", "hash-L16F4", "hash-L10F4", "hash-fp16", "hash-leaky", "dense-levels")
GNGF_MODELS = ("gngf-frozen-K4", "gngf-frozen-K1", "gngf-trainable")


def boundary_tail(n_ls):
    """(row, column) float32 pairs of exact values: the corners and edges of the unit square, and cell boundaries k / N_l"""
    n_ls = [int(n) for n in n_ls]
    tail = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.5, 0.0), (1.0, 0.25)]
    for l in sorted({0, len(n_ls) // 2, len(n_ls) - 1}):
        n = n_ls[l]
        for k, k2 in ((1, 2), (n // 2, n - 1), (n - 1, n // 3), (n, 1)):
            tail.append((np.float32(k) / np.float32(n), np.float32(k2) / np.float32(n)))
        tail.append((np.float32(n // 2) / np.float32(n), 0.3))           # a boundary on one axis only
    return np.array(tail, dtype=np.float32)


def off_lattice(P, n_ls, seed=SEED):
    tail = boundary_tail(n_ls)
    assert P > len(tail)
    rng = np.random.default_rng(seed)
    body = rng.random((P - len(tail), 2), dtype=np.float32)
    xy = np.concatenate([body, tail]).astype(np.float32)
    assert xy.shape == (P, 2) and xy.min() >= 0.0 and xy.max() <= 1.0
    return xy


def outside(P=P_OUTSIDE, seed=SEED_OUTSIDE):
    """P seeded uniform coordinates in [-0.5, 1.5)^2: for the hash source, which is defined on the whole plane"""
    rng = np.random.default_rng(seed)
    xy = (rng.random((P, 2), dtype=np.float32) * np.float32(2.0) - np.float32(0.5)).astype(np.float32)
    assert xy.min() < 0 and xy.max() > 1
    return xy


_WANT = {}


def want(name, xy_key, xy):
    """the oracle's rgb for model `name` of test_gpu_score.MODELS (its seeded parameters) at xy, computed once per key"""
    import test_gpu_render as tr
    import test_gpu_score as ts
    key = (name, xy_key)
    if key not in _WANT:
        c = ts.MODELS[name]
        p = tr.render_params(c)
        if name == "dense-levels":
            from dense_levels_helpers import oracle_model
            got = oracle_model(p, xy, c["T"])[1]
        else:
            got = tr.oracle_rgb(c, p, xy)
        got.setflags(write=False)
        _WANT[key] = got
    return _WANT[key]


def model_n_ls(name):
    import test_gpu_score as ts
    from oracle import gngf_oracle as orc
    c = ts.MODELS[name]
    return orc.level_resolutions(c["n_min"], c["n_max"], c["L"])
