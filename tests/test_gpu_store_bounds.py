"""Where do the kernels write?  Every writing entry point of include/gngf.h, driven through the C ABI with every input, output and
workspace taken from a guard-band arena (tests/guarded.py), at the smallest shapes at which its store addressing can go wrong.

Each case asserts, after one synchronise:
  (a) guards      every arena byte outside the buffers is still 0xFF (a store next to a buffer is seen and named);
  (b) coverage    every element the header says the call writes is written (not 0xFF any more; all zero for a cleared buffer);
  (c) untouched   every region the header says the call leaves alone holds the bytes it held (inputs included);
  (d) values      what was written matches the float64 / oracle reference, at the tolerance the entry point's existing test uses
                  for the same quantity (cited at each check).

CASE_TABLE is plain data — (entry point, shape label, runner name, keyword arguments) — so that tests/test_store_bounds_ledger_cpu.py
can hold it against _lib.SIGNATURES without a device.  No case passes an invalid argument on purpose except where the header
names the rejection (hipErrorInvalidValue, no launch), and every guard lies inside one allocation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
from oracle import gngf_oracle as orc

DEV = "cuda"
F32, F16, F64, I32, I64, U8 = torch.float32, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8

CASE_TABLE = []          # (entry point, shape label, runner name, kwargs)
RUNNERS = {}


def cases(entry, table):
    """registers one case per (label, kwargs) of `table` for `entry`; the decorated function is the runner"""
    def deco(fn):
        RUNNERS[fn.__name__] = fn
        for label, kw in table:
            CASE_TABLE.append((entry, label, fn.__name__, kw))
        return fn
    return deco


def case_id(c):
    return f"{c[0]}-{c[1]}"


def entry_points():
    return sorted({c[0] for c in CASE_TABLE})


# ------------------------------------------------------------------------------------------------ helpers
def lib():
    from collision_handling_in_instantngp_amd import _lib
    return _lib


def close(got, want, rtol, atol, what):
    from conftest import parity_close
    parity_close(got, want, rtol, atol, what)


class Run:
    """one case's arena: inputs (their bytes are compared again at the end), outputs, and the single synchronise"""

    def __init__(self, mib=8):
        self.arena = guarded.Arena(mib << 20, DEV)
        self.frozen = []

    def i(self, values, name, dtype=None, misalign=0):
        t = self.arena.put(np.array(values) if isinstance(values, np.ndarray) else values, name, dtype, misalign)
        self.frozen.append((name, t, t.clone()))
        return t

    def o(self, shape, dtype=F32, name=None, fill=None, misalign=0):
        return self.arena.take(shape, dtype, fill=fill, misalign=misalign, name=name)

    def freeze(self, t, name):
        """an output region (or a whole in/out buffer's part) that this call must leave alone"""
        self.frozen.append((name, t, t.clone()))

    def done(self):
        torch.cuda.synchronize()
        self.arena.check()                                                       # (a)
        for name, t, before in self.frozen:                                      # (c)
            assert guarded.same_bytes(t, before), f"{name} was modified"


def covered(t, what):
    """(b): no element of t is still 0xFF"""
    n = int(guarded.unwritten(t).sum())
    assert n == 0, f"{what}: {n} of {t.numel()} elements never written"


def never_written(t, what):
    n = int((~guarded.unwritten(t)).sum())
    assert n == 0, f"{what}: {n} elements written that the call must leave alone"


def all_zero(t, what):
    """(b) for a cleared buffer: every byte zero"""
    n = int((t.reshape(-1).view(U8) != 0).sum())
    assert n == 0, f"{what}: {n} of {t.numel() * t.element_size()} bytes are not zero after the clear"


def P_(t):
    return lib().ptr(t)


def call(name, *args):
    _l = lib()
    _l.call(name, *args, _l.stream_ptr())


def query(name, *args):
    return lib().query(name, *args)


def host_i32(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


# ================================================================================================ decoder
DEC_P = (1, 127, 128, 129, 32769)        # 32769 = 128 * 256 + 1: the first P at which a workgroup owns a second tile
DEC_OA = [(o, a) for o in (1, 3, 4) for a in (0, 1)]


def dec_mib(P):
    return 8 if P < 1000 else 96


@functools.lru_cache(maxsize=None)
def dec_ref(P, in_dim, out_dim, leaky):
    """inputs and oracle of tests/test_gpu_dense.py::test_fused_decoder_vs_numpy (computed once per shape, read-only)"""
    rng = np.random.default_rng(P + in_dim)
    dims = [in_dim, 64, 64, out_dim]
    W = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(3)]
    B = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(3)]
    x = rng.standard_normal((P, in_dim)).astype(np.float32)
    gy = rng.standard_normal((P, out_dim)).astype(np.float32)
    tgt = rng.random((P, out_dim)).astype(np.float32)
    # THIS FILE'S OWN choice of inputs (everything else is that test's): no pixel sits on an activation's kink.  A pixel one of whose
    # 128 hidden pre-activations lies within the rounding of its own fp32 dot product of 0 — n 2^-24 sum |terms|, the standard bound of
    # an n-term sum, doubled for the rounded inputs of the second layer — has no reference derivative: the order of the sum decides
    # on which side it falls, its d enc moves by O(1) and every summed gradient by that pixel's share (tests/test_gpu_dense.py::
    # _decoder_errors takes a quantile and a slack for this; that test's seeds happen to have no such pixel, 32769 pixels of these
    # have 70 to 140).  Such pixels are drawn again until none is left: decided by the oracle's numbers alone.
    for _round in range(50):
        y, acts, pre = orc.decoder_forward(x, W, B, bool(leaky), keep=True)
        smooth = np.ones(P, bool)
        for i in range(2):
            mass = np.abs(acts[i]).astype(np.float64) @ np.abs(W[i]).T.astype(np.float64) + np.abs(B[i])
            smooth &= (np.abs(pre[i]) > 2 * W[i].shape[1] * 2.0 ** -24 * mass).all(1)
        if smooth.all():
            break
        x[~smooth] = rng.standard_normal((int((~smooth).sum()), in_dim)).astype(np.float32)
    assert smooth.all()
    dx, dW, dB = orc.decoder_backward(x, W, B, gy, bool(leaky))
    gl = np.float32(1.25)
    gy_t = (np.float64(gl) * 2.0 / (P * out_dim) * (y.astype(np.float64) - tgt)).astype(np.float32)
    dx_t, dW_t, dB_t = orc.decoder_backward(x, W, B, gy_t, bool(leaky))
    d = dict(x=x, W=W, B=B, gy=gy, tgt=tgt, gl=gl, y=y, drgb=(dx, dW, dB), target=(dx_t, dW_t, dB_t))
    for v in (x, gy, tgt, y, *W, *B):
        v.setflags(write=False)
    return d


def dec_weights(r, d):
    ws = []
    for i in range(3):
        ws += [r.i(d["W"][i], f"W{i}"), r.i(d["B"][i], f"b{i}")]
    return ws


def dec_grads(r, in_dim, out_dim):
    shapes = [(64, in_dim), (64,), (64, 64), (64,), (out_dim, 64), (out_dim,)]
    return [r.o(s, F32, n) for s, n in zip(shapes, ("dW0", "db0", "dW1", "db1", "dW2", "db2"))]


def check_dec_grads(grads, want, what):
    """tolerances of tests/test_gpu_dense.py::test_fused_decoder_vs_numpy (weight and bias gradients)"""
    _dx, dW, dB = want
    for i in range(3):
        scale = max(1.0, float(np.abs(dW[i]).max()))
        covered(grads[2 * i], f"{what} dW{i}")
        covered(grads[2 * i + 1], f"{what} db{i}")
        close(grads[2 * i], dW[i], 2e-4, 2e-5 * scale, f"{what} dW{i}")
        close(grads[2 * i + 1], dB[i], 2e-4, 2e-5 * scale, f"{what} db{i}")


def slab_maxima(slabs, P, in_dim, out_dim):
    ns, nf = query("gngf_decoder_bwd_slabs", P), query("gngf_decoder_slab_floats", in_dim, out_dim)
    return slabs.view(ns, nf)[:, nf - 1]


@cases("gngf_decoder_fwd", [(f"P{P}_out{o}_{'leaky' if a else 'relu'}_{'hidden' if h else 'nohidden'}", dict(P=P, out_dim=o, leaky=a, hidden=h))
                            for h in (0, 1) for P in DEC_P for o, a in DEC_OA])
def run_decoder_fwd(P, out_dim, leaky, hidden, in_dim=32):
    """hidden: gngf_decoder_hidden_floats(P) floats of workspace in whole 128-pixel tiles — guarded, and its values are held to the
    oracle through the gngf_decoder_bwd that reads them back (d enc)."""
    d = dec_ref(P, in_dim, out_dim, leaky)
    r = Run(dec_mib(P))
    enc, ws = r.i(d["x"], "enc"), dec_weights(r, d)
    rgb = r.o((P, out_dim), F32, "rgb")
    hid = r.o((query("gngf_decoder_hidden_floats", P),), F32, "hidden") if hidden else None
    call("gngf_decoder_fwd", P_(enc), *[P_(w) for w in ws], P_(rgb), P_(hid), P, in_dim, out_dim, leaky)
    if hidden:
        drgb, denc = r.i(d["gy"], "drgb"), r.o((P, in_dim), F32, "denc")
        slabs = r.o((query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", in_dim, out_dim),), F32, "slabs")
        call("gngf_decoder_bwd", P_(enc), P_(rgb), P_(drgb), P_(None), P_(None), *[P_(w) for w in ws[:5]], P_(denc), *[P_(None)] * 6,
             P_(slabs), P_(None), P_(hid), P_(None), 0, P, in_dim, out_dim, leaky)
    r.done()
    covered(rgb, "rgb")
    close(rgb, d["y"], 1e-5, 1e-6, "decoder_fwd rgb")                # test_fused_decoder_vs_numpy: rgb
    if hidden:
        covered(denc, "denc from the saved hidden layers")
        close(denc, d["drgb"][0], 1e-4, 2e-6, "d enc from the saved hidden layers")        # test_fused_decoder_vs_numpy: d enc


DEC_BWD_VARIANTS = {   # in_dim, saved hidden, process-wide hybrid switch (read only at in_dim 32 with saved hidden layers)
    "in16": (16, 0, 1), "in24_sentinel": (24, 0, 1), "in32_hybrid_hidden": (32, 1, 1), "in32_fp32_hidden": (32, 1, 0),
    "in32_fp32_recompute": (32, 0, 1), "in64": (64, 0, 1),
}


def dec_bwd_table(reduce_case):
    out = []
    for vi, v in enumerate(DEC_BWD_VARIANTS):
        for pi, P in enumerate(DEC_P):
            for oi, (o, a) in enumerate(DEC_OA):            # crossed: every (variant, P) sees all three out_dim and both activations
                out.append((f"{v}_P{P}_out{o}_{'leaky' if a else 'relu'}", dict(variant=v, P=P, out_dim=o, leaky=a, grads=not reduce_case,
                                                                                 from_target=bool((vi + pi + oi) & 1))))
    return out


def _decoder_bwd(variant, P, out_dim, leaky, grads, from_target, zero_floats=None):
    in_dim, use_hidden, hybrid = DEC_BWD_VARIANTS[variant]
    d = dec_ref(P, in_dim, out_dim, leaky)
    want = d["target"] if from_target else d["drgb"]
    r = Run(dec_mib(P))
    enc, ws = r.i(d["x"], "enc"), dec_weights(r, d)
    rgb_in = r.i(d["y"], "rgb")
    drgb = None if from_target else r.i(d["gy"], "drgb")
    tgt, gl = (r.i(d["tgt"], "target"), r.i(np.array([d["gl"]], np.float32), "gloss")) if from_target else (None, None)
    hid = None
    if use_hidden:           # filled by an unguarded forward launch on the same inputs: this case is about the backward's stores
        hid = r.o((query("gngf_decoder_hidden_floats", P),), F32, "hidden")
        tmp = torch.empty((P, out_dim), device=DEV)
        call("gngf_decoder_fwd", P_(enc), *[P_(w) for w in ws], P_(tmp), P_(hid), P, in_dim, out_dim, leaky)
        torch.cuda.synchronize()
        r.freeze(hid, "hidden (input of the backward)")
    denc = r.o((P, in_dim), F32, "denc")
    g = dec_grads(r, in_dim, out_dim)
    nslabs = query("gngf_decoder_bwd_slabs", P)
    slabs = r.o((nslabs * query("gngf_decoder_slab_floats", in_dim, out_dim),), F32, "slabs")
    amax = r.o((1,), F32, "denc_absmax")
    zf = r.o((zero_floats,), F32, "zero_fill") if zero_floats else None
    prev = query("gngf_set_decoder_bwd_hybrid", hybrid)
    try:
        call("gngf_decoder_bwd", P_(enc), P_(rgb_in), P_(drgb), P_(tgt), P_(gl), *[P_(w) for w in ws[:5]], P_(denc),
             *[P_(x if grads else None) for x in g], P_(slabs), P_(amax if grads else None), P_(hid), P_(zf), zero_floats or 0,
             P, in_dim, out_dim, leaky)
        if not grads:
            call("gngf_decoder_reduce", P_(slabs), *[P_(x) for x in g], P_(amax), P_(None), P_(None), P, in_dim, out_dim)
    finally:
        query("gngf_set_decoder_bwd_hybrid", prev)
    r.done()
    covered(denc, "denc")
    close(denc, want[0], 1e-4, 2e-6, f"{variant} d enc")           # test_fused_decoder_vs_numpy: d enc
    check_dec_grads(g, want, variant)
    # include/gngf.h: denc_absmax receives max |denc|, and the last float of every slab is that slab's maximum
    top = float(denc.abs().max())
    assert float(amax[0]) == top, (float(amax[0]), top)
    assert float(slab_maxima(slabs, P, in_dim, out_dim).max()) == top
    if zf is not None:
        all_zero(zf, f"zero_fill of {zero_floats} floats")


@cases("gngf_decoder_bwd", dec_bwd_table(False))
def run_decoder_bwd(**kw):
    """all six gradient pointers given: the call reduces its slabs itself"""
    _decoder_bwd(**kw)


@cases("gngf_decoder_reduce", dec_bwd_table(True))
def run_decoder_reduce(**kw):
    """gradient pointers all NULL in gngf_decoder_bwd (it stops at the slabs), then gngf_decoder_reduce: every slab word it needs
    must have been written, or the 0xFF = NaN fill shows in the gradients"""
    _decoder_bwd(**kw)


def zero_floats_table():
    out = []
    for P in (129, 32769):
        ns = min((P + 127) // 128, 256)
        zs = [4, 4 * 255, 4 * 257, 4 * (256 * ns + 1)] + ([4 * (3 * 256 * ns + 5)] if P == 32769 else [])
        out += [(P, z) for z in zs]
    return out


@cases("gngf_decoder_bwd", [(f"{v}_P{P}_zero_fill{z}", dict(variant=v, P=P, zero_floats=z))
                            for v in ("in64", "in32_hybrid_hidden") for P, z in zero_floats_table()])
def run_decoder_bwd_zero_fill(variant, P, zero_floats):
    """zero_fill starts 0xFF and is all zero afterwards: in_dim 64 clears on the way (per workgroup slices: per / zper / my_tiles),
    in_dim 32 takes the memset branch"""
    _decoder_bwd(variant, P, 3, 0, True, True, zero_floats=zero_floats)


@functools.lru_cache(maxsize=None)
def train_ref(P, out_dim, leaky):
    """inputs, float64 evaluation and the errors of the all-fp32 kernels on them: the yardstick of
    tests/test_gpu_dense.py::test_training_decoder_kernels_against_float64"""
    from test_gpu_dense import _decoder_case, _decoder_errors, _decoder_float64
    x, tgt, ws = _decoder_case(P, bool(leaky), out_dim, seed=P)
    gl = 0.37
    want = _decoder_float64(x, tgt, ws, bool(leaky), gl)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    enc, tg, g1, wt = t(x), t(tgt), t(np.array([gl], np.float32)), [t(w) for w in ws]
    rgb, denc = torch.empty((P, out_dim), device=DEV), torch.empty((P, 32), device=DEV)
    grads = [torch.empty_like(w) for w in wt]
    slabs = torch.empty((query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", 32, out_dim),), device=DEV)
    prev = query("gngf_set_decoder_bwd_hybrid", 0)
    try:
        call("gngf_decoder_fwd", P_(enc), *[P_(w) for w in wt], P_(rgb), P_(None), P, 32, out_dim, leaky)
        call("gngf_decoder_bwd", P_(enc), P_(rgb), P_(None), P_(tg), P_(g1), *[P_(w) for w in wt[:5]], P_(denc), *[P_(x_) for x_ in grads],
             P_(slabs), P_(None), P_(None), P_(None), 0, P, 32, out_dim, leaky)
        torch.cuda.synchronize()
    finally:
        query("gngf_set_decoder_bwd_hybrid", prev)
    base = _decoder_errors([rgb, want[1], denc] + grads, want)
    return dict(x=x, tgt=tgt, ws=ws, gl=gl, want=want, base=base)


def _decoder_train(P, out_dim, leaky, grads, zero_floats=None):
    from test_gpu_dense import _decoder_errors
    d = train_ref(P, out_dim, leaky)
    r = Run(dec_mib(P))
    enc, tgt, gl = r.i(d["x"], "enc"), r.i(d["tgt"], "target"), r.i(np.array([d["gl"]], np.float32), "gloss")
    ws = [r.i(w, f"w{i}") for i, w in enumerate(d["ws"])]
    rgb, denc = r.o((P, out_dim), F32, "rgb"), r.o((P, 32), F32, "denc")
    g = dec_grads(r, 32, out_dim)
    slabs = r.o((query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", 32, out_dim),), F32, "slabs")
    amax = r.o((1,), F32, "denc_absmax")
    zf = r.o((zero_floats,), F32, "zero_fill") if zero_floats else None
    call("gngf_decoder_train", P_(enc), P_(tgt), P_(gl), *[P_(w) for w in ws], P_(rgb), P_(denc), *[P_(x if grads else None) for x in g],
         P_(slabs), P_(amax if grads else None), P_(zf), zero_floats or 0, P, 32, out_dim, leaky)
    if not grads:
        call("gngf_decoder_reduce", P_(slabs), *[P_(x) for x in g], P_(amax), P_(None), P_(None), P, 32, out_dim)
    r.done()
    for t, n in [(rgb, "rgb"), (denc, "denc")] + list(zip(g, ("dW0", "db0", "dW1", "db1", "dW2", "db2"))):
        covered(t, n)
    # test_training_decoder_kernels_against_float64: at most twice the error of the all-fp32 kernels + its slack per quantity
    errs = _decoder_errors([rgb, d["want"][1], denc] + g, d["want"])
    names = ("rgb", "loss", "d enc", "dW0", "db0", "dW1", "db1", "dW2", "db2")
    for k, nm in enumerate(names):
        if k == 1:
            continue                                   # (the loss value is not an output of this entry point)
        slack = 1e-7 if k in (0, 2) else 2e-4
        close(np.array([errs[k]]), np.array([0.0]), 0, 2 * d["base"][k] + slack, f"decoder_train vs float64: {nm} (P={P})")
    top = float(denc.abs().max())
    assert float(amax[0]) == top and float(slab_maxima(slabs, P, 32, out_dim).max()) == top
    if zf is not None:
        all_zero(zf, f"zero_fill of {zero_floats} floats")


@cases("gngf_decoder_train", [(f"P{P}_out{o}_{'leaky' if a else 'relu'}_{'grads' if g else 'reduce'}", dict(P=P, out_dim=o, leaky=a, grads=g))
                              for g in (1, 0) for P in DEC_P for o, a in DEC_OA]
       + [(f"P{P}_zero_fill{z}", dict(P=P, out_dim=3, leaky=0, grads=1, zero_floats=z)) for P, z in zero_floats_table()])
def run_decoder_train(**kw):
    _decoder_train(**kw)


# ================================================================================================ dense layers
DENSE_SHAPES = [(1, 1, 1), (127, 3, 33), (128, 128, 32), (129, 128, 32), (128, 129, 32), (128, 128, 48), (256, 128, 64)]
GEMM_CODES = (0, 1, 2, 17)


def shape_label(s):
    return "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def dense_ref(M, N, K):
    """tests/test_gpu_dense.py::test_linear_fwd_bwd_vs_numpy's inputs and float64 expressions"""
    rng = np.random.default_rng(M + N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) * 0.1
    dy = rng.standard_normal((M, N)).astype(np.float32)
    z = x.astype(np.float64) @ w.T.astype(np.float64) + b
    ys = {0: z, 1: np.maximum(z, 0), 2: np.where(z > 0, z, 0.01 * z), 3: 1 / (1 + np.exp(-z))}
    return dict(x=x, w=w, b=b, dy=dy, z=z, y=ys)


def dact(d, act):
    z, y = d["z"], d["y"][act]
    return {0: np.ones_like(z), 1: (z > 0) * 1.0, 2: np.where(z > 0, 1.0, 0.01), 3: y * (1 - y)}[act]


@cases("gngf_linear_fwd", [(shape_label(s), dict(shape=s)) for s in DENSE_SHAPES])
def run_linear_fwd(shape):
    """every activation under every GEMM code (a split code on a shape the split kernels do not take runs the fp32 kernels)"""
    M, N, K = shape
    d = dense_ref(M, N, K)
    for gemm in GEMM_CODES:
        for act in (0, 1, 2, 3):
            r = Run()
            x, w, b = r.i(d["x"], "X"), r.i(d["w"], "W"), r.i(d["b"], "b")
            y = r.o((M, N), F32, "Y")
            call("gngf_linear_fwd", P_(x), P_(w), P_(b), P_(y), M, N, K, act, gemm)
            r.done()
            covered(y, f"Y gemm {gemm} act {act}")
            close(y, d["y"][act], 1e-5, 1e-5, f"linear_fwd gemm {gemm} act {act}")      # test_linear_fwd_bwd_vs_numpy


@cases("gngf_linear_bwd_input", [(shape_label(s), dict(shape=s)) for s in DENSE_SHAPES])
def run_linear_bwd_input(shape):
    M, N, K = shape
    d = dense_ref(M, N, K)
    for act in (0, 1, 2, 3):
        r = Run()
        dy, y, w = r.i(d["dy"], "dY"), r.i(d["y"][act].astype(np.float32), "Y"), r.i(d["w"], "W")
        dx = r.o((M, K), F32, "dX")
        call("gngf_linear_bwd_input", P_(dy), P_(y if act else None), P_(w), P_(dx), M, N, K, act)
        r.done()
        covered(dx, f"dX act {act}")
        close(dx, (d["dy"] * dact(d, act)) @ d["w"].astype(np.float64), 1e-4, 1e-4, f"linear_bwd_input act {act}")   # same test


@cases("gngf_linear_bwd_weight", [(shape_label(s), dict(shape=s)) for s in DENSE_SHAPES])
def run_linear_bwd_weight(shape):
    """accumulating outputs start at 0; db given and NULL"""
    M, N, K = shape
    d = dense_ref(M, N, K)
    for gemm in GEMM_CODES:
        for act in (0, 1, 2, 3):
            for with_db in ((1, 0) if act == 0 else (1,)):
                r = Run()
                dy, y, x = r.i(d["dy"], "dY"), r.i(d["y"][act].astype(np.float32), "Y"), r.i(d["x"], "X")
                dw = r.o((N, K), F32, "dW", fill=0)
                db = r.o((N,), F32, "db", fill=0) if with_db else None
                call("gngf_linear_bwd_weight", P_(dy), P_(y if act else None), P_(x), P_(dw), P_(db), M, N, K, act, gemm)
                r.done()
                dz = d["dy"] * dact(d, act)
                scale = np.abs(dz.T @ d["x"]).max() + 1e-6
                close(dw, dz.T @ d["x"].astype(np.float64), 1e-4, 1e-5 * scale, f"dW gemm {gemm} act {act}")    # same test
                if with_db:
                    close(db, dz.sum(0), 1e-4, 1e-5 * scale, f"db gemm {gemm} act {act}")


@cases("gngf_gemm_acc", [(shape_label(s), dict(shape=s)) for s in DENSE_SHAPES])
def run_gemm_acc(shape):
    """the four layouts under every GEMM code; C starts at 0"""
    M, N, Kc = shape
    rng = np.random.default_rng(3)
    for ta in (0, 1):
        for tb in (0, 1):
            a = rng.standard_normal((Kc, M) if ta else (M, Kc)).astype(np.float32)
            b = rng.standard_normal((N, Kc) if tb else (Kc, N)).astype(np.float32)
            want = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
            for gemm in GEMM_CODES:
                r = Run()
                at, bt = r.i(a, "A"), r.i(b, "B")
                c = r.o((M, N), F32, "C", fill=0)
                call("gngf_gemm_acc", P_(at), P_(bt), P_(c), M, N, Kc, ta, tb, gemm)
                r.done()
                close(c, want, 1e-4, 1e-3, f"gemm_acc ta {ta} tb {tb} gemm {gemm}")     # test_gemm_acc_all_layouts


@cases("gngf_linear_fwd_rowstats", [(shape_label(s), dict(shape=s)) for s in DENSE_SHAPES])
def run_linear_fwd_rowstats(shape):
    """whole 128 x 128 tiles with K % 32 == 0 only: any other shape is rejected (hipErrorInvalidValue, include/gngf.h) and then
    nothing at all may be written.  Accepted: Y bit-identical to gngf_linear_fwd under GNGF_GEMM_PLANES, rowparts (M, N / 64) pairs
    (max, sum exp(y - max)) against numpy on the launch's own Y."""
    M, N, K = shape
    d = dense_ref(M, N, K)
    r = Run()
    x, w, b = r.i(d["x"], "X"), r.i(d["w"], "W"), r.i(d["b"], "b")
    y = r.o((M, N), F32, "Y")
    parts = r.o((M, max(N // 64, 1), 2), F32, "rowparts")
    args = (P_(x), P_(w), P_(b), P_(y), P_(parts), M, N, K)
    if M % 128 or N % 128 or K % 32:
        with pytest.raises(RuntimeError, match="rejected arguments"):
            call("gngf_linear_fwd_rowstats", *args)
        r.done()
        never_written(y, "Y of a rejected call")
        never_written(parts, "rowparts of a rejected call")
        return
    call("gngf_linear_fwd_rowstats", *args)
    y1 = torch.empty((M, N), device=DEV)
    call("gngf_linear_fwd", P_(x), P_(w), P_(b), P_(y1), M, N, K, 0, 1)
    r.done()
    covered(y, "Y")
    covered(parts, "rowparts")
    assert torch.equal(y, y1)                 # test_logits_gemm_with_epilogue_statistics_equals_the_separate_pass: bit-identical logits
    close(y, d["z"], 1e-5, 1e-5, "rowstats Y")                                           # test_linear_fwd_bwd_vs_numpy
    blocks = y.cpu().numpy().astype(np.float64).reshape(M, N // 64, 64)
    mx = blocks.max(-1)
    close(parts[:, :, 0], mx, 0, 0, "rowparts maxima")                                   # same test: row maxima exact
    close(parts[:, :, 1], np.exp(blocks - mx[..., None]).sum(-1), 1e-5, 0, "rowparts sums")   # same test: row sums 1e-5


# ================================================================================================ loss, metrics, optimiser, epoch
@cases("gngf_mse_fwd", [(f"n{n}", dict(n=n)) for n in (1, 3, 4099)])
def run_mse_fwd(n):
    """the workspace is zero before the first call and the kernel puts it back to zero"""
    rng = np.random.default_rng(n)
    a, b = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    r = Run()
    pred, label = r.i(a, "pred"), r.i(b, "label")
    loss = r.o((1,), F32, "loss")
    ws = r.o((query("gngf_mse_workspace_floats"),), F32, "workspace", fill=0)
    for _rep in range(2):
        call("gngf_mse_fwd", P_(pred), P_(label), P_(loss), P_(ws), n)
    r.done()
    covered(loss, "loss")
    all_zero(ws, "mse workspace after the call")
    close(loss, [np.mean((a.astype(np.float64) - b) ** 2)], 2e-6, 0, "mse value")        # test_mse_kernels_vs_numpy


@cases("gngf_mse_bwd", [(f"n{n}", dict(n=n)) for n in (1, 3, 4099)])
def run_mse_bwd(n):
    """pred, label and dpred must be 16-byte aligned (the launcher rejects anything else: nothing may be written then)"""
    rng = np.random.default_rng(n)
    a, b = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    for mis in (0, 4):
        r = Run()
        pred, label, gout = r.i(a, "pred", misalign=mis), r.i(b, "label", misalign=mis), r.i(np.array([3.0], np.float32), "gout")
        dpred = r.o((n,), F32, "dpred", misalign=mis)
        if mis:
            with pytest.raises(RuntimeError, match="rejected arguments"):
                call("gngf_mse_bwd", P_(pred), P_(label), P_(gout), P_(dpred), n)
            r.done()
            never_written(dpred, "dpred of a rejected call")
            continue
        call("gngf_mse_bwd", P_(pred), P_(label), P_(gout), P_(dpred), n)
        r.done()
        covered(dpred, "dpred")
        close(dpred, 3.0 * 2.0 * (a.astype(np.float64) - b) / n, 1e-6, 1e-12, "mse gradient")     # test_mse_kernels_vs_numpy


JS_GAMMA, JS_EPS = -2.0, 1.0     # train.Loss(delta=1, gamma=-2, epsilon=1), what the training tests run: out = JS + KL, no cancellation


def js_kl_case(L, T):
    """tests/test_gpu_dense.py::test_js_kl_kernels_vs_float64_and_torch_expression: its inputs, float64 reference and bounds — but NOT
    its loss weights: the weights are this file's own choice (those of the training tests), made because the kernel MISSES that
    test's bound at this shape under that test's weights.  (With that test's gamma = 1, eps = 0.5 the two terms of a row cancel to a twentieth of
    their size at this seed and T = 77; the kernel rounds every summand to fp32 as torch does, and the row then sits 1.0e-5
    relative / 5.4e-9 absolute from float64 — the summands' rounding, seen against a bound that is relative to the difference.)"""
    from collision_handling_in_instantngp_amd.train import Loss
    rng = np.random.default_rng(L * 7 + T)
    z = rng.standard_normal((L, T)) * 2.0
    p = np.exp(z - z.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    w = rng.standard_normal(L).astype(np.float32)
    loss = Loss(gamma=JS_GAMMA, epsilon=JS_EPS)
    pd = torch.tensor(p, dtype=F64, requires_grad=True)
    want = loss.js_kl_rows_torch(pd)
    (want * torch.tensor(w, dtype=F64)).sum().backward()
    return p, w, want.detach().numpy(), pd.grad.numpy()


@cases("gngf_js_kl_fwd", [("L3_T77", dict(L=3, T=77))])
def run_js_kl_fwd(L, T):
    p, _w, want, _g = js_kl_case(L, T)
    r = Run()
    pbar = r.i(p, "pbar")
    out = r.o((L,), F32, "out")
    ws = r.o((query("gngf_js_kl_workspace_doubles", L),), F64, "workspace")
    call("gngf_js_kl_fwd", P_(pbar), P_(out), P_(ws), L, T, JS_GAMMA, JS_EPS)
    r.done()
    covered(out, "out")
    close(out, want, 2e-6, 1e-9, "js_kl rows")


@cases("gngf_js_kl_bwd", [("L3_T77", dict(L=3, T=77))])
def run_js_kl_bwd(L, T):
    p, w, _want, grad = js_kl_case(L, T)
    r = Run()
    pbar, gout = r.i(p, "pbar"), r.i(w, "gout")
    dp = r.o((L, T), F32, "dpbar")
    call("gngf_js_kl_bwd", P_(pbar), P_(gout), P_(dp), L, T, JS_GAMMA, JS_EPS)
    r.done()
    covered(dp, "dpbar")
    close(dp, grad, 2e-5, 1e-6 * float(np.abs(grad).max()), "js_kl gradient")


@cases("gngf_image_scatter", [(f"P37_C{C}_lo5_n9_{'perm' if perm else 'identity'}", dict(C=C, perm=perm)) for C in (1, 3, 4) for perm in (1, 0)])
def run_image_scatter(C, perm, P=37, lo=5, n=9):
    """rows perm[lo : lo + n] of img are written, every other row keeps its bytes; values exact ((out * 255).int(), no clamp)"""
    rng = np.random.default_rng(C)
    out_h = (rng.random((n, C)) * 1.2 - 0.1).astype(np.float32)
    pm = rng.permutation(P).astype(np.int32)
    rows = pm[lo:lo + n] if perm else np.arange(lo, lo + n)
    r = Run()
    out = r.i(out_h, "out")
    pt = r.i(pm, "perm") if perm else None
    img = r.o((P, C), I32, "img")
    call("gngf_image_scatter", P_(out), P_(pt), P_(img), lo, n, P, C)
    r.done()
    mask = np.zeros(P, bool)
    mask[rows] = True
    never_written(img[torch.from_numpy(~mask).to(DEV)], "image rows outside perm[lo : lo + n]")
    want = (torch.from_numpy(out_h) * 255.0).int().numpy()           # tests/test_gpu_epoch_image.py: exact
    assert np.array_equal(img.cpu().numpy()[rows], want)


@cases("gngf_image_metrics", [(f"n{n}", dict(n=n)) for n in (1, 37 * 3, 70001)])
def run_image_metrics(n):
    rng = np.random.default_rng(n)
    a = rng.integers(-3, 260, n).astype(np.int32)
    b = rng.integers(0, 256, n).astype(np.uint8)
    a[::3] = b[::3]
    r = Run()
    img, tgt = r.i(a, "img"), r.i(b, "target")
    sums = r.o((2,), I64, "sums")
    words = query("gngf_image_metrics_workspace_words", n)
    ws = r.o((words,), I64, "workspace")
    call("gngf_image_metrics", P_(img), P_(tgt), P_(sums), P_(ws), n)
    r.done()
    covered(sums, "sums")
    d = a.astype(np.int64) - b
    assert sums.tolist() == [int((d == 0).sum()), int((d * d).sum())]      # tests/test_gpu_epoch_image.py: exact


ADAM_FLAGS = {"fp32": 0, "fp16": 1, "fp16_grad32": 3}


def adam_table():
    return [(f"{fl}_n_{nn}_{'off1' if off else 'aligned'}", dict(flavour=fl, n_name=nn, off=off))
            for fl in ADAM_FLAGS for nn in ("1", "block-1", "block", "block+1") for off in (0, 1)]


def adam_state(r, n, flags, off, seed, nan_rows=None):
    """tests/test_gpu_adam_masked.py::make_state, in the arena: views `off` elements off 16-byte alignment"""
    gen = torch.Generator().manual_seed(seed)
    pd = F16 if flags & 1 else F32
    gd = F16 if flags == 1 else F32

    def buf(dtype, scale, name, positive=False, src=None):
        x = torch.randn(n, generator=gen) * scale if src is None else src
        x = (x.abs() if positive else x).to(dtype)
        t = r.o((n,), dtype, name, misalign=off * x.element_size())
        t.copy_(x)
        return t
    master = buf(F32, 0.1, "master") if flags & 1 else None
    p = buf(pd, 0.1, "param", src=None if master is None else master.cpu().clone())
    return {"p": p, "g": buf(gd, 1e-2, "grad"), "m": buf(F32, 1e-3, "exp_avg"), "v": buf(F32, 1e-5, "exp_avg_sq", positive=True), "master": master}


def adam_launch(r, st, flags, mask=None, row_elems=0, steps_before=3.0):
    """tests/test_gpu_adam_masked.py::adam_call with the segment table, the mask record and the step counter in the arena"""
    from collision_handling_in_instantngp_amd.train import FusedAdam
    from test_gpu_adam_masked import B1, B2, EPS, LR
    p = st["p"]
    seg = (p.data_ptr(), st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), 0 if st["master"] is None else st["master"].data_ptr(),
           p.numel(), 0, flags)
    masks = None if mask is None else [(mask.data_ptr(), row_elems, 0)]
    raw, blocks = FusedAdam.pack_records([seg], masks, query("gngf_adam_block_elems"))
    table = r.i(raw.copy(), "segments")
    step = r.o((1,), F32, "step", fill=steps_before)
    lr, wd = (ctypes.c_float * 1)(LR), (ctypes.c_float * 1)(0.0)
    args = (P_(table), 1, blocks, P_(step), lr, wd, 1, B1, B2, EPS, 1.0)
    if mask is not None:
        call("gngf_adam_step_masked", *args, ctypes.c_void_p(table.data_ptr() + 64))
    else:
        call("gngf_adam_step", *args)
    return step


def adam_n(n_name):
    be = query("gngf_adam_block_elems")
    return {"1": 1, "block-1": be - 1, "block": be, "block+1": be + 1}[n_name]


def adam_want(st0, flags, steps_before=3.0):
    """oracle/gngf_oracle.py::adam_step (torch.optim.Adam restated in numpy) on the state as the kernel reads it"""
    from test_gpu_adam_masked import B1, B2, EPS, LR
    f = lambda t: t.detach().cpu().numpy().astype(np.float32)
    p = f(st0["master"]) if flags & 1 else f(st0["p"])
    return orc.adam_step(p, f(st0["g"]), f(st0["m"]), f(st0["v"]), int(steps_before) + 1, LR, 0.0, betas=(B1, B2), eps=EPS)


def check_adam(st, st0, flags, keep=None):
    """values: the oracle's torch.optim.Adam at the tolerances of tests/test_gpu_dense.py::test_fused_adam_matches_torch_adam_over_steps
    (parameters 2e-6 / 1e-6, moments 2e-6 / 2e-6 of their largest)"""
    pw, mw, vw = adam_want(st0, flags)
    sel = slice(None) if keep is None else torch.from_numpy(keep).to(DEV)
    seln = slice(None) if keep is None else keep
    tgt = st["master"] if flags & 1 else st["p"]
    close(tgt[sel], pw[seln], 2e-6, 1e-6, "adam parameter")
    close(st["m"][sel], mw[seln], 2e-6, 2e-6 * float(np.abs(mw[seln]).max()), "adam exp_avg")
    close(st["v"][sel], vw[seln], 2e-6, 2e-6 * float(np.abs(vw[seln]).max()), "adam exp_avg_sq")
    if flags & 1:                                   # param = round(master)
        assert torch.equal(st["p"][sel], st["master"][sel].to(F16))


@cases("gngf_adam_step", adam_table())
def run_adam_step(flavour, n_name, off):
    flags, n = ADAM_FLAGS[flavour], adam_n(n_name)
    r = Run()
    st = adam_state(r, n, flags, off, seed=n + off)
    st0 = {k: (None if v is None else v.clone()) for k, v in st.items()}
    r.freeze(st["g"], "grad")
    step = adam_launch(r, st, flags)
    r.done()
    assert float(step[0]) == 4.0
    check_adam(st, st0, flags)


@cases("gngf_adam_step_masked", adam_table())
def run_adam_step_masked(flavour, n_name, off, F=2):
    """rows of F = 2 elements, every third row masked in: masked-out rows keep their bytes (they start 0xFF: never written),
    masked-in rows take the step"""
    flags, n = ADAM_FLAGS[flavour], adam_n(n_name)
    rows = (n + F - 1) // F
    keep_rows = (np.arange(rows) % 3) == 0
    keep = np.repeat(keep_rows, F)[:n]
    r = Run()
    st = adam_state(r, n, flags, off, seed=n + off)
    words = np.zeros(((rows + 31) // 32,), np.uint32)
    for i in np.flatnonzero(keep_rows):
        words[i >> 5] |= np.uint32(1 << (i & 31))
    mask = r.i(words.view(np.int32), "rowmask")
    out = torch.from_numpy(~keep).to(DEV)
    for k in ("p", "m", "v", "master"):
        if st[k] is not None:
            st[k].view(torch.int16 if st[k].dtype == F16 else I32)[out] = -1        # 0xFF again: "never written"
    st0 = {k: (None if v is None else v.clone()) for k, v in st.items()}
    r.freeze(st["g"], "grad")
    step = adam_launch(r, st, flags, mask=mask, row_elems=F)
    r.done()
    assert float(step[0]) == 4.0
    for k in ("p", "m", "v", "master"):
        if st[k] is not None:
            never_written(st[k][out], f"masked-out rows of {k}")
    if keep.any():
        check_adam(st, st0, flags, keep)


@cases("gngf_epoch_tail", [("e0_then_e1_of_3_used", dict(with_used=1)), ("e0_then_e1_of_3_no_used", dict(with_used=0))])
def run_epoch_tail(with_used, epochs=3, nb=3, L=5):
    """two calls (e = 0, then e = 1) on a 3-epoch log: after each, only row e of logf / logi is written; the means are numpy's
    (tests/test_gpu_epoch_loop.py::test_epoch_tail_means_are_numpy_means_bit_for_bit), the integer columns exact"""
    from collision_handling_in_instantngp_amd import train
    rng = np.random.default_rng(11)
    Kc = 2 if with_used else 0
    r = Run()
    state = r.i(train.new_epoch_state(10 ** 6).reshape(1).view(np.uint8).copy(), "state_init")
    r.frozen.pop()                                                # (the state is in/out)
    logf = r.o((epochs, 2 + 2 * L), F64, "logf")
    logi = r.o((epochs, query("gngf_epoch_log_int_columns", Kc, L)), I64, "logi")
    nverts = r.i(np.arange(1, L + 1).astype(np.int64) * 10, "nverts")
    ins = []
    for e in range(2):
        loss, mse = rng.random(nb).astype(np.float32), rng.random(nb).astype(np.float32)
        kls, colls = rng.standard_normal((nb, L)).astype(np.float32), rng.random((nb, L)).astype(np.float32)
        sums = np.array([100 + e, 1000 - e], np.int64)
        used = rng.integers(1, 9, (Kc, L)).astype(np.int32) if with_used else None
        ins.append((loss, mse, kls, colls, sums, used))
        dev = [r.i(loss, f"loss{e}"), r.i(mse, f"mse{e}"), r.i(kls, f"kls{e}"), r.i(colls, f"colls{e}"), r.i(sums, f"sums{e}"),
               r.i(used, f"used{e}") if with_used else None]
        call("gngf_epoch_tail", P_(state), P_(logf), P_(logi), P_(dev[0]), P_(dev[1]), P_(dev[2]), P_(dev[3]), nb, L, P_(dev[4]), P_(dev[5]),
             Kc, 0, P_(nverts), 99.0, 0.0, 1, epochs)
        if e == 0:                                               # between the calls: row 0 only (this sync belongs to the first call)
            torch.cuda.synchronize()
            never_written(logf[1:], "logf rows other than e = 0")
            never_written(logi[1:], "logi rows other than e = 0")
            r.freeze(logf[0], "logf row 0 during the call for e = 1")
            r.freeze(logi[0], "logi row 0 during the call for e = 1")
    r.done()
    never_written(logf[2:], "logf rows other than e")
    never_written(logi[2:], "logi rows other than e")
    covered(logi[:2], "logi rows 0, 1")
    lf, li = logf.cpu().numpy(), logi.cpu().numpy()
    for e, (loss, mse, kls, colls, sums, used) in enumerate(ins):
        want = np.concatenate([[np.mean(loss.astype(np.float64)), np.mean(mse.astype(np.float64))],
                               np.mean(kls.astype(np.float64), axis=0), np.mean(colls.astype(np.float64), axis=0)])
        assert lf[e].tobytes() == want.tobytes(), (e, lf[e], want)
        assert li[e, :2].tolist() == sums.tolist()
        if with_used:
            assert li[e, 6:].tolist() == used.reshape(-1).tolist()
    st = state.cpu().numpy().view(train.EPOCH_STATE)[0]
    assert int(st["epoch"]) == 2 and int(st["finished"]) == 0


# ================================================================================================ collision statistics
STAT_L, STAT_T = 4, 1000


def stat_levels():
    return orc.level_resolutions(8, 32, STAT_L)


@cases("gngf_distinct_slot_counts", [(f"P{P}_K{K}", dict(P=P, K=K)) for P in (1, 333) for K in (1, 3)])
def run_distinct_slot_counts(P, K, V=4):
    """bitmap: gngf_slot_bitmap_words words of workspace, cleared by the call (handed over as 0xFF)"""
    L, T = STAT_L, STAT_T
    rng = np.random.default_rng(P + K)
    idx = rng.integers(0, T, (P, L, V, K)).astype(np.int64)
    r = Run()
    it = r.i(idx if K > 1 else idx[..., 0], "indices")
    words = query("gngf_slot_bitmap_words", L, K, T)
    bitmap = r.o((words,), I32, "bitmap")
    counts = r.o((K, L), I32, "counts")
    call("gngf_distinct_slot_counts", P_(it), P, L, V, K, T, P_(bitmap), P_(counts))
    r.done()
    covered(counts, "counts")
    covered(bitmap, "bitmap (cleared, then marked)")
    want = [[len(np.unique(idx[:, l, :, k])) for l in range(L)] for k in range(K)]       # torch.unique(...).numel(): exact
    assert counts.tolist() == want
    assert int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in bitmap.cpu().numpy())) == int(np.sum(want))


def stat_touched_slots(xy, n_ls, T, vert_idx, vstride):
    """the slots batch xy uses, per (k, level): the slots of its touched vertices"""
    scaled, grid = orc.scale_to_grid(xy, n_ls)
    g = grid.astype(np.int32)                                     # (P,2,L,4)
    if vert_idx is None:
        return [[set(orc.spatial_hash(g, T)[:, l].reshape(-1).tolist()) for l in range(len(n_ls))]]
    vid = g[:, 1].astype(np.int64) * vstride + g[:, 0]            # (P,L,4): vid = gy * vstride + gx
    return [[set(vert_idx[vid[:, l].reshape(-1), k].tolist()) for l in range(len(n_ls))] for k in range(vert_idx.shape[1])]


def stat_xy(P, seed):
    rng = np.random.default_rng(seed)
    xy = rng.random((P, 2)).astype(np.float32)
    xy[0] = (0.0, 1.0)
    if P > 2:
        xy[1], xy[2] = (1.0, 1.0), (0.0, 0.0)
    return xy


@cases("gngf_mark_batch_slots", [(f"P{P}_{src}", dict(P=P, src=src)) for P in (1, 333) for src in ("hash", "table_K3")])
def run_mark_batch_slots(P, src):
    """bitmap is accumulated (the caller clears it once): starts zero with one planted bit — a slot of map (k = K - 1, l = 0) the
    batch does not use — that must survive; afterwards it holds exactly the batch's slots and that bit.  `touched` is workspace of
    L * ceil(NV / 32) words, cleared by the call.  gngf_count_slot_bits then gives the counts (exact)."""
    L, T = STAT_L, STAT_T
    n_ls = stat_levels()
    vstride = int(n_ls.max()) + 2
    NV = vstride * vstride
    K = 1 if src == "hash" else 3
    rng = np.random.default_rng(P)
    vi = None if src == "hash" else rng.integers(0, T, (NV, K)).astype(np.int32)
    xy = stat_xy(P, P + 1)
    r = Run()
    xt, nt = r.i(xy, "xy"), r.i(n_ls, "n_ls")
    vt = None if vi is None else r.i(vi, "vert_idx")
    words = query("gngf_slot_bitmap_words", L, K, T)
    per = (T + 31) // 32
    assert words == K * L * per
    want = stat_touched_slots(xy, n_ls, T, vi, vstride)
    planted = next(s_ for s_ in range(T - 1, -1, -1) if s_ not in want[K - 1][0])
    bits = np.zeros((K * L, per * 32), bool)               # map (k, l) = words [(k L + l) per, ...), bit slot & 31 of word slot >> 5
    for k in range(K):
        for l in range(L):
            bits[k * L + l, sorted(want[k][l])] = True
    bits[(K - 1) * L, planted] = True
    bitmap = r.o((words,), I32, "bitmap", fill=0)
    bitmap[(K - 1) * L * per + (planted >> 5)] = int(np.array([1 << (planted & 31)], np.uint32).view(np.int32)[0])
    touched = r.o((L * ((NV + 31) // 32),), I32, "touched")
    counts = r.o((K, L), I32, "counts")
    call("gngf_mark_batch_slots", P_(xt), P_(nt), P, L, P_(vt), K, T, vstride, NV, P_(touched), P_(bitmap))
    call("gngf_count_slot_bits", P_(bitmap), L, K, T, P_(counts))
    r.done()
    covered(counts, "counts")
    covered(touched, "touched (cleared, then marked)")
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint32), np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(-1))
    assert counts.tolist() == [[len(want[k][l]) + int(k == K - 1 and l == 0) for l in range(L)] for k in range(K)]


@cases("gngf_count_slot_bits", [(f"K{K}_T{T}", dict(K=K, T=T)) for K in (1, 3) for T in (31, 1000)])
def run_count_slot_bits(K, T, L=3):
    rng = np.random.default_rng(K + T)
    words = query("gngf_slot_bitmap_words", L, K, T)
    per = words // (L * K)
    assert per * L * K == words and per >= (T + 31) // 32
    bits = rng.random((K * L, per * 32)) < 0.3
    bits[:, T:] = False
    packed = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(-1)
    r = Run()
    bm = r.i(packed.view(np.int32), "bitmap")
    counts = r.o((K, L), I32, "counts")
    call("gngf_count_slot_bits", P_(bm), L, K, T, P_(counts))
    r.done()
    covered(counts, "counts")
    assert counts.reshape(-1).tolist() == bits.sum(1).tolist()          # map (k, l) is words [(k L + l) words, ...): exact


@cases("gngf_mark_reachable_rows", [(f"T{T}_{src}", dict(T=T, src=src)) for T in (1000, 2048) for src in ("hash", "table_K3")])
def run_mark_reachable_rows(T, src):
    """rowmask (L, ceil(T / 32)) words, OR-accumulated and never cleared: starts zero; against the numpy maps of
    tests/test_adam_mask_cpu.py (exact, as tests/test_gpu_adam_masked.py)"""
    from test_adam_mask_cpu import expected_hash_row_map, expected_table_row_map
    L = STAT_L
    n_ls = stat_levels()
    words = (T + 31) // 32
    assert query("gngf_slot_bitmap_words", L, 1, T) == L * words
    K, vstride, NV, vi = 1, 0, 0, None
    if src != "hash":
        K, vstride = 3, 20                                          # narrower than the finest level: those vertices are skipped
        NV = vstride * vstride - 5
        vi = np.random.default_rng(T).integers(0, T, (NV, K)).astype(np.int32)
    r = Run()
    nt = r.i(n_ls, "n_ls")
    vt = None if vi is None else r.i(vi, "vert_idx")
    m = r.o((L, words), I32, "rowmask", fill=0)
    call("gngf_mark_reachable_rows", P_(nt), host_i32(n_ls), L, P_(vt), K, T, vstride, NV, P_(m))
    r.done()
    want = expected_hash_row_map(n_ls, T) if vi is None else expected_table_row_map(n_ls, T, vi, vstride)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), want)


# ================================================================================================ render
REN = dict(L=4, F=2, n_min=8, n_max=32)
REN_LATTICES = [(1, 1), (3, 43), (129, 1)]
REN_ORIGIN = (5, 7)
REN_DENOM = 160.0


@functools.lru_cache(maxsize=None)
def render_model(out_dim, source, T=512, K=4):
    """a model in numpy and its vertex table; the vertex-table source's reference is the oracle's GNGF branch with the raw blend
    (vert_w are blend WEIGHTS) on indices expanded per instance"""
    rng = np.random.default_rng(1000 + out_dim)
    L, F = REN["L"], REN["F"]
    n_ls = orc.level_resolutions(REN["n_min"], REN["n_max"], L)

    def linear(o, i):
        b = 1.0 / np.sqrt(i)
        return rng.uniform(-b, b, (o, i)).astype(np.float32), rng.uniform(-b, b, (o,)).astype(np.float32)
    tables = rng.uniform(-1, 1, (L, T, F)).astype(np.float32)
    dec = [linear(64, L * F), linear(64, 64), linear(out_dim, 64)]
    vstride = int(n_ls.max()) + 2
    NV = vstride * vstride
    vi = rng.integers(0, T, (NV, K)).astype(np.int32)
    vw = rng.random((NV, K)).astype(np.float32)
    vw /= vw.sum(-1, keepdims=True)
    return dict(n_ls=n_ls, tables=tables, dec_w=[w for w, _ in dec], dec_b=[b for _, b in dec], vi=vi, vw=vw, vstride=vstride, NV=NV, T=T, K=K)


def encode_oracle(xy, m, source, tables=None):
    """enc (P, L F) of the oracle for the spatial hash or the vertex table of model m"""
    n_ls = m["n_ls"]
    tables = m["tables"] if tables is None else tables
    _scaled, grid = orc.scale_to_grid(xy, n_ls)
    g = grid.astype(np.int32)
    if source == "hash":
        feats = orc.encoding_forward(tables, orc.spatial_hash(g, tables.shape[1]))
    else:
        vid = g[:, 1].astype(np.int64) * m["vstride"] + g[:, 0]                      # (P,L,4)
        feats = orc.encoding_forward(tables, m["vi"][vid].astype(np.int64), m["vw"][vid], blend=None)
    return orc.bilinear_forward(xy, n_ls, feats)


def lattice(rows, cols, origin, denom):
    from collision_handling_in_instantngp_amd import train
    return train.lattice_coordinates(rows, cols, denom, origin)


def render_table():
    out = []
    for src in ("hash", "vertex_table"):
        for (rows, cols) in REN_LATTICES:
            for oi, o in enumerate((1, 3, 4)):
                for outs in ("rgb", "img", "both"):
                    out.append((f"{src}_{rows}x{cols}_out{o}_{outs}", dict(source=src, rows=rows, cols=cols, out_dim=o, outs=outs)))
    return out


def check_render_outputs(rgb, img, want, what):
    """tests/test_gpu_render.py: rgb at RTOL, ATOL = 2e-5, 2e-6; image = (rgb * 255).int() of the same launch exactly, and within 1
    of the oracle's integer"""
    if rgb is not None:
        covered(rgb, "rgb")
        close(rgb, want, 2e-5, 2e-6, what)
    if img is not None:
        covered(img, "img")
        if rgb is not None:
            assert bool((img == (rgb * 255).int()).all()), f"{what}: image is not (rgb * 255).int() of the launch's own rgb"
        q = np.floor((want.astype(np.float32) * np.float32(255.0)).astype(np.float32)).astype(np.int64)
        assert np.abs(img.cpu().numpy().astype(np.int64) - q).max() <= 1


@cases("gngf_render", render_table())
def run_render(source, rows, cols, out_dim, outs):
    m = render_model(out_dim, source)
    L, F = REN["L"], REN["F"]
    xy = lattice(rows, cols, REN_ORIGIN, REN_DENOM)
    want = orc.decoder_forward(encode_oracle(xy, m, source), m["dec_w"], m["dec_b"], False)
    r = Run()
    tables, n_ls = r.i(m["tables"], "tables"), r.i(m["n_ls"], "n_ls")
    vt = source == "vertex_table"
    vi, vw = (r.i(m["vi"], "vert_idx"), r.i(m["vw"], "vert_w")) if vt else (None, None)
    dec = []
    for i in range(3):
        dec += [r.i(m["dec_w"][i], f"W{i}"), r.i(m["dec_b"][i], f"b{i}")]
    rgb = r.o((rows * cols, out_dim), F32, "rgb") if outs in ("rgb", "both") else None
    img = r.o((rows * cols, out_dim), I32, "img") if outs in ("img", "both") else None
    call("gngf_render", P_(tables), 0, P_(vi), P_(vw), P_(n_ls), *[P_(x) for x in dec], P_(rgb), P_(img), rows, cols, REN_ORIGIN[0],
         REN_ORIGIN[1], REN_DENOM, L, F, m["T"], m["K"] if vt else 0, 1 if vt else 0, m["vstride"] if vt else 0, m["NV"] if vt else 0,
         out_dim, 0)
    r.done()
    check_render_outputs(rgb, img, want, f"render {source} {rows}x{cols}")


def vertex_grid_oracle(m, source, tables=None, Ls=None):
    """G (vtot, F): row goff_l + gy (N_l + 2) + gx = the table row of the spatial hash, or sum_k vert_w tables[l, vert_idx]"""
    tables = m["tables"] if tables is None else tables
    n_ls = m["n_ls"][: (Ls if Ls is not None else len(m["n_ls"]))]
    T = tables.shape[1]
    out = []
    for l, n in enumerate(n_ls):
        side = int(n) + 2
        gy, gx = np.divmod(np.arange(side * side), side)
        if source == "hash":
            g = np.stack([gx, gy], 0).astype(np.int32).reshape(1, 2, 1, -1)
            out.append(tables[l][orc.spatial_hash(g, T)[0, 0]].astype(np.float32))
        else:
            vid = gy * m["vstride"] + gx
            rows = tables[l][m["vi"][vid].astype(np.int64)].astype(np.float32)            # (V,K,F)
            out.append((rows * m["vw"][vid][..., None]).astype(np.float32).sum(1, dtype=np.float32))
    return np.concatenate(out, 0)


@cases("gngf_render_grid", [(f"{rows}x{cols}_out{o}_{outs}", dict(rows=rows, cols=cols, out_dim=o, outs=outs))
                            for (rows, cols) in REN_LATTICES for o in (1, 3, 4) for outs in ("rgb", "img", "both")])
def run_render_grid(rows, cols, out_dim, outs):
    m = render_model(out_dim, "vertex_table")
    L, F = REN["L"], REN["F"]
    xy = lattice(rows, cols, REN_ORIGIN, REN_DENOM)
    want = orc.decoder_forward(encode_oracle(xy, m, "vertex_table"), m["dec_w"], m["dec_b"], False)
    r = Run()
    grid, n_ls = r.i(vertex_grid_oracle(m, "vertex_table"), "grid"), r.i(m["n_ls"], "n_ls")
    dec = []
    for i in range(3):
        dec += [r.i(m["dec_w"][i], f"W{i}"), r.i(m["dec_b"][i], f"b{i}")]
    rgb = r.o((rows * cols, out_dim), F32, "rgb") if outs in ("rgb", "both") else None
    img = r.o((rows * cols, out_dim), I32, "img") if outs in ("img", "both") else None
    call("gngf_render_grid", P_(grid), P_(n_ls), host_i32(m["n_ls"]), *[P_(x) for x in dec], P_(rgb), P_(img), rows, cols, REN_ORIGIN[0],
         REN_ORIGIN[1], REN_DENOM, L, F, out_dim, 0)
    r.done()
    check_render_outputs(rgb, img, want, f"render_grid {rows}x{cols}")


# ================================================================================================ softmax / top-K
SM_U, SM_K = (1, 3, 130), (1, 32, 33, 128)


def sm_grid():
    return [(U, T, K) for K in SM_K for T in sorted({K, 257, 2049}) if T >= K for U in SM_U]


def sm_label(U, T, K):
    return f"U{U}_T{T}_K{K}"


def sm_table():
    return [(sm_label(*s), dict(U=s[0], T=s[1], K=s[2])) for s in sm_grid()]


@functools.lru_cache(maxsize=None)
def sm_rows(U, T, nan=True):
    """logits of one shape, made once (read-only): row 0 a tie group over its first half (ties resolve to the lower index), row 2
    NaN-poisoned (tests/test_gpu_dense.py::test_softmax_topk_vs_oracle)"""
    rng = np.random.default_rng(U * 31 + T)
    z = (rng.standard_normal((U, T)) * 3).astype(np.float32)
    z[0, : T // 2] = z[0, 0]
    if nan and U > 2:
        z[2, T // 3] = np.nan
    z.setflags(write=False)
    return z


def softmax64(z):
    zz = z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(zz - np.max(np.where(np.isnan(zz), -np.inf, zz), -1, keepdims=True))
        sm = e / e.sum(-1, keepdims=True)
    sm[np.isnan(z).any(-1)] = 0.0
    return sm


def logits_order(z, K):
    """tests/test_gpu_dense.py::test_streaming_logits_topk_pbar_vs_numpy: descending logits, ties to the lower index; NaN row: 0..K-1"""
    T = z.shape[1]
    nan_rows = np.isnan(z).any(-1)
    order = np.argsort(-np.where(nan_rows[:, None], -np.arange(T)[None, :].astype(np.float64), z.astype(np.float64)), axis=-1,
                       kind="stable")[:, :K]
    order[nan_rows] = np.arange(K)[None, :]
    return order


def check_rowstat(rs, z):
    """(row max, row sum of exp(z - max); NaN marks a NaN row): maxima exact (tests/test_gpu_wide_topk.py:115), sums at the 1e-5 of
    tests/test_gpu_dense.py::test_logits_gemm_with_epilogue_statistics_equals_the_separate_pass"""
    covered(rs, "rowstat")
    rs = rs.cpu().numpy()
    nan_rows = np.isnan(z).any(-1)
    assert np.isnan(rs[nan_rows, 1]).all() and np.array_equal(rs[~nan_rows, 0], z[~nan_rows].max(-1))
    zz = z[~nan_rows].astype(np.float64)
    close(rs[~nan_rows, 1], np.exp(zz - zz.max(-1, keepdims=True)).sum(-1), 1e-5, 0, "row sums exp(z - max)")


@cases("gngf_softmax_topk", sm_table())
def run_softmax_topk(U, T, K):
    z = sm_rows(U, T)
    for with_rowstat in (1, 0):
        r = Run()
        lp = r.o((U, T), F32, "logits_probs")
        lp.copy_(torch.from_numpy(np.array(z)))
        tv, ti = r.o((U, K), F32, "topk_val"), r.o((U, K), I32, "topk_idx")
        rs = r.o((U, 2), F32, "rowstat") if with_rowstat else None
        call("gngf_softmax_topk", P_(lp), P_(tv), P_(ti), P_(rs), U, T, K)
        r.done()
        covered(tv, "topk_val")
        covered(ti, "topk_idx")
        close(lp, np.nan_to_num(softmax64(z).astype(np.float32)), 2e-5, 1e-12, "softmax probabilities")      # test_softmax_topk_vs_oracle
        wv, wi = orc.topk_desc(lp.cpu().numpy(), K)            # selection on the GPU's own fp32 probabilities: exact (same test)
        assert np.array_equal(ti.cpu().numpy().astype(np.int64), wi) and np.array_equal(tv.cpu().numpy(), wv)
        if with_rowstat:
            check_rowstat(rs, z)


@cases("gngf_logits_topk_pbar", sm_table())
def run_logits_topk_pbar(U, T, K):
    """pbar (L,T) is accumulated into (starts at 0); L = 0: no p-bar pass at all"""
    z = sm_rows(U, T)
    sm = softmax64(z)
    order = logits_order(z, K)
    for Lv in (5, 0):
        r = Run()
        zt = r.i(z, "logits")
        tv, ti, rs = r.o((U, K), F32, "topk_val"), r.o((U, K), I32, "topk_idx"), r.o((U, 2), F32, "rowstat")
        mw = np.random.default_rng(K).random((U, max(Lv, 1))).astype(np.float32)
        mt = r.i(mw, "mw") if Lv else None
        pbar = r.o((Lv, T), F32, "pbar", fill=0) if Lv else None
        call("gngf_logits_topk_pbar", P_(zt), P_(tv), P_(ti), P_(rs), P_(mt), Lv, P_(pbar), U, T, K)
        r.done()
        covered(tv, "topk_val")
        covered(ti, "topk_idx")
        assert np.array_equal(ti.cpu().numpy().astype(np.int64), order)
        close(tv, np.take_along_axis(sm, order, -1), 3e-5, 1e-12, "streaming top-K probabilities")      # test_streaming_logits_topk_pbar_vs_numpy
        check_rowstat(rs, z)
        if Lv:
            close(pbar, mw.astype(np.float64).T @ sm, 1e-4, 1e-9, "p-bar")                              # same test


@cases("gngf_topk", sm_table())
def run_topk(U, T, K):
    x = sm_rows(U, T, nan=False)
    r = Run()
    xt = r.i(x, "x")
    tv, ti = r.o((U, K), F32, "topk_val"), r.o((U, K), I32, "topk_idx")
    call("gngf_topk", P_(xt), P_(tv), P_(ti), U, T, K)
    r.done()
    covered(tv, "topk_val")
    covered(ti, "topk_idx")
    wv, wi = orc.topk_desc(x, K)                                # tests/test_gpu_wide_topk.py::test_differentiable_topk_wide_vs_oracle: exact
    assert np.array_equal(ti.cpu().numpy().astype(np.int64), wi) and np.array_equal(tv.cpu().numpy(), wv)


def rowparts_of(z):
    """(U, T / 64) pairs (max, sum exp(z - max)) per 64-column block, as gngf_linear_fwd_rowstats leaves them"""
    b = z.astype(np.float64).reshape(z.shape[0], -1, 64)
    mx = b.max(-1)
    return np.stack([mx, np.exp(b - mx[..., None]).sum(-1)], -1).astype(np.float32)


@cases("gngf_rowstats_topk", sm_table() + [(sm_label(*s), dict(U=s[0], T=s[1], K=s[2]))
                                           for s in [(U, T, K) for (T, K) in ((64, 1), (128, 2), (2048, 32), (2112, 33)) for U in SM_U]])
def run_rowstats_topk(U, T, K):
    """takes T % 64 == 0, K <= 32 and K * 64 <= T only (the K largest logits lie inside the K blocks with the largest maxima): every
    other shape — all of the common grid — is rejected and must not write.  Accepted shapes: against gngf_logits_topk_pbar on the same
    logits, as tests/test_gpu_dense.py::test_logits_gemm_with_epilogue_statistics_equals_the_separate_pass holds it."""
    ok = T % 64 == 0 and K <= 32 and K * 64 <= T
    z = sm_rows(U, T, nan=False) if ok else sm_rows(U, T)
    r = Run()
    zt = r.i(z, "logits")
    parts = r.i(rowparts_of(z) if ok else np.zeros((U, max(T // 64, 1), 2), np.float32), "rowparts")
    tv, ti, rs = r.o((U, K), F32, "topk_val"), r.o((U, K), I32, "topk_idx"), r.o((U, 2), F32, "rowstat")
    args = (P_(zt), P_(parts), P_(tv), P_(ti), P_(rs), U, T, K)
    if not ok:
        with pytest.raises(RuntimeError, match="rejected arguments"):
            call("gngf_rowstats_topk", *args)
        r.done()
        for t_, n in ((tv, "topk_val"), (ti, "topk_idx"), (rs, "rowstat")):
            never_written(t_, f"{n} of a rejected call")
        return
    call("gngf_rowstats_topk", *args)
    tv0, ti0, rs0 = torch.empty((U, K), device=DEV), torch.empty((U, K), dtype=I32, device=DEV), torch.empty((U, 2), device=DEV)
    call("gngf_logits_topk_pbar", P_(zt), P_(tv0), P_(ti0), P_(rs0), P_(None), 0, P_(None), U, T, K)
    r.done()
    for t_, n in ((tv, "topk_val"), (ti, "topk_idx"), (rs, "rowstat")):
        covered(t_, n)
    assert torch.equal(ti, ti0)
    close(rs[:, 0], rs0[:, 0], 0, 0, "row maxima from the partials")
    close(rs[:, 1], rs0[:, 1], 1e-5, 0, "row sums from the partials")
    close(tv, tv0, 1e-5, 1e-12, "top-K probabilities from the partials")
    assert np.array_equal(ti.cpu().numpy().astype(np.int64), logits_order(z, K))


@cases("gngf_pbar_accumulate", [(f"U{U}_T{T}_L{L}", dict(U=U, T=T, L=L)) for T in (1, 257, 2049, 2048) for U in SM_U for L in (1, 5, 16)])
def run_pbar_accumulate(U, T, L):
    """pbar (L,T) += mw^T softmax(logits), from the row statistics (max, sum); starts at 0.  T % 32 == 0 with more than 4 levels takes
    the MFMA form."""
    z = sm_rows(U, T)
    sm = softmax64(z)
    mw = np.random.default_rng(L).random((U, L)).astype(np.float32)
    z0 = torch.from_numpy(np.array(z)).to(DEV)              # the statistics as the forward leaves them (unguarded launch)
    tv0, ti0, rowstat = torch.empty((U, 1), device=DEV), torch.empty((U, 1), dtype=I32, device=DEV), torch.empty((U, 2), device=DEV)
    call("gngf_logits_topk_pbar", P_(z0), P_(tv0), P_(ti0), P_(rowstat), P_(None), 0, P_(None), U, T, 1)
    torch.cuda.synchronize()
    r = Run()
    zt, rs, mt = r.i(z, "logits"), r.i(rowstat, "rowstat"), r.i(mw, "mw")
    pbar = r.o((L, T), F32, "pbar", fill=0)
    call("gngf_pbar_accumulate", P_(zt), P_(rs), P_(mt), L, P_(pbar), U, T)
    r.done()
    close(pbar, mw.astype(np.float64).T @ sm, 1e-4, 1e-9, "p-bar from the statistics")       # test_streaming_logits_topk_pbar_vs_numpy: p-bar


@cases("gngf_softmax_bwd", sm_table())
def run_softmax_bwd(U, T, K):
    """dlogits = p .* (g - <p, g>), g = gdense + mw G + dq at topk_idx (tests/test_gpu_dense.py::test_softmax_bwd_dense_and_topk_gradients);
    with every term, and with the top-K term alone"""
    rng = np.random.default_rng(U + T + K)
    p = softmax64(sm_rows(U, T, nan=False) / 3 * 2).astype(np.float32)
    _wv, wi = orc.topk_desc(p, K)
    # THIS FILE'S OWN choice of inputs (the cited test draws gradients of magnitude 1, and at that magnitude the kernel misses the
    # cited absolute part at T = K = 1 by one ulp of g: 1.2e-7 against 1e-7).  Upstream gradients of magnitude 0.1: the absolute part
    # of the cited bound (1e-7, set at T = 500 for probabilities of ~1e-2
    # times gradients of ~1) then still lies above an fp32 ulp of g where a row is ONE probability of 1 (T = K = 1: d logits = 0
    # exactly, and the kernel's p (g - <p, g>) is the rounding of g)
    gp, gq = (0.1 * rng.standard_normal((U, T))).astype(np.float32), (0.1 * rng.standard_normal((U, K))).astype(np.float32)
    L = 3
    mw, G = rng.random((U, L)).astype(np.float32), (0.1 * rng.standard_normal((L, T))).astype(np.float32)
    for full in (1, 0):
        g = (gp.astype(np.float64) + mw.astype(np.float64) @ G) if full else np.zeros((U, T))
        np.put_along_axis(g, wi, np.take_along_axis(g, wi, -1) + gq, -1)
        p64 = p.astype(np.float64)
        want = p64 * (g - (g * p64).sum(-1, keepdims=True))
        r = Run()
        pt, dq, ti = r.i(p, "probs"), r.i(gq, "dq"), r.i(wi.astype(np.int32), "topk_idx")
        gd, mt, Gt = (r.i(gp, "gdense"), r.i(mw, "mw"), r.i(G, "G")) if full else (None, None, None)
        dz = r.o((U, T), F32, "dlogits")
        call("gngf_softmax_bwd", P_(pt), P_(dq), P_(ti), P_(gd), P_(mt), P_(Gt), L if full else 0, P_(dz), U, T, K)
        r.done()
        covered(dz, "dlogits")
        close(dz, want, 1e-4, 1e-7, "softmax backward")


@cases("gngf_softmax_bwd_lowrank", sm_table())
def run_softmax_bwd_lowrank(U, T, K):
    """in place (logits in, d logits out), db (T) accumulated from 0, scratch of U + U K floats
    (tests/test_gpu_dense.py::test_softmax_bwd_lowrank_from_logits_vs_numpy, saved top-K probabilities given and not)"""
    rng = np.random.default_rng(U + T)
    z = np.array(sm_rows(U, T, nan=False)) / 3 * 2
    Lv = 5
    fwd = torch.from_numpy(z).to(DEV)
    tvb, tib, rowstat = torch.empty((U, K), device=DEV), torch.empty((U, K), dtype=I32, device=DEV), torch.empty((U, 2), device=DEV)
    call("gngf_softmax_topk", P_(fwd), P_(tvb), P_(tib), P_(rowstat), U, T, K)
    torch.cuda.synchronize()
    p = fwd.cpu().numpy().astype(np.float64)
    mw, G = rng.random((U, Lv)).astype(np.float32), rng.standard_normal((Lv, T)).astype(np.float32)
    dq = rng.standard_normal((U, K)).astype(np.float32)
    g = mw.astype(np.float64) @ G.astype(np.float64)
    tin = tib.cpu().numpy().astype(np.int64)
    np.put_along_axis(g, tin, np.take_along_axis(g, tin, -1) + dq, -1)
    want = p * (g - (g * p).sum(-1, keepdims=True))
    scale = np.abs(want).max()
    atol, atol_db = 2e-6 * scale, 2e-5 * scale
    if T == 1:
        # THIS FILE'S OWN bound, not the cited test's, for T = 1 only.
        # one probability of 1 per row: d logits is identically 0, `scale` with it, and the cited bound asks for exact zeros.  The
        # kernel forms g = mw G + dq and <p, g> separately in fp32, so p (g - <p, g>) is the difference of two roundings of g:
        # at most 2 ulp of g, 2 * 2^-23 max |g| (measured: 6.0e-8 .. 2.4e-7 at max |g| ~ 3); db sums U of them.
        atol = 2 * 2.0 ** -23 * float(np.abs(g).max())
        atol_db = U * atol
    for saved_p in (1, 0):
        r = Run()
        logits = r.o((U, T), F32, "logits_dz")
        logits.copy_(torch.from_numpy(z))
        rs, dqt, tit = r.i(rowstat, "rowstat"), r.i(dq, "dq"), r.i(tib, "topk_idx")
        mt, Gt = r.i(mw, "mw"), r.i(G, "G")
        tp = r.i(tvb, "topk_p") if saved_p else None
        db = r.o((T,), F32, "db", fill=0)
        scratch = r.o((U + U * K,), F32, "scratch")
        call("gngf_softmax_bwd_lowrank", P_(logits), P_(rs), P_(dqt), P_(tit), P_(mt), P_(Gt), Lv, P_(db), P_(scratch), P_(tp), U, T, K)
        r.done()
        close(logits, want, 2e-4, atol, "low-rank softmax backward")
        close(db, want.sum(0), 2e-4, atol_db, "low-rank softmax backward, bias")


BLEND_FLAGS = {0: True, 1: None, 2: False}          # GNGF_BLEND_SOFTMAX / _RAW / _NORM -> the oracle's flag


def blend_table():
    return [(f"U{U}_K{K}", dict(U=U, K=K)) for K in SM_K for U in SM_U]


@cases("gngf_blend_fwd", blend_table())
def run_blend_fwd(U, K):
    rng = np.random.default_rng(17 + U + K)
    q = rng.random((U, K)).astype(np.float32) * 0.5 + 1e-3
    for code, flag in BLEND_FLAGS.items():
        r = Run()
        qt = r.i(q, "q")
        w = r.o((U, K), F32, "w")
        call("gngf_blend_fwd", P_(qt), P_(w), U, K, code)
        r.done()
        covered(w, "w")
        close(w, orc.blend_weights(q, flag), 2e-6, 1e-9, f"blend fwd code {code}")      # tests/test_gpu_wide_topk.py::test_blend_kernels_wide_all_codes_vs_oracle


@cases("gngf_blend_bwd", blend_table())
def run_blend_bwd(U, K):
    rng = np.random.default_rng(17 + U + K)
    q = rng.random((U, K)).astype(np.float32) * 0.5 + 1e-3
    d = rng.standard_normal((U, K)).astype(np.float32)
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    for code, flag in BLEND_FLAGS.items():
        if flag is None:
            want = d64
        elif flag:
            w64 = np.exp(q64 - q64.max(-1, keepdims=True))
            w64 /= w64.sum(-1, keepdims=True)
            want = w64 * (d64 - (w64 * d64).sum(-1, keepdims=True))
        else:
            s = q64.sum(-1, keepdims=True)
            want = d64 / s - (d64 * q64).sum(-1, keepdims=True) / (s * s)
        scale = float(np.abs(d64 / (q64.sum(-1, keepdims=True) if flag is False else 1.0)).max())
        r = Run()
        qt, dt = r.i(q, "q"), r.i(d, "dw")
        dq = r.o((U, K), F32, "dq")
        call("gngf_blend_bwd", P_(qt), P_(dt), P_(dq), U, K, code)
        r.done()
        covered(dq, "dq")
        close(dq, want, 2e-5, 2e-6 * scale, f"blend bwd code {code}")                    # same test


# ================================================================================================ HPD backward in the GEMM loaders
HPD_SHAPES = [(128, 128, 0, 0), (128, 256, 16, 4)]
HPD_U0, HPD_EXTRA, HPD_HID = 128, 256, 128            # the chunk starts at row 128 of rows_total = U + 256 prepared rows


def hpd_table():
    return [(f"U{U}_T{T}_L{L}_K{K}_planes{pl}", dict(U=U, T=T, L=L, K=K, planes=pl)) for (U, T, L, K) in HPD_SHAPES for pl in (3, 2)]


@functools.lru_cache(maxsize=None)
def hpd_case(U, T, L, K):
    """tests/test_gpu_dense.py::test_softmax_backward_formed_in_the_gemm_loaders: inputs and float64 algebra"""
    rng = np.random.default_rng(U + T + L + K)
    Hd = HPD_HID
    z = (rng.standard_normal((U, T)) * 4).astype(np.float32)
    h = np.maximum(rng.standard_normal((U, Hd)) * 30, 0).astype(np.float32)
    W = ((rng.random((T, Hd)) * 2 - 1) / Hd ** 0.5).astype(np.float32)
    mw = (rng.random((U, max(L, 1))) / (4 * U)).astype(np.float32)
    G = (rng.standard_normal((max(L, 1), T)) * 3).astype(np.float32)
    zd = z.astype(np.float64)
    m = zd.max(1, keepdims=True)
    ssum = np.exp(zd - m).sum(1, keepdims=True)
    p = np.exp(zd - m) / ssum
    rowstat = np.concatenate([m, ssum], 1).astype(np.float32)
    g = (mw.astype(np.float64) @ G.astype(np.float64)) if L else np.zeros_like(zd)
    ti = pk = dq = None
    if K:
        ti = np.argsort(-p, axis=1, kind="stable")[:, :K]
        pk = np.take_along_axis(p, ti, 1).astype(np.float32)
        dq = rng.standard_normal((U, K)).astype(np.float32) * 1e-3
        np.add.at(g, (np.arange(U)[:, None], ti), dq.astype(np.float64))
    dot = (p * g).sum(1, keepdims=True)
    dz = p * (g - dot)
    rows_total = U + HPD_EXTRA
    h_all = np.concatenate([np.full((HPD_U0, Hd), 7.0, np.float32), h, np.full((rows_total - U - HPD_U0, Hd), -3.0, np.float32)])
    mw_all = np.concatenate([np.ones((HPD_U0, max(L, 1)), np.float32), mw, np.ones((rows_total - U - HPD_U0, max(L, 1)), np.float32)])
    return dict(z=z, h=h, W=W, mw=mw, G=G, rowstat=rowstat, ti=None if ti is None else ti.astype(np.int32), pk=pk, dq=dq, dot=dot[:, 0],
                dW=dz.T @ h.astype(np.float64), db=dz.sum(0), dH=dz @ W.astype(np.float64), h_all=h_all, mw_all=mw_all, rows_total=rows_total)


@cases("gngf_hpd_bwd_dot", [(f"U{U}_T{T}_L{L}_K{K}", dict(U=U, T=T, L=L, K=K)) for (U, T, L, K) in HPD_SHAPES])
def run_hpd_bwd_dot(U, T, L, K):
    d = hpd_case(U, T, L, K)
    r = Run()
    z, rs = r.i(d["z"], "logits"), r.i(d["rowstat"], "rowstat")
    dq, pk = (r.i(d["dq"], "dq"), r.i(d["pk"], "topk_p")) if K else (None, None)
    mw, G = (r.i(d["mw"], "mw"), r.i(d["G"], "G")) if L else (None, None)
    dot = r.o((U,), F32, "dot")
    call("gngf_hpd_bwd_dot", P_(z), P_(rs), P_(dq), P_(pk), P_(mw), P_(G), L, P_(dot), U, T, K)
    r.done()
    covered(dot, "dot")
    close(dot, d["dot"], 2e-5, 1e-9, "row dots")                # test_softmax_backward_formed_in_the_gemm_loaders


def planes_sum(t):
    """(planes, rows, cols) int16 holding bf16 bit patterns -> the fp64 sum of the planes"""
    return t.view(torch.bfloat16).float().double().sum(dim=0)


@cases("gngf_hpd_bwd_prepare", hpd_table())
def run_hpd_bwd_prepare(U, T, L, K, planes):
    """hp (planes, rows, 128) and Wp (planes, T, 128), mwp (3, rows, 16) and Gtp (3, T, 16; transposed), each a split of an fp32
    operand into bf16 terms: three planes add up to the fp32 value exactly (same test), columns L..15 are zero padding (L = 0: all
    sixteen, mw / G NULL).  Either half
    alone (h == NULL / W == NULL) leaves the other half's outputs unwritten."""
    d = hpd_case(U, T, L, K)
    rows, Hd = d["rows_total"], HPD_HID
    for half in ("both", "h", "W"):
        r = Run()
        h = r.i(d["h_all"], "h") if half != "W" else None
        mw = r.i(d["mw_all"], "mw") if (L and half != "W") else None
        W = r.i(d["W"], "W") if half != "h" else None
        G = r.i(d["G"], "G") if (L and half != "h") else None
        hp, mwp = r.o((planes, rows, Hd), torch.int16, "hp"), r.o((3, rows, 16), torch.int16, "mwp")
        Wp, Gtp = r.o((planes, T, Hd), torch.int16, "Wp"), r.o((3, T, 16), torch.int16, "Gtp")
        call("gngf_hpd_bwd_prepare", P_(h), P_(mw), rows, P_(hp), P_(mwp), P_(W), P_(G), T, P_(Wp), P_(Gtp), L, Hd, planes)
        r.done()
        if half != "W":
            covered(hp, "hp")
            if planes == 3:
                assert torch.equal(planes_sum(hp).float(), h)
            if L:
                covered(mwp, "mwp")
                assert torch.equal(planes_sum(mwp)[:, :L].float(), mw) and float(planes_sum(mwp)[:, L:].abs().max() if L < 16 else 0) == 0
            else:
                all_zero(mwp, "mwp at L = 0: sixteen columns of zero padding")
        else:
            never_written(hp, "hp without h")
            never_written(mwp, "mwp without h")
        if half != "h":
            covered(Wp, "Wp")
            if planes == 3:
                assert torch.equal(planes_sum(Wp).float(), W)
            if L:
                covered(Gtp, "Gtp")
                assert torch.equal(planes_sum(Gtp)[:, :L].float(), G.T.contiguous())
            else:
                all_zero(Gtp, "Gtp at L = 0: sixteen columns of zero padding")
        else:
            never_written(Wp, "Wp without W")
            never_written(Gtp, "Gtp without W")


@cases("gngf_hpd_bwd_fused", hpd_table())
def run_hpd_bwd_fused(U, T, L, K, planes):
    """dW (T,128), db (T) and dH accumulate from 0.  hp / mwp are handed over at the chunk's first row of rows_total prepared rows
    and dH at the chunk's rows of a (rows_total, 128) buffer: the rows outside the chunk keep their bytes.  Values: float64, at most
    max(2e-5, 4 x the error of the three separate entry points) of the largest element (same test)."""
    d = hpd_case(U, T, L, K)
    rows, Hd, u0 = d["rows_total"], HPD_HID, HPD_U0
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # the operands split once, unguarded (gngf_hpd_bwd_prepare has its own cases), then copied into the arena
    hp0, mwp0 = torch.zeros((planes, rows, Hd), dtype=torch.int16, device=DEV), torch.zeros((3, rows, 16), dtype=torch.int16, device=DEV)
    Wp0, Gtp0 = torch.zeros((planes, T, Hd), dtype=torch.int16, device=DEV), torch.zeros((3, T, 16), dtype=torch.int16, device=DEV)
    ha, ma, Wd, Gd = dev(d["h_all"]), dev(d["mw_all"]) if L else None, dev(d["W"]), dev(d["G"]) if L else None
    call("gngf_hpd_bwd_prepare", P_(ha), P_(ma), rows, P_(hp0), P_(mwp0), P_(Wd), P_(Gd), T, P_(Wp0), P_(Gtp0), L, Hd, planes)
    torch.cuda.synchronize()
    r = Run()
    z, rs, dot = r.i(d["z"], "logits"), r.i(d["rowstat"], "rowstat"), r.i(d["dot"].astype(np.float32), "dot")
    dq, pk, ti = (r.i(d["dq"], "dq"), r.i(d["pk"], "topk_p"), r.i(d["ti"], "topk_idx")) if K else (None, None, None)
    hp, mwp, Wp, Gtp = r.i(hp0, "hp"), r.i(mwp0, "mwp"), r.i(Wp0, "Wp"), r.i(Gtp0, "Gtp")
    h, W = r.i(d["h"], "h"), r.i(d["W"], "W")
    dW, db = r.o((T, Hd), F32, "dW", fill=0), r.o((T,), F32, "db", fill=0)
    dH_all = r.o((rows, Hd), F32, "dH")
    dH_all[u0:u0 + U].zero_()
    r.freeze(dH_all[:u0], "dH rows in front of the chunk")
    r.freeze(dH_all[u0 + U:], "dH rows behind the chunk")
    _P = ctypes.c_void_p
    call("gngf_hpd_bwd_fused", P_(z), P_(rs), P_(dot), P_(dq), P_(pk), P_(ti), _P(hp.data_ptr() + 2 * u0 * Hd), _P(mwp.data_ptr() + 2 * u0 * 16),
         rows, P_(Wp), P_(Gtp), P_(h), P_(W), P_(dW), P_(db), _P(dH_all.data_ptr() + 4 * u0 * Hd), U, T, K, Hd, planes)
    # the three entry points it replaces, unguarded: the yardstick of the bound
    dz1 = dev(d["z"])
    scratch = torch.empty((U * (1 + max(K, 1)),), device=DEV)
    dW1, db1, dH1 = torch.zeros((T, Hd), device=DEV), torch.zeros((T,), device=DEV), torch.zeros((U, Hd), device=DEV)
    call("gngf_softmax_bwd_lowrank", P_(dz1), P_(rs), P_(dq), P_(ti), P_(ma[u0:u0 + U].contiguous() if L else None), P_(Gd), L, P_(db1),
         P_(scratch), P_(pk), U, T, K)
    hd = dev(d["h"])
    call("gngf_linear_bwd_weight", P_(dz1), P_(None), P_(hd), P_(dW1), P_(None), U, T, Hd, 0, 0)
    call("gngf_gemm_acc", P_(dz1), P_(Wd), P_(dH1), U, Hd, T, 0, 0, 0)
    r.done()

    def rel(a, ref):
        err, top = np.abs(a.cpu().numpy().astype(np.float64) - ref).max(), np.abs(ref).max()
        return float(err) if top == 0 else float(err / top)        # (L = 0 and K = 0: every gradient is exactly zero)
    e = {"dW": rel(dW, d["dW"]), "db": rel(db, d["db"]), "dH": rel(dH_all[u0:u0 + U], d["dH"])}
    e1 = {"dW": rel(dW1, d["dW"]), "db": rel(db1, d["db"]), "dH": rel(dH1, d["dH"])}
    for k in e:
        assert e[k] <= (max(2e-5, 4 * e1[k]) if (L or K) else 0.0), (k, e, e1)


# ================================================================================================ per-vertex helpers
VTX_L = 4


def vtx_levels():
    return orc.level_resolutions(8, 32, VTX_L)


def vtx_xy(P, one_tile=False, seed=0):
    """P coordinates in [0,1]^2: random (all inside one tile when asked), with the lattice edges 0.0 and 1.0 from three pixels on"""
    rng = np.random.default_rng(1000 * seed + P)
    xy = rng.random((P, 2)).astype(np.float32)
    if one_tile:
        xy = (xy * np.float32(0.2) + np.float32(0.3)).astype(np.float32)
    elif P >= 3:
        xy[0], xy[1], xy[2] = (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)
        if P > 8:
            xy[3:6, 0], xy[6:8, 1] = 1.0, 0.0
    return xy


def vtx_ids(xy, n_ls, vstride):
    """vid (P,L,4) = gy * vstride + gx of the four corners, corner order v = dx + 2 dy"""
    _s, grid = orc.scale_to_grid(xy, n_ls)
    g = grid.astype(np.int64)
    return g[:, 1] * vstride + g[:, 0]


@cases("gngf_vertex_coords", [(f"u{u0}_count{n}", dict(u0=u0, count=n)) for u0, n in ((0, 1), (5, 3), (7, 1025))])
def run_vertex_coords(u0, count, vstride=34):
    r = Run()
    v = r.o((count, 2), F32, "verts")
    call("gngf_vertex_coords", P_(v), u0, count, vstride)
    r.done()
    covered(v, "verts")
    u = np.arange(u0, u0 + count)
    assert np.array_equal(v.cpu().numpy(), np.stack([u % vstride, u // vstride], 1).astype(np.float32))     # exact integers


@cases("gngf_vertex_multiplicity", [(f"P{P}", dict(P=P)) for P in (1, 1025, 3001)])
def run_vertex_multiplicity(P):
    """counts (L,NV) += instances (starts at 0); exact"""
    n_ls = vtx_levels()
    vstride = int(n_ls.max()) + 2
    NV = vstride * vstride
    xy = vtx_xy(P)
    r = Run()
    xt, nt = r.i(xy, "xy"), r.i(n_ls, "n_ls")
    counts = r.o((VTX_L, NV), I32, "counts", fill=0)
    call("gngf_vertex_multiplicity", P_(xt), P_(nt), P_(counts), P, VTX_L, vstride, NV)
    r.done()
    want = np.zeros((VTX_L, NV), np.int32)
    vid = vtx_ids(xy, n_ls, vstride)
    for l in range(VTX_L):
        np.add.at(want[l], vid[:, l].reshape(-1), 1)
    assert np.array_equal(counts.cpu().numpy(), want)


@cases("gngf_multiplicity_weights", [(f"NV{NV}_L{L}", dict(NV=NV, L=L)) for NV, L in ((1, 1), (1156, 4), (1157, 3))])
def run_multiplicity_weights(NV, L):
    """mw (NV,L) = counts (L,NV) / denom: one fp32 division, exact"""
    counts = np.random.default_rng(NV).integers(0, 50, (L, NV)).astype(np.int32)
    r = Run()
    ct = r.i(counts, "counts")
    mw = r.o((NV, L), F32, "mw")
    call("gngf_multiplicity_weights", P_(ct), P_(mw), NV, L, 12.0)
    r.done()
    covered(mw, "mw")
    assert np.array_equal(mw.cpu().numpy(), (counts.T.astype(np.float32) / np.float32(12.0)).astype(np.float32))


@cases("gngf_expand_vertex_table", [(f"P{P}_K{K}_{outs}", dict(P=P, K=K, outs=outs)) for P in (1, 1025, 3001)
                                    for K, outs in ((4, "all"), (4, "idx"), (4, "vid_idx"), (3, "all"), (33, "val"), (0, "vid"))])
def run_expand_vertex_table(P, K, outs):
    """vid_out (P,L,4) int64, out_idx (P,L,4,K) int64, out_val (P,L,4,K) fp32, any of them NULL: gathers, exact (K = 4 with
    indices alone takes a vector kernel)"""
    n_ls = vtx_levels()
    vstride = int(n_ls.max()) + 2
    NV = vstride * vstride
    rng = np.random.default_rng(P + K)
    xy = vtx_xy(P)
    si, sv = rng.integers(0, 1000, (NV, max(K, 1))).astype(np.int32), rng.random((NV, max(K, 1))).astype(np.float32)
    want_vid, want_idx, want_val = {"all": (1, 1, 1), "idx": (0, 1, 0), "vid_idx": (1, 1, 0), "val": (0, 0, 1), "vid": (1, 0, 0)}[outs]
    r = Run()
    xt, nt = r.i(xy, "xy"), r.i(n_ls, "n_ls")
    sit = r.i(si, "src_idx") if want_idx else None
    svt = r.i(sv, "src_val") if want_val else None
    vo = r.o((P, VTX_L, 4), I64, "vid_out") if want_vid else None
    oi = r.o((P, VTX_L, 4, K), I64, "out_idx") if want_idx else None
    ov = r.o((P, VTX_L, 4, K), F32, "out_val") if want_val else None
    call("gngf_expand_vertex_table", P_(xt), P_(nt), P_(sit), P_(svt), P_(vo), P_(oi), P_(ov), P, VTX_L, K, vstride, NV)
    r.done()
    vid = vtx_ids(xy, n_ls, vstride)
    if want_vid:
        covered(vo, "vid_out")
        assert np.array_equal(vo.cpu().numpy(), vid)
    if want_idx:
        covered(oi, "out_idx")
        assert np.array_equal(oi.cpu().numpy(), si[vid].astype(np.int64))
    if want_val:
        covered(ov, "out_val")
        assert np.array_equal(ov.cpu().numpy(), sv[vid])


# ================================================================================================ encoder
ENC_L, ENC_LS, ENC_K = 4, 3, 4            # levels 8..32; the tiled form stages levels [0, 3), level 3 is somebody else's
ENC_CFGS = {"F2_f32": (2, 0, 1024), "F1_f32": (1, 0, 1000), "F4_f32": (4, 0, 1000), "F2_f16": (2, 1, 1024),     # F, feat_dtype, T
            "F4_f16": (4, 1, 1000)}                                  # (the module-boundary kernels only)
ENC_P = {"P1": (1, False), "P1025_one_tile": (1025, True), "P3001_edges": (3001, False)}
ENC_CHUNK = 1024                          # a tile of 1025 pixels splits into two work items


def enc_levels():
    return orc.level_resolutions(8, 32, ENC_L)


@functools.lru_cache(maxsize=None)
def enc_model(cfg):
    """tables (L,T,F) as the kernels see them (fp16 storage: rounded), a K = 4 vertex table, everything read-only"""
    F, half, T = ENC_CFGS[cfg]
    rng = np.random.default_rng(40 + F + half)
    n_ls = enc_levels()
    raw = (rng.random((ENC_L, T, F), dtype=np.float32) - 0.5) * (2e-2 if half else 2e-4)
    stored = raw.astype(np.float16) if half else raw
    vstride = int(n_ls.max()) + 2
    NV = vstride * vstride
    vi = rng.integers(0, T, (NV, ENC_K)).astype(np.int32)
    vw = rng.random((NV, ENC_K), dtype=np.float32)
    m = dict(F=F, half=half, T=T, n_ls=n_ls, stored=stored, tables=stored.astype(np.float32), vi=vi, vw=vw, vstride=vstride, NV=NV, K=ENC_K)
    for v in (stored, m["tables"], vi, vw):
        v.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def enc_batch(pname, cfg):
    """coordinates, upstream gradient and every oracle quantity of one (batch, model): computed once, read-only"""
    P, one_tile = ENC_P[pname]
    m = enc_model(cfg)
    F, T, n_ls = m["F"], m["T"], m["n_ls"]
    xy = vtx_xy(P, one_tile, seed=3)
    genc = np.random.default_rng(P).standard_normal((P, ENC_L * F)).astype(np.float32)
    _s, grid = orc.scale_to_grid(xy, n_ls)
    g = grid.astype(np.int64)                                          # (P,2,L,4)
    hidx = orc.spatial_hash(grid.astype(np.int32), T)                  # (P,L,4)
    vid = g[:, 1] * m["vstride"] + g[:, 0]
    dfe = orc.bilinear_backward(xy, n_ls, genc, F)                     # (P,F,L,4): the fp32 terms c_v g
    goff = np.concatenate([[0], np.cumsum((n_ls.astype(np.int64) + 2) ** 2)])
    gi = goff[None, :ENC_L, None] + g[:, 1] * (n_ls.astype(np.int64)[None, :, None] + 2) + g[:, 0]       # (P,L,4) vertex-grid rows
    vtot = int(goff[ENC_LS])
    dG = np.zeros((int(goff[ENC_L]), F))
    np.add.at(dG, gi.reshape(-1), dfe.transpose(0, 2, 3, 1).reshape(-1, F).astype(np.float64))
    b = dict(P=P, xy=xy, genc=genc, hidx=hidx, vid=vid, dfe=dfe, gi=gi, vtot=vtot, goff=goff, dG=dG)
    b["enc_hash"] = orc.bilinear_forward(xy, n_ls, orc.encoding_forward(m["tables"], hidx))
    b["enc_vt"] = orc.bilinear_forward(xy, n_ls, orc.encoding_forward(m["tables"], m["vi"][vid].astype(np.int64), m["vw"][vid], None))
    dt_h = np.zeros((ENC_L, T, F))
    lv = np.broadcast_to(np.arange(ENC_L)[None, :, None], hidx.shape)
    np.add.at(dt_h, (lv.reshape(-1), hidx.reshape(-1)), dfe.transpose(0, 2, 3, 1).reshape(-1, F).astype(np.float64))
    b["dt_hash"] = dt_h                                                # (L,T,F) float64: the fp32 terms summed in double
    dt_v, dw_inst = orc.encoding_backward(m["tables"], m["vi"][vid].astype(np.int64), m["vw"][vid], None, dfe)
    dvw = np.zeros((m["NV"], ENC_K))
    np.add.at(dvw, vid.reshape(-1), dw_inst.reshape(-1, ENC_K).astype(np.float64))
    b["dt_vt"], b["dvw"], b["dw_inst"] = dt_v, dvw, dw_inst
    for v in (xy, genc):
        v.setflags(write=False)
    return b


def enc_geo(pname, cfg):
    """the tiled form's geometry for levels [0, 3) from ops.EncodePlan (every level staged whatever the batch size), with the chunk
    held at 1024 and two binning blocks from 3001 pixels on"""
    import types
    from collision_handling_in_instantngp_amd import ops
    P = ENC_P[pname][0]
    F = ENC_CFGS[cfg][0]
    n_host = [int(n) for n in enc_levels()[:ENC_LS]]
    prev = ops.TILED_CELLS_PER_PIXEL
    ops.TILED_CELLS_PER_PIXEL = 1e12
    try:
        plan = ops.EncodePlan(P, n_host, F, "tiled")
    finally:
        ops.TILED_CELLS_PER_PIXEL = prev
    assert plan.Ls == ENC_LS and plan.ntiles == 4
    geo = types.SimpleNamespace(P=P, F=F, Ls=ENC_LS, n_ls_host=n_host, tile_shift=plan.tile_shift, ntiles=plan.ntiles, lds_bytes=plan.lds_bytes,
                                chunk=ENC_CHUNK, NB=2 if P > 3000 else 1, vtot=plan.vtot, n_ls_c=host_i32(n_host))
    geo.max_items = -(-P // geo.chunk) + geo.ntiles
    geo.interleaved = lambda backward: bool(query("gngf_tiled_interleaved_applies", geo.n_ls_c, geo.Ls, F, geo.tile_shift, geo.lds_bytes, int(backward)))
    # F = 2 takes the level-interleaved pixel-stage kernels, F in {1, 4} the generic ones (fp16 tables: the generic fused forward)
    assert geo.interleaved(0) == (F == 2) and geo.interleaved(1) == (F == 2)
    return geo


class Bins:
    """the outputs of one binning job, in the arena"""

    def __init__(self, r, geo, tag=""):
        self.blockhist = r.o((geo.ntiles * (geo.NB + 1),), I32, "blockhist" + tag)
        self.tile_off = r.o((geo.ntiles + 1,), I32, "tile_off" + tag)
        self.tile_item_base = r.o((geo.ntiles + 1,), I32, "tile_item_base" + tag)
        self.items = r.o((geo.max_items, 4), I32, "items" + tag)
        self.n_items = r.o((4,), I32, "n_items" + tag)
        self.sorted = r.o((geo.P, 4), F32, "sorted" + tag)

    def pointers(self):
        return [P_(b) for b in (self.tile_off, self.tile_item_base, self.items, self.n_items, self.sorted)]


def check_bins(bins, xy, geo):
    """tests/test_gpu_binning.py: the counting-sort model, exact.  Of `items` only the first n_items[0] rows are contract-written."""
    from test_gpu_binning import _check, _model
    for t_, n in ((bins.tile_off, "tile_off"), (bins.tile_item_base, "tile_item_base"), (bins.n_items, "n_items"), (bins.sorted, "sorted")):
        covered(t_, n)
    _check(bins, xy, _model(xy, geo.tile_shift, geo.chunk))
    covered(bins.items[: int(bins.n_items[0])], "items[:n_items[0]]")


def binned(r, geo, xy_t):
    """gngf_bin_pixels into arena buffers (a launch of its own in front of the call under test, guarded all the same)"""
    bins = Bins(r, geo)
    call("gngf_bin_pixels", P_(xy_t), geo.P, geo.tile_shift, geo.NB, geo.chunk, P_(bins.blockhist), *bins.pointers())
    return bins


def src_args(r, m, source):
    """(vert_idx, vert_w, K, mode, vstride, NV) of an index source"""
    if source == "hash":
        return None, None, 0, 0, 0, 0
    return r.i(m["vi"], "vert_idx"), r.i(m["vw"], "vert_w"), m["K"], 1, m["vstride"], m["NV"]


def hashed_rows(n_ls, Ls, T):
    """bool (L, T): the rows hash(gx, gy) of every vertex of levels [0, Ls)"""
    out = np.zeros((len(n_ls), T), bool)
    for l in range(Ls):
        side = int(n_ls[l]) + 2
        gy, gx = np.divmod(np.arange(side * side), side)
        g = np.stack([gx, gy], 0).astype(np.int32).reshape(1, 2, 1, -1)
        out[l, orc.spatial_hash(g, T)[0, 0]] = True
    return out


def check_grid(G, m, source, what):
    """the vertex grid against the oracle: the spatial hash is a pure gather (bit-exact, tests/test_gpu_encode.py:48); the vertex
    table a K-term fp32 sum (2e-6 / 1e-9, test_fused_encode_vertex_table_vs_oracle: the same sum, before interpolation)"""
    covered(G, what)
    want = vertex_grid_oracle(m, source, Ls=ENC_LS)
    if source == "hash":
        assert np.array_equal(G.cpu().numpy(), want), what
    else:
        close(G, want, 2e-6, 1e-9, what)


# ---- index and module-boundary kernels
@cases("gngf_hash_indices", [(f"{pn}_T{T}", dict(pname=pn, T=T)) for pn in ENC_P for T in (1000, 1024)])
def run_hash_indices(pname, T):
    P, one_tile = ENC_P[pname]
    xy, n_ls = vtx_xy(P, one_tile, seed=3), enc_levels()
    r = Run()
    xt, nt = r.i(xy, "xy"), r.i(n_ls, "n_ls")
    idx = r.o((P, ENC_L, 4), I64, "idx")
    call("gngf_hash_indices", P_(xt), P_(nt), P_(idx), P, ENC_L, T)
    r.done()
    covered(idx, "idx")
    _s, grid = orc.scale_to_grid(xy, n_ls)
    assert np.array_equal(idx.cpu().numpy(), orc.spatial_hash(grid.astype(np.int32), T))       # test_hash_indices_bit_exact_vs_reference_golden


def mrhe_table():
    return [(f"{cfg}_{pn}_K{K}", dict(cfg=cfg, pname=pn, K=K)) for cfg in ("F2_f32", "F1_f32", "F4_f16") for pn in ("P1", "P3001_edges")
            for K in (0, 4, 33)]



def mrhe_case(cfg, pname, K):
    m = enc_model(cfg)
    P = ENC_P[pname][0]
    rng = np.random.default_rng(P + K)
    idx = rng.integers(0, m["T"], (P, ENC_L, 4, K) if K else (P, ENC_L, 4))
    probs = (rng.random((P, ENC_L, 4, K), dtype=np.float32) * 0.01 + 1e-3) if K else None
    return m, P, idx, probs


@cases("gngf_mrhe_fwd", mrhe_table())
def run_mrhe_fwd(cfg, pname, K):
    """out (P,F,L,4); K = 0: the hash branch (a pure gather, bit-exact); K = 4 / 33: the three blends"""
    m, P, idx, probs = mrhe_case(cfg, pname, K)
    F, T = m["F"], m["T"]
    for code, flag in (BLEND_FLAGS.items() if K else [(0, True)]):
        r = Run(64 if K > 4 else 8)
        tt, it = r.i(m["stored"], "tables"), r.i(idx, "idx")
        pt = r.i(probs, "probs") if K else None
        out = r.o((P, F, ENC_L, 4), F32, "out")
        call("gngf_mrhe_fwd", P_(tt), m["half"], P_(it), P_(pt), P_(out), P, ENC_L, F, T, K, code)
        r.done()
        covered(out, "out")
        want = orc.encoding_forward(m["tables"], idx, probs, flag)
        if not K:
            assert np.array_equal(out.cpu().numpy(), want)                  # test_mrhe_boundary_vs_reference_golden: bit-exact
        else:
            # tests/test_gpu_wide_topk.py::test_mrhe_boundary_wide_vs_oracle: 2e-6 and the recursive-summation bound of a K-term sum
            terms = np.abs(m["tables"][np.arange(ENC_L)[None, :, None, None], idx]) * orc.blend_weights(probs, flag)[..., None]
            close(out, want, 2e-6, 2 * K * 2.0 ** -24 * float(terms.sum(3).max()), f"mrhe fwd blend {code}")


@cases("gngf_mrhe_bwd", mrhe_table())
def run_mrhe_bwd(cfg, pname, K):
    """dtables (L,T,F) fp32 is accumulated into (starts at 0), dprobs (P,L,4,K) is written"""
    m, P, idx, probs = mrhe_case(cfg, pname, K)
    F, T = m["F"], m["T"]
    gout = np.random.default_rng(7).standard_normal((P, F, ENC_L, 4)).astype(np.float32)
    for code, flag in (BLEND_FLAGS.items() if K else [(0, True)]):
        dt, dp = orc.encoding_backward(m["tables"], idx, probs, flag, gout)
        r = Run(64 if K > 4 else 8)
        tt, it, gt = r.i(m["stored"], "tables"), r.i(idx, "idx"), r.i(gout, "gout")
        pt = r.i(probs, "probs") if K else None
        dtab = r.o((ENC_L, T, F), F32, "dtables", fill=0)
        dpr = r.o((P, ENC_L, 4, K), F32, "dprobs") if K else None
        call("gngf_mrhe_bwd", P_(tt), m["half"], P_(it), P_(pt), P_(gt), P_(dtab), P_(dpr), P, ENC_L, F, T, K, code)
        r.done()
        if not K:
            close(dtab, dt, 1e-5, 1e-6, "mrhe bwd d tables (hash)")            # test_mrhe_boundary_vs_reference_golden
        else:
            covered(dpr, "dprobs")
            close(dtab, dt, 1e-4, 1e-6, f"mrhe bwd d tables blend {code}")     # same test
            # d probs: 1e-4 / 2e-7 (2e-5 for the normalising blend) in that test, on fp32 tables of +-1e-4; the fp16 tables here are
            # 100 times larger and the absolute part scales with them (test_mrhe_boundary_fp16_tables_cfg5_feature_width_vs_oracle: 1e-6)
            # (the factor 100 on the normalising blend's absolute part at fp16 tables is THIS FILE'S OWN: no existing test runs it)
            atol = (2e-5 * (100 if m["half"] else 1)) if flag is False else (1e-6 if m["half"] else 2e-7)
            close(dpr, dp, 1e-4, atol, f"mrhe bwd d probs blend {code}")


@cases("gngf_bilinear_fwd", [(f"{cfg}_{pn}", dict(cfg=cfg, pname=pn)) for cfg in ("F2_f32", "F1_f32", "F4_f32") for pn in ENC_P])
def run_bilinear_fwd(cfg, pname):
    F = ENC_CFGS[cfg][0]
    P, one_tile = ENC_P[pname]
    xy, n_ls = vtx_xy(P, one_tile, seed=3), enc_levels()
    feats = np.random.default_rng(P + F).standard_normal((P, F, ENC_L, 4)).astype(np.float32)
    r = Run()
    xt, nt, ft = r.i(xy, "xy"), r.i(n_ls, "n_ls"), r.i(feats, "feats")
    enc = r.o((P, ENC_L * F), F32, "enc")
    call("gngf_bilinear_fwd", P_(xt), P_(nt), P_(ft), P_(enc), P, ENC_L, F)
    r.done()
    covered(enc, "enc")
    close(enc, orc.bilinear_forward(xy, n_ls, feats), 1e-6, 1e-6, "bilinear fwd")          # test_bilinear_vs_reference_golden


@cases("gngf_bilinear_bwd", [(f"{cfg}_{pn}", dict(cfg=cfg, pname=pn)) for cfg in ("F2_f32", "F1_f32", "F4_f32") for pn in ENC_P])
def run_bilinear_bwd(cfg, pname):
    F = ENC_CFGS[cfg][0]
    P, one_tile = ENC_P[pname]
    xy, n_ls = vtx_xy(P, one_tile, seed=3), enc_levels()
    genc = np.random.default_rng(P + F).standard_normal((P, ENC_L * F)).astype(np.float32)
    r = Run()
    xt, nt, gt = r.i(xy, "xy"), r.i(n_ls, "n_ls"), r.i(genc, "genc")
    df = r.o((P, F, ENC_L, 4), F32, "dfeats")
    call("gngf_bilinear_bwd", P_(xt), P_(nt), P_(gt), P_(df), P, ENC_L, F)
    r.done()
    covered(df, "dfeats")
    close(df, orc.bilinear_backward(xy, n_ls, genc, F), 1e-6, 1e-7, "bilinear bwd")        # same test


# ---- direct form
def direct_table():
    return [(f"{cfg}_{src}_{pn}_levels1to3{'_tile_order' if order else ''}", dict(cfg=cfg, source=src, pname=pn, order=order))
            for cfg in ENC_CFGS if cfg != "F4_f16" for src in ("hash", "vt") for pn in ENC_P for order in ((0, 1) if src == "hash" else (0,))]


@cases("gngf_encode_fwd", direct_table())
def run_encode_fwd(cfg, source, pname, order, l0=1, l1=3):
    """levels [1, 3) of 4: the columns of the other levels keep their bytes; pixel_order: walked in binned order, written by
    original index"""
    m, b = enc_model(cfg), enc_batch(pname, cfg)
    F, T, P = m["F"], m["T"], b["P"]
    r = Run()
    xt, tt, nt = r.i(b["xy"], "xy"), r.i(m["stored"], "tables"), r.i(m["n_ls"], "n_ls")
    vi, vw, K, mode, vstride, NV = src_args(r, m, source)
    srt = binned(r, enc_geo(pname, cfg), xt).sorted if order else None
    enc = r.o((P, ENC_L * F), F32, "enc")
    call("gngf_encode_fwd", P_(xt), P_(tt), m["half"], P_(vi), P_(vw), P_(nt), P_(enc), P, ENC_L, F, T, K, mode, vstride, NV, l0, l1, P_(srt))
    r.done()
    covered(enc[:, l0 * F:l1 * F], "enc columns of levels [1, 3)")
    never_written(enc[:, :l0 * F], "enc columns of level 0")
    never_written(enc[:, l1 * F:], "enc columns of level 3")
    want = b["enc_hash" if source == "hash" else "enc_vt"]
    # test_fused_encode_hash_vs_oracle 1e-6 / 1e-9, test_fused_encode_vertex_table_vs_oracle 2e-6 / 1e-9
    close(enc[:, l0 * F:l1 * F], want[:, l0 * F:l1 * F], 1e-6 if source == "hash" else 2e-6, 1e-9, "direct encode fwd")


@cases("gngf_encode_bwd", [c for c in direct_table() if not c[1]["order"]])
def run_encode_bwd(cfg, source, pname, order, l0=1, l1=3):
    """dtables (L,T,F) and dvert_w (NV,K) are accumulated into: levels [1, 3) start at 0, levels 0 and 3 at 0xFF and stay there"""
    m, b = enc_model(cfg), enc_batch(pname, cfg)
    F, T, P = m["F"], m["T"], b["P"]
    r = Run()
    xt, tt, nt, gt = r.i(b["xy"], "xy"), r.i(m["stored"], "tables"), r.i(m["n_ls"], "n_ls"), r.i(b["genc"], "genc")
    vi, vw, K, mode, vstride, NV = src_args(r, m, source)
    dt = r.o((ENC_L, T, F), F32, "dtables")
    dt[l0:l1].zero_()
    dvw = r.o((NV, K), F32, "dvert_w", fill=0) if source == "vt" else None
    call("gngf_encode_bwd", P_(xt), P_(tt), m["half"], P_(vi), P_(vw), P_(nt), P_(gt), P_(dt), P_(dvw), P, ENC_L, F, T, K, mode, vstride, NV, l0, l1)
    r.done()
    never_written(dt[:l0], "dtables of level 0")
    never_written(dt[l1:], "dtables of level 3")
    want = b["dt_hash"] if source == "hash" else b["dt_vt"]
    close(dt[l0:l1], want[l0:l1], 1e-4, 1e-6, "direct encode bwd d tables")           # test_fused_encode_{hash,vertex_table}_vs_oracle
    if source == "vt":
        # d vert_w of levels [1, 3) only: the oracle's per-instance terms of those levels
        dw_inst = b["dw_inst"]
        want_w = np.zeros((NV, K))
        np.add.at(want_w, b["vid"][:, l0:l1].reshape(-1), dw_inst[:, l0:l1].reshape(-1, K).astype(np.float64))
        # 1e-4 / 1e-7 on tables of +-1e-4 in that test; fp16 tables are 100 times larger and d w is linear in them: the factor 100 is
        # THIS FILE'S OWN bound (no existing test holds the direct form's d w at fp16 tables)
        close(dvw, want_w, 1e-4, 1e-7 * (100 if m["half"] else 1), "direct encode bwd d vert_w")


@cases("gngf_encode_bwd_bucketed", [(f"{cfg}_{pn}_levels1to3_{'add' if acc else 'write'}{'_tile_order' if order else ''}",
                                     dict(cfg=cfg, pname=pn, accumulate=acc, order=order))
                                    for cfg in ("F2_f32", "F1_f32", "F4_f32") for pn in ENC_P for acc in (0, 1) for order in (0, 1)])
def run_encode_bwd_bucketed(cfg, pname, accumulate, order, l0=1, l1=3, image=65536):
    """accumulate = 0 WRITES every row of levels [1, 3) (they start 0xFF) and nothing else; accumulate = 1 adds (they start 0).
    matrix / base / items: scratch of the sizes the plan names, guarded.  Values: the elementwise bound of
    tests/test_gpu_bucket.py::test_bucketed_direct_backward_vs_oracle_and_atomics (exact integer sums, one rounding)."""
    m, b = enc_model(cfg), enc_batch(pname, cfg)
    F, T, P = m["F"], m["T"], b["P"]
    plan = (ctypes.c_int64 * 6)()
    assert query("gngf_encode_bwd_bucketed_plan", P, F, T, l1 - l0, image, plan) == 1
    r = Run()
    xt, nt, gt = r.i(b["xy"], "xy"), r.i(m["n_ls"], "n_ls"), r.i(b["genc"], "genc")
    srt = binned(r, enc_geo(pname, cfg), xt).sorted if order else None
    dt = r.o((ENC_L, T, F), F32, "dtables")
    if accumulate:
        dt[l0:l1].zero_()
    matrix, base, items = r.o((plan[3],), I32, "matrix"), r.o((plan[4],), I32, "base"), r.o((plan[5],), U8, "items")
    call("gngf_encode_bwd_bucketed", P_(xt), P_(nt), P_(gt), P_(dt), P, ENC_L, F, T, l0, l1, image, accumulate, P_(matrix), P_(base), P_(items),
         P_(srt))
    r.done()
    never_written(dt[:l0], "dtables of level 0")
    never_written(dt[l1:], "dtables of level 3")
    covered(dt[l0:l1], "every row of levels [1, 3)")
    from oracle import c_oracle
    want = c_oracle.encode_bwd_f64(np.array(b["xy"]), (ENC_L, T, F), m["n_ls"], np.array(b["genc"]))[l0:l1]     # the fp32 terms, summed in double
    got = dt[l0:l1].cpu().numpy().astype(np.float64)
    count = np.zeros((l1 - l0, T, 1))
    for l in range(l0, l1):
        np.add.at(count[l - l0, :, 0], b["hidx"][:, l].reshape(-1), 1)
    room = min(50, 61 - int(np.ceil(np.log2(max(1.0, count.max())))))
    quantum = count * (2.0 ** -room) * float(np.abs(b["genc"]).max())
    bound = 6.0e-8 * np.abs(want) + quantum + 1e-45
    err = np.abs(got - want)
    assert np.all(err <= bound), float((err / bound).max())


@cases("gngf_clear_hashed_rows", [(f"{cfg}_Ls{Ls}", dict(cfg=cfg, Ls=Ls)) for cfg in ("F2_f32", "F1_f32", "F4_f32") for Ls in (1, 3, 4)])
def run_clear_hashed_rows(cfg, Ls):
    """zeroes row hash(gx, gy) of level l for every vertex of levels [0, Ls); every other row of the buffer keeps its bytes"""
    m = enc_model(cfg)
    F, T, n_ls = m["F"], m["T"], m["n_ls"]
    vtot = int(((n_ls[:Ls].astype(np.int64) + 2) ** 2).sum())
    r = Run()
    nt = r.i(n_ls, "n_ls")
    dt = r.o((ENC_L, T, F), F32, "dtables")
    call("gngf_clear_hashed_rows", P_(dt), P_(nt), Ls, F, T, vtot)
    r.done()
    rows = torch.from_numpy(hashed_rows(n_ls, Ls, T)).to(DEV)
    assert 0 < int(rows[0].sum()) < T                                   # (the coarse level leaves rows out)
    all_zero(dt[rows], "hashed rows")
    never_written(dt[~rows], "rows no vertex hashes to")


# ---- binning
@cases("gngf_bin_pixels", [(f"{pn}", dict(pname=pn)) for pn in ENC_P])
def run_bin_pixels(pname):
    geo = enc_geo(pname, "F2_f32")
    xy = enc_batch(pname, "F2_f32")["xy"]
    r = Run()
    xt = r.i(xy, "xy")
    bins = binned(r, geo, xt)
    r.done()
    check_bins(bins, xy, geo)
    if pname == "P1025_one_tile":
        assert int(bins.n_items[0]) == 2                                # one tile, two work items


@cases("gngf_bin_pixels2", [(f"{pn}_{'zero_fill' if z else 'plain'}", dict(pname=pn, zero=z)) for pn in ENC_P for z in (0, 4 * 257)])
def run_bin_pixels2(pname, zero):
    """the reserving form: persistent_ws (2 * 4^tile_shift + 3) int32, zero before its first use and never reset; zero_fill cleared
    by riders of the count launch"""
    geo = enc_geo(pname, "F2_f32")
    xy = enc_batch(pname, "F2_f32")["xy"]
    r = Run()
    xt = r.i(xy, "xy")
    bins = Bins(r, geo)
    pws = r.o((2 * geo.ntiles + 3,), I32, "persistent_ws", fill=0)
    zf = r.o((zero,), F32, "zero_fill") if zero else None
    job = lib().BinJob(P_(xt), geo.P, geo.tile_shift, geo.NB, geo.chunk, P_(bins.blockhist), P_(pws), *bins.pointers())
    call("gngf_bin_pixels2", ctypes.byref(job), P_(zf), zero)
    r.done()
    check_bins(bins, xy, geo)
    from test_gpu_binning import _model
    w, counts = pws.cpu().numpy(), _model(xy, geo.tile_shift, geo.chunk).counts
    assert np.array_equal(w[:geo.ntiles], counts) and np.array_equal(w[geo.ntiles:2 * geo.ntiles], counts) and w[2 * geo.ntiles + 2] == 0
    if zf is not None:
        all_zero(zf, "zero_fill")


PREPARE_VARIANTS = {   # zero_fill floats, dG_zero words (0: none), persistent_ws, clear_rows, G
    "plain_dG1": (0, 1, 0, 0, 1), "zero_fill_dG2": (4 * (2 * 4096 + 5), 2, 0, 0, 1), "counters_dG1": (0, 1, 1, 0, 1),
    "counters_dG2_clear_rows": (0, 2, 1, 1, 1), "zero_fill_clear_rows_noG": (4 * 257, 0, 0, 1, 0), "no_dG": (0, 0, 0, 0, 1),
}


@cases("gngf_encode_tiled_prepare", [(f"{cfg}_{src}_{pn}_{v}", dict(cfg=cfg, source=src, pname=pn, variant=v))
                                     for cfg in ("F2_f32", "F1_f32", "F2_f16") for src in ("hash", "vt") for pn in ENC_P for v in PREPARE_VARIANTS
                                     if not (src == "vt" and PREPARE_VARIANTS[v][3])])
def run_encode_tiled_prepare(cfg, source, pname, variant):
    """the binning + the vertex stage forward (G) + the clears riding on it: dG_zero (words 1: vtot F floats; 2: vtot F + 2 64-bit
    words, the two trailing ones included), zero_fill, clear_rows (hash source: the hashed rows of the staged levels, nothing else),
    persistent_ws (zero before, zero after)"""
    zero_floats, words, counters, clear, with_G = PREPARE_VARIANTS[variant]
    m, b, geo = enc_model(cfg), enc_batch(pname, cfg), enc_geo(pname, cfg)
    F, T = m["F"], m["T"]
    r = Run()
    xt, tt, nt = r.i(b["xy"], "xy"), r.i(m["stored"], "tables"), r.i(m["n_ls"], "n_ls")
    vi, vw, K, mode, vstride, NV = src_args(r, m, source)
    bins = Bins(r, geo)
    G = r.o((geo.vtot, F), F32, "G") if with_G else None
    dGz = r.o((geo.vtot * F,), F32, "dG_zero") if words == 1 else (r.o((geo.vtot * F + 2,), I64, "dG_zero") if words == 2 else None)
    zf = r.o((zero_floats,), F32, "zero_fill") if zero_floats else None
    pws = r.o((2 * geo.ntiles + 3,), I32, "persistent_ws", fill=0) if counters else None
    cr = r.o((ENC_L, T, F), F32, "clear_rows") if clear else None
    call("gngf_encode_tiled_prepare", P_(xt), geo.P, geo.tile_shift, geo.NB, geo.chunk, P_(bins.blockhist), *bins.pointers(), P_(tt), m["half"],
         P_(vi), P_(vw), P_(nt), geo.n_ls_c, P_(G), P_(dGz), words or 1, geo.Ls, F, T, K, mode, vstride, NV, P_(zf), zero_floats, P_(pws), P_(cr))
    r.done()
    check_bins(bins, b["xy"], geo)
    if with_G:
        check_grid(G, m, source, "G of the vertex riders")
    if dGz is not None:
        all_zero(dGz, f"dG_zero (words {words})")
    if zf is not None:
        all_zero(zf, "zero_fill")
    if pws is not None:
        all_zero(pws, "persistent_ws after the call")
    if cr is not None:
        rows = torch.from_numpy(hashed_rows(m["n_ls"], geo.Ls, T)).to(DEV)
        all_zero(cr[rows], "hashed rows of the staged levels")
        never_written(cr[~rows], "rows no staged vertex hashes to")


# ---- vertex stage
def vstage_table(sources=("hash", "vt"), cfgs=("F2_f32", "F1_f32", "F4_f32", "F2_f16")):
    return [(f"{cfg}_{src}_Ls3of4", dict(cfg=cfg, source=src)) for cfg in cfgs for src in sources]


@cases("gngf_vertex_grid_fwd", vstage_table())
def run_vertex_grid_fwd(cfg, source):
    m = enc_model(cfg)
    F, T = m["F"], m["T"]
    vtot = int(((m["n_ls"][:ENC_LS].astype(np.int64) + 2) ** 2).sum())
    r = Run()
    tt, nt = r.i(m["stored"], "tables"), r.i(m["n_ls"], "n_ls")
    vi, vw, K, mode, vstride, NV = src_args(r, m, source)
    G = r.o((vtot, F), F32, "G")
    call("gngf_vertex_grid_fwd", P_(tt), m["half"], P_(vi), P_(vw), P_(nt), host_i32(m["n_ls"]), P_(G), ENC_LS, F, T, K, mode, vstride, NV)
    r.done()
    check_grid(G, m, source, "G")


@functools.lru_cache(maxsize=None)
def vstage_exact(cfg):
    """integers all round (tests/test_gpu_vertex_bwd_flat.py::test_exact_sums_equal_int64_evaluation_bit_for_bit): vertex-grid
    gradient in [-8, 8], weights in {1, 2}, table values in [-4, 4] — every sum is exact in fp32 in any order"""
    m = enc_model(cfg)
    F, T, n_ls = m["F"], m["T"], m["n_ls"]
    rng = np.random.default_rng(12 + F)
    vtot = int(((n_ls[:ENC_LS].astype(np.int64) + 2) ** 2).sum())
    q = rng.integers(-8, 9, (vtot, F)).astype(np.int64)
    w = rng.integers(1, 3, (m["NV"], ENC_K)).astype(np.int64)
    tab = rng.integers(-4, 5, (ENC_L, T, F)).astype(np.int64)
    dt_h, dt_v, dvw = np.zeros((ENC_L, T, F), np.int64), np.zeros((ENC_L, T, F), np.int64), np.zeros((m["NV"], ENC_K), np.int64)
    goff = 0
    for l in range(ENC_LS):
        side = int(n_ls[l]) + 2
        gy, gx = np.divmod(np.arange(side * side), side)
        ql = q[goff:goff + side * side]
        g = np.stack([gx, gy], 0).astype(np.int32).reshape(1, 2, 1, -1)
        np.add.at(dt_h[l], orc.spatial_hash(g, T)[0, 0], ql)
        vid = gy * m["vstride"] + gx
        for k in range(ENC_K):
            np.add.at(dt_v[l], m["vi"][vid, k], w[vid, k][:, None] * ql)
            np.add.at(dvw[:, k], vid, (tab[l][m["vi"][vid, k]] * ql).sum(-1))
        goff += side * side
    assert max(int(np.abs(a).max()) for a in (dt_h, dt_v, dvw)) < 2 ** 24
    return dict(q=q, w=w, tab=tab, vtot=vtot, dt_hash=dt_h, dt_vt=dt_v, dvw=dvw)


def vstage_inputs(r, cfg, source):
    m, e = enc_model(cfg), vstage_exact(cfg)
    tt = r.i(e["tab"].astype(np.float16 if m["half"] else np.float32), "tables")
    nt = r.i(m["n_ls"], "n_ls")
    dG = r.i(e["q"].astype(np.float32), "dG")
    vi, vw = (r.i(m["vi"], "vert_idx"), r.i(e["w"].astype(np.float32), "vert_w")) if source == "vt" else (None, None)
    dt = r.o((ENC_L, m["T"], m["F"]), F32, "dtables")
    dt[:ENC_LS].zero_()
    return m, e, tt, nt, dG, vi, vw, dt


def check_vstage(dt, e, source, dvw=None):
    never_written(dt[ENC_LS:], "dtables of the level that is not staged")
    assert np.array_equal(dt[:ENC_LS].cpu().numpy(), e["dt_hash" if source == "hash" else "dt_vt"][:ENC_LS].astype(np.float32))
    if dvw is not None:
        covered(dvw, "dvert_w")
        assert np.array_equal(dvw.cpu().numpy(), e["dvw"].astype(np.float32))


@cases("gngf_vertex_grid_bwd", vstage_table())
def run_vertex_grid_bwd(cfg, source):
    """dtables (L,T,F) accumulated (levels [0, 3) start at 0, level 3 keeps its 0xFF), dvert_w (NV,K) accumulated (starts at 0)"""
    r = Run()
    m, e, tt, nt, dG, vi, vw, dt = vstage_inputs(r, cfg, source)
    dvw = r.o((m["NV"], ENC_K), F32, "dvert_w", fill=0) if source == "vt" else None
    call("gngf_vertex_grid_bwd", P_(tt), m["half"], P_(vi), P_(vw), P_(nt), host_i32(m["n_ls"]), P_(dG), P_(dt), P_(dvw), ENC_LS, m["F"], m["T"],
         ENC_K if source == "vt" else 0, 1 if source == "vt" else 0, m["vstride"] if source == "vt" else 0, m["NV"] if source == "vt" else 0)
    r.done()
    check_vstage(dt, e, source, dvw)


@cases("gngf_vertex_grid_bwd_sorted", [(f"{l}_{'dw' if dw else 'nodw'}_{'dG64' if g64 else 'dG'}", dict(cfg=kw["cfg"], with_dw=dw, from64=g64))
                                       for l, kw in vstage_table(sources=("vt",)) for dw in (0, 1) for g64 in ((0, 1) if kw["cfg"] == "F2_f32" else (0,))])
def run_vertex_grid_bwd_sorted(cfg, with_dw, from64):
    """slot order; dvert_w (NV,K) is WRITTEN without atomics (starts 0xFF).  dG64: the gradient read from the 64-bit fixed-point grid
    (vtot F + 2 words: the integers with scale word 0, not poisoned — as the flat form's exact test hands them over)"""
    from collision_handling_in_instantngp_amd import ops
    r = Run()
    m, e, tt, nt, dG, vi, vw, dt = vstage_inputs(r, cfg, "vt")
    order = r.i(ops.slot_order(vi, [int(n) for n in m["n_ls"][:ENC_LS]], m["vstride"]), "order")
    dG64 = r.i(np.concatenate([e["q"].reshape(-1), [0, 0]]).astype(np.int64), "dG64") if from64 else None
    dvw = r.o((m["NV"], ENC_K), F32, "dvert_w") if with_dw else None
    call("gngf_vertex_grid_bwd_sorted", P_(tt), m["half"], P_(vi), P_(vw), P_(order), P_(nt), P_(None if from64 else dG), P_(dG64), e["vtot"],
         P_(dt), P_(dvw), ENC_LS, m["F"], m["T"], ENC_K, m["vstride"], m["NV"])
    r.done()
    never_written(dt[ENC_LS:], "dtables of the level that is not staged")
    assert np.array_equal(dt[:ENC_LS].cpu().numpy(), e["dt_vt"][:ENC_LS].astype(np.float32))
    if with_dw:
        # WRITTEN (include/gngf.h), every entry: ops.py hands over torch.empty_like and adds the result to the direct levels' d w, so
        # the vertices that belong to no staged level's grid must come back as zero, not as whatever the buffer held
        covered(dvw, "dvert_w")
        assert np.array_equal(dvw.cpu().numpy(), e["dvw"].astype(np.float32))


@cases("gngf_vertex_grid_bwd_flat", [(f"{cfg}_{'dG64' if g64 else 'dG'}", dict(cfg=cfg, from64=g64)) for cfg in ("F2_f32", "F1_f32", "F4_f32")
                                     for g64 in ((0, 1) if cfg == "F2_f32" else (0,))])
def run_vertex_grid_bwd_flat(cfg, from64):
    """the static item list (ops.vertex_flat_list: built unguarded, copied into the arena); dtables (rows = Ls T, F) accumulated"""
    from collision_handling_in_instantngp_amd import ops
    r = Run()
    m, e, _tt, _nt, dG, vi, vw, dt = vstage_inputs(r, cfg, "vt")
    lst = ops.vertex_flat_list(vi, vw, [int(n) for n in m["n_ls"][:ENC_LS]], m["vstride"], m["T"])
    gi, w, dest = r.i(lst.gi, "item_gi"), r.i(lst.w, "item_w"), r.i(lst.dest, "item_dest")
    dG64 = r.i(np.concatenate([e["q"].reshape(-1), [0, 0]]).astype(np.int64), "dG64") if from64 else None
    call("gngf_vertex_grid_bwd_flat", P_(gi), P_(w), P_(dest), lst.n, P_(None if from64 else dG), P_(dG64), e["vtot"], P_(dt), ENC_LS * m["T"], m["F"])
    r.done()
    check_vstage(dt, e, "vt")


# ---- pixel stage
def pixel_inputs(r, cfg, pname):
    m, b, geo = enc_model(cfg), enc_batch(pname, cfg), enc_geo(pname, cfg)
    xt, nt = r.i(b["xy"], "xy"), r.i(m["n_ls"], "n_ls")
    bins = binned(r, geo, xt)
    return m, b, geo, xt, nt, bins


def check_counters(bins, b, geo):
    """n_items: [0] the number of items, [1..3] the work counters the persistent kernels put back to zero"""
    from test_gpu_binning import _model
    n = bins.n_items.cpu().numpy()
    assert n[0] == len(_model(b["xy"], geo.tile_shift, geo.chunk).items) and np.all(n[1:] == 0), n


def check_enc(enc, b, m, source, what):
    F = m["F"]
    covered(enc[:, :ENC_LS * F], "enc columns of the staged levels")
    never_written(enc[:, ENC_LS * F:], "enc columns of the level that is not staged")
    want = b["enc_hash" if source == "hash" else "enc_vt"]
    # test_tiled_encode_hash_vs_oracle 1e-6 / 1e-9, test_tiled_encode_vertex_table_vs_oracle 2e-6 / 1e-9
    close(enc[:, :ENC_LS * F], want[:, :ENC_LS * F], 1e-6 if source == "hash" else 2e-6, 1e-9, what)


@cases("gngf_encode_tiled_fwd", [(f"{cfg}_{src}_{pn}", dict(cfg=cfg, source=src, pname=pn)) for cfg in ("F2_f32", "F1_f32", "F4_f32")
                                 for src in ("hash", "vt") for pn in ENC_P])
def run_encode_tiled_fwd(cfg, source, pname):
    """enc (P, L F) is written by original pixel index, levels [0, 3) only; G is the oracle's vertex grid"""
    r = Run()
    m, b, geo, _xt, nt, bins = pixel_inputs(r, cfg, pname)
    F = m["F"]
    G = r.i(vertex_grid_oracle(m, source, Ls=ENC_LS), "G")
    enc = r.o((geo.P, ENC_L * F), F32, "enc")
    call("gngf_encode_tiled_fwd", P_(bins.sorted), P_(bins.items), P_(bins.n_items), geo.max_items, P_(nt), geo.n_ls_c, P_(G), P_(enc), ENC_L,
         geo.Ls, F, geo.tile_shift, geo.lds_bytes)
    r.done()
    check_counters(bins, b, geo)
    check_enc(enc, b, m, source, "tiled fwd")


@cases("gngf_encode_tiled_fwd_fused", [(f"{cfg}_{src}_{pn}", dict(cfg=cfg, source=src, pname=pn)) for cfg in ENC_CFGS
                                       for src in ("hash", "vt") for pn in ENC_P if src == "hash" or cfg == "F2_f32"])
def run_encode_tiled_fwd_fused(cfg, source, pname):
    """the vertex stage inside the staging loop: the level-interleaved kernel (F = 2, fp32 tables) takes both index sources, the
    generic one (F in {1, 4}; fp32 or fp16 tables) the spatial hash.  fp16 tables at a shape the interleaved kernel takes (F = 2)
    are rejected, and then nothing may be written."""
    r = Run()
    m, b, geo, _xt, nt, bins = pixel_inputs(r, cfg, pname)
    F = m["F"]
    tt = r.i(m["stored"], "tables")
    vi, vw, K, mode, vstride, NV = src_args(r, m, source)
    enc = r.o((geo.P, ENC_L * F), F32, "enc")
    args = (P_(bins.sorted), P_(bins.items), P_(bins.n_items), geo.max_items, P_(nt), geo.n_ls_c, P_(tt), m["half"], P_(vi), P_(vw), P_(enc),
            ENC_L, geo.Ls, F, m["T"], K, mode, vstride, NV, geo.tile_shift, geo.lds_bytes, None)
    if m["half"] and F == 2:
        with pytest.raises(RuntimeError, match="rejected arguments"):
            call("gngf_encode_tiled_fwd_fused", *args)
        r.done()
        never_written(enc, "enc of a rejected call")
        return
    call("gngf_encode_tiled_fwd_fused", *args)
    r.done()
    check_counters(bins, b, geo)
    check_enc(enc, b, m, source, "tiled fwd, vertex stage fused")


TILED_BWD_SINKS = ("dG_partials", "dG_partials_bound", "dG64", "dG64_only", "hash_dtables", "hash_dtables_bound", "hash_dtables_gather", "riders")


def tiled_bwd_table():
    out = []
    for cfg in ("F2_f32", "F1_f32", "F4_f32"):
        for sink in TILED_BWD_SINKS:
            if sink.startswith("dG64") and cfg != "F2_f32":
                continue                                      # only the interleaved backward fills the fixed-point grid
            for pn in ENC_P:
                out.append((f"{cfg}_{pn}_{sink}", dict(cfg=cfg, pname=pn, sink=sink)))
    return out


def tiled_bwd_call(bins, geo, nt, genc, absmax, dG, partials, F, ride=None, mse=None, hash_dt=None, hash_T=0, dG64=None):
    from collision_handling_in_instantngp_amd import ops
    tlo = ops.tile_level_offsets(geo, torch.device(DEV, torch.cuda.current_device()))
    ride_args = [P_(None)] * 7 + [0, 0, 0] if ride is None else [P_(ride[0])] + [P_(x) for x in ride[1]] + list(ride[2])
    mse_args = [P_(None)] * 4 + [0] if mse is None else [P_(x) for x in mse[:4]] + [mse[4]]
    call("gngf_encode_tiled_bwd", P_(bins.sorted), P_(bins.items), P_(bins.n_items), geo.max_items, P_(bins.tile_item_base), P_(tlo), P_(nt),
         geo.n_ls_c, P_(genc), P_(absmax), 1 if absmax is not None else 0, 0, P_(dG), P_(partials), ENC_L, geo.Ls, F, geo.tile_shift,
         geo.lds_bytes, geo.chunk, *ride_args, P_(None), P_(None), *mse_args, P_(hash_dt), hash_T, P_(dG64),
         max(1, int(geo.P - 1).bit_length()) if dG64 is not None else 0, None)


@cases("gngf_encode_tiled_bwd", tiled_bwd_table())
def run_encode_tiled_bwd(cfg, pname, sink):
    """each sink of the pixel-stage backward.  partials (max_items lds_bytes / 4 floats) is scratch, guarded.  tile_level_off comes
    from ops.tile_level_offsets, which allocates it itself: an input, unguarded.
      dG_partials[_bound]   fp32 dG (vtot, F), accumulated from 0, through the partial images and the gather pass
      dG64[_only]           the fixed-point grid (vtot F + 2 words, zero on entry) and its conversion into dG (0xFF before: written);
                            _only: dG NULL, the grid must hold the same words
      hash_dtables[_bound]  no vertex grid: the items add to rows hash(gx, gy) of levels [0, 3) of (L,T,F); level 3 keeps its 0xFF
      hash_dtables_gather   with dG (zero on entry: the gather pass reads it): the gather pass adds to the table rows and leaves dG
                            as it was — coordinates inside [0,1]^2 with every level staged add nothing to it either
      riders                ride_* (the slab reduction of a decoder backward) and mse_* (the pixel loss value) in extra workgroups
    Values: the float64 sums of the oracle's fp32 terms at the bound of test_tiled_encode_hash_vs_oracle (2e-4 / 2e-6 max(1, max))."""
    r = Run(16)
    m, b, geo, _xt, nt, bins = pixel_inputs(r, cfg, pname)
    F, T, P = m["F"], m["T"], geo.P
    genc = r.i(b["genc"], "genc")
    bound = sink.endswith("_bound") or sink.startswith("dG64")
    absmax = r.i(np.array([np.abs(b["genc"]).max()], np.float32), "genc_absmax") if bound else None
    partials = r.o((geo.max_items * (geo.lds_bytes // 4),), F32, "partials")
    want_dG = b["dG"][:geo.vtot]
    tol = lambda w: 2e-6 * max(1.0, float(np.abs(w).max()))
    dG = dG64 = hdt = grads = loss = None
    if sink.startswith("dG_partials"):
        dG = r.o((geo.vtot, F), F32, "dG", fill=0)
        tiled_bwd_call(bins, geo, nt, genc, absmax, dG, partials, F)
    elif sink.startswith("dG64"):
        dG64 = r.o((geo.vtot * F + 2,), I64, "dG64", fill=0)
        dG = r.o((geo.vtot, F), F32, "dG") if sink == "dG64" else None
        tiled_bwd_call(bins, geo, nt, genc, absmax, dG, partials, F, dG64=dG64)
    elif sink == "hash_dtables_gather":
        dG = r.o((geo.vtot, F), F32, "dG", fill=0)
        hdt = r.o((ENC_L, T, F), F32, "hash_dtables")
        hdt[:ENC_LS].zero_()
        tiled_bwd_call(bins, geo, nt, genc, absmax, dG, partials, F, hash_dt=hdt, hash_T=T)
    elif sink.startswith("hash_dtables"):
        hdt = r.o((ENC_L, T, F), F32, "hash_dtables")
        hdt[:ENC_LS].zero_()
        tiled_bwd_call(bins, geo, nt, genc, absmax, None, partials, F, hash_dt=hdt, hash_T=T)
    else:
        d = dec_ref(P, ENC_L * F, 3, 0)
        slabs0 = torch.empty((query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", ENC_L * F, 3),), device=DEV)
        t_ = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        e_, y_, gy_, ws_ = t_(d["x"]), t_(d["y"]), t_(d["gy"]), [t_(w) for pair in zip(d["W"], d["B"]) for w in pair]
        de_ = torch.empty_like(e_)
        call("gngf_decoder_bwd", P_(e_), P_(y_), P_(gy_), P_(None), P_(None), *[P_(w) for w in ws_[:5]], P_(de_), *[P_(None)] * 6, P_(slabs0),
             P_(None), P_(None), P_(None), 0, P, ENC_L * F, 3, 0)
        torch.cuda.synchronize()
        slabs = r.i(slabs0, "ride_slabs")
        grads = dec_grads(r, ENC_L * F, 3)
        pred, label = r.i(d["y"], "mse_pred"), r.i(d["tgt"], "mse_label")
        loss, mws = r.o((1,), F32, "mse_loss"), r.o((query("gngf_mse_workspace_floats"),), F32, "mse_workspace", fill=0)
        dG = r.o((geo.vtot, F), F32, "dG", fill=0)
        tiled_bwd_call(bins, geo, nt, genc, None, dG, partials, F, ride=(slabs, grads, (P, ENC_L * F, 3)), mse=(pred, label, loss, mws, P * 3))
    r.done()
    check_counters(bins, b, geo)
    if sink in ("dG_partials", "dG_partials_bound", "dG64", "riders"):
        covered(dG, "dG")
        close(dG, want_dG, 2e-4, tol(want_dG), f"vertex-grid gradient ({sink})")
    if sink == "dG64_only":
        # the same launch with dG given (unguarded) leaves the same fixed-point words
        ref64, refG = torch.zeros((geo.vtot * F + 2,), dtype=I64, device=DEV), torch.empty((geo.vtot, F), device=DEV)
        tiled_bwd_call(bins, geo, nt, genc, absmax, refG, torch.empty_like(partials), F, dG64=ref64)
        torch.cuda.synchronize()
        assert torch.equal(dG64[:-2], ref64[:-2])            # tests/test_gpu_encode.py::test_fixed_point_vertex_grid_is_exact_and_order_free
        close(refG, want_dG, 2e-4, tol(want_dG), "vertex-grid gradient converted from the fixed-point grid")
    if hdt is not None:
        never_written(hdt[ENC_LS:], "table gradient of the level that is not staged")
        want = b["dt_hash"][:ENC_LS]
        close(hdt[:ENC_LS], want, 2e-4, tol(want), f"table gradient ({sink})")
        if sink == "hash_dtables_gather":
            all_zero(dG, "dG, which the hash-scattering gather pass reads (zero on entry) and leaves unwritten")
    if grads is not None:
        check_dec_grads(grads, d["drgb"], "ridden slab reduction")
        covered(loss, "mse_loss")
        all_zero(mws, "mse workspace after the launch")
        close(loss, [np.mean((d["y"].astype(np.float64) - d["tgt"]) ** 2)], 2e-6, 0, "ridden mse value")        # test_mse_kernels_vs_numpy


# ================================================================================================ the test
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASE_TABLE, ids=[case_id(c) for c in CASE_TABLE])
def test_store_bounds(c):
    _entry, _label, runner, kw = c
    RUNNERS[runner](**kw)
