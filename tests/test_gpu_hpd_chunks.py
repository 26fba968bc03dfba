"""ops.HpdVertexFunction (the HashProbDistribution of reference models.py:45-123 evaluated once per distinct grid vertex, in row
chunks) against a float64 CPU reference written here, at chunk layouts where the chunks of ONE call take different paths.

Every chunk decides on its own whether its row statistics come from the logits GEMM's epilogue (`epi`), whether its logits are
kept for the backward (`kept`), whether its d-logits are formed inside the dW / dh GEMM loaders (`fused`), and the chunks may run
software-pipelined over two streams.  The kernels are tested one by one in test_gpu_dense.py; this file tests the code that
strings them together, and proves from the `hpd_chunk` records of ops.STEP_TRACE which path every chunk took.

Reference: verts[u] = (u % vstride, u // vstride); hidden layers with ReLU; z = h W^T + b; p = softmax(z); tv = p.gather(ti_gpu);
pbar = mw^T p; probs = p (dense mode); parameter gradients by torch.autograd of
S = sum g_tv tv + sum g_pbar pbar (+ sum g_probs probs), with the same random upstream gradients as the GPU call.

Error model (u = 2^-24, fp32 unit roundoff; fp32 dot products of length k carry ~sqrt(k) u of the sum of |terms|):
  * logits:  |dz_ut| <= C_Z s_u u,   s_u = max_t sum_k |h_uk||W_tk| + |b_t|,   C_Z = 2 n_layers sqrt(H_max + 1)
    (one dot product per layer of the hidden chain, H_max the widest layer).
  * probabilities: softmax turns an absolute logit error into a relative one, dp_t = p_t (dz_t - sum_j p_j dz_j), which is at
    most 2 (1 - p_t) max|dz| (it vanishes as a row peaks), plus the rounding of exp, the division and a row sum over T terms:
    |dp_ut| <= r_ut p_ut,  r_ut = (2 (1 - p_ut) C_Z s_u + 2 log2 T + 8) u.
  * p-bar: |d pbar_lt| <= sum_u mw_ul r_ut p_ut + (log2 NV + 8) u pbar_lt  (the atomics / GEMM sum over the vertices).
  * gradients: with g = d S / d p and dot_u = sum_t p g, the d-logits dz = p (g - dot) carry at most
    e_ut = r_ut p_ut |g_ut - dot_u| + p_ut sum_j r_uj p_uj |g_uj| + eps |dz_ut| + 4 u p_ut (|g_ut| + |dot_u|), where
    eps = C_Z u (the hidden activations) + 2 n_layers (3 * 2^-18 + 2 sqrt(N) u) (per GEMM of the backward chain: the two-plane
    split, the least exact product any path uses, and the fp32 sum over N = max(NV, T) terms).  These errors come from
    independent roundings, so
    they add in quadrature: e^2 is pushed through the backward pass with squared weights and activations, and K_SIGMA = 4
    times its square root, at its maximum, relative to the gradient's own maximum, is what the GPU gradient must meet.
    (Pushing |e| through on absolute values instead gives bounds at or above the gradients' own size for the first layers:
    they sum ~10^3 vertices and ~10^3 slots with heavy cancellation.)
A path that needs more than 4x the error of the exact-fp32, unfused, serial path (plus a 16-ulp floor of the quantity's
maximum, for the order of float atomics) fails as well.

Observed on the MI355X over every path of every case: the largest max |err| / bound was 5.1e-2 (tv), 2.8e-2 (dense probs),
5.3e-2 (p-bar) and 2.9e-3 .. 4.9e-2 (the eight gradients); relative to the reference's maximum: tv 1.8e-5, probs 2.2e-6,
p-bar 6.1e-7, gradients 5.9e-6 .. 9.3e-5.  Paths with two-plane dW / dh products (hpd_bwd_two_planes, the default) reach 5-12x
the exact path's gradient error; every other path stays within 4x of it.
"""
import dataclasses
import math

import pytest
import torch

from conftest import parity_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
FLT_MIN = 2.0 ** -126
TWO_PLANES = 3 * 2.0 ** -18
K_SIGMA = 4.0            # gradient bound: this many times the quadrature sum of the per-element error bounds

# largest (max |err| / bound) per quantity over the session, printed at the end of the module (the docstring's numbers)
OBSERVED = {}


def close(a, b, rtol, atol, msg):
    """assert_allclose + a row in the achieved-error report (tests/conftest.py: ParityRecorder)"""
    parity_close(a, b, rtol, atol, msg)


@pytest.fixture(scope="module")
def ops():
    from collision_handling_in_instantngp_amd import ops as o
    yield o
    if OBSERVED:
        print("\nHPD chunks, largest max |err| / bound:", {k: f"{v:.2e}" for k, v in sorted(OBSERVED.items())})


@dataclasses.dataclass(frozen=True)
class Case:
    T: int
    widths: tuple
    NV: int
    rows: int            # chunk_bytes = rows * 4 * T (the op clamps rows to >= 64 and <= NV)
    L: int               # 0: mw = None (no p-bar)
    K: int
    vstride: int
    keep_probs: bool = False
    g_tv: bool = True    # False: the loss reaches the op through p-bar only
    ties: bool = False   # W_last / b_last rows t and t + T/2 identical
    # what the case is named for, under the default tuning: per chunk (epi, fused) in the first pass, and pipelined
    mix: tuple = ()
    pipelined: bool = True

    @property
    def rows_eff(self):
        return int(max(64, min(self.NV, self.rows)))

    @property
    def chunks(self):
        return [(u0, min(self.rows_eff, self.NV - u0)) for u0 in range(0, self.NV, self.rows_eff)]


W3 = (32, 64, 128)
CASES = {
    # unfused / non-epi 200-row chunk + fused / epi 128-row tail (the planes of the pipelined backward were missing)
    "A": Case(2048, W3, 328, 200, 16, 4, 33, mix=((0, 0), (1, 1))),
    # fused / epi whole chunks + ragged unfused tail
    "B": Case(2048, W3, 677, 128, 16, 4, 1024, mix=((1, 1),) * 5 + ((0, 0),)),
    # exact multiple: every chunk fused, no tail
    "C": Case(4096, W3, 768, 256, 16, 4, 33, mix=((1, 1),) * 3),
    # tiny chunk_bytes: the 64-row floor, 16 chunks, none fused
    "D": Case(1024, W3, 1000, 1, 5, 4, 1024, mix=((0, 0),) * 16),
    # NV < rows: one chunk, never pipelined
    "E37": Case(2048, W3, 37, 64, 16, 4, 33, mix=((0, 0),), pipelined=False),
    "E1": Case(2048, W3, 1, 64, 16, 4, 1024, mix=((0, 0),), pipelined=False),
    # T % 128 != 0: no epi, no fused, several chunks
    "F": Case(1000, W3, 500, 128, 16, 4, 1024, mix=((0, 0),) * 4),
    # last hidden width 64: epi yes, fused never
    "G": Case(2048, (32, 64), 600, 256, 16, 4, 33, mix=((1, 0), (1, 0), (0, 0))),
    # K = GNGF_MAX_TOPK with epi; K * 64 > T forces the separate statistics pass
    "H32": Case(2048, W3, 384, 128, 16, 32, 1024, mix=((1, 1),) * 3),
    "H20": Case(1024, W3, 384, 128, 16, 20, 33, mix=((0, 1),) * 3),
    # no p-bar; the loss only through p-bar
    "I_nopbar": Case(2048, W3, 400, 128, 0, 4, 33, mix=((1, 1),) * 3 + ((0, 0),)),
    "I_pbaronly": Case(2048, W3, 400, 128, 16, 4, 1024, g_tv=False, mix=((1, 1),) * 3 + ((0, 0),)),
    # dense distribution with a dense upstream gradient, several chunks (no epi, no z-cache, serial)
    "J": Case(2048, W3, 300, 128, 16, 4, 1024, keep_probs=True, mix=((0, 0),) * 3, pipelined=False),
    # a larger T: several fused chunks + tail
    "K": Case(16384, W3, 1100, 384, 16, 4, 1024, mix=((1, 1), (1, 1), (0, 0))),
    # ties: paired columns t, t + T/2
    "L": Case(2048, W3, 256, 128, 16, 4, 33, ties=True, mix=((1, 1),) * 2),
}


# ------------------------------------------------------------------------------------------------ inputs and the float64 reference
class Data:
    """params (fp32, CPU) from a seeded models.HashProbDistribution, upstream gradients, the float64 reference and its bounds"""

    def __init__(self, name, case):
        from collision_handling_in_instantngp_amd import models
        seed = sum(map(ord, name))
        torch.manual_seed(seed)
        hpd = models.HashProbDistribution(list(case.widths), out_features=case.T, k=max(case.K, 1))
        self.params = [p.detach().to("cpu", torch.float32).clone() for p in hpd.flat_params()]
        T, NV, L, K = case.T, case.NV, case.L, case.K
        if case.ties:
            self.params[-2][T // 2:] = self.params[-2][:T // 2]
            self.params[-1][T // 2:] = self.params[-1][:T // 2]
        g = torch.Generator().manual_seed(seed + 1)
        self.mw = torch.rand((NV, L), generator=g) / NV if L else None
        self.g_tv = torch.randn((NV, K), generator=g) if case.g_tv else None
        self.g_pbar = torch.randn((L, T), generator=g) * 10 if L else None
        self.g_probs = torch.randn((NV, T), generator=g) if case.keep_probs else None
        self.dev = {k: (v.to(DEV) if v is not None else None) for k, v in
                    dict(mw=self.mw, g_tv=self.g_tv, g_pbar=self.g_pbar, g_probs=self.g_probs).items()}

        n_layers = len(self.params) // 2
        p64 = [p.double() for p in self.params]
        u = torch.arange(NV, dtype=torch.int64)
        self.verts = torch.stack([u % case.vstride, u // case.vstride], 1).double()
        hs = [self.verts]
        for i in range(n_layers - 1):
            hs.append(torch.relu(hs[-1] @ p64[2 * i].T + p64[2 * i + 1]))
        W, b = p64[-2], p64[-1]
        self.hs, self.p64 = hs, p64
        self.p = torch.softmax(hs[-1] @ W.T + b, dim=1)
        self.pbar = (self.mw.double().T @ self.p) if L else None
        # the error model (module docstring)
        s = (hs[-1].abs() @ W.abs().T + b.abs()).amax(dim=1)
        c_z = 2 * n_layers * math.sqrt(max(case.widths) + 1)
        self.r = (2 * (1 - self.p) * c_z * s[:, None] + 2 * math.log2(T) + 8) * U32     # relative bound of every probability
        self.c_z = c_z
        if L:
            self.pbar_bound = self.mw.double().T @ (self.p * self.r) + (math.log2(NV) + 8) * U32 * self.pbar
        self.n_layers = n_layers
        self._grads = {}

    def upstream(self, ti):
        """g (NV, T): the gradient of S with respect to p, for the GPU's top-K indices"""
        g = torch.zeros_like(self.p)
        if self.mw is not None:
            g += self.mw.double() @ self.g_pbar.double()
        if self.g_tv is not None:
            g.scatter_add_(1, ti, self.g_tv.double())
        if self.g_probs is not None:
            g += self.g_probs.double()
        return g

    def grads(self, case, ti):
        """(reference gradients, bounds) for the GPU's top-K indices (one autograd run per distinct index set)"""
        key = ti.numpy().tobytes()
        if key in self._grads:
            return self._grads[key]
        ps = [p.clone().requires_grad_() for p in self.p64]
        h = self.verts
        for i in range(self.n_layers - 1):
            h = torch.relu(h @ ps[2 * i].T + ps[2 * i + 1])
        p = torch.softmax(h @ ps[-2].T + ps[-1], dim=1)
        S = 0.0
        if self.g_tv is not None:
            S = S + (p.gather(1, ti) * self.g_tv.double()).sum()
        if self.mw is not None:
            S = S + ((self.mw.double().T @ p) * self.g_pbar.double()).sum()
        if self.g_probs is not None:
            S = S + (p * self.g_probs.double()).sum()
        ref = torch.autograd.grad(S, ps)
        # the bound: the d-logit errors, independent from element to element, pushed through the backward pass in quadrature
        N = max(case.NV, case.T)
        eps = self.c_z * U32 + 2 * self.n_layers * (TWO_PLANES + 2 * math.sqrt(N) * U32)
        g = self.upstream(ti)
        dot = (self.p * g).sum(dim=1, keepdim=True)
        dz = self.p * (g - dot)
        V = (self.r * self.p * (g - dot).abs() + self.p * (self.r * self.p * g.abs()).sum(dim=1, keepdim=True)
             + eps * dz.abs() + 4 * U32 * self.p * (g.abs() + dot.abs())) ** 2
        var = [None] * len(ps)
        var[-2], var[-1] = V.T @ self.hs[-1] ** 2, V.sum(dim=0)
        vH = V @ self.p64[-2] ** 2
        for i in range(self.n_layers - 2, -1, -1):
            vG = vH * (self.hs[i + 1] > 0)
            var[2 * i], var[2 * i + 1] = vG.T @ self.hs[i] ** 2, vG.sum(dim=0)
            vH = vG @ self.p64[2 * i] ** 2
        bnd = [K_SIGMA * v.sqrt() for v in var]
        out = self._grads[key] = ([r.detach() for r in ref], [float(b_.max()) for b_ in bnd])
        return out


_DATA = {}
_EXACT = {}          # case name -> {quantity: max |err|} of the exact-fp32, unfused, serial path


def data(name):
    if name not in _DATA:
        _DATA[name] = Data(name, CASES[name])
    return _DATA[name]


# ------------------------------------------------------------------------------------------------ one call of the op
@dataclasses.dataclass
class Run:
    tv: torch.Tensor
    ti: torch.Tensor
    pbar: object
    probs: object
    grads: list
    stats: dict
    trace: list
    mean_calls: int


def run(ops, name, tuning, mean=None, twice=False):
    case, d = CASES[name], data(name)
    ps = [p.to(DEV).requires_grad_() for p in d.params]
    stats, trace, calls = {}, [], []

    def hook(pbar):
        calls.append(1)
        mean(pbar)
    saved, saved_trace = ops.TUNING, ops.STEP_TRACE
    ops.TUNING, ops.STEP_TRACE = tuning, trace
    try:
        tv, ti, pbar, probs = ops.HpdVertexFunction.apply(case.NV, case.vstride, case.K, d.dev["mw"], case.keep_probs,
                                                          case.rows * 4 * case.T, ops.HpdAux(hook if mean else None, stats), *ps)
        outs, ups = [], []
        for o, gname in ((tv, "g_tv"), (pbar, "g_pbar"), (probs, "g_probs")):
            if o is not None and d.dev[gname] is not None:
                outs.append(o)
                ups.append(d.dev[gname])
        torch.autograd.backward(outs, ups, retain_graph=twice)
        if twice:
            torch.autograd.backward(outs, ups)
        torch.cuda.synchronize()
    finally:
        ops.TUNING, ops.STEP_TRACE = saved, saved_trace
    cpu = lambda x: x.detach().cpu() if x is not None else None      # noqa: E731
    return Run(cpu(tv), cpu(ti).long(), cpu(pbar), cpu(probs), [cpu(p.grad) for p in ps], stats,
               [f for w, f in trace if w == "hpd_chunk"], len(calls))


# ------------------------------------------------------------------------------------------------ what each call must show
def expected_trace(case, tun, passes=("fwd", "bwd")):
    """the hpd_chunk records the documented dispatch rules give: None where the budget depends on the device's free memory"""
    T, K, Hd = case.T, case.K, case.widths[-1]
    NV, rows = case.NV, case.rows_eff
    kp = case.keep_probs
    known_budget = tun.hpd_z_cache_reserve == 0 or tun.hpd_z_cache_bytes == 0
    keep_z = (not kp) and tun.hpd_z_cache_bytes > 0
    kept, cached = {}, 0
    for u0, n in case.chunks:
        if not known_budget:
            kept[u0] = None
        else:
            kept[u0] = keep_z and cached + n * T * 4 <= tun.hpd_z_cache_bytes
            cached += n * T * 4 if kept[u0] else 0
    pipe_f = tun.hpd_pipeline and tun.hpd_pipeline_fwd and not kp and NV > rows and tun.use_side_stream
    pipe_b = tun.hpd_pipeline and not kp and NV > rows and tun.use_side_stream
    Lq = case.L
    out = []
    for ps in passes:
        for u0, n in case.chunks:
            if ps == "fwd":
                epi = (tun.hpd_epilogue_stats and tun.hpd_gemm_split_bf16 and not kp and n % 128 == 0 and T % 128 == 0
                       and Hd % 32 == 0 and K * 64 <= T and T < (1 << 22))
                out.append(dict(pass_="fwd", u0=u0, n=n, epi=epi, kept=kept[u0], fused=False, pipelined=pipe_f))
            else:
                fused = (not kp and tun.hpd_bwd_fused and tun.hpd_gemm_split_bf16 and n % 128 == 0 and T % 128 == 0
                         and T < (1 << 22) and Hd == 128 and Lq <= 16 and K <= 32)
                out.append(dict(pass_=ps[:3], u0=u0, n=n, epi=False, kept=False if ps == "bwd2" else kept[u0], fused=fused,
                                pipelined=pipe_b))
    return out


def check_trace(case, tun, r, twice=False):
    want = expected_trace(case, tun, ("fwd", "bwd", "bwd2") if twice else ("fwd", "bwd"))
    assert len(r.trace) == len(want), (r.trace, want)
    nch = len(case.chunks)
    for got, w in zip(r.trace, want):
        if w["kept"] is None:                        # budget from the device's free memory: the backward uses what the forward kept
            w = dict(w, kept=got["kept"])
        assert got == w, (got, w)
    fwd_kept = [t["kept"] for t in r.trace[:nch]]
    assert [t["kept"] for t in r.trace[nch:2 * nch]] == fwd_kept
    assert r.stats == dict(rows_total=case.NV, T=case.T, rows_per_chunk=case.rows_eff, chunks=nch, chunks_kept=sum(fwd_kept)), r.stats


def check_values(name, r, tag):
    """r against the float64 reference.  Returns {quantity: (achieved max |err|, max |reference|)}."""
    case, d = CASES[name], data(name)
    T, K, NV = case.T, case.K, case.NV
    errs = {}
    ti = r.ti
    # top-K: indices in range and distinct; the float64 top-K set up to ties at the K-th value (test_gpu_dense.py rule)
    assert ti.shape == (NV, K) and int(ti.min()) >= 0 and int(ti.max()) < T
    assert bool((ti.sort(dim=1).values.diff(dim=1) > 0).all()), f"{tag}: repeated top-K index"
    ref_v, ref_i = torch.topk(d.p, K, dim=1)
    kth = ref_v[:, -1]
    same = (ti.sort(dim=1).values == ref_i.sort(dim=1).values).all(dim=1)
    for u in torch.nonzero(~same).flatten().tolist():
        for e in set(ti[u].tolist()) - set(ref_i[u].tolist()):
            assert abs(float(d.p[u, e] - kth[u])) <= 2 * float(d.r[u].max() * kth[u]) + FLT_MIN, (tag, u, e)
    # probabilities
    rb = d.r.gather(1, ti)
    tv_ref = d.p.gather(1, ti)
    close(r.tv, tv_ref, float(d.r.max()), 2 * FLT_MIN, f"{tag} tv")
    assert bool(((r.tv.double() - tv_ref).abs() <= rb * tv_ref + 2 * FLT_MIN).all()), f"{tag}: tv outside its bound"
    errs["tv"] = (float((r.tv.double() - tv_ref).abs().max()), float(tv_ref.max()))
    observe("tv", (r.tv.double() - tv_ref).abs() / (rb * tv_ref + 2 * FLT_MIN))
    if case.keep_probs:
        close(r.probs, d.p, float(d.r.max()), 2 * FLT_MIN, f"{tag} probs")
        err = (r.probs.double() - d.p).abs()
        assert bool((err <= d.r * d.p + 2 * FLT_MIN).all()), f"{tag}: probs outside their bound"
        errs["probs"] = (float(err.max()), float(d.p.max()))
        observe("probs", err / (d.r * d.p + 2 * FLT_MIN))
    if case.L:
        err = (r.pbar.double() - d.pbar).abs()
        close(r.pbar, d.pbar, 0, float(d.pbar_bound.max()), f"{tag} pbar")
        assert bool((err <= d.pbar_bound + FLT_MIN).all()), f"{tag}: pbar outside its bound"
        errs["pbar"] = (float(err.max()), float(d.pbar.max()))
        observe("pbar", err / (d.pbar_bound + FLT_MIN))
    else:
        assert r.pbar is None
    # gradients: within the bound relative to each gradient's own maximum
    ref, bnd = d.grads(case, ti)
    for i, (g, gr, b_) in enumerate(zip(r.grads, ref, bnd)):
        assert g is not None, f"{tag}: no gradient for parameter {i}"
        gmax = float(gr.abs().max())
        close(g, gr, 0, b_, f"{tag} grad[{i}] (bound / max {b_ / max(gmax, 1e-300):.1e})")
        err = float((g.double() - gr).abs().max())
        errs[f"grad{i}"] = (err, gmax)
        observe(f"grad{i}", torch.tensor(err / b_ if b_ > 0 else (0.0 if err == 0 else math.inf)))
    return errs


def observe(q, ratio):
    OBSERVED[q] = max(OBSERVED.get(q, 0.0), float(ratio.max()))


def two_plane_products(tun, r):
    """did any dW / dh product of the backward run on two bf16 planes (3 * 2^-18 per product by design)?"""
    fused = any(t["fused"] for t in r.trace)
    unfused = any(t["pass_"] == "bwd" and not t["fused"] for t in r.trace)
    return (tun.hpd_gemm_split_bf16 and tun.hpd_bwd_two_planes and r.probs is None
            and (fused or (unfused and tun.hpd_gemm_kernel == 1)))


def check_against_exact(name, errs, tag, two_planes):
    """no path may need more than 4x the error of the exact-fp32, unfused, serial path (16 ulps of the quantity's maximum
    aside: float atomics sum in no fixed order).  Gradients of paths with two-plane products are held to the error model only:
    on the MI355X they reach 5-12x the exact path's error (the documented price of hpd_bwd_two_planes), within the model."""
    ex = _EXACT[name]
    for k, (err, scale) in errs.items():
        if two_planes and k.startswith("grad"):
            continue
        assert err <= 4 * ex[k][0] + 16 * U32 * scale, (tag, k, err, ex[k][0])


def exact_tuning(saved):
    return dataclasses.replace(saved, hpd_gemm_split_bf16=False, hpd_bwd_fused=False, hpd_pipeline=False)


def run_exact(ops, name):
    if name not in _EXACT:
        tun = exact_tuning(ops.TUNING)
        r = run(ops, name, tun)
        check_trace(CASES[name], tun, r)
        _EXACT[name] = check_values(name, r, f"{name} exact")
    return _EXACT[name]


def one(ops, name, tun, tag):
    case = CASES[name]
    run_exact(ops, name)
    r = run(ops, name, tun)
    check_trace(case, tun, r)
    errs = check_values(name, r, tag)
    check_against_exact(name, errs, tag, two_plane_products(tun, r))
    return r


# ------------------------------------------------------------------------------------------------ the tests
def test_reference_vertex_coordinates_equal_the_op(ops):
    for name in ("A", "D", "E1"):
        case, d = CASES[name], data(name)
        v = ops.vertex_coords(0, case.NV, case.vstride, torch.device(DEV)).cpu().double()
        assert torch.equal(v, d.verts), name


def _cross(saved, pipe, rows):
    """every distinct dispatch of cases A / B for one pipelining mode; settings that select the same code are left out
    (without the split-bf16 GEMMs the kernel choice, the fused backward, the planes and the epilogue statistics do nothing)"""
    zc = {"z0": 0, "zfirst": rows * 4, "zall": 1 << 40}
    p, pf = pipe
    out = []
    for split in (False, True):
        inner = [dict()] if not split else [dict(hpd_gemm_kernel=k, hpd_bwd_fused=f, hpd_bwd_two_planes=tp, hpd_epilogue_stats=e)
                                            for k in (1, 17) for f in (False, True) for tp in (False, True) for e in (False, True)]
        for kw in inner:
            for zname, zb in zc.items():
                tun = dataclasses.replace(saved, hpd_pipeline=p, hpd_pipeline_fwd=pf, hpd_gemm_split_bf16=split,
                                          hpd_z_cache_bytes=zb, hpd_z_cache_reserve=0, **kw)
                out.append((f"pipe={p}/{pf} split={split} {kw} {zname}", tun))
    return out


@pytest.mark.parametrize("pipe", [(False, True), (True, False), (True, True)], ids=["serial", "pipe_bwd", "pipe_fwd_bwd"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_dispatch_of_mixed_chunk_layouts_matches_float64(ops, name, pipe):
    """cases A and B: the cross of every HPD path switch (z-cache budget none / first chunk / all) against float64"""
    case = CASES[name]
    saved = ops.TUNING
    for tag, tun in _cross(saved, pipe, case.rows_eff * case.T):
        r = one(ops, name, tun, f"{name} {tag}")
        if tun.hpd_z_cache_bytes == case.rows_eff * case.T * 4:
            assert r.stats["chunks_kept"] == 1
    assert ops.TUNING is saved


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("A", "B")])
def test_chunk_layout_matches_float64(ops, name):
    """default, serial, exact-fp32 and z-cache none / all, against float64"""
    saved = ops.TUNING
    tuns = {"default": saved, "serial": dataclasses.replace(saved, hpd_pipeline=False), "exact": exact_tuning(saved),
            "z0": dataclasses.replace(saved, hpd_z_cache_bytes=0, hpd_z_cache_reserve=0),
            "zall": dataclasses.replace(saved, hpd_z_cache_bytes=1 << 40, hpd_z_cache_reserve=0)}
    for tag, tun in tuns.items():
        one(ops, name, tun, f"{name} {tag}")
    assert ops.TUNING is saved


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_takes_the_paths_it_is_named_for(ops, name):
    """under the default tuning (z-cache off, so the budget does not depend on the device): per chunk of the forward pass the
    epilogue statistics or not, per chunk of the backward pass the fused loaders or not, and pipelining, as the case names"""
    case = CASES[name]
    tun = dataclasses.replace(ops.TUNING, hpd_z_cache_bytes=0)
    r = run(ops, name, tun)
    nch = len(case.chunks)
    fwd, bwd = r.trace[:nch], r.trace[nch:]
    assert [(int(f["epi"]), int(b["fused"])) for f, b in zip(fwd, bwd)] == list(case.mix), (fwd, bwd)
    assert all(t["pipelined"] == case.pipelined for t in bwd), bwd
    assert all(t["pipelined"] == case.pipelined for t in fwd), fwd
    assert r.stats["rows_per_chunk"] == case.rows_eff and r.stats["chunks"] == nch and r.stats["chunks_kept"] == 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_mean_hook_runs_once_after_every_chunk(ops, name):
    """aux.mean doubling p-bar is called exactly once and sees every chunk's share, also with the pipelined forward"""
    for pf in (True, False):
        tun = dataclasses.replace(ops.TUNING, hpd_pipeline=True, hpd_pipeline_fwd=pf)
        r = run(ops, name, tun, mean=lambda pbar: pbar.mul_(2.0))
        assert r.mean_calls == 1
        assert all(t["pipelined"] == pf for t in r.trace[:len(CASES[name].chunks)])
        tag = f"{name} mean hook x2 pipe_fwd={pf}"
        case, d = CASES[name], data(name)
        err = (r.pbar.double() - 2 * d.pbar).abs()
        close(r.pbar, 2 * d.pbar, 0, 2 * float(d.pbar_bound.max()), f"{tag} pbar")
        assert bool((err <= 2 * d.pbar_bound + FLT_MIN).all()), tag


@pytest.mark.parametrize("name", ["A", "B", "J"])
def test_retained_graph_backward_twice_accumulates_twice_the_gradient(ops, name):
    """the second backward pass finds the kept logits and the hidden layers consumed: it recomputes them"""
    case = CASES[name]
    tun = dataclasses.replace(ops.TUNING, hpd_z_cache_bytes=1 << 40, hpd_z_cache_reserve=0)
    r = run(ops, name, tun, twice=True)
    check_trace(case, tun, r, twice=True)
    ref, bnd = data(name).grads(case, r.ti)
    for i, (g, gr, b_) in enumerate(zip(r.grads, ref, bnd)):
        close(g, 2 * gr, 0, 2 * b_, f"{name} backward twice grad[{i}]")


def test_ties_go_to_the_lower_index(ops):
    """case L: columns t and t + T/2 have identical weights and bias.  Their logits are bit-identical, and on every path the
    top-K takes t before t + T/2 (oracle/gngf_oracle.py topk_desc; the epilogue merge and the streaming pass both)"""
    name = "L"
    case, d = CASES[name], data(name)
    h = case.T // 2
    with torch.no_grad():
        ps = [p.to(DEV) for p in d.params]
        _, _, _, probs = ops.HpdVertexFunction.apply(case.NV, case.vstride, case.K, d.dev["mw"], True, case.rows * 4 * case.T,
                                                     None, *ps)
    assert torch.equal(probs[:, :h], probs[:, h:])
    saved = ops.TUNING
    for tun in (saved, dataclasses.replace(saved, hpd_epilogue_stats=False), dataclasses.replace(saved, hpd_gemm_split_bf16=False)):
        r = run(ops, name, tun)
        assert any(t["epi"] for t in r.trace) == (tun.hpd_epilogue_stats and tun.hpd_gemm_split_bf16)
        for row in r.ti.tolist():
            s = set(row)
            for t_ in row:
                if t_ >= h:
                    assert t_ - h in s, row
        check_values(name, r, f"L ties {tun.hpd_epilogue_stats}/{tun.hpd_gemm_split_bf16}")


# ------------------------------------------------------------------------------------------------ issue order and streams
# position of the rows argument of every per-chunk entry point (include/gngf.h)
ROWS_ARG = {"gngf_linear_fwd": 4, "gngf_linear_fwd_rowstats": 5, "gngf_rowstats_topk": 5, "gngf_pbar_accumulate": 5,
            "gngf_logits_topk_pbar": 7, "gngf_hpd_bwd_dot": 8, "gngf_softmax_bwd_lowrank": 10, "gngf_hpd_bwd_fused": 16,
            "gngf_linear_bwd_weight": 5, "gngf_gemm_acc": 3}
SIDE_FWD = {"gngf_rowstats_topk", "gngf_pbar_accumulate", "gngf_logits_topk_pbar"}
SIDE_BWD = {"gngf_hpd_bwd_dot", "gngf_softmax_bwd_lowrank"}


def _is_stage(name, args, T):
    """is this launch a per-chunk stage (a T-wide product or a pass over the logits), not a hidden layer of all vertices?"""
    if name not in ROWS_ARG:
        return False
    wide = {"gngf_linear_fwd": 5, "gngf_linear_bwd_weight": 6, "gngf_gemm_acc": 5}       # N, N, Kc
    return name not in wide or args[wide[name]] == T


def _stages(case, tun, rec):
    """what each chunk issues, stage by stage, from the documented dispatch rules: [(A, B, C)] per pass, lists of (entry, rows)"""
    nch = len(case.chunks)
    fwd, bwd = [], []
    for w, got in zip(expected_trace(case, tun), rec):
        n = w["n"]
        if w["pass_"] == "fwd":
            b = ["gngf_rowstats_topk"] + ["gngf_pbar_accumulate"] * bool(case.L) if w["epi"] else ["gngf_logits_topk_pbar"]
            fwd.append(([("gngf_linear_fwd_rowstats" if w["epi"] else "gngf_linear_fwd", n)], [(e, n) for e in b], []))
        else:
            c = ["gngf_hpd_bwd_fused"] if w["fused"] else ["gngf_linear_bwd_weight", "gngf_gemm_acc"]
            bwd.append(([] if got["kept"] else [("gngf_linear_fwd", n)],
                        [("gngf_hpd_bwd_dot" if w["fused"] else "gngf_softmax_bwd_lowrank", n)], [(e, n) for e in c]))
    assert len(fwd) == len(bwd) == nch
    return fwd, bwd


def _check_issue_order(case, tun, mode, trace, log):
    """log: (entry, rows or None, on the main stream?) per launch, with a ("backward", None, True) mark between the passes"""
    cut = log.index(("backward", None, True))
    passes = {"fwd": log[:cut], "bwd": log[cut + 1:]}
    stages = dict(zip(("fwd", "bwd"), _stages(case, tun, trace)))
    any_fused = any(t["fused"] for t in trace)
    assert [e for e, _, _ in log].count("gngf_hpd_bwd_prepare") == [e for e, _, _ in passes["bwd"]].count("gngf_hpd_bwd_prepare") \
        == int(any_fused)
    for ps, side_set in (("fwd", SIDE_FWD), ("bwd", SIDE_BWD)):
        got = [(e, n, m) for e, n, m in passes[ps] if n is not None]
        assert all(m for e, n, m in passes[ps] if n is None), passes[ps]           # hidden layers, planes: main stream
        if mode == "default":
            assert all(t["pipelined"] for t in trace)
            assert {e for e, _, m in got if not m} == {e for _, b, _ in stages[ps] for e, _ in b} <= side_set
            assert all((e in side_set) == (not m) for e, _, m in got), got
            want_side = [x for _, b, _ in stages[ps] for x in b]
            want_main, prev = [], []
            for a, _, c in stages[ps]:
                want_main += a + prev
                prev = c
            want_main += prev
            assert [(e, n) for e, n, m in got if not m] == want_side
            assert [(e, n) for e, n, m in got if m] == want_main
        else:
            assert not any(t["pipelined"] for t in trace)
            assert all(m for _, _, m in got), got
            assert [(e, n) for e, n, _ in got] == [x for a, b, c in stages[ps] for x in a + b + c]


ORDER_RUNS = {
    # z-cache off: every chunk of the backward pass has its A, whatever memory the device has free
    "B": ("B", dict(hpd_z_cache_bytes=0)),
    "D": ("D", dict(hpd_z_cache_bytes=0)),
    # the first chunk's logits are kept: it has no A in the backward pass
    "B_first_kept": ("B", dict(hpd_z_cache_bytes=CASES["B"].rows_eff * CASES["B"].T * 4, hpd_z_cache_reserve=0)),
}


@pytest.mark.parametrize("mode", ["default", "no_pipeline", "no_side_stream"])
@pytest.mark.parametrize("which", list(ORDER_RUNS))
def test_stages_are_issued_in_the_documented_order_on_the_documented_stream(ops, monkeypatch, which, mode):
    """Default tuning: A and C on the main stream in the order A0 A1 C0 A2 C1 ... C_last (a kept chunk has no A), B on the helper
    stream and nothing else there; gngf_hpd_bwd_prepare once per backward pass with a fused chunk, never otherwise.
    hpd_pipeline=False / use_side_stream=False: everything on the main stream, A_i B_i C_i per chunk."""
    name, kw = ORDER_RUNS[which]
    case = CASES[name]
    kw = dict(kw, **{"default": {}, "no_pipeline": dict(hpd_pipeline=False), "no_side_stream": dict(use_side_stream=False)}[mode])
    tun = dataclasses.replace(ops.TUNING, **kw)
    data(name)
    main = torch.cuda.current_stream()
    log, real_call, real_backward = [], ops.call, torch.autograd.backward

    def call(entry, *args):
        on_main = torch.cuda.current_stream().stream_id == main.stream_id
        log.append((entry, args[ROWS_ARG[entry]] if _is_stage(entry, args, case.T) else None, on_main))
        return real_call(entry, *args)

    def backward(*a, **k):
        log.append(("backward", None, True))
        return real_backward(*a, **k)
    monkeypatch.setattr(ops, "call", call)
    monkeypatch.setattr(torch.autograd, "backward", backward)
    r = run(ops, name, tun)
    assert torch.cuda.current_stream().stream_id == main.stream_id
    check_trace(case, tun, r)
    if which == "B_first_kept":
        assert [t["kept"] for t in r.trace[:len(case.chunks)]] == [True] + [False] * (len(case.chunks) - 1)
    _check_issue_order(case, tun, mode, r.trace, log)


# ------------------------------------------------------------------------------------------------ the kernel of every T-wide product
GEMM_ENTRIES = ("gngf_linear_fwd", "gngf_linear_bwd_weight", "gngf_gemm_acc")       # `gemm` is their argument before the stream


def _gemm_codes(tun):
    """(logits, accumulating dW / dh) codes of include/gngf.h: 0 exact fp32 without hpd_gemm_split_bf16; else hpd_gemm_kernel (1 three
    planes, 17 per wave), and 2 — two planes — for the accumulating products under hpd_bwd_two_planes with kernel 1"""
    if not tun.hpd_gemm_split_bf16:
        return 0, 0
    return tun.hpd_gemm_kernel, (2 if tun.hpd_bwd_two_planes and tun.hpd_gemm_kernel == 1 else tun.hpd_gemm_kernel)


def _logged_gemms(ops, monkeypatch, name, tun):
    log, real_call = [], ops.call

    def call(entry, *args):
        if entry in GEMM_ENTRIES:
            log.append((entry, args))
        return real_call(entry, *args)
    with monkeypatch.context() as m:
        m.setattr(ops, "call", call)
        run(ops, name, tun)
    return log


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("kw", [dict(), dict(hpd_gemm_split_bf16=False), dict(hpd_gemm_kernel=17), dict(hpd_bwd_two_planes=False)],
                         ids=["default", "fp32", "per_wave", "three_planes"])
def test_every_t_wide_product_names_its_kernel(ops, monkeypatch, kw, fused):
    """case B: the kernel of a product is an argument of its call.  Every per-chunk logits product carries the logits code, every
    per-chunk dW / dh product the accumulating code, every hidden-layer product 0 (exact fp32)."""
    case = CASES["B"]
    tun = dataclasses.replace(ops.TUNING, hpd_z_cache_bytes=0, hpd_bwd_fused=fused, **kw)
    logits, acc = _gemm_codes(tun)
    log = _logged_gemms(ops, monkeypatch, "B", tun)
    seen = {e: 0 for e in GEMM_ENTRIES}
    for entry, args in log:
        if _is_stage(entry, args, case.T):
            seen[entry] += 1
            assert args[-2] == (logits if entry == "gngf_linear_fwd" else acc), (entry, args[-2], logits, acc)
        else:
            assert args[-2] == 0, (entry, args[-2])
    # the chunks that issue them: logits again for every chunk of the backward (+ the forward's chunks without epilogue statistics);
    # dW and dh for the chunks the fused loaders do not take
    want = expected_trace(case, tun)
    n_logits = sum(1 for w in want if w["pass_"] == "bwd" or not w["epi"])
    n_acc = sum(1 for w in want if w["pass_"] == "bwd" and not w["fused"])
    assert n_acc >= 1 and seen == {"gngf_linear_fwd": n_logits, "gngf_linear_bwd_weight": n_acc, "gngf_gemm_acc": n_acc}, seen


@pytest.mark.parametrize("kw", [dict(), dict(hpd_gemm_kernel=17), dict(hpd_bwd_two_planes=False), dict(hpd_gemm_split_bf16=False)],
                         ids=["default", "per_wave", "three_planes", "fp32"])
def test_dense_pass_names_its_kernels(ops, monkeypatch, kw):
    """case J (dense distribution kept, dense gradient on it): the logits and dh carry hpd_gemm_kernel — three planes also under
    hpd_bwd_two_planes — while dW and the forward's p-bar product are exact fp32."""
    case = CASES["J"]
    tun = dataclasses.replace(ops.TUNING, **kw)
    code = tun.hpd_gemm_kernel if tun.hpd_gemm_split_bf16 else 0
    T, L, Hd, nch = case.T, case.L, case.widths[-1], len(case.chunks)
    got = {"logits": [], "pbar": [], "dW": [], "dh": []}
    for entry, args in _logged_gemms(ops, monkeypatch, "J", tun):
        if entry == "gngf_linear_fwd" and args[5] == T:
            got["logits"].append(args[-2])
        elif entry == "gngf_linear_bwd_weight" and args[6] == T:
            got["dW"].append(args[-2])
        elif entry == "gngf_gemm_acc" and (args[3], args[4]) == (L, T):
            got["pbar"].append(args[-2])
        elif entry == "gngf_gemm_acc":
            assert (args[4], args[5]) == (Hd, T), args[3:6]
            got["dh"].append(args[-2])
        else:
            assert args[-2] == 0, (entry, args[-2])                     # hidden layers
    assert got == {"logits": [code] * nch, "pbar": [0] * nch, "dW": [0] * nch, "dh": [code] * nch}, got
