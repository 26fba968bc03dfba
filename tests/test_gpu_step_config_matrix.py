"""GPU: ONE case of every kernel chain ops.StepConfig.choose can reach (the enumeration of tests/test_step_config_cpu.py: nine shapes
x two index sources x two decoder forms x three data-parallel states) is RUN through the model for TWO training steps — forward,
loss, backward, `p.grad = None` in between as a loop's zero_grad does — on a NaN-poisoned allocator, and held to the C oracle
(oracle/gngf_oracle_c.c) on both steps:
  * rgb, the MSE value and the six decoder gradients (encode_fwd, decoder_fwd, the MSE gradient, decoder_bwd);
  * EVERY row of the table gradient, every level, staged and direct, against the double-precision sum of the exact terms of the
    d enc the step itself produced (captured by a spy on ops.decoder_apply; c_oracle.encode_bwd_f64(..., exact_products=True)),
    within a bound relative to the row's absolute mass that the error model below gives for the path the row's sum took;
  * every entry whose mass is zero — no pixel reaches it, or (step 2) only step 1's batch did — EXACTLY zero.
Step 2's batch has the same P (same plan, same chain) but all its pixels in the [0, 1/8)^2 corner: most rows step 1 wrote are not
reached by it, so the clears these chains rely on (the binning riders, the training decoder, the sparse `rows` clear of the
step-to-step buffer) must have run, and the binning sees a few very heavy tiles.  The chain that ran is asserted on both steps
(ops.SEEN_STEP_CONFIGS).  Step 1 is also compared, as before, with the same step through the direct form (one lane per (pixel,
level), float atomics); that comparison cannot see a fault in the direct levels' own kernel (both passes run it) and, for the
vertex-table source, only bounds the error to 5e-3 of the largest row: the oracle check is the one that holds the chain.

  decoder form "fused_loss": net.fused_mse(target, gloss=1) — the one-launch training decoder at 32 encoder features (it clears the
      gradient block), the two-kernel decoder whose backward clears at 64; "plain": MSELoss outside, the binning riders clear.
  data-parallel state "exchange": a vertex-grid exchange is set up (here the identity on one rank: the kernels are the same as
      with two — tests/test_gpu_parallel.py runs real ranks); "single+persist_ok": the loop's owner allows the step-to-step buffer.
  vertex-table source: a frozen HPD whose per-vertex (slot, weight) table is injected (uniform random slots): evaluating a real HPD
      over the 16.8 M vertices of the 4096^2 shape against 2^22 slots is learning-mode work, not what this test is about.

Error model of one table-gradient entry (u = 2^-24; A = the entry's absolute mass, sum |g c (w)| over its terms, from
encode_bwd_f64 of |d enc|; n = the row's number of (pixel, corner[, k]) terms, a bincount of the indices):
  staged levels — the sink the pixel-stage launch reports (ops.PIXEL_BWD_TRACE):
    hash source, exact 64-bit per-item / per-vertex sums rounded to fp32 once and added to the row ("table_rows", or the fixed-point
        vertex grid "dG64" read by the vertex stage): 4e-7 A (a row adds a few such sums; measured on the bench chain)
    vertex-table source reading the fixed-point grid ("dG64"): 4e-6 A (the (vertex, k) entries of a row meet through a segmented
        scan, a chain across waves and float atomics: tens of roundings; measured on the bench's gngf_frozen chain)
    "fp32_grid" (item sums added to an fp32 vertex grid, then to the rows): (n + 2) u A — an fp32 sum of at most n terms in any
        order, the rounding of the products included
    + for all three, the fixed-point quantisation: at most 2^-(S+1) per term, n 2^-(S+1), for the launch's scale
        S = 60 - max(10, log2_chunk) - e (csrc/encode_tiled.hip), e the exponent of the bound on |d enc|; taken here one lower than
        the max of the captured d enc gives (the bound handed over may sit a binade above it) and log2_chunk = ceil log2 max(P, chunk)
  direct levels (float atomics of fp32 products, or the bucketed form's 64-bit sums rounded once): (n + 2) u A + n 2^-50 G_l, G_l
        the level's largest |d enc| (the bucketed form's quantum is 2^-50 of its bucket's largest term, csrc/encode_bucket.hip)"""
import math

import numpy as np
import pytest
import torch

from conftest import PARITY, parity_close
from oracle import c_oracle
from test_gpu_bench_chain import _numpy_state, _poison_allocator
from test_step_config_cpu import SHAPES, _reachable

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
STAGED_REL = {("hash", "table_rows"): 4e-7, ("hash", "dG64"): 4e-7, ("vertex_table", "dG64"): 4e-6}     # else (n + 2) u
STEP2_SIDE = 0.125              # step 2's pixels all lie in [0, STEP2_SIDE)^2
DECODER_GRADS = ["mlp.0.0.weight", "mlp.0.0.bias", "mlp.1.0.weight", "mlp.1.0.bias", "mlp.2.0.weight", "mlp.2.0.bias"]

_REACH = _reachable()
CASES = sorted((chain, cases[0]) for chain, cases in _REACH.items())


def _build(models, ops, name, source):
    L, F, T, n_min, n_max, fp32, P = SHAPES[name]
    models.should_use_hash_function = source == "hash"
    torch.manual_seed(17)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T, num_levels=L, n_min=n_min, n_max=n_max,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=T, feature_dim=F, topk_k=4,
                                          table_dtype=(torch.float32 if fp32 else torch.float16)).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    with torch.no_grad():
        net.encoding.packed_tables().mul_(100.0)
    if source != "hash":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
        vstride = n_max + 2
        NV, K = vstride * vstride, 4
        g = torch.Generator(device=DEV).manual_seed(5)
        ti = torch.randint(0, T, (NV, K), device=DEV, generator=g, dtype=torch.int32)
        tv = torch.rand((NV, K), device=DEV, generator=g) * 0.5 + 1e-3
        blend = ops.BLEND_CODES[True]
        w = ops.BlendFunction.apply(tv, blend)
        key = (tuple((p.data_ptr(), p._version) for p in net.HPD.flat_params()), blend, net._topk_k)
        net._frozen_table = (key, tv, ti, w, vstride, NV, ops.slot_order(ti, net._n_ls_host, vstride))
    return net, (L, F, T, P, fp32)


def _table_grad(net, L):
    out = []
    for l in range(L):
        w = net.encoding._hash_tables[l].weight
        g = getattr(w, "grad_fp32", None)
        out.append((g if g is not None else w.grad).float())
    return torch.stack(out).clone()


def _step(net, ops, xy, target, fused):
    """one training step: gradients let go first (zero_grad), forward, loss, backward -> (rgb, loss value)"""
    for p in net.parameters():
        p.grad = None
        if getattr(p, "grad_fp32", None) is not None:
            p.grad_fp32 = None
    if fused:
        with net.fused_mse(target, gloss=1.0):
            rgb, _p, _i, _c = net(xy, 1.0)
        loss = ops.mse_loss(rgb, target)
    else:
        rgb, _p, _i, _c = net(xy, 1.0)
        loss = torch.nn.functional.mse_loss(rgb, target)
    loss.backward()
    torch.cuda.synchronize()
    return rgb.detach().clone(), float(loss.detach())


def _case_step(net, ops, chain, xy, target, fused):
    """_step on the case's own chain, with the d enc it produces captured by a spy on ops.decoder_apply (a tensor hook on the
    encoder output): -> (rgb, loss, d enc (P, L F) float32 numpy, the pixel-stage launch records).  Asserts that the chain ran."""
    captured, trace = [], []
    real = ops.decoder_apply

    def spy(enc, *a, **kw):
        enc.register_hook(lambda g: captured.append(g.detach().clone()))
        return real(enc, *a, **kw)
    seen = ops.SEEN_STEP_CONFIGS if ops.SEEN_STEP_CONFIGS is not None else set()
    ops.SEEN_STEP_CONFIGS = mine = set()
    prev_trace, ops.PIXEL_BWD_TRACE = ops.PIXEL_BWD_TRACE, trace
    ops.decoder_apply = spy
    try:
        rgb, loss = _step(net, ops, xy, target, fused)
    finally:
        ops.decoder_apply = real
        ops.PIXEL_BWD_TRACE = prev_trace
        seen.update(mine)
        ops.SEEN_STEP_CONFIGS = seen if seen is not mine else None
    assert mine == {chain}, f"expected {chain!r} (with the d enc spy in place), the pass took {sorted(mine)}"
    assert len(captured) == 1, len(captured)
    return rgb, loss, np.ascontiguousarray(captured[0].float().cpu().numpy()), trace


def term_counts(xy, n_ls, T, vidx=None, vstride=0):
    """(L, T) int32 on the GPU: the number of (pixel, corner[, k]) terms that reach each table row — the same cell and hash
    (models.py _scale_to_grid / _fast_hash: int32 wrap-around of the prime product, non-negative remainder) or vertex slot as
    oracle/gngf_oracle_c.c, computed with torch ops"""
    out = torch.zeros((len(n_ls), T), dtype=torch.int32, device=xy.device)
    x, y = xy[:, 0].contiguous(), xy[:, 1].contiguous()
    for l, n in enumerate(n_ls):
        ax, ay = torch.floor(x * float(n)).long(), torch.floor(y * float(n)).long()
        for v in range(4):
            gx, gy = ax + (v & 1), ay + (v >> 1)
            if vidx is None:
                s = (gy * 2654435761) & 0xFFFFFFFF
                s = torch.where(s >= 2 ** 31, s - 2 ** 32, s)
                rows = torch.remainder(gx ^ s, T)
            else:
                rows = vidx[gy * vstride + gx].reshape(-1).long()
            out[l] += torch.bincount(rows, minlength=T).int()
    return out


def staged_sink(trace, source):
    """the sink the staged levels' backward used, from the pixel-stage launch records (ops.PIXEL_BWD_TRACE)"""
    sinks = set()
    for r in trace:
        sinks.add("fp32_grid" if r["fp32_grid"] else "dG64" if r["dG64"] else "table_rows" if r["direct_hash"] else None)
    assert len(sinks) == 1 and None not in sinks, trace
    return sinks.pop()


def _oracle_table_grad_f64(x_np, n_ls, genc, T, F, vidx=None, vw=None, vstride=0):
    """(want, mass): c_oracle.encode_bwd_f64(..., exact_products=True) of d enc and of |d enc|.  Vertex-table source: per level,
    the float64 per-vertex sums first (the same call with the identity as the slot table), then their products with the blend
    weights summed per slot by np.bincount (sequential float64) — the same double-precision sum in another order.  (A trained
    HPD sends a million (vertex, k) entries to a few dozen rows: per-term double atomics on those rows would serialise.)"""
    L = len(n_ls)
    if vidx is None:
        return tuple(c_oracle.encode_bwd_f64(x_np, (L, T, F), n_ls, g, exact_products=True) for g in (genc, np.abs(genc)))
    P, (NV, K) = x_np.shape[0], vidx.shape
    ident, ones = np.arange(NV, dtype=np.int32)[:, None], np.ones((NV, 1), np.float32)
    want, mass = np.zeros((L, T, F), np.float64), np.zeros((L, T, F), np.float64)
    for l in range(L):
        g_l = np.ascontiguousarray(genc.reshape(P, L, F)[:, l, :])
        gv, gm = (c_oracle.encode_bwd_f64(x_np, (1, NV, F), n_ls[l:l + 1], g, ident, ones, vstride, exact_products=True)[0]
                  for g in (g_l, np.abs(g_l)))
        nz = np.flatnonzero(gm.sum(1) > 0)                       # the vertices this batch reaches at this level
        rows, w = vidx[nz].ravel(), vw[nz].astype(np.float64)
        for f in range(F):
            want[l, :, f] = np.bincount(rows, weights=(gv[nz, f, None] * w).ravel(), minlength=T)
            mass[l, :, f] = np.bincount(rows, weights=(gm[nz, f, None] * w).ravel(), minlength=T)
        del gv, gm
    return want, mass


def check_rows_against_oracle(tag, got, xy, genc, n_ls, T, F, Ls, sink, source, chunk, vidx=None, vw=None, vstride=0,
                              prev_counts=None, min_stale=1):
    """Every entry of the (L, T, F) table gradient `got` (a GPU tensor) against c_oracle.encode_bwd_f64 of the step's own d enc
    `genc`, within the bound of the module docstring's error model; entries of mass zero exactly zero.  prev_counts: term_counts
    of the previous step's batch — rows it reached and this batch does not are counted (at least `min_stale` of them) and must be
    zero.  Prints and records the worst |err| / mass and |err| / bound per level group; returns this batch's term_counts."""
    L = len(n_ls)
    P = xy.shape[0]
    n_ls = np.ascontiguousarray(n_ls, np.int32)
    x_np = np.ascontiguousarray(xy.cpu().numpy())
    vidx_np = None if vidx is None else np.ascontiguousarray(vidx.cpu().numpy().astype(np.int32))
    vw_np = None if vw is None else np.ascontiguousarray(vw.detach().float().cpu().numpy())
    want, mass = _oracle_table_grad_f64(x_np, n_ls, genc, T, F, vidx_np, vw_np, vstride)
    counts = term_counts(xy, [int(n) for n in n_ls], T, vidx, vstride)
    g_level = np.abs(genc.reshape(P, L, F)).max(axis=(0, 2)).astype(np.float64)
    e = math.frexp(float(g_level.max()))[1] + 1 if g_level.max() > 0 else 0
    S = 60 - max(10, (max(P, chunk) - 1).bit_length()) - e
    q_staged = 2.0 ** -(S + 1)
    groups = {}            # name -> [worst |err| / mass, worst |err| / bound, entries checked]
    n_bad = n_empty_nonzero = n_stale = n_stale_zero = 0
    bad = []
    for l in range(L):
        g = got[l].double()
        assert tuple(g.shape) == (T, F)
        assert bool(torch.isfinite(g).all()), f"{tag}: level {l}: non-finite table gradient (NaN-poisoned allocator)"
        w = torch.from_numpy(want[l]).to(DEV)
        m = torch.from_numpy(mass[l]).to(DEV)
        n = counts[l].double()[:, None]
        if l < Ls:
            grp = "staged/" + sink
            rel = STAGED_REL.get((source, sink))
            bound = (rel if rel is not None else (n + 2) * U) * m + n * q_staged
        else:
            grp = "direct"
            bound = (n + 2) * U * m + n * (2.0 ** -50 * g_level[l])
        err = (g - w).abs()
        pos = m > 0
        over = pos & (err > bound)
        if bool(over.any()):
            n_bad += int(over.sum())
            r = int(torch.nonzero(over)[0, 0])
            bad.append(f"level {l} row {r}: got {g[r].tolist()} want {w[r].tolist()} mass {m[r].tolist()} n {int(n[r, 0])} "
                       f"bound {bound[r].tolist()}")
        n_empty_nonzero += int((~pos & (g != 0)).sum())
        if bool(pos.any()):
            st = groups.setdefault(grp, [0.0, 0.0, 0])
            st[0] = max(st[0], float((err[pos] / m[pos]).max()))
            st[1] = max(st[1], float((err[pos] / bound[pos]).max()))
            st[2] += int(pos.sum())
        if prev_counts is not None:
            stale = (prev_counts[l] > 0) & (counts[l] == 0)
            n_stale += int(stale.sum())
            n_stale_zero += int((g[stale] == 0).all(dim=1).sum())
        del g, w, m, n, bound, err, pos, over
    del want, mass
    line = "; ".join(f"{k}: worst |err|/mass {v[0]:.2e}, |err|/bound {v[1]:.2f} ({v[2]} entries)" for k, v in sorted(groups.items()))
    stale_txt = "" if prev_counts is None else f"; {n_stale_zero} of {n_stale} rows only the previous batch reached exactly zero"
    print(f"[{tag}] table gradient vs float64 oracle: {line}{stale_txt}")
    for k, v in sorted(groups.items()):
        PARITY.record(f"{tag}: table gradient, {k} levels: |err| / (bound of the error model), every entry with mass > 0",
                      np.array([v[1]]), np.zeros(1), 0, 1.0)
    assert n_bad == 0, (tag, n_bad, bad[:4])
    assert n_empty_nonzero == 0, (tag, "entries no term reaches are not exactly zero", n_empty_nonzero)
    if prev_counts is not None:
        assert n_stale >= min_stale, (tag, "no row was reached by the previous batch only", n_stale)
        assert n_stale_zero == n_stale, (tag, n_stale, n_stale_zero)
    return counts


def check_step_against_oracle(tag, net, L, xy, target, rgb, loss, vidx=None, vw=None, vstride=0):
    """rgb, the MSE value and the six decoder gradients of the step that just ran, against the C oracle"""
    tables, dw, db = _numpy_state(net, L)          # (fp16 storage: the stored values, converted to fp32)
    n_ls = np.array(net._n_ls_host, np.int32)
    x_np, y_np = np.ascontiguousarray(xy.cpu().numpy()), np.ascontiguousarray(target.cpu().numpy())
    vidx_np = None if vidx is None else np.ascontiguousarray(vidx.cpu().numpy().astype(np.int32))
    vw_np = None if vw is None else np.ascontiguousarray(vw.detach().float().cpu().numpy())
    enc = c_oracle.encode_fwd(x_np, tables, n_ls, vidx_np, vw_np, vstride)
    rgb_o, h1, h2 = c_oracle.decoder_fwd(enc, dw, db)
    parity_close(rgb, rgb_o, 0, 1e-5, f"{tag}: rgb vs C oracle")
    parity_close(loss, float(np.mean((rgb_o.astype(np.float64) - y_np) ** 2)), 1e-5, 0, f"{tag}: MSE value vs C oracle")
    drgb = ((2.0 / rgb_o.size) * (rgb_o - y_np)).astype(np.float32)
    _genc, gdec = c_oracle.decoder_bwd(enc, h1, h2, rgb_o, drgb, dw)
    # A decoder gradient is a sum over all P pixels, and both sides round it in fp32: its error scales with the sum of the terms'
    # magnitudes, not with the result.  Where the terms cancel (a flat decoder, random targets) that mass is orders of magnitude
    # above the gradient itself, so the absolute tolerance is 2e-5 of the largest mass (= the largest |gradient| when nothing
    # cancels; a pixel block left out moves a gradient by ~ block / P of its mass, far above it).
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float64)      # noqa: E731
    y64 = t(rgb_o)
    dz3 = t(drgb) * y64 * (1 - y64)
    dz2 = (dz3 @ t(dw[2])) * (t(h2) > 0)
    dz1 = (dz2 @ t(dw[1])) * (t(h1) > 0)
    masses = [dz1.abs().T @ t(enc).abs(), dz1.abs().sum(0), dz2.abs().T @ t(h1).abs(), dz2.abs().sum(0), dz3.abs().T @ t(h2).abs(),
              dz3.abs().sum(0)]
    params = dict(net.named_parameters())
    for nm, wg, ms in zip(DECODER_GRADS, gdec, masses):
        scale = max(float(np.abs(wg).max()), float(ms.max())) + 1e-30
        parity_close(params[nm].grad, wg, 1e-3, 2e-5 * scale, f"{tag}: grad {nm} vs C oracle")
    del dz1, dz2, dz3, masses


@pytest.mark.skipif(not c_oracle.available(), reason="oracle/libgngf_oracle_c.so not built (make -C oracle)")
@pytest.mark.parametrize("chain,case", CASES, ids=[f"{c[1][0]}-{c[1][1]}-{c[1][2]}-{c[1][3]}" for c in CASES])
def test_every_reachable_chain_runs_and_matches_the_direct_form(chain, case):
    from collision_handling_in_instantngp_amd import models, ops
    name, source, decoder, dpstate = case
    fused = decoder == "fused_loss"
    prev_tuning = ops.TUNING
    try:
        net, (L, F, T, P, fp32) = _build(models, ops, name, source)
        ops.FP16_TABLE_GRAD_FP32 = not fp32
        g = torch.Generator(device=DEV).manual_seed(23)
        xy = torch.rand((P, 2), device=DEV, generator=g)
        target = torch.rand((P, 3), device=DEV, generator=g)
        xy2 = torch.rand((P, 2), device=DEV, generator=g) * STEP2_SIDE       # step 2: same P, every pixel in one corner
        target2 = torch.rand((P, 3), device=DEV, generator=g)
        n_ls = np.array(net._n_ls_host, np.int32)
        chunk = getattr(ops.EncodePlan(P, [int(n) for n in n_ls], F), "chunk", 0)     # (no staged level: no chunk)
        vidx = vw = None
        vstride = 0
        if source != "hash":
            _key, _tv, vidx, vw, vstride = net._frozen_table[:5]
        # ---- the case's own configuration, two steps
        net.dp.persist_ok = dpstate == "single+persist_ok"
        if dpstate == "exchange":
            net.dp.exchange = lambda t: None            # one rank: the mean over the ranks is the tensor itself
        _poison_allocator()
        prev_counts = None
        for k, (xb, tb) in enumerate(((xy, target), (xy2, target2))):
            tag = f"{name}-{source}-{decoder}-{dpstate} step {k + 1}"
            rgb_k, loss_k, genc, trace = _case_step(net, ops, chain, xb, tb, fused)
            got = _table_grad(net, L)
            if k == 0:
                rgb, got1 = rgb_k, got
            check_step_against_oracle(tag, net, L, xb, tb, rgb_k, loss_k, vidx, vw, vstride)
            Ls = trace[0]["Ls"] if trace else 0
            sink = staged_sink(trace, source) if trace else "none"
            prev_counts = check_rows_against_oracle(tag, got, xb, genc, n_ls, T, F, Ls, sink, source, chunk, vidx, vw, vstride,
                                                    prev_counts=prev_counts)
            del got
        # ---- step 1 again through the direct form, single rank, loss outside
        net.dp.exchange = None
        net.dp.persist_ok = False
        ops.ENCODE_PATH = "direct"
        hold = ops.SEEN_STEP_CONFIGS
        ops.SEEN_STEP_CONFIGS = None                    # (the comparison pass is not this test's chain)
        try:
            rgb_ref, _loss = _step(net, ops, xy, target, fused=False)
        finally:
            ops.SEEN_STEP_CONFIGS = hold
        want = _table_grad(net, L)
        assert bool(torch.isfinite(got1).all()) and float(want.abs().max()) > 0
        assert float((rgb - rgb_ref).abs().max()) <= 2e-6
        mx = float(want.abs().max())
        # (vertex-table source: several vertices — each with up to thousands of pixels at the coarse levels — meet in one table row, and the
        # DIRECT form adds them one float atomic per (pixel, corner, k) in whatever order: its own fp32 accumulation error on rows whose
        # sum is far below their absolute mass is what the looser bound covers.  This agreement only guards against gross faults; the
        # row-by-row comparison with the float64 oracle above is what holds every chain, the direct levels' own kernels included)
        tol = (2e-5 if source == "hash" else 5e-3) * mx
        err = float((got1 - want).abs().max())
        print(f"[{chain}] table gradient vs the direct form: max |err| {err / mx:.2e} of the largest")
        assert err <= tol, (err / mx, chain)
    finally:
        ops.TUNING = prev_tuning
        models.should_use_hash_function = False
