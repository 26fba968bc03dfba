"""GPU: d vert_w — the gradient of the encoder with respect to the per-vertex blend weights, the one quantity that carries the
training signal from the pixels to a trainable HPD — of EVERY branch of ops.EncodeFunction.backward, held to the float64 oracle
(oracle/dvw_oracle.py) entry by entry, within the bound the error model of tests/test_encode_dw_cpu.py derives from the kernels
(check_vertex_weight_grad: relative to the entry's own absolute mass; entries no pixel reaches exactly zero).  The branches:

  A  0 < Ls < L: vertex_bwd_sorted_kernel writes into a buffer of its own, the direct levels' atomics go to a zeroed one, summed
  B  Ls == L: vertex_bwd_sorted_kernel writes d vert_w itself
  C  only vert_w wants a gradient (no slot order is computed): vertex_bwd_kernel, one float atomic per (level, vertex, k)
  D  Ls == 0: encode_bwd_kernel, one float atomic per (pixel, corner, k), the dot product over the feature lanes by __shfl_xor
  E  a model-level pass whose decoder hands over the bound on |d enc|: the pixel stage fills the fixed-point grid (sink "dG64"),
     it is converted to fp32 and the sorted kernel reads that copy (FROM64 = false)
  F  as E with a data-parallel exchange set up: the exchange sees the fp32 grid, the vertex stage is not deferred

Op level (ops.encode_apply, injected vertex table, chosen d enc): two passes per case on a NaN-poisoned allocator, the second on
another batch of the same P crowded into the [0, 1/8)^2 corner, so that most vertices the first pass reached must come back exactly
zero.  The table gradient of the same passes goes through check_rows_against_oracle of tests/test_gpu_step_config_matrix.py.  Model
level (branches E, F): a GeneralNeuralGaugeFields with a trainable, freshly initialised HPD; vert_idx, vert_w, its gradient and d enc
are captured by spies on ops.encode_apply / ops.decoder_apply."""
import types

import numpy as np
import pytest
import torch

from oracle import c_oracle
from test_encode_dw_cpu import (DW_SHAPES, SUBRECT, check_vertex_weight_grad, dvw_error_model, fixed_point_scale, make_case)
from test_gpu_bench_chain import _poison_allocator
from test_gpu_step_config_matrix import _step, _table_grad, check_rows_against_oracle

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not c_oracle.available(), reason="oracle/libgngf_oracle_c.so not built (make -C oracle)")]
DEV = "cuda"


def t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _sink(trace):
    """the sink of the staged levels' pixel-stage launch (ops.PIXEL_BWD_TRACE).  "dG64" first: with d vert_w wanted the launch that
    fills the fixed-point grid ALSO writes its fp32 copy (branches E, F), which staged_sink of the matrix test would name"""
    sinks = {"dG64" if r["dG64"] else "fp32_grid" if r["fp32_grid"] else None for r in trace}
    assert len(sinks) == 1 and None not in sinks, trace
    return sinks.pop()


class _BackwardSpy:
    """records the vertex-stage and direct-form launches of the backward passes inside it (ops._vertex_bwd / ops._direct_bwd) and the
    pixel-stage launch records (ops.PIXEL_BWD_TRACE): which branch of EncodeFunction.backward produced d vert_w"""

    def __init__(self, ops):
        self.ops, self.calls, self.trace = ops, [], []

    def __enter__(self):
        ops = self.ops
        self._prev = (ops._vertex_bwd, ops._direct_bwd, ops.PIXEL_BWD_TRACE)
        real_v, real_d = ops._vertex_bwd, ops._direct_bwd

        def vertex(plan, tables, vert_idx, vert_w, n_ls, vstride, dG, dtables, dvw, order=None, dG64=None):
            self.calls.append(("vertex", dict(sorted=vert_idx is not None and order is not None, dvw=dvw, fp32_grid=dG is not None,
                                              from64=dG64 is not None)))
            return real_v(plan, tables, vert_idx, vert_w, n_ls, vstride, dG, dtables, dvw, order, dG64)

        def direct(xy, tables, vert_idx, vert_w, n_ls, genc, dtables, dvw, *a, **kw):
            self.calls.append(("direct", dict(dvw=dvw)))
            return real_d(xy, tables, vert_idx, vert_w, n_ls, genc, dtables, dvw, *a, **kw)
        ops._vertex_bwd, ops._direct_bwd, ops.PIXEL_BWD_TRACE = vertex, direct, self.trace
        return self

    def __exit__(self, *exc):
        self.ops._vertex_bwd, self.ops._direct_bwd, self.ops.PIXEL_BWD_TRACE = self._prev

    def branch(self):
        """"A" | "B" | "C" | "D" of the module docstring ("E" / "F" are A / B with the sink "dG64" in the trace: test_branches_E_F_learning_mode_step)"""
        v = [c for k, c in self.calls if k == "vertex"]
        d = [c for k, c in self.calls if k == "direct"]
        assert len(v) <= 1 and len(d) <= 1, self.calls
        assert all(c["dvw"] is not None for c in v + d), "a launch of the backward was not asked for d vert_w"
        if not v:
            return "D"
        if not v[0]["sorted"]:
            return "C"
        if d:
            assert v[0]["dvw"] is not d[0]["dvw"], "the sorted kernel WRITES d vert_w: the direct levels need a buffer of their own"
            return "A"
        return "B"


def _check_pass(ops, tag, case, b, got_dvw, got_dt, Ls, sink, chunk, branch, prev, tables_np=None, vidx=None, vw=None, min_stale=1):
    """d vert_w (and, got_dt given, the table gradient) of pass b of `case` against the float64 oracles.  prev: (n of the previous
    pass, its term_counts) or None.  -> (n, term_counts)"""
    x, genc = case["x"][b], case["genc"][b]
    tables_np = case["tables"] if tables_np is None else tables_np
    vidx_np = case["vidx"]
    L, F, T = case["L"], case["F"], case["T"]
    S = fixed_point_scale(genc, case["P"], chunk)
    want, mass, n, rel, quant = dvw_error_model(x, case["n_ls"], genc, tables_np, vidx_np, case["vstride"], Ls, sink if Ls else "none", S)
    got = got_dvw.detach().double().cpu().numpy()
    assert got.shape == (case["NV"], case["K"])
    check_vertex_weight_grad(tag, got, want, mass, n, rel, quant, L, F, branch)
    # vertices of the table outside every level's grid (none when the table is sized by the batch's own extent) hold exactly zero
    vid = np.arange(case["NV"])
    outside = np.maximum(vid % case["vstride"], vid // case["vstride"]) > int(case["n_ls"][-1]) + 1
    assert (n[outside] == 0).all() and (got[outside] == 0).all(), (tag, "a vertex outside every level grid is not exactly zero")
    if prev is not None:
        stale = (prev[0] > 0) & (n == 0)
        assert int(stale.sum()) >= 1, (tag, "no vertex was reached by the previous pass only")
        assert (got[stale] == 0).all(), (tag, "vertices only the previous pass reached are not exactly zero", int((got[stale] != 0).sum()))
    counts = None
    if got_dt is not None:
        counts = check_rows_against_oracle(tag, got_dt, t(x), genc, case["n_ls"], T, F, Ls, sink if Ls else "none", "vertex_table", chunk,
                                           vidx, vw, case["vstride"], prev_counts=None if prev is None else prev[1], min_stale=min_stale)
    return n, counts


def _run_case(ops, name, want_branch, kind="uniform", fp16=False, subrect=False, tables_grad=True, second_backward=False):
    case = make_case(name, kind=kind, fp16=fp16, subrect=subrect)
    L, F, P = case["L"], case["F"], case["P"]
    plan = ops.EncodePlan(P, case["n_host"], F)
    chunk = getattr(plan, "chunk", 0)
    n_t = t(case["n_ls"], torch.int32)
    vi = t(case["vidx"], torch.int32)
    tag0 = f"{name}-{kind}" + ("-fp16" if fp16 else "") + ("-subrect" if subrect else "") + ("" if tables_grad else "-frozen tables")
    sink_obj = None
    if fp16 and tables_grad:
        # fp16 storage: the fp32 accumulation buffer itself is handed over (what train.FusedAdam consumes), not its fp16 rounding
        levels = tuple(torch.zeros((), device=DEV, requires_grad=True) for _ in range(L))
        sink_obj = (types.SimpleNamespace(), levels)
    _poison_allocator()
    prev = None
    for b in (0, 1):
        tt = t(case["tables"]).requires_grad_(tables_grad)
        tw = t(case["vw"]).requires_grad_()
        xb, gb = t(case["x"][b]), t(case["genc"][b])
        passes = (1, 2) if (second_backward and b == 0) else (1,)
        enc = ops.encode_apply(xb, n_t, case["n_host"], tt, vi, tw, case["vstride"], sink=sink_obj)
        for rep in passes:
            tag = f"{tag0} pass {b + 1}" + (" second backward" if rep == 2 else "")
            for w in (tt, tw):
                w.grad = None
            if sink_obj is not None:
                for w in sink_obj[1]:
                    w.grad_fp32 = None
            with _BackwardSpy(ops) as spy:
                enc.backward(gb, retain_graph=rep < len(passes))
                torch.cuda.synchronize()
            branch = spy.branch()
            assert branch == want_branch, f"{tag}: expected branch {want_branch} of EncodeFunction.backward, branch {branch} ran"
            if plan.Ls:
                assert len(spy.trace) == 1 and spy.trace[0]["Ls"] == plan.Ls and spy.trace[0]["interleaved"] == plan.interleaved(backward=True)
                assert _sink(spy.trace) == "fp32_grid", spy.trace      # (no bound on |d enc| at op level)
            else:
                assert not spy.trace
            got_dt = None
            if tables_grad:
                got_dt = torch.stack([w.grad_fp32 for w in sink_obj[1]]) if sink_obj is not None else tt.grad
                assert got_dt.dtype == torch.float32
            degenerate = kind != "uniform"
            out = _check_pass(ops, tag, case, b, tw.grad, got_dt, plan.Ls, "fp32_grid", chunk, branch, None if rep == 2 else prev,
                              vidx=vi, vw=tw.detach(), min_stale=0 if degenerate else 1)
        prev = out
    return plan


@pytest.fixture(scope="module")
def ops():
    from collision_handling_in_instantngp_amd import ops as o
    return o


@pytest.mark.parametrize("name", ["direct_f1", "direct_f2", "direct_f4", "direct_k1", "direct_k7"])
def test_branch_D_direct_form_only(ops, name):
    """encode_bwd_kernel at every feature width (the lane-shuffle dot), K = 1 and K = 7; P L F is no multiple of the block size"""
    L, _a, _b, F, _T, _K, P = DW_SHAPES[name]
    assert (P * L * F) % 256 != 0
    plan = _run_case(ops, name, "D")
    assert plan.Ls == 0, "branch D wants no staged level"


@pytest.mark.parametrize("name,kind,subrect", [("staged", "uniform", False), ("staged", "one_slot", False), ("staged", "few_slots", False),
                                               ("staged", "k_equal", False), ("staged_k1", "uniform", False), ("staged_k7", "uniform", False),
                                               ("staged", "uniform", True)])
def test_branch_B_sorted_kernel_writes_the_gradient(ops, name, kind, subrect):
    plan = _run_case(ops, name, "B", kind=kind, subrect=subrect)
    assert plan.Ls == DW_SHAPES[name][0] and plan.interleaved(backward=True), "branch B wants every level staged, interleaved"


@pytest.mark.parametrize("kind,subrect", [("uniform", False), ("one_slot", False), ("few_slots", False), ("k_equal", False), ("uniform", True)])
def test_branch_A_sorted_kernel_plus_direct_levels(ops, kind, subrect):
    plan = _run_case(ops, "mixed", "A", kind=kind, subrect=subrect)
    assert 0 < plan.Ls < DW_SHAPES["mixed"][0] and plan.interleaved(backward=True), "branch A wants staged AND direct levels"


def test_branch_A_second_backward_through_the_same_graph(ops):
    """the forward pass's buffers are consumed by the first backward: the second one allocates its own and meets the same bound"""
    plan = _run_case(ops, "mixed", "A", second_backward=True)
    assert 0 < plan.Ls < DW_SHAPES["mixed"][0]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32_tables", "fp16_tables"])
def test_branch_B_generic_kernels_fp32_grid(ops, fp16):
    """F = 4: the generic pixel-stage kernels; fp16 tables: tload of __half rows inside the dot products, oracle on the stored values"""
    plan = _run_case(ops, "generic", "B", fp16=fp16)
    assert plan.Ls == DW_SHAPES["generic"][0] and not plan.interleaved(backward=True), "the generic kernels are wanted here"


def test_branch_C_unsorted_kernel_when_only_vert_w_wants_a_gradient(ops):
    plan = _run_case(ops, "staged", "C", tables_grad=False)
    assert plan.Ls == DW_SHAPES["staged"][0]


# ------------------------------------------------------------------------------------------------ model level: branches E and F
MODEL_SHAPES = {      # name: (L, F, T, n_min, n_max, P)
    "cfg1": (4, 2, 256, 8, 32, 57404),
    "l16": (16, 2, 2 ** 12, 16, 512, 2 ** 14),
}


def _learning_net(models, name):
    L, F, T, n_min, n_max, P = MODEL_SHAPES[name]
    models.should_use_hash_function = False
    torch.manual_seed(17)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T, num_levels=L, n_min=n_min, n_max=n_max,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=T, feature_dim=F, topk_k=4).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    net.compute_pbar = False
    with torch.no_grad():
        net.encoding.packed_tables().mul_(100.0)
    assert not net.hpd_is_frozen()
    return net


def _learning_step(net, ops, xy, target, fused):
    """one training step (_step of the matrix test) with spies: -> dict(vidx, vw, vstride, tables, dvw, genc) and the _BackwardSpy"""
    cap, gencs = {}, []
    real_enc, real_dec = ops.encode_apply, ops.decoder_apply

    def spy_enc(x, n_ls, n_host, tables, vert_idx, vert_w, vstride, **kw):
        cap.update(vidx=vert_idx.detach().clone(), vw=vert_w.detach().clone(), vstride=int(vstride), tables=tables.detach().clone())
        vert_w.register_hook(lambda g: cap.__setitem__("dvw", g.detach().clone()))
        return real_enc(x, n_ls, n_host, tables, vert_idx, vert_w, vstride, **kw)

    def spy_dec(enc, *a, **kw):
        enc.register_hook(lambda g: gencs.append(g.detach().clone()))
        return real_dec(enc, *a, **kw)
    ops.encode_apply, ops.decoder_apply = spy_enc, spy_dec
    try:
        with _BackwardSpy(ops) as spy:
            _step(net, ops, xy, target, fused)
    finally:
        ops.encode_apply, ops.decoder_apply = real_enc, real_dec
    assert len(gencs) == 1 and "dvw" in cap, (len(gencs), sorted(cap))
    cap["genc"] = np.ascontiguousarray(gencs[0].float().cpu().numpy())
    return cap, spy


@pytest.mark.parametrize("name,decoder,dpstate", [("cfg1", "fused_loss", "single"), ("cfg1", "plain", "single"),
                                                  ("l16", "fused_loss", "single"), ("l16", "fused_loss", "exchange")])
def test_branches_E_F_learning_mode_step(name, decoder, dpstate):
    from collision_handling_in_instantngp_amd import models, ops
    L, F, T, n_min, n_max, P = MODEL_SHAPES[name]
    prev_tuning = ops.TUNING
    try:
        net = _learning_net(models, name)
        n_ls = np.array(net._n_ls_host, np.int32)
        plan = ops.EncodePlan(P, [int(n) for n in n_ls], F)
        assert plan.Ls > 0 and plan.interleaved(backward=True)
        g = torch.Generator(device=DEV).manual_seed(29)
        xy1 = torch.rand((P, 2), device=DEV, generator=g)
        xy2 = torch.rand((P, 2), device=DEV, generator=g) * torch.tensor(SUBRECT, device=DEV)     # step 2: a sub-rectangular table
        targets = [torch.rand((P, 3), device=DEV, generator=g) for _ in range(2)]
        exchanged = []
        if dpstate == "exchange":
            net.dp.exchange = lambda grid: exchanged.append(tuple(grid.shape))       # one rank: the mean over the ranks is the tensor itself
        _poison_allocator()
        for k, (xb, tb) in enumerate(((xy1, targets[0]), (xy2, targets[1]))):
            tag = f"learning {name}-{decoder}-{dpstate} step {k + 1}"
            del exchanged[:]
            cap, spy = _learning_step(net, ops, xb, tb, decoder == "fused_loss")
            vstride, NV = cap["vstride"], cap["vidx"].shape[0]
            if k == 1:
                assert vstride < n_max + 2 and NV // vstride < vstride, (vstride, NV)
            sink = _sink(spy.trace)
            if decoder == "fused_loss":
                assert sink == "dG64", f"{tag}: the fused decoder hands over the bound on |d enc|: sink dG64 expected, {sink} ran"
            v = [c for kk, c in spy.calls if kk == "vertex"]
            assert len(v) == 1 and v[0]["sorted"] and v[0]["dvw"] is not None, spy.calls
            branch = spy.branch()                                                # "A" | "B": how the sorted kernel's sum meets the direct levels'
            if sink == "dG64":
                # d vert_w wanted: the fixed-point grid is not read directly — converted to fp32 first, FROM64 = false
                assert v[0]["fp32_grid"] and not v[0]["from64"], spy.calls
                model_branch = "F" if dpstate == "exchange" else "E"
                assert model_branch == ("F" if exchanged else "E"), (tag, exchanged)
                if model_branch == "F":
                    assert exchanged == [(plan.vtot, F)] and net.dp.deferred is None, "branch F: exchanged in line, vertex stage not deferred"
                branch = f"{model_branch} ({branch} on the fp32 copy of dG64)"
            case = dict(x=(np.ascontiguousarray(xb.cpu().numpy()),), genc=(cap["genc"],), tables=cap["tables"].float().cpu().numpy(),
                        vidx=np.ascontiguousarray(cap["vidx"].cpu().numpy().astype(np.int32)), L=L, F=F, T=T, K=4, P=P, n_ls=n_ls,
                        vstride=vstride, NV=NV)
            _check_pass(ops, tag, case, 0, cap["dvw"], _table_grad(net, L), plan.Ls, sink, plan.chunk, branch, None,
                        vidx=cap["vidx"], vw=cap["vw"])
    finally:
        ops.TUNING = prev_tuning
        models.should_use_hash_function = False
