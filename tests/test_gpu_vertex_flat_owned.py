"""GPU: the flat vertex backward that OWNS its rows (gngf_ext3_vertex_grid_bwd_flat_owned) and the row-clear rider of the pixel-stage
backward's launch (gngf_ext3_encode_tiled_bwd_clear_rows), through the C-ABI and through the model.

Kernel level: hand-made lists (sorted dest, seeded gi / w, a seeded int64 grid with its scale word).  The new entry runs on a buffer
pre-filled with the sentinel 123.0 whose crossing rows (ops.flat_crossing_rows, held to a numpy model in
tests/test_vertex_flat_owned_cpu.py) were zeroed by hand; gngf_vertex_grid_bwd_flat on a zeroed buffer is the reference.
  rows in no run             still the sentinel, bit for bit
  runs with <= 2 parts       bit for bit the adding kernel's result (same partial sums, same order; a two-term add commutes)
  runs with >= 3 parts       BOTH kernels within n 2^-24 sum|term| of the float64 sum of the run's n fp32 terms — the bound of
                             recursive fp32 summation in any order (derived, not measured); only case D has such rows
  repetition                 three calls on the same buffers, three grids, the last all zeros: each equals a fresh run
  poison                     every run's row NaN, every other row the sentinel
Model level: the smallest frozen-HPD model on the fused chain, VERTEX_BWD_OWNED = 1 against 0, graphed (unroll 2, cross_replay) and
eager; a rebuilt table; a held gradient; the signature's marker."""
import numpy as np
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = 2
BLOCK = 1024
SENTINEL = 123.0
VTOT = 3001
SCALE = 30


def ext3_entry_points():
    return ["gngf_ext3_vertex_grid_bwd_flat_owned", "gngf_ext3_encode_tiled_bwd_clear_rows"]


# ------------------------------------------------------------------------------------------------ kernel level
def _runs(lengths, first=2, step=3):
    return np.concatenate([np.full(n, first + step * k, dtype=np.int64) for k, n in enumerate(lengths)])


def _dest(case):
    rng = np.random.default_rng(101)
    if case == "A_one_ragged_workgroup":
        return np.sort(rng.integers(0, 300, size=884)), 300
    if case == "B_short_runs_nine_workgroups":
        return np.sort(rng.integers(0, 12000, size=8420)), 12000
    if case == "C_one_full_block":
        return _runs([300, 1, 723]), 16
    if case == "C_four_full_blocks":
        # run boundaries exactly on items 1024 and 3072; the run over item 2048 crosses
        return _runs([1000, 24, 500, 1100, 448, 1, 1023]), 32
    if case == "D_degenerate_table":
        return _runs([1296, 2500, 4624]), 16
    raise KeyError(case)


CASES = ["A_one_ragged_workgroup", "B_short_runs_nine_workgroups", "C_one_full_block", "C_four_full_blocks", "D_degenerate_table"]


def _parts(dest, rows):
    """per row: how many 1024-item blocks its run touches (0: in no run), and the run's length"""
    blocks = np.arange(len(dest)) // BLOCK
    first = np.full(rows, -1, dtype=np.int64)
    last = np.full(rows, -1, dtype=np.int64)
    np.maximum.at(last, dest, blocks)
    first[dest[::-1]] = blocks[::-1]
    n = np.bincount(dest, minlength=rows)
    return np.where(n > 0, last - first + 1, 0), n


def _grid(seed, zero=False, poison=0):
    q = np.zeros((VTOT, F), np.int64) if zero else np.random.default_rng(seed).integers(-2 ** 44, 2 ** 44, size=(VTOT, F)).astype(np.int64)
    return q, np.concatenate([q.reshape(-1), [SCALE, poison]]).astype(np.int64)


def _inputs(case):
    dest, rows = _dest(case)
    rng = np.random.default_rng(202)
    gi = rng.integers(0, VTOT, size=len(dest)).astype(np.int32)
    w = rng.random(len(dest), dtype=np.float32)
    return dest, rows, gi, w


def _call(name, gi, w, dest, n, dG64, dt, rows):
    from collision_handling_in_instantngp_amd import _lib
    p = _lib.ptr
    _lib.call(name, p(gi, torch.int32), p(w, torch.float32), p(dest, torch.int32), n, p(None), p(dG64, torch.int64), VTOT,
              p(dt, torch.float32), rows, F, _lib.stream_ptr())
    torch.cuda.synchronize()


def _terms(q, gi, w):
    """the items' fp32 values, formed as the kernels form them: (float)((double) q 2^-S) * w, the product rounded to fp32"""
    v = (q[gi].astype(np.float64) * 2.0 ** -SCALE).astype(np.float32)
    return (v * w[:, None]).astype(np.float32)


def _check(case, got, ref, q, dest, rows, gi, w):
    parts, n = _parts(dest, rows)
    sentinel = np.full((rows, F), SENTINEL, np.float32)
    assert np.array_equal(got[parts == 0].view(np.uint32), sentinel[parts == 0].view(np.uint32)), "a row in no run changed"
    few = (parts > 0) & (parts <= 2)
    bad = np.argwhere(got[few].view(np.uint32) != ref[few].view(np.uint32))
    assert bad.size == 0, (case, len(bad), got[few][tuple(bad[0])], ref[few][tuple(bad[0])])
    many = parts >= 3
    assert bool(many.any()) == case.startswith("D_"), (case, int(many.sum()))
    if many.any():
        t = _terms(q, gi, w).astype(np.float64)
        want, mass = np.zeros((rows, F)), np.zeros((rows, F))
        np.add.at(want, dest, t)
        np.add.at(mass, dest, np.abs(t))
        bound = n[:, None] * 2.0 ** -24 * mass
        for what, x in (("owned", got), ("adding", ref)):
            err = np.abs(x.astype(np.float64) - want)
            print(f"{case} {what}: worst error / bound over rows with >= 3 parts = {float((err[many] / np.maximum(bound[many], 1e-300)).max()):.2e}")
            assert bool((err[many] <= bound[many]).all()), (case, what)


def _owned_fresh(ins, g64):
    from collision_handling_in_instantngp_amd import ops
    dest, rows, gi, w = ins
    cross = ops.flat_crossing_rows(torch.as_tensor(dest)).to(DEV).long()
    dt = torch.full((rows, F), SENTINEL, dtype=torch.float32, device=DEV)
    dt[cross] = 0
    dev = [torch.as_tensor(a).to(DEV) for a in (gi, w, dest.astype(np.int32))]
    _call("gngf_ext3_vertex_grid_bwd_flat_owned", *dev, len(dest), torch.as_tensor(g64).to(DEV), dt, rows)
    return dt, dev, cross


def _adding(ins, g64):
    dest, rows, gi, w = ins
    dt = torch.zeros((rows, F), dtype=torch.float32, device=DEV)
    dev = [torch.as_tensor(a).to(DEV) for a in (gi, w, dest.astype(np.int32))]
    _call("gngf_vertex_grid_bwd_flat", *dev, len(dest), torch.as_tensor(g64).to(DEV), dt, rows)
    return dt.cpu().numpy()


def test_the_cases_are_what_they_say():
    d, _ = _dest("A_one_ragged_workgroup")
    assert len(d) == 884
    d, rows = _dest("B_short_runs_nine_workgroups")
    assert len(d) == 8420 and -(-len(d) // BLOCK) == 9 and rows == 12000
    assert int(np.bincount(d).max()) < BLOCK and int(_parts(d, rows)[0].max()) == 2          # no run has more than two parts
    d, _ = _dest("C_one_full_block")
    assert len(d) == BLOCK
    d, rows = _dest("C_four_full_blocks")
    assert len(d) == 4 * BLOCK and d[1023] != d[1024] and d[2047] == d[2048] and d[3071] != d[3072]
    assert int(_parts(d, rows)[0].max()) == 2
    d, rows = _dest("D_degenerate_table")
    assert sorted(np.bincount(d)[np.bincount(d) > 0]) == [1296, 2500, 4624]
    assert sorted(_parts(d, rows)[0][_parts(d, rows)[0] > 0]) == [2, 3, 6]


@pytest.mark.parametrize("case", CASES)
def test_owned_rows_equal_the_adding_kernel_and_other_rows_keep_the_sentinel(case):
    ins = _inputs(case)
    q, g64 = _grid(303)
    dt, _dev, _cross = _owned_fresh(ins, g64)
    _check(case, dt.cpu().numpy(), _adding(ins, g64), q, ins[0], ins[1], ins[2], ins[3])


@pytest.mark.parametrize("case", CASES)
def test_three_calls_on_the_same_buffers_each_equal_a_fresh_run(case):
    from collision_handling_in_instantngp_amd import ops
    ins = _inputs(case)
    dest, rows, gi, w = ins
    parts, _n = _parts(dest, rows)
    grids = [_grid(404), _grid(405), _grid(0, zero=True)]
    dt, dev, cross = _owned_fresh(ins, grids[0][1])
    for k, (q, g64) in enumerate(grids):
        if k:
            dt[cross] = 0                                            # what the rider does before every step
            _call("gngf_ext3_vertex_grid_bwd_flat_owned", *dev, len(dest), torch.as_tensor(g64).to(DEV), dt, rows)
        got = dt.cpu().numpy()
        fresh = _owned_fresh(ins, g64)[0].cpu().numpy()
        few = parts <= 2                                             # (rows in no run included: the sentinel)
        assert np.array_equal(got[few].view(np.uint32), fresh[few].view(np.uint32)), (case, k)
        _check(case, got, _adding(ins, g64), q, dest, rows, gi, w)
    # the all-zero grid: every run's row was overwritten with +0.0, stale values and all
    assert bool((got[parts > 0].view(np.uint32) == 0).all())


@pytest.mark.parametrize("case", ["B_short_runs_nine_workgroups", "D_degenerate_table"])
def test_poison_makes_every_runs_row_nan_and_leaves_the_sentinel_elsewhere(case):
    ins = _inputs(case)
    dest, rows, _gi, _w = ins
    _q, g64 = _grid(505, poison=1)
    got = _owned_fresh(ins, g64)[0].cpu().numpy()
    parts, _n = _parts(dest, rows)
    assert bool(np.isnan(got[parts > 0]).all())
    assert np.array_equal(got[parts == 0].view(np.uint32), np.full_like(got[parts == 0], SENTINEL).view(np.uint32))


def test_rejected_arguments_do_not_launch():
    from collision_handling_in_instantngp_amd import _lib
    ins = _inputs("A_one_ragged_workgroup")
    dest, rows, gi, w = ins
    p = _lib.ptr
    gi_t, w_t, d_t = (torch.as_tensor(a).to(DEV) for a in (gi, w, dest.astype(np.int32)))
    g = torch.zeros((VTOT * F + 2,), dtype=torch.int64, device=DEV)
    dt = torch.full((rows * F + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    for gi_, n, r, out in ((gi_t[1:], len(dest) - 1, rows, dt), (gi_t, 0, rows, dt), (gi_t, len(dest), 0, dt), (gi_t, len(dest), rows, dt[1:])):
        with pytest.raises(RuntimeError, match="hipErrorInvalidValue"):       # misaligned list, no items, no rows, misaligned rows
            _lib.call("gngf_ext3_vertex_grid_bwd_flat_owned", p(gi_), p(w_t), p(d_t), n, p(None), p(g), VTOT, p(out), r, F, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dt == SENTINEL).all())


def test_flat_owned_guarded_writes_its_runs_rows_and_nothing_else():
    """every buffer in a guard-band arena: the rows of runs are written (equal to the adding kernel's), rows in no run and the
    inputs keep their bytes, nothing lands next to a buffer"""
    from collision_handling_in_instantngp_amd import ops
    ins = _inputs("B_short_runs_nine_workgroups")
    dest, rows, gi, w = ins
    q, g64 = _grid(606)
    arena = guarded.Arena(4 << 20, DEV)
    a_gi, a_w, a_d = arena.put(gi, "item_gi"), arena.put(w, "item_w"), arena.put(dest.astype(np.int32), "item_dest")
    a_g = arena.put(g64, "dG64")
    dt = arena.take((rows, F), torch.float32, name="dtables")
    dt[ops.flat_crossing_rows(torch.as_tensor(dest)).to(DEV).long()] = 0
    _call("gngf_ext3_vertex_grid_bwd_flat_owned", a_gi, a_w, a_d, len(dest), a_g, dt, rows)
    arena.check()
    parts, _n = _parts(dest, rows)
    unwritten = guarded.unwritten(dt).cpu().numpy()
    assert bool(unwritten[parts == 0].all()) and not bool(unwritten[parts > 0].any())
    ref = _adding(ins, g64)
    assert np.array_equal(dt.cpu().numpy()[parts > 0].view(np.uint32), ref[parts > 0].view(np.uint32))
    for t, v in ((a_gi, gi), (a_w, w), (a_d, dest.astype(np.int32)), (a_g, g64)):
        assert guarded.same_bytes(t.cpu(), torch.as_tensor(v))


def test_tiled_bwd_clear_rows_guarded_zeroes_the_listed_rows_and_nothing_else():
    """the rider: the listed rows of clear_base are zero after the launch, every other row of it is unwritten, a negative row number
    is skipped, and the launch's own result (the fixed-point vertex grid) is, word for word, gngf_encode_tiled_bwd's"""
    from collision_handling_in_instantngp_amd import _lib, ops
    rng = np.random.default_rng(707)
    n_host, P, L = [16, 23, 33], 5000, 3
    plan = ops.EncodePlan(P, n_host, F, "tiled")
    assert plan.Ls == L and plan.interleaved(backward=True)
    xy = torch.as_tensor(rng.random((P, 2), dtype=np.float32)).to(DEV)
    n_ls = torch.as_tensor(np.array(n_host, np.int32)).to(DEV)
    genc = torch.as_tensor(rng.standard_normal((P, L * F)).astype(np.float32)).to(DEV)
    am = genc.abs().max().reshape(1)
    ws = ops.TiledWorkspace(plan, xy)
    R = 5000
    listed = np.sort(rng.choice(R, size=1500, replace=False)).astype(np.int32)          # two rider workgroups, the second ragged
    rows_np = np.concatenate([listed[:700], [-1], listed[700:]]).astype(np.int32)
    arena = guarded.Arena(4 << 20, DEV)
    base = arena.take((R, F), torch.float32, name="clear_base")
    rows_t = arena.put(rows_np, "clear_rows")
    g_new = arena.take((plan.vtot * F + 2,), torch.int64, fill=0, name="dG64")
    g_old = torch.zeros((plan.vtot * F + 2,), dtype=torch.int64, device=DEV)
    _lib.PROFILE = {}
    try:
        ops._pixel_bwd(plan, ws, n_ls, genc, None, L, F, absmax=(am, 1, 0), dG64=g_new, clear=(base, rows_t))
        ops._pixel_bwd(plan, ws, n_ls, genc, None, L, F, absmax=(am, 1, 0), dG64=g_old)
        torch.cuda.synchronize()
        names = list(_lib.PROFILE)
    finally:
        _lib.PROFILE = None
    assert names == ["gngf_ext3_encode_tiled_bwd_clear_rows", "gngf_encode_tiled_bwd"]
    arena.check()
    is_listed = np.zeros(R, bool)
    is_listed[listed] = True
    unwritten = guarded.unwritten(base).cpu().numpy()
    assert bool(unwritten[~is_listed].all())
    assert bool((base.cpu().numpy()[is_listed].view(np.uint32) == 0).all())
    assert guarded.same_bytes(rows_t.cpu(), torch.as_tensor(rows_np))
    assert bool(g_old.ne(0).any()) and torch.equal(g_new, g_old)
    # without rows the new entry is the old one; with rows and no buffer it is rejected
    with pytest.raises(RuntimeError, match="hipErrorInvalidValue"):
        ops._pixel_bwd(plan, ws, n_ls, genc, None, L, F, absmax=(am, 1, 0), dG64=g_old, clear=(None, rows_t))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ model level
P_MODEL = 20000
T_MODEL = 2 ** 12


def _model(seed=3):
    from collision_handling_in_instantngp_amd import models
    models.should_use_hash_function = False
    torch.manual_seed(seed)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T_MODEL, num_levels=8, n_min=16, n_max=128,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=T_MODEL, feature_dim=2, topk_k=4).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    for p in net.HPD.parameters():
        p.requires_grad = False
    net.compute_pbar = False
    return net


def _batches(n=4):
    gen = torch.Generator().manual_seed(4)
    X, Y = torch.rand((n * P_MODEL, 2), generator=gen).to(DEV), torch.rand((n * P_MODEL, 3), generator=gen).to(DEV)
    return [(X[b * P_MODEL:(b + 1) * P_MODEL].contiguous(), Y[b * P_MODEL:(b + 1) * P_MODEL].contiguous()) for b in range(n)]


class _Tap:
    """records every vertex-stage backward: the list, the fixed-point grid it read (a copy) and the table gradient it left (a copy)"""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from collision_handling_in_instantngp_amd import ops
        self.ops, self.inner = ops, ops._vertex_bwd
        tap = self

        def wrapped(plan, tables, vert_idx, vert_w, n_ls, vstride, dG, dtables, dvw, order=None, dG64=None, flat=None, mode=None, owned=False):
            grid = dG64.clone()
            tap.inner(plan, tables, vert_idx, vert_w, n_ls, vstride, dG, dtables, dvw, order, dG64, flat, mode, owned)
            tap.calls.append(dict(flat=flat, grid=grid, grad=dtables.clone(), owned=owned))
        ops._vertex_bwd = wrapped
        return self

    def __exit__(self, *exc):
        self.ops._vertex_bwd = self.inner


def _eager_steps(net, batches, hold=False):
    from collision_handling_in_instantngp_amd import train
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    empty = torch.tensor([], device=DEV)
    net.dp.persist_ok = True
    out = []
    for xy, tgt in batches:
        net.zero_grad(set_to_none=True)
        rgb, probs, _i, _c = net(xy, 1.0)
        mse, kls, coll = loss_fn(rgb, tgt, None, probs, empty, empty)
        loss = train.assemble_loss(mse, kls, coll, 1, 1, 1e-3)
        loss.backward()
        torch.cuda.synchronize()
        out.append(dict(rgb=rgb.detach().clone(), loss=loss.detach().clone(), sig=net.dp.step_config.signature(),
                        dec={k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and not k.startswith("encoding.")}))
    return out


def _graphed_steps(net, batches):
    from collision_handling_in_instantngp_amd import train
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    gs = train.GraphedStep(net, loss_fn, None, 1, 1, 1e-3, unroll=2, cross_replay=True)
    out = []
    for k in range(0, len(batches), 2):
        pair = batches[k:k + 2]
        nxt = batches[k + 2][0] if k + 2 < len(batches) else None
        rs = gs.run_many(pair, next_first=nxt)
        torch.cuda.synchronize()
        sig = net.dp.step_config.signature()
        dec = {k_: p.grad.clone() for k_, p in net.named_parameters() if p.grad is not None and not k_.startswith("encoding.")}
        out += [dict(rgb=r.out.clone(), loss=r.loss.clone(), sig=sig, dec=dec if j == 1 else None) for j, r in enumerate(rs)]
    return out


def _run(kind, owned, n=4):
    from collision_handling_in_instantngp_amd import ops
    prev = ops.VERTEX_BWD_OWNED
    ops.VERTEX_BWD_OWNED = owned
    try:
        net = _model()
        with _Tap() as tap:
            steps = (_graphed_steps if kind == "graphed" else _eager_steps)(net, _batches(n))
        torch.cuda.synchronize()
    finally:
        ops.VERTEX_BWD_OWNED = prev
    return net, steps, tap.calls


def _compare_table_grads(new, old):
    """the rule of the kernel cases, per recorded vertex stage: bitwise where a row's run has at most two parts, elsewhere both
    within n 2^-24 sum|term| of the float64 sum of the run's fp32 terms"""
    assert new["owned"] and not old["owned"]
    assert torch.equal(new["grid"], old["grid"])                       # exact integer sums: the same words in both runs
    flat = new["flat"]
    rows = flat.Ls * flat.T
    dest = flat.dest.cpu().numpy().astype(np.int64)
    parts, n = _parts(dest, rows)
    a = new["grad"].reshape(-1, F)[:rows].cpu().numpy()
    b = old["grad"].reshape(-1, F)[:rows].cpu().numpy()
    few = parts <= 2
    assert bool((a[parts == 0].view(np.uint32) == 0).all())
    assert np.array_equal(a[few].view(np.uint32), b[few].view(np.uint32))
    many = ~few
    if many.any():
        g = new["grid"].cpu().numpy()
        q, scale, poison = g[:-2].reshape(-1, F), int(g[-2]), int(g[-1])
        assert poison == 0
        v = (q[flat.gi.cpu().numpy()].astype(np.float64) * 2.0 ** -scale).astype(np.float32)
        t = (v * flat.w.cpu().numpy()[:, None]).astype(np.float32).astype(np.float64)
        want, mass = np.zeros((rows, F)), np.zeros((rows, F))
        np.add.at(want, dest, t)
        np.add.at(mass, dest, np.abs(t))
        bound = n[:, None] * 2.0 ** -24 * mass
        for x in (a, b):
            assert bool((np.abs(x.astype(np.float64) - want)[many] <= bound[many]).all())
    return int(many.sum())


@pytest.mark.parametrize("kind", ["graphed", "eager"])
def test_consecutive_steps_equal_the_parent_chain(kind):
    _net, new, taps_new = _run(kind, 1)
    _net0, old, taps_old = _run(kind, 0)
    assert all("bin=pipeline vfwd=fused" in s["sig"] and " vbwd=flat" in s["sig"] for s in new + old), new[0]["sig"]
    assert all(s["sig"].endswith(" rows=owned") for s in new) and not any("rows=owned" in s["sig"] for s in old)
    # (the graphed run records its warm-up and capture passes as well: the same number in both runs)
    assert len(taps_new) == len(taps_old) >= len(new) >= 3
    for a, b in zip(taps_new, taps_old):
        _compare_table_grads(a, b)
    for a, b in zip(new, old):
        assert guarded.same_bytes(a["rgb"], b["rgb"]) and guarded.same_bytes(a["loss"], b["loss"])
        if a["dec"] is not None:
            assert a["dec"].keys() == b["dec"].keys() and len(a["dec"]) >= 6
            assert all(guarded.same_bytes(a["dec"][k], b["dec"][k]) for k in a["dec"])


def test_a_rebuilt_table_leaves_no_row_of_the_old_list_behind():
    from collision_handling_in_instantngp_amd import ops
    assert ops.VERTEX_BWD_OWNED == 1
    net = _model()
    batches = _batches(2)
    _eager_steps(net, batches[:1])
    assert net.dp.step_config.owned_rows
    old_list = net.dp.owned_for
    old_rows = torch.unique(old_list.dest.long())
    assert bool(net.dp.owned_grad.reshape(-1, F)[old_rows].ne(0).any())
    with torch.no_grad():
        gen = torch.Generator().manual_seed(9)
        for p in net.HPD.parameters():
            p.add_(0.5 * torch.randn(p.shape, generator=gen).to(DEV))
    _eager_steps(net, batches[1:])
    new_list = net.dp.owned_for
    assert net.dp.step_config.owned_rows and new_list is not old_list
    gone = old_rows[~torch.isin(old_rows, torch.unique(new_list.dest.long()))]
    assert gone.numel() > 0
    grad = torch.stack([p.grad for p in net.dp.level_params]).reshape(-1, F)
    assert bool((grad[gone].view(torch.int32) == 0).all())


def test_a_held_gradient_sends_the_next_step_down_the_parent_chain():
    """the level parameters keep .grad of step 1 while step 2 runs: step 2 takes the parent's chain (a cleared allocation of its
    own), so no kernel writes the held tensors — torch accumulates step 2's gradient into them, as it does for any .grad that is
    kept: held == step 1's + step 2's, exactly"""
    from collision_handling_in_instantngp_amd import ops, train
    net = _model()
    (x1, y1), (x2, y2) = _batches(2)
    _eager_steps(net, [(x1, y1)])
    assert net.dp.step_config.owned_rows
    held = [p.grad for p in net.dp.level_params]
    before = [g.clone() for g in held]
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    empty = torch.tensor([], device=DEV)
    ops.STEP_TRACE = []
    try:
        with _Tap() as tap:
            rgb, probs, _i, _c = net(x2, 1.0)                                # no zero_grad: the gradients of step 1 are kept
            mse, kls, coll = loss_fn(rgb, y2, None, probs, empty, empty)
            train.assemble_loss(mse, kls, coll, 1, 1, 1e-3).backward()
            torch.cuda.synchronize()
        trace = list(ops.STEP_TRACE)
    finally:
        ops.STEP_TRACE = None
    sigs = [f["signature"] for what, f in trace if what == "step_config"]
    assert len(sigs) == 1 and " vbwd=flat" in sigs[0] and "rows=owned" not in sigs[0]
    assert [f["source"] for what, f in trace if what == "table_grad"] == ["forward_alloc"]
    assert len(tap.calls) == 1 and not tap.calls[0]["owned"]
    g2 = tap.calls[0]["grad"]
    for l, (g, b) in enumerate(zip(held, before)):
        assert net.dp.level_params[l].grad is g
        assert guarded.same_bytes(g, b + g2[l])


def test_the_signature_carries_the_marker_in_the_owned_case_only():
    from collision_handling_in_instantngp_amd import ops
    net = _model()
    batch = _batches(1)
    _eager_steps(net, batch)
    assert net.dp.step_config.signature().endswith(" vbwd=flat rows=owned")
    net.dp.persist_ok = False                                               # a loop that did not opt in
    net.zero_grad(set_to_none=True)
    rgb, *_ = net(batch[0][0], 1.0)
    assert net.dp.step_config.signature().endswith(" vbwd=flat")
    prev, ops.VERTEX_BWD_OWNED = ops.VERTEX_BWD_OWNED, 0
    try:
        net.dp.persist_ok = True
        rgb, *_ = net(batch[0][0], 1.0)
        assert net.dp.step_config.signature().endswith(" vbwd=flat")
    finally:
        ops.VERTEX_BWD_OWNED = prev
