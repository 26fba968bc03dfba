"""GPU: the vertex stage backward over the static item list of a frozen vertex table (gngf_vertex_grid_bwd_flat, through the C-ABI)
against numpy evaluations of  dtables[l*T + vert_idx[vid,k]] += vert_w[vid,k] * g[goff[l] + gy*(n_l+2) + gx]  enumerated directly
from (vert_idx, vert_w, n_ls) — not from the list.

  exact    w in {1, 2}, small integers in the fixed-point grid (scale 0) and in the pre-filled dtables: every fp32 sum is exact in
           any order, so the result equals the int64 evaluation BIT FOR BIT — an item dropped or counted twice at a thread, wave
           or workgroup boundary shows.
  rounded  random w, random 64-bit grid: |got - float64 sum| <= (n_run + 2) 2^-24 sum|w g| per (row, f) — the recursive-summation
           bound, valid for any order (one rounding of g to fp32, one of the product, n_run - 1 adds) — also on the fp32 grid.
  poison   flag set: every touched row is NaN, no other row changes.

Shapes: n_ls = (16, 23, 33), K = 4 -> 8 696 items: 8.5 workgroups of 1024 items, no multiple of any chunk; (14, 30) -> 5 120 items
= 5 whole workgroups; K = 1 / 3 -> 2 174 / 6 522 items (ragged ends of the 16-byte loads).  Slots: one slot (one run per level
across all workgroups), ~40 slots (long runs ending at arbitrary lanes), uniform over T = 64 / 2048 / 2^19 (runs of ~45, of 1-3, of 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = 2
BASE = (16, 23, 33)


def _table(n_ls, K, T, slots, seed, exact):
    rng = np.random.default_rng(seed)
    vstride = max(n_ls) + 2
    NV = vstride * vstride
    if slots == "one":
        vi = np.full((NV, K), 5 % T, dtype=np.int32)
    elif slots == "forty":
        vi = rng.choice(rng.permutation(T)[:40], size=(NV, K)).astype(np.int32)
    else:
        vi = rng.integers(0, T, size=(NV, K)).astype(np.int32)
    w = rng.integers(1, 3, size=(NV, K)).astype(np.float32) if exact else rng.random((NV, K), dtype=np.float32)
    return vi, w, vstride


def _enumerate(n_ls, vstride, vi, K, T):
    """(gi, vid, dest) of every (l, vertex, k), straight from the definition"""
    gi, vid, lv, goff = [], [], [], 0
    for l, n in enumerate(n_ls):
        gw = n + 2
        gy, gx = np.divmod(np.arange(gw * gw, dtype=np.int64), gw)
        gi.append(goff + gy * gw + gx)
        vid.append(gy * vstride + gx)
        lv.append(np.full(gw * gw, l, dtype=np.int64))
        goff += gw * gw
    gi, vid, lv = (np.concatenate(a) for a in (gi, vid, lv))
    dest = lv[:, None] * T + vi[vid].astype(np.int64)                      # (vtot, K)
    return np.repeat(gi, K), np.repeat(vid, K), dest.reshape(-1), goff


def _launch(lst, dG, dG64, dt, rows):
    from collision_handling_in_instantngp_amd import _lib
    _lib.call("gngf_vertex_grid_bwd_flat", _lib.ptr(lst.gi, torch.int32), _lib.ptr(lst.w, torch.float32), _lib.ptr(lst.dest, torch.int32),
              lst.n, _lib.ptr(dG), _lib.ptr(dG64, torch.int64), lst.vtot, _lib.ptr(dt, torch.float32), rows, F, _lib.stream_ptr())
    torch.cuda.synchronize()


def _list(n_ls, K, T, slots, seed, exact):
    from collision_handling_in_instantngp_amd import ops
    vi, w, vstride = _table(n_ls, K, T, slots, seed, exact)
    lst = ops.vertex_flat_list(torch.as_tensor(vi).to(DEV), torch.as_tensor(w).to(DEV), list(n_ls), vstride, T)
    gi, vid, dest, vtot = _enumerate(n_ls, vstride, vi, K, T)
    assert lst.n == gi.size == vtot * K and lst.vtot == vtot
    wk = w[vid, np.tile(np.arange(K), vtot)]
    return lst, gi, wk, dest, vtot


CASES = [  # n_ls, K, T, slots
    (BASE, 4, 64, "one"), (BASE, 4, 64, "forty"), (BASE, 4, 64, "uniform"), (BASE, 4, 2048, "uniform"), (BASE, 4, 2 ** 19, "uniform"),
    ((14, 30), 4, 64, "forty"), ((14, 30), 4, 2048, "uniform"),
    (BASE, 1, 64, "forty"), (BASE, 1, 2048, "uniform"), (BASE, 3, 64, "forty"), (BASE, 3, 2048, "uniform"), (BASE, 3, 64, "one"),
]
IDS = [f"n{'_'.join(map(str, c[0]))}-K{c[1]}-T{c[2]}-{c[3]}" for c in CASES]


def test_shapes_cover_whole_and_ragged_workgroups():
    items = {c: sum((n + 2) ** 2 for n in c[0]) * c[1] for c in CASES}
    assert items[CASES[0]] == 8696 and 8696 % 1024 != 0 and 8696 // 1024 >= 4
    assert items[CASES[5]] == 5120 and 5120 % 1024 == 0
    assert items[CASES[7]] % 4 != 0 and items[CASES[9]] % 4 != 0           # ragged ends of the four-item loads


@pytest.mark.parametrize("n_ls,K,T,slots", CASES, ids=IDS)
def test_exact_sums_equal_int64_evaluation_bit_for_bit(n_ls, K, T, slots):
    lst, gi, wk, dest, vtot = _list(n_ls, K, T, slots, 11, exact=True)
    rng = np.random.default_rng(12)
    rows = len(n_ls) * T
    q = rng.integers(-8, 9, size=(vtot, F)).astype(np.int64)
    pre = rng.integers(-4, 5, size=(rows, F)).astype(np.int64)
    want = pre.copy()
    np.add.at(want, dest, wk.astype(np.int64)[:, None] * q[gi])
    assert int(np.abs(want).max()) < 2 ** 24 and int((np.abs(wk[:, None] * q[gi])).sum(0).max()) < 2 ** 24      # exact in fp32, any order
    dG64 = torch.as_tensor(np.concatenate([q.reshape(-1), [0, 0]])).to(DEV)                                       # scale 0, not poisoned
    dt = torch.as_tensor(pre.astype(np.float32)).to(DEV)
    _launch(lst, None, dG64, dt, rows)
    got = dt.cpu().numpy()
    bad = np.argwhere(got != want.astype(np.float32))
    assert bad.size == 0, (len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    # the fp32 grid as the source: the same integers
    dt2 = torch.as_tensor(pre.astype(np.float32)).to(DEV)
    _launch(lst, torch.as_tensor(q.astype(np.float32)).to(DEV), None, dt2, rows)
    assert np.array_equal(dt2.cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("n_ls,K,T,slots", CASES, ids=IDS)
def test_rounded_sums_within_the_recursive_summation_bound(n_ls, K, T, slots):
    lst, gi, wk, dest, vtot = _list(n_ls, K, T, slots, 21, exact=False)
    rng = np.random.default_rng(22)
    rows = len(n_ls) * T
    S = 30
    q = rng.integers(-2 ** 44, 2 ** 44, size=(vtot, F)).astype(np.int64)
    n_run = np.bincount(dest, minlength=rows).astype(np.float64)

    def check(g64, got, what):
        terms = wk.astype(np.float64)[:, None] * g64[gi]
        want, mass = np.zeros((rows, F)), np.zeros((rows, F))
        np.add.at(want, dest, terms)
        np.add.at(mass, dest, np.abs(terms))
        bound = (n_run[:, None] + 2) * 2.0 ** -24 * mass
        err = np.abs(got.astype(np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300))[mass > 0].max())
        print(f"{what}: worst error / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (what, worst)
        assert bool((got[mass == 0] == 0).all())

    dG64 = torch.as_tensor(np.concatenate([q.reshape(-1), [S, 0]])).to(DEV)
    dt = torch.zeros((rows, F), dtype=torch.float32, device=DEV)
    _launch(lst, None, dG64, dt, rows)
    check(q.astype(np.float64) * 2.0 ** -S, dt.cpu().numpy(), "fixed-point grid")
    g32 = rng.standard_normal((vtot, F)).astype(np.float32)
    dt2 = torch.zeros((rows, F), dtype=torch.float32, device=DEV)
    _launch(lst, torch.as_tensor(g32).to(DEV), None, dt2, rows)
    check(g32.astype(np.float64), dt2.cpu().numpy(), "fp32 grid")


@pytest.mark.parametrize("slots,T", [("one", 64), ("forty", 64), ("uniform", 2048)])
def test_poison_flag_makes_every_touched_row_nan(slots, T):
    lst, gi, wk, dest, vtot = _list(BASE, 4, T, slots, 31, exact=False)
    rows = len(BASE) * T
    q = np.random.default_rng(32).integers(-2 ** 40, 2 ** 40, size=(vtot, F)).astype(np.int64)
    dG64 = torch.as_tensor(np.concatenate([q.reshape(-1), [30, 1]])).to(DEV)
    dt = torch.zeros((rows, F), dtype=torch.float32, device=DEV)
    _launch(lst, None, dG64, dt, rows)
    got = dt.cpu().numpy()
    touched = np.bincount(dest, minlength=rows) > 0
    assert touched.any() and bool(np.isnan(got[touched]).all()) and bool((got[~touched] == 0).all())


def test_rejected_arguments_do_not_launch():
    from collision_handling_in_instantngp_amd import _lib
    lst, *_ = _list(BASE, 4, 64, "forty", 41, exact=True)
    dt = torch.zeros((3 * 64, F), dtype=torch.float32, device=DEV)
    g = torch.zeros((lst.vtot, F), dtype=torch.float32, device=DEV)
    p = _lib.ptr
    for gi_, n, rows in ((lst.gi[1:], lst.n - 1, 192), (lst.gi, 0, 192), (lst.gi, lst.n, 0)):       # misaligned list, no items, no rows
        with pytest.raises(RuntimeError, match="hipErrorInvalidValue"):
            _lib.call("gngf_vertex_grid_bwd_flat", p(gi_), p(lst.w), p(lst.dest), n, p(g), p(None), lst.vtot, p(dt), rows, F, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dt == 0).all())


def test_graphed_step_with_the_flat_vertex_stage_equals_eager_steps():
    """One captured train.GraphedStep of a frozen-HPD model, replayed for three different batches, against the three eager steps (the
    tolerance of tests/test_gpu_model.py's replay test: float atomics arrive in any order, everything else is the same arithmetic).  The
    captured launches read the item list from buffers that live with the model's frozen table: same addresses before and after."""
    from collision_handling_in_instantngp_amd import models, ops, train
    assert ops.VERTEX_BWD_FLAT == 1
    models.should_use_hash_function = False
    torch.manual_seed(3)
    T = 2 ** 12
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T, num_levels=8, n_min=16, n_max=128,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=T, feature_dim=2, topk_k=4).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    for p in net.HPD.parameters():
        p.requires_grad = False
    net.compute_pbar = False
    gen = torch.Generator().manual_seed(4)
    P = 20000
    X, Y = torch.rand((3 * P, 2), generator=gen).to(DEV), torch.rand((3 * P, 3), generator=gen).to(DEV)
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    gs = train.GraphedStep(net, loss_fn, None, 1, 1, 1e-3)
    ptrs = None
    empty = torch.tensor([], device=DEV)
    for b in range(3):
        xy, tgt = X[b * P:(b + 1) * P].contiguous(), Y[b * P:(b + 1) * P].contiguous()
        net.zero_grad(set_to_none=True)
        rgb, probs, _i, _c = net(xy, 1.0)
        mse, kls, coll = loss_fn(rgb, tgt, None, probs, empty, empty)
        train.assemble_loss(mse, kls, coll, 1, 1, 1e-3).backward()
        assert net.dp.step_config.vertex_bwd_flat, net.dp.step_config.signature()
        eager = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        eager_rgb = rgb.detach().clone()
        r = gs(xy, tgt)
        torch.cuda.synchronize()
        assert net.dp.step_config.vertex_bwd_flat
        lists = net._frozen_table[6].flat_lists._lists
        assert lists and all(v is not None for v in lists.values())
        now = sorted((Ls, v.gi.data_ptr(), v.w.data_ptr(), v.dest.data_ptr()) for Ls, v in lists.items())
        assert ptrs is None or now == ptrs
        ptrs = now
        assert torch.equal(r.out, eager_rgb)
        assert any(k.startswith("encoding.") for k in eager)
        for k, p in net.named_parameters():
            if k in eager:
                scale = float(eager[k].abs().max()) + 1e-30
                assert float((p.grad - eager[k]).abs().max()) <= 2e-5 * scale, (b, k)
    assert len(gs._graphs) == 1
