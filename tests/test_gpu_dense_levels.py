"""GPU: the dense-where-it-fits index source (GNGF_MODE_DENSE_HASH, models.GeneralNeuralGaugeFields(dense_levels=True)): a level
whose vertex grid fits the table, (N_l + 2)^2 <= T, is indexed one-to-one — row gy (N_l + 2) + gx — and only finer levels are hashed.

Expected values come from the oracle's own pieces (scale_to_grid, spatial_hash, encoding_forward / _backward, bilinear_*, decoder_*)
on an index array formed HERE by that rule (dense_hash_idx).  Shapes: L = 4, N = 8, 12, 20, 32 and
T = 512 (three dense levels, one hashed), 484 = 22^2 (N = 20 just fits), 483 (it just does not), 500 (not a power of two),
64 (nothing dense), 2048 (everything dense).  Every case fails without the feature: mode 2 is hipErrorInvalidValue there, and the
constructor has no dense_levels keyword."""
import numpy as np
import pytest
import torch

from oracle import gngf_oracle as orc

import test_gpu_render as tr

pytestmark = pytest.mark.gpu

DEV = "cuda"
from dense_levels_helpers import L, N_LS, N_MAX, N_MIN, cfg, dense_hash_idx, oracle_model
TS = (512, 484, 483, 500, 64, 2048)
PS = (1, 257, 4099)


def t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)      # (a copy: the cached oracle arrays are read-only)


def close(a, b, rtol, atol, msg):
    from conftest import parity_close
    parity_close(a, b, rtol, atol, msg)


@pytest.fixture(scope="module")
def ops():
    from collision_handling_in_instantngp_amd import ops as o
    return o


def coords(P, rng):
    x = rng.random((P, 2), dtype=np.float32)
    edge = np.array([[1, 1], [0, 0], [0, 1], [1, 0], [0.5, 0.5], [1 / 32, 31 / 32], [0.99999994, 1e-8]], np.float32)[:P]
    x[: len(edge)] = edge
    return x


_CASES = {}


def case(P, T, F, fp16):
    """inputs and oracle values of one shape, computed once and never modified.
    The upstream gradient is |N(0, 1)|: a table row is an fp32 sum, in whatever order the atomics land, of up to 4 P / (N + 2)^2 ~ 160
    contributions; without cancellation its relative error is at most ~n 2^-24 = 1e-5, inside the cited rtol for ANY order, while a
    sum of mixed signs that lands near zero keeps an absolute error of n 2^-24 max |partial sum| ~ 4e-6 > the cited atol whatever
    kernel forms it (the spatial hash's included) — that would test the draw, not the rows and weights"""
    key = (P, T, F, fp16)
    if key not in _CASES:
        rng = np.random.default_rng(7 * P + T + F)
        x = coords(P, rng)
        if P > 200:
            x[100:200] = x[100]                                  # many pixels in one cell
        tables = ((rng.random((L, T, F), dtype=np.float32) - 0.5) * 2e-4)
        if fp16:
            tables = tables.astype(np.float16).astype(np.float32)
        g = np.abs(rng.standard_normal((P, L * F))).astype(np.float32)
        idx = dense_hash_idx(x, N_LS, T)
        want = orc.bilinear_forward(x, N_LS, orc.encoding_forward(tables, idx))
        dt, _ = orc.encoding_backward(tables, idx, None, True, orc.bilinear_backward(x, N_LS, g, F))
        for a in (x, tables, g, idx, want, dt):
            a.setflags(write=False)
        _CASES[key] = (x, tables, g, idx, want, dt)
    return _CASES[key]


def grad_tolerance(rtol, atol, fp16):
    """an fp16 table's .grad is the fp32 accumulation buffer rounded ONCE to fp16 (ops._grad_out): half an ulp, 2^-11 relative,
    and half the smallest subnormal, 2^-25, on top of the fp32 tolerance"""
    return (rtol + 2.0 ** -11, atol + 2.0 ** -25) if fp16 else (rtol, atol)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("P", PS)
def test_direct_form_vs_oracle(ops, P, T, F, fp16):
    x, tables, g, idx, want, dt = case(P, T, F, fp16)
    tt = t(tables, torch.float16 if fp16 else None).requires_grad_()
    enc = ops.EncodeDirectFunction.apply(t(x), t(N_LS, torch.int32), tt, None, None, 0, ops.MODE_DENSE_HASH)
    close(enc, want, 1e-6, 1e-9, f"dense direct enc P{P} T{T} F{F}")          # test_gpu_encode.py::test_fused_encode_hash_vs_oracle
    enc.backward(t(g))
    close(tt.grad, dt, *grad_tolerance(1e-4, 1e-6, fp16), f"dense direct d tables P{P} T{T} F{F}")      # (the same test's d tables)
    for l, n in enumerate(N_LS):
        if (n + 2) ** 2 <= T:                                    # rows past a dense level's grid receive exactly nothing
            assert not tt.grad[l, (n + 2) ** 2:].any()


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("P", PS + (101,))
def test_tiled_chain_vs_oracle(ops, P, T, F, fp16):
    """through ops.encode_apply(path="tiled"): P = 4099 and 257 stage all four levels, 101 stages three and leaves N = 32 to the direct
    form, 1 stages none.  F = 2 runs the level-interleaved pixel-stage kernels, F = 1 and 4 the generic ones."""
    x, tables, g, idx, want, dt = case(P, T, F, fp16)
    n_host = [int(n) for n in N_LS]
    plan = ops.EncodePlan(P, n_host, F, "tiled")
    assert plan.Ls == {1: 0, 101: 3, 257: 4, 4099: 4}[P]
    if plan.Ls:
        assert plan.interleaved(backward=True) == (F == 2) and plan.interleaved(backward=False) == (F == 2)
    tt = t(tables, torch.float16 if fp16 else None).requires_grad_()
    enc = ops.encode_apply(t(x), t(N_LS, torch.int32), n_host, tt, None, None, 0, path="tiled", mode=ops.MODE_DENSE_HASH)
    close(enc, want, 1e-6, 1e-9, f"dense tiled enc P{P} T{T} F{F}")           # test_gpu_encode.py::test_tiled_encode_hash_vs_oracle
    enc.backward(t(g))
    rtol, atol = grad_tolerance(2e-4, 2e-6 * max(1.0, float(np.abs(dt).max())), fp16)       # (the same test's d tables)
    close(tt.grad, dt, rtol, atol, f"dense tiled d tables P{P} T{T} F{F}")
    for l, n in enumerate(N_LS):
        if (n + 2) ** 2 <= T:
            assert not tt.grad[l, (n + 2) ** 2:].any()
    # the two forms agree bit for bit in the forward direction
    enc_d = ops.encode_apply(t(x), t(N_LS, torch.int32), n_host, tt.detach(), None, None, 0, path="direct", mode=ops.MODE_DENSE_HASH)
    assert torch.equal(enc_d, enc.detach())


def exact_inputs(P, F, rng):
    """coordinates k / 16 and whole-numbered non-zero gradients in [-4, 4]: x N is exact, the bilinear weights are multiples of 1/16, every
    contribution a multiple of 2^-8 and every partial sum below 4 P < 2^15 — 23 bits: all sums are exact in fp32 (and in the
    power-of-two fixed point of the tiled backward), so the table gradient does not depend on the order or the chain that formed it"""
    x = (rng.integers(0, 17, (P, 2)) / 16.0).astype(np.float32)
    g = (rng.integers(1, 5, (P, L * F)) * rng.choice([-1, 1], (P, L * F))).astype(np.float32)
    return x, g


def run(ops, x, g, tables, mode, path, fp16=False):
    tt = t(tables, torch.float16 if fp16 else None).requires_grad_()
    enc = ops.encode_apply(t(x), t(N_LS, torch.int32), [int(n) for n in N_LS], tt, None, None, 0, path=path, mode=mode)
    enc.backward(t(g))
    return enc.detach(), tt.grad


@pytest.mark.parametrize("path", ["direct", "tiled"])
@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("P", PS)
def test_identities_bit_for_bit(ops, P, F, path):
    rng = np.random.default_rng(P + F)
    x, g = exact_inputs(P, F, rng)
    # T = 64: nothing is dense — the new source IS the spatial hash, in every output
    tables = rng.uniform(-1, 1, (L, 64, F)).astype(np.float32)
    e0, d0 = run(ops, x, g, tables, ops.MODE_HASH, path)
    e2, d2 = run(ops, x, g, tables, ops.MODE_DENSE_HASH, path)
    assert torch.equal(e2, e0) and torch.equal(d2, d0) and bool(d0.any())
    # T = 512: the hashed level (N = 32) reads and writes what the spatial hash reads and writes there
    tables = rng.uniform(-1, 1, (L, 512, F)).astype(np.float32)
    e0, d0 = run(ops, x, g, tables, ops.MODE_HASH, path)
    e2, d2 = run(ops, x, g, tables, ops.MODE_DENSE_HASH, path)
    assert torch.equal(e2[:, 3 * F:], e0[:, 3 * F:]) and torch.equal(d2[3], d0[3]) and bool(d0[3].any())
    if P > 1:                                                    # (and the dense levels do not)
        assert not torch.equal(e2[:, :3 * F], e0[:, :3 * F])


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("T", TS)
def test_vertex_grid_entry_points(ops, T, F, fp16):
    """gngf_vertex_grid_fwd / _bwd (mode 2) on their own: G_l is the first (N_l + 2)^2 rows of a dense level's table and
    hash-gathered elsewhere; the backward adds dG to exactly those rows (odd T and odd level offsets take the unaligned path)"""
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr
    rng = np.random.default_rng(T + F)
    tables = rng.uniform(-1, 1, (L, T, F)).astype(np.float32)
    if fp16:
        tables = tables.astype(np.float16).astype(np.float32)
    n_host = [int(n) for n in N_LS]
    plan = ops.EncodePlan(4099, n_host, F, "tiled")
    tt, n_ls = t(tables, torch.float16 if fp16 else None), t(N_LS, torch.int32)
    G = torch.full((plan.vtot, F), float("nan"), device=DEV)
    ops._vertex_fwd(plan, tt, None, None, n_ls, 0, G, ops.MODE_DENSE_HASH)
    want = np.empty((plan.vtot, F), np.float32)
    dG = rng.integers(-4, 5, (plan.vtot, F)).astype(np.float32)              # whole numbers: sums are exact in any order
    dwant = np.zeros((L, T, F), np.float32)
    off = 0
    for l, n in enumerate(n_host):
        gw = n + 2
        gy, gx = np.divmod(np.arange(gw * gw), gw)
        rows = np.arange(gw * gw) if gw * gw <= T else orc.spatial_hash(
            np.stack([gx, gy])[None, :, None, :].astype(np.int32), T)[0, 0]
        want[off:off + gw * gw] = tables[l, rows]
        np.add.at(dwant[l], rows, dG[off:off + gw * gw])
        off += gw * gw
    assert np.array_equal(G.cpu().numpy(), want)
    dtab = torch.ones((L, T, F), device=DEV)                                 # accumulated INTO: the ones stay underneath
    ops._vertex_bwd(plan, tt, None, None, n_ls, 0, t(dG), dtab, None, mode=ops.MODE_DENSE_HASH)
    assert np.array_equal(dtab.cpu().numpy(), dwant + 1.0)


# ------------------------------------------------------------------------------------------------ model level
def build_net(c, dense=True):
    """test_gpu_render.build_net with the dense_levels keyword; call inside tr.switches(c)"""
    from collision_handling_in_instantngp_amd import models
    p = tr.render_params(c)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=c["T"], num_levels=c["L"], n_min=c["n_min"], n_max=c["n_max"],
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=c["T"], feature_dim=c["F"], topk_k=c["K"],
                                          table_dtype=torch.float16 if c["fp16"] else torch.float32, dense_levels=dense)
    sd = net.state_dict()
    new = {f"encoding._hash_tables.{l}.weight": p["tables"][l] for l in range(c["L"])}
    for i in range(3):
        new[f"mlp.{i}.0.weight"], new[f"mlp.{i}.0.bias"] = p["dec_w"][i], p["dec_b"][i]
    net.load_state_dict({k: (torch.from_numpy(new[k]).to(v.dtype) if k in new else v) for k, v in sd.items()})
    return net, p


@pytest.mark.parametrize("T", [512, 483, 2048])
@pytest.mark.parametrize("P", [257, 20001])
def test_model_forward_backward_vs_oracle(P, T):
    """net(x): rgb, the returned indices (the dense rows in dense levels) and every gradient of an MSE step.  P = 20001 takes the tiled
    chain (>= ops.TUNING.tiled_min_pixels), 257 the direct form."""
    c = cfg(T)
    rng = np.random.default_rng(P + T)
    x = coords(P, rng)
    target = rng.random((P, 3), dtype=np.float32)
    with tr.switches(c):
        net, p = build_net(c)
        assert net.dense_level_mask == [(n + 2) ** 2 <= T for n in N_LS]
        rgb, probs, idx, counts = net(t(x))
        torch.nn.functional.mse_loss(rgb, t(target)).backward()
    want_idx, want, dt, dWs, dbs = oracle_model(p, x, T, target)
    close(rgb, want, 0, 1e-5, f"dense model rgb P{P} T{T}")
    assert probs is None and counts == [] and idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_idx)
    # gradients: tests/test_gpu_model.py::test_three_training_steps_match_reference's bound for step 0
    for l in range(L):
        gr = net.encoding._hash_tables[l].weight.grad
        close(gr, dt[l], 5e-3, 2e-4 * (np.abs(dt).max() + 1e-30), f"dense model d table {l} P{P} T{T}")
        if net.dense_level_mask[l]:
            assert not gr[(int(N_LS[l]) + 2) ** 2:].any()
    for i in range(3):
        close(net.mlp[i][0].weight.grad, dWs[i], 5e-3, 2e-4 * (np.abs(dWs[i]).max() + 1e-30), f"dense model dW{i} P{P} T{T}")
        close(net.mlp[i][0].bias.grad, dbs[i], 5e-3, 2e-4 * (np.abs(dbs[i]).max() + 1e-30), f"dense model db{i} P{P} T{T}")


def test_collisions_of_a_full_image_are_zero_on_dense_levels():
    """65 x 65 points r / 65 < 1 touch every vertex 0..N of every level and none beyond: a dense level uses (N + 1)^2 distinct rows for
    its (N + 1)^2 vertices — calc_hash_collisions gives 0 — and the hashed level (33^2 vertices, 512 rows) reports what the spatial hash reports there"""
    from collision_handling_in_instantngp_amd import train
    c = cfg(512)
    x = t(train.lattice_coordinates(65, 65, 65))
    with tr.switches(c):
        net, _ = build_net(c)
        hashed, _ = build_net(c, dense=False)
        with torch.no_grad():
            coll, minc = net.calc_hash_collisions(net(x)[2])
            coll_h, _ = hashed.calc_hash_collisions(hashed(x)[2])
        with pytest.raises(RuntimeError, match="dense_levels"):
            net.start_collision_tracking()
    assert coll.tolist()[:3] == [0, 0, 0] and coll.tolist()[3] == coll_h.tolist()[3] > 0
    assert minc.tolist() == [0, 0, 0, 33 * 33 - 512]


def adam_check(name, before, after, g, moments, k, lr, wd):
    """One FusedAdam step against oracle.adam_step run on the ORACLE's gradients and the oracle's own moments.  With eps = 1e-15 the
    update lr m^ / sqrt(v^) is homogeneous of degree 0 in the gradients seen so far: where every one of them is at least 5 % of its
    tensor's largest, the device's gradient (held to the oracle's within 5e-3 relative + 2e-4 of that largest: at most 1e-2 relative
    there) moves the update by at most 2.5 x 1e-2 lr — bound 0.05 lr; a wrong sign moves it by 2 lr, a gradient that never arrived by
    lr.  Where every gradient is exactly zero and there is no weight decay, the entry does not move at all."""
    m, v = moments.get(name, (np.zeros_like(before), np.zeros_like(before)))
    want, m, v = orc.adam_step(before, g, m, v, k, lr, wd)
    hist = moments.setdefault(name + "/g", [])
    hist.append(g)
    moments[name] = (m, v)
    big = np.all([np.abs(h) > 0.05 * np.abs(h).max() for h in hist], axis=0)
    assert big.any(), name
    worst = float(np.abs(after - want)[big].max())
    assert worst <= 0.05 * lr, (name, k, worst, lr)
    if wd == 0:
        still = np.all([h == 0 for h in hist], axis=0)
        assert np.array_equal(after[still], before[still]), name
        return bool(still.any())
    return True


def test_two_train_steps_with_the_oracle_carried_along(monkeypatch):
    """train.train_step twice — one batch of 150 x 140 = 21 000 shuffled pixels each: the tiled chain, with the pixel loss fused into the
    decoder and its promised gradient, so a decoder kernel clears the table gradient (StepConfig clear = "decoder": the chain
    profiles/dense_levels.json times) — eager and replayed from a hipGraph.  Every step is held to the oracle evaluated at the
    parameters the step started from: rgb at atol 1e-5, the indices handed back (the dense rows in dense levels), every gradient at
    tests/test_gpu_model.py::test_three_training_steps_match_reference's bound (eager: the step's own .grad), and the optimizer's update of every tensor against
    oracle.adam_step (adam_check) — so the second step runs on tables whose dense rows the first one moved.  Eager and graph then
    agree as G8 / G11 ask of them (PSNR within 0.01 dB, MSE within 2e-3)."""
    from collision_handling_in_instantngp_amd import data, train
    H_, W_, T = 150, 140, 512
    c = cfg(T)
    img = np.random.default_rng(11).integers(0, 256, size=(H_, W_, 3)).astype(np.uint8)
    X = data.normalise_coordinates(torch.from_numpy(data.pixel_grid(H_, W_)).float(), W_, H_).to(DEV)
    Y = torch.tensor(img.reshape(-1, 3) / 255).float().to(DEV)
    shuffled, _ = data.make_permutation(H_ * W_, torch.Generator().manual_seed(5))
    perm = shuffled.long().numpy()
    x_b, y_b = X.cpu().numpy()[perm], Y.cpu().numpy()[perm]
    recs = []
    real_epoch = train.train_epoch

    def epoch(*a, **k):                                          # train_step's own call, its record kept: the outputs and indices
        recs.append(real_epoch(*a, **k))
        return recs[-1]
    monkeypatch.setattr(train, "train_epoch", epoch)
    curve = {False: [], True: []}
    for graph in (False, True):
        with tr.switches(c):
            net, _ = build_net(c)
            loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
            opt = train.get_optimizer(net, 1e-4, 1e-3, 1e-3, 0, 1e-6, 1e-6)
            moments = {}
            for k in (1, 2):
                before = tr.state_params(c, net)
                want_idx, want_rgb, dt, dWs, dbs = oracle_model(before, x_b, T, y_b)
                r = train.train_step(net, loss_fn, opt, X, Y, W_, H_, T, 4, 1, 1, 1e-3, batch_percentage=1, num_levels=L,
                                     should_shuffle=True, shuffled_indices=shuffled.to(DEV), graph=graph)
                loss, show, coll, minc, _cnt, mse, kls, colls, _ipl = r
                rec = recs[-1]
                sc = net.dp.step_config
                assert (sc.source, sc.staged, sc.vertex_fwd, sc.grad_sink, sc.clear) == ("dense_hash", L, "riders", "dG64", "decoder")
                close(rec["outputs"], want_rgb, 0, 1e-5, f"dense train_step {k} rgb (graph={graph})")
                assert np.array_equal(rec["indices"].cpu().numpy(), want_idx)
                # (|d mse| <= 2 atol_rgb mean |rgb - y| <= 2e-5 sqrt(mse): 1e-4 relative for an mse above 0.04, as a random picture's is)
                want_mse = float(np.mean((want_rgb.astype(np.float64) - y_b) ** 2))
                assert want_mse > 0.04
                close(np.array(mse), want_mse, 1e-4, 0, f"dense train_step {k} mse (graph={graph})")
                curve[graph].append((train.calc_psnr(show, img), float(mse)))
                assert kls is None and show.shape == (H_, W_, 3) and coll.shape == (L,)
                after = tr.state_params(c, net)
                for l in range(L):
                    gr = net.encoding._hash_tables[l].weight.grad
                    if not graph:                                # (a replayed step keeps its gradients in the graph's own buffers)
                        close(gr, dt[l], 5e-3, 2e-4 * (np.abs(dt).max() + 1e-30), f"dense train_step {k} d table {l} (graph={graph})")
                        if net.dense_level_mask[l]:
                            assert not gr[(int(N_LS[l]) + 2) ** 2:].any()
                    still = adam_check(f"table{l}", before["tables"][l], after["tables"][l], dt[l], moments, k, 1e-4, 0)
                    assert still or not net.dense_level_mask[l]  # (a dense level has rows past its grid; they did not move)
                for i in range(3):
                    for nm, par, g_, b_, a_ in (("W", net.mlp[i][0].weight, dWs[i], before["dec_w"][i], after["dec_w"][i]),
                                                ("b", net.mlp[i][0].bias, dbs[i], before["dec_b"][i], after["dec_b"][i])):
                        if not graph:
                            close(par.grad, g_, 5e-3, 2e-4 * (np.abs(g_).max() + 1e-30), f"dense train_step {k} d{nm}{i} (graph={graph})")
                        adam_check(f"{nm}{i}", b_, a_, g_, moments, k, 1e-3, 1e-6)
    for e in range(2):
        assert abs(curve[True][e][0] - curve[False][e][0]) < 0.01
        close(np.array(curve[True][e][1]), np.array(curve[False][e][1]), 2e-3, 0, f"dense train_step {e + 1} MSE, graph vs eager")


@pytest.mark.parametrize("T,F,fp16", [(512, 2, False), (483, 2, False), (2048, 4, False), (500, 1, False), (512, 2, True)])
def test_render_and_bake_vs_module_forward(T, F, fp16):
    """train.render and BakedGrid.render against net(x) at train.lattice_coordinates under tests/test_gpu_render.py's rule (rgb
    within its tolerance, the integer image different only inside the rounding zone), and the bake IS the dense levels' tables"""
    from collision_handling_in_instantngp_amd import train
    c = cfg(T, F, fp16)
    rows, cols = 61, 67
    with tr.switches(c):
        net, p = build_net(c)
        with torch.no_grad():
            want = net(t(train.lattice_coordinates(rows, cols, 66)))[0].cpu().numpy()
        rgb, image = train.render(net, rows, cols, image=True)
        tr.check_render(rgb, image, want, f"dense render T{T} F{F}")
        baked = train.bake(net)
        rgb_b, image_b = baked.render(rows, cols, image=True)
        tr.check_render(rgb_b, image_b, want, f"dense baked render T{T} F{F}")
    offsets, _ = train.baked_level_offsets([int(n) for n in N_LS])
    tables = net.encoding.packed_tables().float()
    for l, n in enumerate(int(v) for v in N_LS):
        if net.dense_level_mask[l]:
            assert torch.equal(baked.grid[offsets[l]:offsets[l] + (n + 2) ** 2], tables[l, :(n + 2) ** 2])
    assert any(net.dense_level_mask)


def test_fit_three_epochs_and_score_the_best_snapshot():
    from collision_handling_in_instantngp_amd import data, train
    W_, H_ = 24, 20
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(H_, W_, 3)).astype(np.uint8)
    X = data.normalise_coordinates(torch.from_numpy(data.pixel_grid(H_, W_)).float(), W_, H_).to(DEV)
    Y = torch.tensor(img.reshape(-1, 3) / 255).float().to(DEV)
    shuffled, _ = data.make_permutation(H_ * W_, torch.Generator().manual_seed(4))
    c = cfg(512)
    with tr.switches(c):
        net, _ = build_net(c)
        net.return_indices = False                               # no tracking for this source: fit() falls back to "no statistic"
        opt = train.get_optimizer(net, 1e-3, 1e-3, 1e-3, 0, 1e-6, 1e-6)
        res = train.fit(net, train.Loss(delta=1, gamma=-2, epsilon=1), opt, X, Y, W_, H_, img, epochs=3, tolerance=6, min_delta=0.0,
                        l_mse=1, l_js_kl=1, l_collisions=1e-3, batch_percentage=1 / 3, should_shuffle=True, shuffled_indices=shuffled,
                        graph=True, poll_every=3)
        assert res.issued == 3 and res.best_epoch >= 0 and not net.track_collisions
        res.best.restore()
        image, psnr, acc = train.render_psnr(net, img)
        mask = net.reachable_rows()
    assert tuple(image.shape) == (H_, W_, 3) and image.dtype == torch.int32 and np.isfinite(psnr) and psnr > 0 and 0.0 <= acc <= 1.0
    # reachable_rows(): the dense prefixes on top of the hashed rows
    bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :512]
    for l, n in enumerate(int(v) for v in N_LS):
        if (n + 2) ** 2 <= 512:
            assert bits[l, :(n + 2) ** 2].all()
