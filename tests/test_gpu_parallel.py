"""GPU, 2 ranks on ONE device over gloo (tensor staging through host): a 2-way pixel-sharded step with the
vertex-grid gradient exchange equals the single-rank step on the concatenated batch (SURVEY.md §4 iv)."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _grads(net):
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}


def _make(models, mode):
    mode = mode.replace("_overlap", "").replace("_deferred", "")
    half = mode.endswith("_fp16")
    mode = mode.replace("_fp16", "")
    partial = mode.endswith("_partial")
    mode = mode.replace("_partial", "")
    models.should_use_hash_function = (mode.startswith("hash"))
    torch.manual_seed(7)
    # "hash_partial": n_max = 1024 at 2^15 pixels leaves the finest levels to the direct form (N_l^2 > 4 P): the exchange
    # then covers the staged levels through dG and the direct levels through their slice of the table gradient
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=2 ** 14, num_levels=8, n_min=16,
                                          n_max=(1024 if partial else 128),
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=2 ** 14, feature_dim=2, topk_k=4,
                                          table_dtype=(torch.float16 if half else torch.float32))
    if half:
        with torch.no_grad():
            for m in net.encoding._hash_tables:
                m.weight.mul_(100.0)                  # 1e-2-scale features: gradients well above fp16 subnormals
    net.return_indices = False
    net.dense_probs = False
    if mode == "gngf_frozen":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
    return net


def _worker(rank, world, port, mode, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from collision_handling_in_instantngp_amd import models, parallel, ops
    chains = ops.SEEN_STEP_CONFIGS = set()              # the kernel chains this rank's forward passes take (reported to the parent test)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    P = 2 ** 15
    xy = torch.rand((P, 2), generator=g).to(dev)
    tgt = torch.rand((P, 3), generator=g).to(dev)
    net = _make(models, mode)
    parallel.broadcast_parameters(net)
    from collision_handling_in_instantngp_amd import train
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    empty = torch.tensor([], device=dev)

    def loss_of(bx, by):
        rgb, probs, _i, _c = net(bx, 1.0)
        if mode.startswith("gngf_learning"):      # MSE + KL/JS of the batch-mean distribution (functions.py:243-245)
            mse, kls, coll = loss_fn(rgb, by, probs.shape[-1], probs, empty, empty)
            return train.assemble_loss(mse, kls, coll, 1, 1, 1e-3)
        return torch.nn.functional.mse_loss(rgb, by) * (4096.0 if "fp16" in mode else 1.0)     # loss scaling for fp16 gradients

    # single-rank reference on the whole batch (rank 0 only)
    ref = None
    if rank == 0:
        loss_of(xy, tgt).backward()
        ref = _grads(net)
        net.zero_grad()
    parallel.enable_vertex_grid_exchange(net, world)
    overlap = mode.endswith("_overlap")          # exchange + deferred vertex stage on the model's communication stream
    defer = mode.replace("_overlap", "").endswith("_deferred")
    parallel.defer_vertex_stage(net, defer)
    lo, hi = parallel.shard_batch(P, rank, world)
    loss_of(xy[lo:hi], tgt[lo:hi]).backward()
    reduced_flag = net.dp.tables_reduced
    if defer:
        assert net.dp.deferred is not None, "the vertex stage was not deferred"
    parallel.allreduce_gradients(net, world, overlap=overlap)
    if overlap:
        assert net.dp.comm_done is not None and net.dp.comm_stream is not None
        torch.ones(8, device=dev).sum()                   # (work on the main stream beside the exchange)
        parallel.wait_for_gradients(net)
        assert net.dp.comm_done is None
    parallel.defer_vertex_stage(net, False)
    got = _grads(net)
    ok = True
    if rank == 0:
        for k in ref:
            scale = np.abs(ref[k].astype(np.float64)).max() + 1e-30
            tol = 2e-3 if ref[k].dtype == np.float16 else 2e-4           # fp16 gradients: one rounding each side
            assert scale > 1e-20, k                                     # a gradient that is all zero proves nothing
            ok &= bool(np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)).max() <= tol * scale)
    with open(os.path.join(ret, f"rank{rank}.json"), "w") as fh:      # (a Manager would fork this GPU-initialised process)
        json.dump([bool(ok), int(reduced_flag), sorted(chains)], fh)
    parallel.enable_vertex_grid_exchange(net, 1)
    models.should_use_hash_function = False
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["hash", "gngf_frozen", "gngf_learning", "hash_partial", "hash_deferred", "gngf_frozen_deferred",
                                  "hash_partial_deferred", "hash_partial_fp16_deferred", "hash_fp16_deferred", "hash_partial_fp16",
                                  "hash_deferred_overlap", "gngf_frozen_deferred_overlap", "hash_partial_overlap",
                                  "gngf_frozen_partial", "gngf_frozen_partial_deferred"])
def test_two_rank_sharded_step_equals_single_rank(mode, tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), mode, str(tmp_path)), nprocs=2, join=True)
    ret = {r: json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)}
    from collision_handling_in_instantngp_amd import ops
    if ops.SEEN_STEP_CONFIGS is not None:               # (tests/conftest.py: which kernel chains did this test run? — the ranks report theirs)
        for r in range(2):
            ops.SEEN_STEP_CONFIGS.update(ret[r][2])
    assert any(" xchg" in c for c in ret[1][2]), ret[1][2]
    assert ret[0][0], "sharded gradients differ from the single-rank step"
    assert ret[0][1] and ret[1][1], "the vertex-grid exchange did not engage"
    if "_partial" in mode:
        assert 0 < ret[0][1] < 8, f"expected a partially staged plan, got {ret[0][1]} staged levels"
    else:
        assert ret[0][1] == 8


def test_decoder_gradients_are_one_flat_buffer():
    """The fused decoder backward returns its six gradients as consecutive views of one buffer, and they arrive in the
    parameters' .grad without a copy: the data-parallel exchange then all-reduces that buffer in place."""
    from collision_handling_in_instantngp_amd import models, parallel
    net = _make(models, "hash").to("cuda")
    x = torch.rand((4096, 2), device="cuda")
    rgb, _p, _i, _c = net(x, 1.0)
    rgb.sum().backward()
    flat = parallel._flat_alias([p.grad for p in net.mlp.parameters()])
    assert flat is not None and flat.numel() == sum(p.numel() for p in net.mlp.parameters())
    models.should_use_hash_function = False


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["gngf_frozen", "cfg4_hash"])
def test_bench_with_two_ranks_runs_as_a_fresh_process(mode, tmp_path):
    """the N > 1 path of bench.py — one hipGraph per rank with the next batch's binning riding on it
    (GraphedStep(cross_replay=True), one step per replay), parallel.allreduce_gradients(overlap=True) on the communication stream,
    the deferred vertex stage behind the exchange, wait_for_gradients at the top of the next replay — started exactly as the driver
    starts it (`python bench.py --gpus 2 ...` as a child process that spawns its own ranks), with two ranks SHARING this box's one
    GPU over gloo.  Not a measurement: the first contact with N > 1 hardware must not be the first run of this code."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (two ranks on one card; the exchange is staged through the host.  cfg4 at the full 2^20 pixels per rank: fewer would stage fewer
    # levels and take the level-interleaved kernels instead of the generic ones the 4-GPU config runs)
    pixels = 2 ** 20 if mode == "cfg4_hash" else 2 ** 18
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--mode", mode, "--pixels", str(pixels), "--ramp-steps", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=840, cwd=root)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["collective_ranks"] == 2 and d["backend"] == "gloo" and d["rccl_ranks"] is None
    assert d["steps"] == 4 and d["config"]["mode"] == mode and d["config"]["pixels_per_gpu"] == pixels
    assert len(d["ms_per_step_per_rank"]) == 2 and all(np.isfinite(t) and t > 0 for t in d["ms_per_step_per_rank"])
    assert np.isfinite(d["value"]) and d["value"] > 0 and d["ms_per_step"] >= max(d["ms_per_step_per_rank"]) - 1e-9
    ex = d["modes"][mode]["exchange"]
    assert ex["n"] == 2 and ex["exchange_bytes_per_step"] > 0 and ex["vertex_grid_bytes"] > 0
    assert (ex["direct_level_table_bytes"] > 0) == (mode == "cfg4_hash")
    assert "hipGraph" in d["config"]["launch"], d["config"]["launch"]
    chain = d["modes"][mode]["step_chain"]
    assert chain.endswith(" xchg") and ("px=generic" in chain) == (mode == "cfg4_hash"), chain
    from collision_handling_in_instantngp_amd import ops
    if ops.SEEN_STEP_CONFIGS is not None:
        ops.SEEN_STEP_CONFIGS.add(chain)


def _worker_zero(rank, world, port, half, ret):
    """parallel.shard_direct_levels: three optimisation steps, two ranks, each on its half of every batch — the direct levels'
    gradient slice reduce-scattered, each rank's FusedAdam updating its rows only, the parameter rows all-gathered — against the
    same three steps of one rank on the whole batches."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from collision_handling_in_instantngp_amd import models, parallel, ops, train
    chains = ops.SEEN_STEP_CONFIGS = set()
    dev = torch.device("cuda", 0)
    ops.FP16_TABLE_GRAD_FP32 = bool(half)
    P, steps, lr = 2 ** 15, 3, 1e-3
    g = torch.Generator().manual_seed(11)
    xs = [torch.rand((P, 2), generator=g).to(dev) for _ in range(steps)]
    ys = [torch.rand((P, 3), generator=g).to(dev) for _ in range(steps)]
    mode = "hash_partial_fp16" if half else "hash_partial"

    def run(net, sharded):
        opt = train.FusedAdam([{"params": list(net.encoding.parameters())}, {"params": list(net.mlp.parameters())}], lr=lr, betas=(0.9, 0.99), eps=1e-8)
        first_grad = None
        for k in range(steps):
            opt.zero_grad()
            lo, hi = parallel.shard_batch(P, rank, world) if sharded else (0, P)
            rgb, _p, _i, _c = net(xs[k][lo:hi], 1.0)
            torch.nn.functional.mse_loss(rgb, ys[k][lo:hi]).backward()
            if sharded:
                parallel.allreduce_gradients(net, world)
            if k == 0:
                first_grad = torch.stack([(getattr(m.weight, "grad_fp32", None) if m.weight.grad is None else m.weight.grad).float().clone()
                                          for m in net.encoding._hash_tables])
            opt.step()
            if sharded:
                parallel.gather_direct_levels(net)
        torch.cuda.synchronize()
        return first_grad

    net = _make(models, mode)
    parallel.broadcast_parameters(net)
    p0 = net.encoding.packed_tables().detach().float().clone()
    ok, info = True, {}
    if rank == 0:
        ref = _make(models, mode)
        ref.load_state_dict(net.state_dict())
        g_ref = run(ref, sharded=False)
        d_ref = ref.encoding.packed_tables().detach().float() - p0
        mlp_ref = [p.detach().clone() for p in ref.mlp.parameters()]
    parallel.enable_vertex_grid_exchange(net, world)
    Ls, lo, hi = parallel.shard_direct_levels(net, world, rank, P // world)
    assert 0 < Ls < 8 and hi > lo, (Ls, lo, hi)
    ranges = [m.weight._adam_range for m in net.encoding._hash_tables]
    assert all(r is None for r in ranges[:Ls]) and any(r is not None and r[1] > r[0] for r in ranges[Ls:]), ranges
    run(net, sharded=True)
    if rank == 0:
        d = net.encoding.packed_tables().detach().float() - p0
        sig = g_ref.abs() > 1e-3 * g_ref.abs().max()                 # entries whose first gradient is well above rounding (Adam's update is sign-like)
        assert int(sig[Ls:].sum()) > 1000 and int(sig[:Ls].sum()) > 1000
        err = (d - d_ref).abs()[sig]
        moved = d_ref.abs()[sig]
        info = {"max_err": float(err.max()), "max_move": float(moved.max()), "frac_moved": float((d.abs()[sig] > 0).float().mean())}
        ok &= info["max_err"] <= (3e-3 if half else 2e-2) * lr * steps + (1e-3 if half else 0.0) * float(moved.max())
        ok &= info["frac_moved"] > 0.999                              # incl. the rows the OTHER rank updated (all-gather)
        for a, b in zip(net.mlp.parameters(), mlp_ref):
            ok &= bool((a.detach() - b).abs().max() <= 2e-2 * lr * steps)
    with open(os.path.join(ret, f"rank{rank}.json"), "w") as fh:
        json.dump([bool(ok), info, sorted(chains)], fh)
    parallel.shard_direct_levels(net, 1, 0, P)
    parallel.enable_vertex_grid_exchange(net, 1)
    ops.FP16_TABLE_GRAD_FP32 = False
    models.should_use_hash_function = False
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
def test_sharded_update_of_the_direct_levels_equals_the_single_rank_steps(half, tmp_path):
    """VERDICT r4 item 5(c), built: ZeRO-1 for the direct levels (parallel.shard_direct_levels / gather_direct_levels) — the
    cfg5 answer to an exchange as long as the step.  fp32 tables and fp16 tables with the fp32 gradient hand-over."""
    mp.spawn(_worker_zero, args=(2, _free_port(), half, str(tmp_path)), nprocs=2, join=True)
    ret = {r: json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)}
    assert ret[0][0], ret[0][1]
    from collision_handling_in_instantngp_amd import ops
    if ops.SEEN_STEP_CONFIGS is not None:
        for r in range(2):
            ops.SEEN_STEP_CONFIGS.update(ret[r][2])
