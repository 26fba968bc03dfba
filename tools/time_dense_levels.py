#!/usr/bin/env python
"""Step and render times of the three index sources at the cfg2 shape, in ONE process ("dense levels"):

    hash          the spatial hash on every level                                  (ops.MODE_HASH)
    vertex_table  GNGF indexing through the frozen HPD's per-vertex table, K = 4   (ops.MODE_VERTEX_TABLE)
    dense_hash    dense where the level fits the table, hashed elsewhere           (ops.MODE_DENSE_HASH; at cfg2 every level fits)

The training step is built the way bench.py builds it — bench.make_batch's 2^20 strawberry pixels, the fused pixel loss with a
promised gradient, train.GraphedStep(unroll, cross_replay=True), three calls to capture, the clock ramp — and timed with HIP
events around whole replays: `--windows` windows of `--steps` steps each, per source, the sources interleaved window by window so
that a drift of the clock falls on all three alike.  The render is train.render on a 1024 x 1024 lattice into preallocated
outputs, `--render-launches` launches per window.

    python tools/time_dense_levels.py [--out profiles/dense_levels.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(source, dev, bench):
    import torch
    from collision_handling_in_instantngp_amd import models
    c = bench.SHAPES["cfg2"]
    models.should_use_hash_function = source != "vertex_table"
    torch.manual_seed(65535)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=c["T"], num_levels=c["L"], n_min=c["n_min"], n_max=c["n_max"],
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=c["T"], feature_dim=c["F"], topk_k=c["K"],
                                          dense_levels=(source == "dense_hash")).to(dev)
    net.return_indices = False
    net.dense_probs = False
    if source == "vertex_table":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
    return net


def event_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_levels.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--unroll", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ramp-steps", type=int, default=60)
    ap.add_argument("--render-launches", type=int, default=20)
    a = ap.parse_args()
    import torch
    import bench
    from collision_handling_in_instantngp_amd import models, train
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = bench.P_PER_GPU
    xy, target, _bounds = bench.make_batch("cfg2", P, 0, dev)
    sources = ("hash", "vertex_table", "dense_hash")
    prev = models.should_use_hash_function
    steppers, renders, info = {}, {}, {}
    try:
        for s in sources:
            net = build(s, dev, bench)
            loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
            gs = train.GraphedStep(net, loss_fn, None, 1, 1, 1e-3, unroll=a.unroll, cross_replay=True)
            for _ in range(3):
                gs.run_many([(xy, target)] * a.unroll, next_first=xy)
            steppers[s] = gs.replay_steady
            sc = net.dp.step_config
            info[s] = {"step_config": sc.signature(), "dense_levels": sum(net.dense_level_mask), "levels": net._num_levels}
            out_rgb = torch.empty((1024 * 1024, 3), dtype=torch.float32, device=dev)
            train.render(net, 1024, 1024, out_rgb=out_rgb)                      # (a frozen HPD builds its vertex table here, once)
            renders[s] = (lambda net=net, out_rgb=out_rgb: train.render(net, 1024, 1024, out_rgb=out_rgb))
        replays = a.steps // a.unroll
        for s in sources:
            for _ in range(a.ramp_steps // a.unroll):
                steppers[s]()
        torch.cuda.synchronize()
        step_ms = {s: [] for s in sources}
        render_ms = {s: [] for s in sources}
        for _w in range(a.windows):
            for s in sources:
                step_ms[s].append(event_ms(steppers[s], replays) / (replays * a.unroll))
        for _w in range(a.windows):
            for s in sources:
                render_ms[s].append(event_ms(renders[s], a.render_launches) / a.render_launches)
    finally:
        models.should_use_hash_function = prev
    res = {"shape": {k: v for k, v in bench.SHAPES["cfg2"].items()}, "pixels_per_step": P, "steps_per_window": replays * a.unroll,
           "unroll": a.unroll, "windows": a.windows, "render_lattice": [1024, 1024], "render_launches_per_window": a.render_launches,
           "device": torch.cuda.get_device_name(dev), "sources": {}}
    for s in sources:
        res["sources"][s] = dict(info[s], step_ms_median=statistics.median(step_ms[s]), step_ms_windows=step_ms[s],
                                 render_ms_median=statistics.median(render_ms[s]), render_ms_windows=render_ms[s])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({s: {"step_ms": round(v["step_ms_median"], 4), "render_ms": round(v["render_ms_median"], 4)}
                      for s, v in res["sources"].items()}))


if __name__ == "__main__":
    main()
