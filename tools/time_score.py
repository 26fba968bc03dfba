#!/usr/bin/env python
"""Scoring a model against its image, in ONE process ("score in one launch"):

    score          train.score(net, image, out=buf): the render kernel's scoring form + a one-workgroup finish
    two_call       the parent's way with the target already on the device: train.render(net, h, w, image=True, out_image=buf)
                   (int32 image, 4 B per element) + ops.image_metrics on it

at `--sides` (default 1024 and 2048) squared x 3, headline model shape (bench.SHAPES["cfg3"]: L = 16, F = 2, T = 2^19, n_max = 512)
in hash mode and with GNGF indexing on a frozen HPD.  A window is `--calls` calls timed with HIP events around all of them; the two
ways alternate window by window; median and range over `--windows` windows.  Peak allocation of one call of each way
(torch.cuda.max_memory_allocated delta, buffers for the outputs allocated by the caller beforehand — for two_call that buffer IS
the int32 image, reported as two_call_image_bytes).  Also: step = 4 against step = 1 at the largest side, and train.fit_sampled's
per-round time at steps_per_round in {16, 64} against the same number of bare train_sampled steps plus one score.  No thresholds.

    python tools/time_score.py [--out profiles/score.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def event_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(ways, windows, calls, ramp=2):
    """{name: per-call ms of each window}: the ways alternate window by window, after `ramp` untimed rounds"""
    out = {k: [] for k in ways}
    for r in range(ramp + windows):
        for k, fn in ways.items():
            ms = event_ms(fn, calls)
            if r >= ramp:
                out[k].append(ms)
    return out


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_windows": ms}


def peak_delta(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2 ** 20)
    ap.add_argument("--fit-rounds", type=int, default=6)
    a = ap.parse_args()
    import torch
    import bench
    import time_sampler as ts
    from collision_handling_in_instantngp_amd import data, models, ops, train
    if not torch.cuda.is_available():
        raise SystemExit("time_score.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    c = bench.SHAPES["cfg3"]
    res = {"shape": dict(c), "windows": a.windows, "calls_per_window": a.calls, "device": torch.cuda.get_device_name(dev), "score": {}}
    prev = models.should_use_hash_function
    try:
        images = {side: torch.from_numpy(ts.formula_image(side)).to(dev) for side in a.sides}
        for kind in ("hash", "gngf_frozen"):
            models.should_use_hash_function = kind == "hash"
            net, _loss_fn, _opt = ts.build(dev, c)
            with torch.no_grad():
                for m in net.encoding._hash_tables:
                    m.weight.uniform_(-1.0, 1.0)          # (the +-1e-4 start would render one colour)
            if kind != "hash":
                for p in net.HPD.parameters():
                    p.requires_grad = False
                net.compute_pbar = False                  # the frozen-HPD forward on the cached per-vertex table
            for side in a.sides:
                img = images[side]
                n = side * side * 3
                sums_a = torch.zeros((2,), dtype=torch.int64, device=dev)
                sums_b = torch.zeros((2,), dtype=torch.int64, device=dev)
                buf = torch.empty((side, side, 3), dtype=torch.int32, device=dev)
                ws = ops.image_metrics_workspace(n, dev)
                flat = img.reshape(-1)

                def score(step=1):
                    train.score(net, img, step=step, out=sums_a)

                def two_call():
                    train.render(net, side, side, rgb=False, out_image=buf)
                    ops.image_metrics(buf, flat, sums_b, ws)

                score()
                two_call()
                torch.cuda.synchronize()
                if not torch.equal(sums_a, sums_b):
                    raise SystemExit(f"{kind} {side}: score {sums_a.tolist()} != two-call {sums_b.tolist()}")
                ms = alternate({"score": score, "two_call": two_call}, a.windows, a.calls)
                rec = {"eq_sse": sums_a.tolist(), "score": summary(ms["score"]), "two_call": summary(ms["two_call"]),
                       "score_peak_alloc_bytes": peak_delta(score), "two_call_peak_alloc_bytes": peak_delta(two_call),
                       "two_call_image_bytes": buf.numel() * 4, "image_bytes": img.numel()}
                if side == max(a.sides):
                    ms4 = alternate({"step1": score, "step4": lambda: score(4)}, a.windows, a.calls)
                    rec["step"] = {"step1": summary(ms4["step1"]), "step4": summary(ms4["step4"]),
                                   "scored_elements": [train.scored_elements(side, side, 3, 1), train.scored_elements(side, side, 3, 4)]}
                res["score"][f"{kind}_{side}"] = rec
                print(kind, side, {k: round(v["ms_median"], 4) for k, v in rec.items() if isinstance(v, dict) and "ms_median" in v},
                      flush=True)
                del buf
            del net
        # fit_sampled's round against its parts, hash mode, the largest image
        models.should_use_hash_function = True
        side = max(a.sides)
        weights = dict(l_mse=1, l_js_kl=1, l_collisions=1e-3)
        res["fit_sampled"] = {"image": [side, side, 3], "batch": a.batch, "rounds_per_window": a.fit_rounds}
        for spr in (16, 64):
            net, loss_fn, opt = ts.build(dev, c)
            s = data.ImageSampler(images[side], a.batch, seed=65535, continuous=True)
            sums = torch.zeros((2,), dtype=torch.int64, device=dev)

            def fit():
                train.fit_sampled(net, loss_fn, opt, s, rounds=a.fit_rounds, steps_per_round=spr, tolerance=10 ** 6, min_delta=0.0,
                                  poll_every=a.fit_rounds, exact_final=True, **weights)

            def bare():
                for _ in range(a.fit_rounds):
                    train.train_sampled(net, loss_fn, opt, s, spr, **weights)
                    train.score(net, s, out=sums)

            ms = alternate({"fit_sampled": fit, "bare": bare}, max(3, a.windows // 2), 1)
            per = {k: [m / a.fit_rounds for m in v] for k, v in ms.items()}
            res["fit_sampled"][f"steps_per_round_{spr}"] = {
                "fit_sampled_round": summary(per["fit_sampled"]), "bare_round": summary(per["bare"]),
                "excess_ms_median": statistics.median(per["fit_sampled"]) - statistics.median(per["bare"]),
                "note": "fit_sampled also allocates its snapshots, log and state once per call: that is inside its windows"}
            print("fit_sampled", spr, round(statistics.median(per["fit_sampled"]), 4), round(statistics.median(per["bare"]), 4), flush=True)
            del net, opt
    finally:
        models.should_use_hash_function = prev
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
