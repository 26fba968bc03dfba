#!/usr/bin/env python
"""A model evaluated at given coordinates, in ONE process ("query at arbitrary coordinates"):

    query          train.query(net, xy, out_rgb=buf, check=False): one launch of the render kernel's query form
    module         the parent's general way: net(xy) under torch.no_grad() — binning, vertex stage, tiled pixel stage, the (P, L F)
                   encoding in memory, the decoder (return_indices / dense_probs off, as bench.py runs the model)
    render         (lattice points only) the parent's lattice way: train.render(net, side, side, out_rgb=buf)

at P = `--side`^2 points (default 1024^2 = 2^20) for two kinds of points — (a) `random`: seeded uniform in [0, 1)^2; (b) `lattice`: the
side x side lattice's own coordinates (train.lattice_coordinates), row-major — headline model shape (bench.SHAPES["cfg3"]: L = 16,
F = 2, T = 2^19, n_max = 512) in hash mode and with GNGF indexing on a frozen HPD.  A window is `--calls` calls timed with HIP
events around all of them; the ways alternate window by window; median and range over `--windows` windows.  Peak allocation of one
call of each way (torch.cuda.max_memory_allocated delta; query's and render's output buffer is allocated by the caller beforehand
and reported as out_bytes).  Before timing, the ways are compared: query == render bit for bit on the lattice, query within the
forward tolerance of net(xy).  No thresholds.

    python tools/time_query.py [--out profiles/query.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query.json"))
    ap.add_argument("--side", type=int, default=1024, help="P = side^2 points")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import time_sampler as ts
    from time_score import alternate, peak_delta, summary
    from collision_handling_in_instantngp_amd import models, train
    if not torch.cuda.is_available():
        raise SystemExit("time_query.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    c = bench.SHAPES["cfg3"]
    side = a.side
    P = side * side
    res = {"shape": dict(c), "points": P, "windows": a.windows, "calls_per_window": a.calls,
           "device": torch.cuda.get_device_name(dev), "query": {}}
    rng = np.random.default_rng(65535)
    points = {"random": torch.from_numpy(rng.random((P, 2), dtype=np.float32)).to(dev),
              "lattice": torch.from_numpy(train.lattice_coordinates(side, side, side - 1)).to(dev)}
    prev = models.should_use_hash_function
    try:
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
            C = 3
            buf = torch.empty((P, C), dtype=torch.float32, device=dev)
            buf_r = torch.empty((P, C), dtype=torch.float32, device=dev)
            for which, xy in points.items():
                def query():
                    train.query(net, xy, out_rgb=buf, check=False)

                def module():
                    with torch.no_grad():
                        return net(xy, 1.0)[0]

                def render():
                    train.render(net, side, side, out_rgb=buf_r)

                query()
                out = module()
                torch.cuda.synchronize()
                diff = (buf - out).abs()
                rec = {"max_abs_diff_vs_module": float(diff.max()),
                       "within_forward_tolerance_of_module": bool((diff <= 2e-6 + 2e-5 * out.abs()).all())}
                del out, diff
                ways = {"query": query, "module": module}
                if which == "lattice":
                    render()
                    torch.cuda.synchronize()
                    rec["bit_equal_to_render"] = bool(torch.equal(buf, buf_r))
                    ways["render"] = render
                ms = alternate(ways, a.windows, a.calls)
                for k, fn in ways.items():
                    rec[k] = summary(ms[k])
                    rec[k + "_peak_alloc_bytes"] = peak_delta(fn)
                rec["out_bytes"] = buf.numel() * 4
                rec["xy_bytes"] = xy.numel() * 4
                res["query"][f"{kind}_{which}"] = rec
                print(kind, which, {k: round(v["ms_median"], 4) for k, v in rec.items() if isinstance(v, dict)},
                      {k: v for k, v in rec.items() if not isinstance(v, dict)}, flush=True)
            del net, buf, buf_r
    finally:
        models.should_use_hash_function = prev
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
