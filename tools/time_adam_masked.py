"""Times train.FusedAdam.step() alone, dense (gngf_adam_step) against row-masked (gngf_adam_step_masked), at the level-table
shapes of cfg2, cfg4 and cfg5 in hash mode, and one GraphedStep with the optimizer at the headline shape (cfg2, frozen HPD) —
the quantity bench.py reports as with_adam_ms_per_step — dense against masked.

Device events around windows of enough steps to last --window seconds; both variants warmed up; the two alternate in the same
process and the pair is repeated --repeats times, so the dense kernel's own run-to-run spread stands next to the difference.
Bytes per step are computed from the shapes and the map's popcount (what the algorithm needs, not what the memory system moved).

    python tools/time_adam_masked.py --out profiles/adam_masked.json
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from collision_handling_in_instantngp_amd import models, train  # noqa: E402
from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr  # noqa: E402


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps                      # ms per step


def alternate(variants, seconds, repeats, warm=5):
    """variants: {name: fn}.  -> {name: [ms per step of each window]}, windows of >= `seconds`, the variants taking turns"""
    steps = {}
    for name, fn in variants.items():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        est = window(fn, 10)
        steps[name] = max(10, int(np.ceil(seconds * 1e3 / max(est, 1e-3))))
    out = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            fn()                                            # (switching variants re-uploads the segment table: not in the window)
            torch.cuda.synchronize()
            out[name].append(window(fn, steps[name]))
    return out, steps


def summary(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"ms_per_step": [round(float(x), 5) for x in a], "median_ms": float(np.median(a)), "min_ms": float(a.min()),
            "max_ms": float(a.max()), "spread_rel": float((a.max() - a.min()) / np.median(a))}


def row_map(n_ls, T, dev):
    L = len(n_ls)
    m = torch.zeros((L, (T + 31) // 32), dtype=torch.int32, device=dev)
    host = (ctypes.c_int32 * L)(*[int(n) for n in n_ls])
    vs = int(max(n_ls)) + 2
    call("gngf_mark_reachable_rows", ptr(torch.tensor([int(n) for n in n_ls], dtype=torch.int32, device=dev)), host, L, ptr(None), 1,
         T, vs, vs * vs, ptr(m), stream_ptr())
    return m


def unpack(words, T):
    w = words.reshape(-1)
    return ((w[:, None] >> torch.arange(32, device=w.device, dtype=torch.int32)) & 1).bool().reshape(-1)[:T]


def adam_alone(name, dev, seconds, repeats):
    c = bench.SHAPES[name]
    L, F, T, half = c["L"], c["F"], c["T"], c["half"]
    n_ls = [int(n) for n in models.level_resolutions(c["n_min"], c["n_max"], L)]
    rows = row_map(n_ls, T, dev)
    base = (torch.rand((L, T, F), device=dev) * 2e-4 - 1e-4).to(torch.float16 if half else torch.float32)
    grad = torch.empty((L, T, F), dtype=torch.float32, device=dev)
    reach = []
    for l in range(L):
        bits = unpack(rows[l], T)
        reach.append(int(bits.sum()))
        grad[l] = torch.randn((T, F), device=dev) * 1e-3 * bits[:, None]       # unreachable rows never receive a gradient
    params = [torch.nn.Parameter(base[l]) for l in range(L)]
    for l, p in enumerate(params):
        if half:
            p.grad_fp32 = grad[l]                           # the fp32 hand-over of fp16 tables (bench.py's cfg5)
        else:
            p.grad = grad[l]
    opt = train.FusedAdam([{"params": params, "lr": 1e-2, "weight_decay": 0.0}], betas=(0.9, 0.99), eps=1e-15)

    def source():
        return {p: (rows[l], F) for l, p in enumerate(params)}

    def dense():
        if opt._mask_source is not None:
            opt.set_mask_source(None)
        opt.step()

    def masked():
        if opt._mask_source is None:
            opt.set_mask_source(source)                     # (state exists: the next step checks it against the map, outside the window)
            opt.step()
            assert opt._mask_source is not None, "the state guard dropped the map"
        opt.step()
    times, steps = alternate({"dense": dense, "masked": masked}, seconds, repeats)
    assert opt._last_call == "gngf_adam_step_masked"
    per_elem = 30 if half else 28                          # fp32: p rw 8 + g 4 + m rw 8 + v rw 8; fp16 tables: master, m, v rw 24 + fp32 g 4 + fp16 p w 2
    total = L * T * F
    reach_elems = sum(reach) * F
    d, m = summary(times["dense"]), summary(times["masked"])
    res = {"shape": {"L": L, "F": F, "T": T, "n_min": c["n_min"], "n_max": c["n_max"], "fp16_tables": half, "elements": total},
           "rows_reachable": sum(reach), "rows_total": L * T, "reachable_share": sum(reach) / (L * T),
           "reachable_share_per_level": [round(r / T, 5) for r in reach],
           "bytes_per_step": {"dense": total * per_elem, "masked": reach_elems * per_elem + rows.numel() * 4,
                              "note": "needed by the algorithm, from shapes and the map's popcount; memory lines are coarser than rows"},
           "steps_per_window": steps, "dense": d, "masked": m,
           "masked_over_dense": m["median_ms"] / d["median_ms"],
           "dense_GBps": total * per_elem / d["median_ms"] * 1e-6,
           "verdict": ("masked is faster beyond the dense spread" if m["max_ms"] < d["min_ms"] else
                       "masked is slower beyond the dense spread" if m["min_ms"] > d["max_ms"] else "within the dense spread")}
    del opt, params, base, grad, rows
    torch.cuda.empty_cache()
    return res


def graphed_step_cfg2(dev, seconds, repeats, pixels):
    """bench.py's with_adam_ms_per_step (headline mode: cfg2, frozen HPD, 2^20 pixels), dense and masked"""
    mode = "gngf_frozen"
    xy, target, bounds = bench.make_batch(bench.MODES[mode], pixels, 0, dev)
    net, _ = bench.build_model(mode, dev, bounds)
    # One model, two optimizers with their own moments, stepped in turns by the two captured steps: the parameters see both
    # updates.  That is fine for timing (the work per step does not depend on the values), not a way to train.
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    fns = {}
    for name, skip in (("dense", False), ("masked", True)):
        opt = train.get_optimizer(net, 1e-2, 1e-3, 1e-3, 0.0, 0.0, 1e-6, skip_unreachable_rows=skip)
        gs = train.GraphedStep(net, loss_fn, opt, 1, 1, 1e-3)
        gs(xy, target)
        torch.cuda.synchronize()
        assert opt._last_call == ("gngf_adam_step_masked" if skip else "gngf_adam_step"), opt._last_call
        fns[name] = gs.replay_only
    times, steps = alternate(fns, seconds, repeats)
    rows = net.reachable_rows()
    T = net._hash_table_size
    reach = [int(unpack(rows[l], T).sum()) for l in range(rows.shape[0])]
    d, m = summary(times["dense"]), summary(times["masked"])
    return {"mode": mode, "pixels": pixels, "steps_per_window": steps, "dense": d, "masked": m,
            "masked_over_dense": m["median_ms"] / d["median_ms"], "reachable_share": sum(reach) / (len(reach) * T),
            "reachable_share_per_level": [round(r / T, 5) for r in reach]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg4,cfg5")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pixels", type=int, default=2 ** 20)
    ap.add_argument("--no-graphed-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_masked.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_adam_masked.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "window_seconds": a.window, "repeats": a.repeats, "adam_step_alone": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        res["adam_step_alone"][name] = adam_alone(name, dev, a.window, a.repeats)
        r = res["adam_step_alone"][name]
        print(f"[{name}] reachable {r['reachable_share']:.3f}  dense {r['dense']['median_ms']:.4f} ms  masked {r['masked']['median_ms']:.4f} ms  "
              f"({r['verdict']})", flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.no_graphed_step:
        res["graphed_step_cfg2"] = graphed_step_cfg2(dev, a.window, a.repeats, a.pixels)
        r = res["graphed_step_cfg2"]
        print(f"[GraphedStep cfg2] dense {r['dense']['median_ms']:.4f} ms  masked {r['masked']['median_ms']:.4f} ms", flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
