#!/usr/bin/env python3
"""Times gngf_logits_topk_pbar (statistics + top-K, no p-bar: L = 0) per (U, T, K) with HIP events: after a warm-up, `--reps` launches
timed one by one, median / min / max in ms.  One process times ONE tree (--root: the repository whose package is imported, so a
clean checkout of the parent commit can be timed beside this one on the same box); --merge puts the per-tree files of a session
together into profiles/topk_wide.json and evaluates the condition "K = 128 takes at most 4x the parent's K = 32 on the same (U, T)".

    python tools/time_topk_wide.py --label branch --ks 32,33,64,128 --out out/topk_branch_1.json
    python tools/time_topk_wide.py --root PARENT_CHECKOUT --label parent --ks 32 --out out/topk_parent_1.json
    python tools/time_topk_wide.py --merge out/topk_parent_1.json out/topk_branch_1.json ... --out profiles/topk_wide.json
"""
import argparse
import json
import os
import socket
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_tree(args):
    root = os.path.abspath(args.root or HERE)
    sys.path.insert(0, root)
    import torch
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = "cuda"
    rows = []
    for shape in args.shapes.split(","):
        U, T = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(U + T)
        z = torch.empty((U, T), device=dev)
        for r0 in range(0, U, 512):                                 # (logits of an HPD's scale, drawn in slabs)
            z[r0:r0 + 512].normal_(0.0, 3.0, generator=gen)
        for K in (int(k) for k in args.ks.split(",")):
            if K > T:
                continue
            tv = torch.empty((U, K), device=dev)
            ti = torch.empty((U, K), dtype=torch.int32, device=dev)
            rowstat = torch.empty((U, 2), device=dev)

            def launch():
                call("gngf_logits_topk_pbar", ptr(z), ptr(tv), ptr(ti), ptr(rowstat), ptr(None), 0, ptr(None), U, T, K, stream_ptr())
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            assert int(ti.min()) >= 0 and int(ti.max()) < T
            rows.append({"U": U, "T": T, "K": K, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms),
                         "logit_bytes": 4 * U * T})
            print(f"{args.label}: U={U} T={T} K={K}: median {rows[-1]['median_ms']:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, n={len(ms)})",
                  flush=True)
        del z
        torch.cuda.empty_cache()
    out = {"label": args.label, "commit": args.commit, "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "method": f"HIP events around each launch, {args.warmup} warm-up launches, median of {args.reps}", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def merge(args):
    runs = [json.load(open(p)) for p in args.merge]
    out = {"what": "gngf_logits_topk_pbar (statistics + top-K, L = 0) at (U, T) = (4096, 2^19) and (324, 256): the parent commit at K = 32 "
                   "and this change at K = 32, 33, 64, 128, one box, one session, the trees alternating; tools/time_topk_wide.py",
           "runs": runs}
    med = {}
    for r in runs:
        for row in r["rows"]:
            med.setdefault((r["label"], row["U"], row["T"], row["K"]), []).append(row["median_ms"])
    cond = []
    for (label, U, T, K), v in sorted(med.items()):
        if label == "branch" and K == 128 and ("parent", U, T, 32) in med:
            p32 = med[("parent", U, T, 32)]
            ratio = statistics.median(v) / statistics.median(p32)
            cond.append({"U": U, "T": T, "branch_K128_ms": v, "parent_K32_ms": p32, "ratio": ratio, "limit": 4.0, "met": ratio <= 4.0})
    narrow = []
    for (label, U, T, K), v in sorted(med.items()):
        if label == "branch" and K == 32 and ("parent", U, T, 32) in med:
            narrow.append({"U": U, "T": T, "parent_K32_ms": med[("parent", U, T, 32)], "branch_K32_ms": v})
    out["narrow_path_parity"] = narrow
    out["wide_condition"] = cond
    if args.bench:
        out["headline_bench"] = [json.loads(line) for p in args.bench for line in open(p) if line.startswith("{")]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"narrow_path_parity": narrow, "wide_condition": cond}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="repository whose package is timed (default: this one)")
    ap.add_argument("--label", default="branch")
    ap.add_argument("--commit", default="")
    ap.add_argument("--shapes", default="4096x524288,324x256")
    ap.add_argument("--ks", default="32,33,64,128")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "out", "topk_wide_run.json"))
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench", nargs="*", default=None, help="--merge: files holding bench.py lines to carry along")
    args = ap.parse_args()
    if args.merge:
        merge(args)
    else:
        time_tree(args)


if __name__ == "__main__":
    main()
