"""Times the epoch loop at the headline shape (BASELINE configs[1]: L = 16, F = 2, T = 2^19, K = 4, N 16 -> 512; a synthetic
1024 x 1024 image, 2^20 pixels, one batch per epoch; hash and frozen-GNGF indexing), per epoch, in one process:

  (i)   bare steps    train.train_epoch(graph=True, slot_counts=True): the epoch's step replayed from its hipGraph, nothing after it
  (ii)  train.fit     the steps + EpochImage + gngf_epoch_tail + the predicated snapshot copies, polled every 16 epochs
  (iii) today's loop  what a user writes without fit: train.train_step(graph=True, image=...) + EpochImage.psnr() + a host
                      EarlyStopping + data.save_checkpoint whenever the PSNR does not fall (functions.py:761-780)

(ii) and (iii) alternate, --passes times each, after a warm-up pass of each; every pass is a host clock around the whole
call, device synchronised either side, divided by its epochs.  (ii) - (i) is the loop's overhead.  The two kernels' own
times come from HIP events; the snapshot's bytes from the DeviceSnapshot.

    python tools/time_epoch_loop.py --out profiles/epoch_loop.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from collision_handling_in_instantngp_amd import data, models, ops, train  # noqa: E402

LRS = (1e-4, 1e-3, 1e-3, 0, 1e-6, 1e-6)         # the reference's params.py
WEIGHTS = dict(l_mse=1, l_js_kl=1, l_collisions=1e-3)


def commit_of_tree():
    try:
        head = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(["git", "status", "--porcelain"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        return head + ("+" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def summary(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "passes": int(a.size)}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_events(fn, warmup, passes):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return summary(out)


def measure(mode, a, dev, folder):
    side = a.side
    P = side * side
    rng = np.random.default_rng(0)
    og = rng.integers(0, 256, size=(side, side, 3)).astype(np.uint8)
    X = data.normalise_coordinates(torch.from_numpy(data.pixel_grid(side, side)).float(), side, side).to(dev)
    Y = torch.from_numpy(og.reshape(-1, 3).astype(np.float64) / 255).float().to(dev)
    shuffled, reordered = data.make_permutation(P, torch.Generator().manual_seed(1))
    shuffled, reordered = shuffled.to(dev), reordered.to(dev)
    net, _models = bench.build_model(mode, dev, (1.0, 1.0))
    c = bench.SHAPES[bench.MODES[mode]]
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    opt = train.get_optimizer(net, *LRS)
    assert isinstance(opt, train.FusedAdam)

    def bare(n):
        for _ in range(n):
            train.train_epoch(net, loss_fn, opt, X, Y, side, side, WEIGHTS["l_mse"], WEIGHTS["l_js_kl"], WEIGHTS["l_collisions"],
                              batch_percentage=1.0, should_shuffle=True, shuffled_indices=shuffled, graph=True, slot_counts=True)

    def fit(n):
        # a tolerance no run reaches: every pass runs its n epochs
        return train.fit(net, loss_fn, opt, X, Y, side, side, og, epochs=n, tolerance=10 ** 9, min_delta=1e-6, batch_percentage=1.0,
                         should_shuffle=True, shuffled_indices=shuffled, graph=True, poll_every=16, **WEIGHTS)

    ep = train.EpochImage(og, shuffled, device=dev)

    def todays_loop(n):
        stopper = train.EarlyStopping(tolerance=10 ** 9, min_delta=1e-6)
        best, saves = 0, 0
        pc = pm = None
        for e in range(n):
            out = train.train_step(net, loss_fn, opt, X, Y, side, side, c["T"], c["K"], WEIGHTS["l_mse"], WEIGHTS["l_js_kl"],
                                   WEIGHTS["l_collisions"], 1.0, c["L"], False, False, True, shuffled, reordered, pc, pm, graph=True,
                                   image=ep)
            pc, pm = out[2], out[3]
            psnr = ep.psnr()
            if psnr >= best:
                best = psnr
                data.save_checkpoint(net, opt, folder)
                saves += 1
            if stopper.early_stop:
                break
            if e != 0:
                stopper(out[0])
        return saves

    # warm-up: graph capture, lazy workspaces, the file system
    bare(a.warmup_epochs)
    fit(a.warmup_epochs)
    todays_loop(2)
    res = {"bare_steps": [], "fit": [], "todays_loop": [], "fit_saved_epochs": [], "todays_loop_saves": []}
    for _ in range(a.passes):
        ms, _o = clocked(lambda: bare(a.epochs))
        res["bare_steps"].append(ms / a.epochs)
        ms, r = clocked(lambda: fit(a.epochs))
        assert r.last_epoch == a.epochs - 1 and r.stop_reason == "epochs" and r.issued == a.epochs
        res["fit"].append(ms / a.epochs)
        res["fit_saved_epochs"].append(int(r.log["saved"].sum()))
        ms, saves = clocked(lambda: todays_loop(a.loop_epochs))
        res["todays_loop"].append(ms / a.loop_epochs)
        res["todays_loop_saves"].append(saves)
    out = {"per_epoch_ms": {k: dict(summary(res[k]), per_pass_ms=res[k]) for k in ("bare_steps", "fit", "todays_loop")},
           "epochs_per_pass": {"bare_steps": a.epochs, "fit": a.epochs, "todays_loop": a.loop_epochs},
           "fit_saved_epochs_per_pass": res["fit_saved_epochs"], "todays_loop_saves_per_pass": res["todays_loop_saves"]}
    over = [f - b for f, b in zip(res["fit"], res["bare_steps"])]
    out["fit_overhead_over_bare_steps_ms"] = dict(summary(over), per_pass_ms=over)
    out["fit_is_not_slower_than_todays_loop"] = bool(max(res["fit"]) <= min(res["todays_loop"]))
    out["todays_loop_over_fit_median"] = out["per_epoch_ms"]["todays_loop"]["median_ms"] / out["per_epoch_ms"]["fit"]["median_ms"]

    # the two kernels alone, at this model's snapshot
    snap = train.DeviceSnapshot(train.state_tensors(net, opt))
    flag = torch.ones((1,), dtype=torch.int32, device=dev)
    out["snapshot_bytes"] = int(snap.bytes)
    out["kernels"] = {"snapshot_if_taken": device_events(lambda: snap.take_if(flag), 5, 25)}
    flag.zero_()
    out["kernels"]["snapshot_if_not_taken"] = device_events(lambda: snap.take_if(flag), 5, 25)
    out["kernels"]["snapshot_if_taken"]["GBps_read_plus_written"] = 2 * snap.bytes / (out["kernels"]["snapshot_if_taken"]["median_ms"] * 1e6)
    L = c["L"]
    state = train.epoch_state_tensor(10 ** 12, dev)
    n_tail = 64
    logf = torch.zeros((n_tail * 40, 2 + 2 * L), dtype=torch.float64, device=dev)
    logi = torch.zeros((n_tail * 40, 6 + L), dtype=torch.int64, device=dev)
    one = torch.rand((1,), device=dev)
    sums = torch.tensor([5, 10 ** 9], dtype=torch.int64, device=dev)
    used = torch.full((1, L), 7, dtype=torch.int32, device=dev)
    nverts = torch.from_numpy(np.asarray(net._level_vertex_counts(), dtype=np.int64)).to(dev)
    out["kernels"]["epoch_tail"] = device_events(
        lambda: ops.epoch_tail(state, logf, logi, one, one, None, None, sums, used, nverts, hash_source=True, tolerance=10 ** 9,
                               min_delta=1e-6, should_reset=True, epochs=n_tail * 40), 5, 25)
    models.should_use_hash_function = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024, help="the image is side x side x 3 (default: 2^20 pixels)")
    ap.add_argument("--modes", default="hash,gngf_frozen")
    ap.add_argument("--epochs", type=int, default=200, help="epochs per timed pass of the bare steps and of fit")
    ap.add_argument("--loop-epochs", type=int, default=12, help="epochs per timed pass of today's loop (it writes files)")
    ap.add_argument("--warmup-epochs", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit the tree was built from (default: asked of git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_loop.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_epoch_loop.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_of_tree(),
           "shape": {"config": "cfg2", "side": a.side, "pixels": a.side * a.side, "batches_per_epoch": 1},
           "method": "host clock around each pass of N epochs, device synchronised either side, divided by N; fit and today's loop "
                     "alternate in one process after a warm-up pass of each; kernels: HIP events around the entry point",
           "modes": {}}
    with tempfile.TemporaryDirectory() as folder:
        for mode in a.modes.split(","):
            res["modes"][mode] = measure(mode, a, dev, folder)
            m = res["modes"][mode]["per_epoch_ms"]
            print(f"{mode}: bare steps {m['bare_steps']['median_ms']:.3f} ms/epoch, fit {m['fit']['median_ms']:.3f}, today's loop "
                  f"{m['todays_loop']['median_ms']:.3f}; snapshot {res['modes'][mode]['snapshot_bytes']} bytes", flush=True)
    res["fit_is_not_slower_than_todays_loop"] = bool(all(m["fit_is_not_slower_than_todays_loop"] for m in res["modes"].values()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["fit_is_not_slower_than_todays_loop"]:
        sys.exit("fit() was slower than today's loop in this run")


if __name__ == "__main__":
    main()
