"""Writes tests/golden/G20_epoch_loop.npz: what the reference's epoch loop decides on planted inputs.  Runs on the CPU of
the build machine, where the reference is present (oracle.ref_harness); the file holds data only.

  es/<name>/...    traces of the reference's utils.EarlyStopping: constructor arguments, the losses it was called with and
                   (counter, best_loss, early_stop) after every call
  loop/<name>/...  runs of the reference's own functions.grid_search_loop with functions.train_step replaced, at run time, by
                   a stub that returns planted (loss, int32 image, collisions) per epoch: the inputs, the epochs at which it
                   saved (torch.save of whole_model.pt), how many epochs it ran and why it stopped (from what it printed)

    python tools/make_epoch_loop_golden.py [--out tests/golden/G20_epoch_loop.npz]
"""
import argparse
import contextlib
import io
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def f32(values):
    """planted losses are fp32 values (what a training step produces), handed to the reference as float64 as np.mean does"""
    return np.asarray(values, dtype=np.float32).astype(np.float64)


def es_cases():
    nan, inf = float("nan"), float("inf")
    fall = [1.0 - 0.05 * i for i in range(6)]
    return {
        "equal": dict(tolerance=3, min_delta=1e-3, should_reset=True, losses=[0.5] * 8),
        "within_delta_above": dict(tolerance=3, min_delta=1e-2, should_reset=True, losses=[0.5, 0.505, 0.507, 0.509, 0.5, 0.52, 0.54, 0.56]),
        "within_delta_below": dict(tolerance=3, min_delta=1e-2, should_reset=True, losses=[0.5, 0.495, 0.493, 0.491, 0.4, 0.399, 0.398, 0.397]),
        "min_delta_0": dict(tolerance=2, min_delta=0.0, should_reset=True, losses=[0.5, 0.5, 0.4, 0.4, 0.45, 0.3, 0.35, 0.36]),
        "tolerance_1": dict(tolerance=1, min_delta=1e-3, should_reset=True, losses=fall + [0.9, 0.1]),
        "tolerance_0": dict(tolerance=0, min_delta=1e-3, should_reset=True, losses=[0.5, 0.4]),
        "no_reset": dict(tolerance=3, min_delta=1e-3, should_reset=False, losses=[0.5, 0.6, 0.4, 0.7, 0.8, 0.3, 0.9, 1.0, 1.1]),
        "no_reset_from_zero": dict(tolerance=2, min_delta=1e-3, should_reset=False, losses=[0.5, 0.5, 0.5]),
        "nan": dict(tolerance=2, min_delta=1e-3, should_reset=True, losses=[0.5, 0.6, nan, 0.7, 0.8, 0.9, 0.1]),
        "inf": dict(tolerance=2, min_delta=1e-3, should_reset=True, losses=[0.5, inf, 0.6, inf, inf, 0.7, 0.8]),
        "inf_first": dict(tolerance=2, min_delta=1e-3, should_reset=True, losses=[inf, inf, 0.5, 0.6, 0.7]),
        "growing": dict(tolerance=4, min_delta=1e-6, should_reset=True, losses=fall + [0.8, 0.81, 0.82, 0.7, 0.83, 0.84, 0.85, 0.86]),
    }


def trace_early_stopping(utils, case):
    es = utils.EarlyStopping(tolerance=case["tolerance"], min_delta=case["min_delta"], should_reset=case["should_reset"])
    losses = f32(case["losses"])
    counter, best, stop = [], [], []
    with np.errstate(invalid="ignore"):
        for v in losses:
            es(np.float64(v))
            counter.append(es.counter), best.append(es.best_loss), stop.append(es.early_stop)
    return {"tolerance": np.int64(case["tolerance"]), "min_delta": np.float64(case["min_delta"]),
            "should_reset": np.bool_(case["should_reset"]), "losses": losses, "counter": np.asarray(counter, dtype=np.int64),
            "best_loss": np.asarray(best, dtype=np.float64), "early_stop": np.asarray(stop, dtype=bool)}


def loop_cases():
    """per case: epochs, tolerance, min_delta, peak (every element of the target), per-epoch loss, per-epoch difference
    image - target as a list of 12 integers (or one integer for all 12 elements), per-epoch collisions (L values)"""
    fall = lambda n, a=1.0, s=0.03: [a - s * i for i in range(n)]      # noqa: E731
    busy = [5, 3, 2, 1]
    free = [7, 4, 0, 0]
    cases = {}
    # the loss falls, then grows three times in a row: the stopper fires in epoch 10, the loop breaks in epoch 11
    cases["plateau_tol3"] = dict(epochs=40, tolerance=3, min_delta=1e-4, peak=255, losses=fall(8) + [0.9, 0.95, 1.0, 1.05, 1.1, 1.15],
                                 diff=[20, 18, 16, 14, 12, 10, 9, 8, 9, 10, 7, 11, 12, 13], collisions=[busy] * 14)
    # ten epochs (1..10) without collisions at the last two levels: stop in epoch 10 itself
    cases["zero_collisions"] = dict(epochs=40, tolerance=50, min_delta=1e-4, peak=255, losses=fall(14),
                                    diff=[30 - 2 * i for i in range(14)], collisions=[busy] + [free] * 13)
    # one of the ten checks fails: the rule never fires, the run reaches `epochs`
    cases["zero_collisions_broken"] = dict(epochs=14, tolerance=50, min_delta=1e-4, peak=255, losses=fall(14),
                                           diff=[30 - 2 * i for i in range(14)], collisions=[free] * 5 + [[7, 4, 0, 1]] + [free] * 8)
    # only the last level is free: not enough
    cases["zero_last_level_only"] = dict(epochs=13, tolerance=50, min_delta=1e-4, peak=255, losses=fall(13),
                                         diff=[30 - 2 * i for i in range(13)], collisions=[[7, 4, 2, 0]] * 13)
    # one level (L = 1): the check looks at that level twice
    cases["zero_collisions_one_level"] = dict(epochs=40, tolerance=50, min_delta=1e-4, peak=255, losses=fall(14),
                                              diff=[30 - 2 * i for i in range(14)], collisions=[[0]] * 14)
    # PSNR ties (equal sse: saved again), an sse = 0 epoch (PSNR inf: afterwards only another inf saves), reaches `epochs`
    cases["ties_and_exact"] = dict(epochs=10, tolerance=50, min_delta=1e-4, peak=255, losses=fall(10),
                                   diff=[9, 9, 8, 10, 8, 0, 1, 0, 3, 0], collisions=[busy] * 10)
    # the same sse from different images: a tie of the sums, not of the pictures
    cases["tie_other_image"] = dict(epochs=5, tolerance=50, min_delta=1e-4, peak=255, losses=fall(5),
                                    diff=[[2] * 12, [4, 4, 4] + [0] * 9, [0] * 9 + [4, 4, 4], [5] + [0] * 11, [3, 4] + [0] * 10],
                                    collisions=[busy] * 5)
    # target peak 1: PSNR = -10 log10(mse) is negative while mse > 1 — nothing is saved until it reaches 0
    cases["negative_psnr_first"] = dict(epochs=8, tolerance=50, min_delta=1e-4, peak=1, losses=fall(8),
                                        diff=[5, 3, 2, [1] * 12, [1] * 11 + [2], [1] * 11 + [0], 2, 0], collisions=[busy] * 8)
    # the stopper fires in epoch 9 and the zero-collision rule in epoch 10: one break, in epoch 10
    cases["stopper_then_zero"] = dict(epochs=40, tolerance=2, min_delta=1e-4, peak=255, losses=fall(8) + [0.9, 1.0, 1.1, 1.2, 1.3],
                                      diff=[30 - 2 * i for i in range(13)], collisions=[busy] + [free] * 12)
    # the stopper fires in the very last epoch: the run ends because `epochs` is reached
    cases["fires_in_last_epoch"] = dict(epochs=8, tolerance=2, min_delta=1e-4, peak=255, losses=fall(6) + [0.9, 1.0],
                                        diff=[30 - 2 * i for i in range(8)], collisions=[busy] * 8)
    # ... and one epoch earlier: the break comes in the last epoch
    cases["fires_before_last_epoch"] = dict(epochs=8, tolerance=2, min_delta=1e-4, peak=255, losses=fall(5) + [0.9, 1.0, 1.1],
                                            diff=[30 - 2 * i for i in range(8)], collisions=[busy] * 8)
    # improvements smaller than min_delta count as a stall (first branch of the stopper)
    cases["stall_below_delta"] = dict(epochs=40, tolerance=3, min_delta=1e-2, peak=255,
                                      losses=[1.0, 0.9, 0.899, 0.898, 0.897, 0.896, 0.895, 0.894], diff=[12, 11, 10, 9, 8, 7, 6, 5],
                                      collisions=[busy] * 8)
    # a NaN loss becomes best_loss and resets the stopper at every call from then on: runs to `epochs`
    cases["nan_loss"] = dict(epochs=9, tolerance=2, min_delta=1e-4, peak=255, losses=[1.0, 0.9, 1.0, float("nan"), 2.0, 3.0, 4.0, 5.0, 6.0],
                             diff=[12, 11, 10, 9, 8, 7, 6, 5, 4], collisions=[busy] * 9)
    cases["inf_loss"] = dict(epochs=12, tolerance=2, min_delta=1e-4, peak=255,
                             losses=[1.0, 0.9, float("inf"), 0.8, float("inf"), float("inf"), 0.7, 0.6, 0.5, 0.4, 0.3, 0.2],
                             diff=[12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1], collisions=[busy] * 12)
    # tolerance 0: the first call of the stopper (epoch 1) fires
    cases["tolerance_0"] = dict(epochs=9, tolerance=0, min_delta=1e-4, peak=255, losses=fall(4), diff=[12, 11, 10, 9], collisions=[busy] * 4)
    cases["one_epoch"] = dict(epochs=1, tolerance=3, min_delta=1e-4, peak=255, losses=[1.0], diff=[3], collisions=[busy])
    return cases


H, W = 2, 2                     # the planted image: 2 x 2 x 3 = 12 elements


def run_reference_loop(ref, case):
    import torch
    import matplotlib.pyplot as plt
    functions, utils, _models, _params = ref
    from oracle import ref_harness

    n_planted = len(case["losses"])
    losses = f32(case["losses"])
    target = np.full((H, W, 3), case["peak"], dtype=np.uint8)
    images = np.stack([target.astype(np.int32) + np.broadcast_to(np.asarray(d, dtype=np.int32), (12,)).reshape(H, W, 3)
                       for d in case["diff"]])
    collisions = np.asarray(case["collisions"], dtype=np.int64)
    assert len(images) == n_planted == len(collisions)
    calls = []

    def stub_train_step(**_kw):
        e = len(calls)
        if e >= n_planted:
            raise RuntimeError(f"the reference asked for epoch {e}: {n_planted} were planted")
        calls.append(e)
        plt.close("all")
        return (np.float64(losses[e]), images[e].copy(), torch.from_numpy(collisions[e].copy()), torch.zeros(collisions.shape[1]),
                [], np.float64(losses[e]), np.zeros(collisions.shape[1]), np.zeros(collisions.shape[1]), [])

    class StandIn(torch.nn.Module):
        def __init__(self, **_kw):
            super().__init__()
            self.encoding, self.HPD, self.mlp = torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)

    saved = []
    real_save = torch.save

    def recording_save(obj, path, *a, **k):
        if os.path.basename(str(path)) == "whole_model.pt":
            saved.append(calls[-1])
        return real_save(obj, path, *a, **k)

    ref_harness.set_flag((functions,), "epochs", int(case["epochs"]))
    ref_harness.set_flag((functions,), "tolerance", case["tolerance"])
    ref_harness.set_flag((functions,), "min_delta", case["min_delta"])
    ref_harness.set_flag((functions,), "should_save_params", True)
    ref_harness.set_flag((functions,), "histograms_rate", 10 ** 9)
    real = (functions.train_step, getattr(functions.wandb, "finish", None), plt.show)
    functions.train_step = stub_train_step
    functions.wandb.finish = lambda *a, **k: None
    plt.show = functions.plt.show = lambda *a, **k: None
    torch.save = recording_save
    params = dict(should_shuffle_pixels=False, should_keep_topk_only=False, should_sum_js_kl_div=False, loss_gamma=0, should_js_div=False,
                  l_mse=1, l_js_kl=1, l_collisions=1, MLP_lr=1e-3, HPD_lr=1e-3, topk_k=1)
    out = io.StringIO()
    try:
        with tempfile.TemporaryDirectory() as folder, contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()), \
                np.errstate(all="ignore"):
            functions.grid_search_loop([params], torch.zeros(H * W, 2), torch.zeros(H * W, 3), W, H, "planted", target,
                                       torch.arange(H * W), torch.arange(H * W), StandIn, lambda **kw: None, utils.EarlyStopping,
                                       is_test_only=True, wandb_name="golden", drive_folder=folder)
    finally:
        functions.train_step, plt.show = real[0], real[2]
        functions.plt.show = real[2]
        if real[1] is not None:
            functions.wandb.finish = real[1]
        torch.save = real_save
        plt.close("all")
    # why it stopped, from what the loop printed (functions.py:687, 800): the first message whose break was reached
    said = [(int(m.group(1)), "zero_collisions" if m.group(2) else "early_stopping")
            for m in re.finditer(r"!!! Stopping at epoch: (\d+) (?:( because of 0 collisions)|)!!!", out.getvalue())]
    run = len(calls)
    reason = "epochs"
    for at, why in said:
        broke_at = at if why == "zero_collisions" else at + 1
        if broke_at == run - 1:
            reason = why
            break
    if reason == "epochs":
        assert run == case["epochs"], (run, case["epochs"], said)
    diff = images - target.astype(np.int32)[None]
    return {"epochs": np.int64(case["epochs"]), "tolerance": np.int64(case["tolerance"]), "min_delta": np.float64(case["min_delta"]),
            "losses": losses, "target": target, "images": images.astype(np.int32), "collisions": collisions,
            "sse": (diff.astype(np.int64) ** 2).reshape(n_planted, -1).sum(1), "eq": (diff == 0).reshape(n_planted, -1).sum(1).astype(np.int64),
            "saved_epochs": np.asarray(saved, dtype=np.int64), "epochs_run": np.int64(run), "stop_reason": np.str_(reason)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "G20_epoch_loop.npz"))
    args = ap.parse_args()
    from oracle import ref_harness
    if not ref_harness.available():
        sys.exit("the reference is not present: the golden can only be regenerated where it is")
    ref = ref_harness.load_reference()
    data = {}
    es = es_cases()
    for name, case in es.items():
        for k, v in trace_early_stopping(ref[1], case).items():
            data[f"es/{name}/{k}"] = v
    loops = loop_cases()
    for name, case in loops.items():
        got = run_reference_loop(ref, case)
        print(f"{name}: ran {int(got['epochs_run'])} of {case['epochs']} epochs, saved at {got['saved_epochs'].tolist()}, "
              f"stopped by {got['stop_reason']}")
        for k, v in got.items():
            data[f"loop/{name}/{k}"] = v
    data["es_names"] = np.asarray(sorted(es), dtype=np.str_)
    data["loop_names"] = np.asarray(sorted(loops), dtype=np.str_)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
