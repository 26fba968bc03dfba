"""Times what a driver loop does after every epoch — the reassembled image, train_accuracy and train_psnr (reference
functions.py:308, 332-335, 690-692) — at the headline image size (2^20 pixels x 3 channels), on random outputs and a random
image, in one process:

  host tail     data.reassemble_image (gather, * 255, int, copy of the whole image to the host) + train.calc_psnr +
                train.calc_accuracy in numpy: what the tree did before train.EpochImage
  device tail   EpochImage.begin() + add() per batch + psnr() + accuracy(), with 1 and 3 batches per epoch, once without and
                once with image() (the bulk copy, on demand)

Host clock around each pass, a device synchronise before and after; --warmup passes, then the median and min-max of --passes
passes.  The two kernels' own times come from HIP events around their entry points.  Checks first that both tails give the
same numbers.

    python tools/time_epoch_tail.py --out profiles/epoch_tail.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collision_handling_in_instantngp_amd import data, ops, train  # noqa: E402


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


def host_clock(fn, warmup, passes):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return summary(out)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024, help="the image is side x side x 3 (default: 2^20 pixels)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--commit", default=None, help="commit the tree was built from (default: asked of git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_tail.json"))
    a = ap.parse_args()
    if a.passes < 20:
        sys.exit("at least 20 passes")
    if not torch.cuda.is_available():
        sys.exit("time_epoch_tail.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    h = w = a.side
    P, C = h * w, 3
    rng = np.random.default_rng(0)
    og = rng.integers(0, 256, size=(h, w, C)).astype(np.uint8)
    outputs = torch.rand((P, C), generator=torch.Generator().manual_seed(0)).to(dev)
    shuffled, reordered = data.make_permutation(P, torch.Generator().manual_seed(1))
    reordered_dev = reordered.to(dev)
    ep = train.EpochImage(og, shuffled, device=dev)

    def slices(nb):
        step = P if nb == 1 else int(P / nb)
        return [(b * step, step) for b in range(nb)]

    def host_tail():
        img = data.reassemble_image(outputs, reordered_dev, h, w)
        return train.calc_psnr(img, og), train.calc_accuracy(img, og, img.size)

    def device_tail(nb, with_image):
        batches = [(outputs[lo:lo + n], lo) for lo, n in slices(nb)]      # (contiguous row slices: views, as a step's outputs are)

        def run():
            ep.begin()
            for out, lo in batches:
                ep.add(out, lo)
            res = (ep.psnr(), ep.accuracy())
            if with_image:
                ep.image()
            return res
        return run

    # the two tails agree exactly (one batch: every pixel visited, so the host tail on `outputs` is the same epoch)
    want = host_tail()
    got = device_tail(1, False)()
    assert got == (float(want[0]), float(want[1])), (got, want)
    assert np.array_equal(ep.image(), data.reassemble_image(outputs, reordered_dev, h, w))

    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_of_tree(),
           "shape": {"h": h, "w": w, "channels": C, "pixels": P, "elements": P * C},
           "warmup_passes": a.warmup, "timed_passes": a.passes,
           "method": "host clock around each pass, device synchronise before and after; kernels: HIP events around the entry point",
           "psnr": got[0], "accuracy": got[1], "tails_agree_exactly": True}
    res["host_tail"] = host_clock(host_tail, a.warmup, a.passes)
    res["host_tail"]["what"] = "data.reassemble_image + train.calc_psnr + train.calc_accuracy"
    res["host_tail_parts"] = {
        "reassemble_image": host_clock(lambda: data.reassemble_image(outputs, reordered_dev, h, w), a.warmup, a.passes)}
    img_host = data.reassemble_image(outputs, reordered_dev, h, w)
    res["host_tail_parts"]["calc_psnr"] = host_clock(lambda: train.calc_psnr(img_host, og), a.warmup, a.passes)
    res["host_tail_parts"]["calc_accuracy"] = host_clock(lambda: train.calc_accuracy(img_host, og, img_host.size), a.warmup, a.passes)
    res["device_tail"] = {}
    for nb in (1, 3):
        res["device_tail"][f"batches_{nb}"] = {
            "begin_add_psnr_accuracy": host_clock(device_tail(nb, False), a.warmup, a.passes),
            "with_image_copy": host_clock(device_tail(nb, True), a.warmup, a.passes)}
    # the kernels alone
    third = int(P / 3)
    sums, ws = torch.zeros(2, dtype=torch.int64, device=dev), ops.image_metrics_workspace(P * C, dev)
    ident = torch.arange(P, dtype=torch.int32, device=dev)
    res["kernels"] = {
        "image_scatter_whole_epoch_permuted": device_events(lambda: ops.image_scatter(outputs, ep.perm, ep.img, 0), a.warmup, a.passes),
        "image_scatter_whole_epoch_identity_perm": device_events(lambda: ops.image_scatter(outputs, ident, ep.img, 0), a.warmup, a.passes),
        "image_scatter_whole_epoch_no_perm": device_events(lambda: ops.image_scatter(outputs, None, ep.img, 0), a.warmup, a.passes),
        "image_scatter_one_third_permuted": device_events(lambda: ops.image_scatter(outputs[:third], ep.perm, ep.img, 0), a.warmup, a.passes),
        "image_metrics": device_events(lambda: ops.image_metrics(ep.img, ep.target, sums, ws), a.warmup, a.passes),
        "begin_zero_fill": device_events(ep.begin, a.warmup, a.passes),
        "bytes": {"image_scatter": {"read": P * C * 4 + P * 4, "written": P * C * 4},
                  "image_metrics": {"read": P * C * 5, "written": 8 * int(ws.numel()) + 16}}}
    d1 = res["device_tail"]["batches_1"]["begin_add_psnr_accuracy"]
    res["host_over_device_median"] = {
        f"batches_{nb}": res["host_tail"]["median_ms"] / res["device_tail"][f"batches_{nb}"]["begin_add_psnr_accuracy"]["median_ms"]
        for nb in (1, 3)}
    res["device_tail_is_shorter"] = bool(all(
        res["device_tail"][f"batches_{nb}"]["begin_add_psnr_accuracy"]["max_ms"] < res["host_tail"]["min_ms"] for nb in (1, 3)))
    print(f"host tail {res['host_tail']['median_ms']:.3f} ms; device tail {d1['median_ms']:.3f} ms (1 batch), "
          f"{res['device_tail']['batches_3']['begin_add_psnr_accuracy']['median_ms']:.3f} ms (3 batches)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
