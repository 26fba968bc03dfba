"""Times the picture of a model on a pixel lattice, two ways in one process, for two models (L = 16, F = 2, T = 2^19, N_l 16 .. 512:
the headline shape) — the spatial hash and a frozen HPD (per-vertex table):

  render        train.render(net, side, side, image=True): one launch of gngf_render (csrc/render.inc), outputs preallocated
  module path   what the tree offered before: net(x, 1.0) under no_grad with return_indices = False on an explicit (P, 2)
                coordinate tensor — binning, tiled / direct encoder, (P, L F) encoding, gngf_decoder_fwd — followed by
                data.reassemble_image_device

HIP events around each pass, a device synchronise before and after; --warmup passes, then the median and min-max of --passes
passes; the module path's entry points are timed once more, one by one (HIP events through _lib.PROFILE).  Then one render at
--big x --big with torch.cuda.max_memory_allocated for both ways (the module path's only if it fits).  Checks first that both
ways give the same image up to the integer rounding of values the two evaluations round differently.

    python tools/time_render.py --out profiles/render.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collision_handling_in_instantngp_amd import _lib, data, models, train  # noqa: E402


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


def build(mode, T):
    """(the caller has set models.should_use_hash_function for `mode`)"""
    torch.manual_seed(0)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T, num_levels=16, n_min=16, n_max=512,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=T, feature_dim=2, topk_k=4)
    with torch.no_grad():
        for m in net.encoding._hash_tables:
            m.weight.uniform_(-1.0, 1.0)              # (the +-1e-4 start would render one colour)
    net.return_indices = False
    if mode != "hash":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.dense_probs, net.compute_pbar = False, False      # the frozen-HPD forward on the cached per-vertex table
    return net


def coords(side, dev):
    return data.normalise_coordinates(torch.from_numpy(data.pixel_grid(side, side)).float(), side, side).to(dev)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"peak_bytes_above_start": int(torch.cuda.max_memory_allocated() - base)}


def measure(mode, a, dev):
    models.should_use_hash_function = mode == "hash"
    try:
        net = build(mode, a.table)
        side = a.side
        x = coords(side, dev)
        out_image = torch.empty((side, side, 3), dtype=torch.int32, device=dev)
        out_rgb = torch.empty((side * side, 3), dtype=torch.float32, device=dev)

        def render():
            return train.render(net, side, side, out_rgb=out_rgb, out_image=out_image)

        def module_path():
            with torch.no_grad():
                out = net(x, 1.0)[0]
            return data.reassemble_image_device(out, None, side, side, should_shuffle=False)

        a_img = render()[1].clone()
        b_img = module_path()
        differ = int((a_img != b_img).sum())
        assert int((a_img - b_img).abs().max()) <= 1 and differ < 0.02 * a_img.numel(), (differ, a_img.numel())
        res = {"mode": mode, "lattice": [side, side], "pixels": side * side, "elements_that_differ_by_one": differ,
               "render": device_events(render, a.warmup, a.passes), "module_path": device_events(module_path, a.warmup, a.passes)}
        _lib.PROFILE = {}
        try:
            for _ in range(5):
                module_path()
            torch.cuda.synchronize()
            res["module_path_entry_points_ms"] = {k: float(np.median([e0.elapsed_time(e1) for e0, e1 in v])) for k, v in _lib.PROFILE.items()}
            _lib.PROFILE = {}
            for _ in range(5):
                render()
            torch.cuda.synchronize()
            res["render_entry_points_ms"] = {k: float(np.median([e0.elapsed_time(e1) for e0, e1 in v])) for k, v in _lib.PROFILE.items()}
        finally:
            _lib.PROFILE = None
        res["render_is_not_slower"] = bool(res["render"]["median_ms"] <= res["module_path"]["median_ms"])
        # the large lattice: peak allocation of each way (outputs included: a caller who wants the picture needs them)
        big = a.big
        del x, out_image, out_rgb, a_img, b_img
        torch.cuda.empty_cache()
        res["big"] = {"lattice": [big, big], "render": peak_of(lambda: train.render(net, big, big, rgb=False, image=True))}
        res["big"]["render"].update(device_events(lambda: train.render(net, big, big, rgb=False, image=True), 2, 5))
        try:
            xb = coords(big, dev)

            def big_module():
                with torch.no_grad():
                    out = net(xb, 1.0)[0]
                data.reassemble_image_device(out, None, big, big, should_shuffle=False)
            big_module()
            res["big"]["module_path"] = peak_of(big_module)
            res["big"]["module_path"]["coordinate_tensor_bytes"] = int(xb.numel() * 4)
            del xb
        except torch.OutOfMemoryError:
            res["big"]["module_path"] = "did not fit"
        torch.cuda.empty_cache()
        return res
    finally:
        models.should_use_hash_function = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--table", type=int, default=2 ** 19)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_render.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_of_tree(),
           "model": {"L": 16, "F": 2, "T": a.table, "n_min": 16, "n_max": 512, "K": 4},
           "warmup_passes": a.warmup, "timed_passes": a.passes,
           "method": "HIP events around each pass, device synchronise before and after; both ways in one process",
           "shapes": [measure(mode, a, dev) for mode in ("hash", "frozen_hpd")]}
    for s in res["shapes"]:
        print(f"{s['mode']}: render {s['render']['median_ms']:.3f} ms, module path {s['module_path']['median_ms']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
