"""Times the picture of a BAKED model (train.bake -> BakedGrid.render: gngf_render_grid, csrc/render.inc) against the ways the tree
already had, all in one process, for the headline shape (L = 16, F = 2, T = 2^19, N_l 16 .. 512, K = 4) with the spatial hash and
with a frozen HPD:

  render        train.render(net, side, side): one launch of gngf_render from the tables (hash | per-vertex table)
  module_path   net(x, 1.0) under no_grad on an explicit coordinate tensor + data.reassemble_image_device
  bake          train.bake(net, out=baked): gngf_vertex_grid_fwd over all levels + six decoder copies
  baked_render  baked.render(side, side): one launch of gngf_render_grid from the baked grid

Outputs are preallocated for every way.  HIP events around each pass, a device synchronise before and after; --warmup passes of
every way first, then --passes rounds, each round timing every way once in turn (the ways alternate, so a drift of the machine
falls on all of them alike); medians and min-max per way.  The peak allocation of one pass of each way follows (outputs and the
bake's own tensors included where the pass creates them).  Checks first that the baked image is the unbaked render's up to the
integer rounding of values the two evaluations round differently.

    python tools/time_render_baked.py --out profiles/render_baked.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from collision_handling_in_instantngp_amd import data, models, train  # noqa: E402
from time_render import build, commit_of_tree, coords, peak_of, summary  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ways_of(mode, a, dev):
    """{name: callable} for one model, plus what the peak measurement needs"""
    models.should_use_hash_function = mode == "hash"
    try:
        net = build(mode, a.table)
    finally:
        models.should_use_hash_function = False
    side = a.side
    x = coords(side, dev)
    out_image = torch.empty((side, side, 3), dtype=torch.int32, device=dev)
    out_rgb = torch.empty((side * side, 3), dtype=torch.float32, device=dev)
    baked = train.bake(net)

    def module_path():
        with torch.no_grad():
            out = net(x, 1.0)[0]
        return data.reassemble_image_device(out, None, side, side, should_shuffle=False)

    def in_mode(fn):
        # (the module's forward reads the process-wide index-source switch on every call: each pass sets its own model's)
        def run():
            models.should_use_hash_function = mode == "hash"
            try:
                return fn()
            finally:
                models.should_use_hash_function = False
        return run

    ways = {"render": lambda: train.render(net, side, side, out_rgb=out_rgb, out_image=out_image),
            "module_path": module_path,
            "bake": lambda: train.bake(net, out=baked),
            "baked_render": lambda: baked.render(side, side, out_rgb=out_rgb, out_image=out_image)}
    fresh = {"render": lambda: train.render(net, side, side, image=True),
             "module_path": module_path,
             "bake": lambda: train.bake(net),
             "baked_render": lambda: baked.render(side, side, image=True)}
    ways, fresh = {k: in_mode(f) for k, f in ways.items()}, {k: in_mode(f) for k, f in fresh.items()}
    a_img = ways["render"]()[1].clone()
    b_img = ways["baked_render"]()[1].clone()
    differ = int((a_img != b_img).sum())
    assert int((a_img - b_img).abs().max()) <= 1 and differ < 0.02 * a_img.numel(), (differ, a_img.numel())
    info = {"mode": mode, "lattice": [side, side], "pixels": side * side, "elements_that_differ_by_one": differ,
            "baked_bytes": int(baked.nbytes), "grid_shape": list(baked.grid.shape),
            "table_bytes": int(net.encoding.packed_tables().numel() * net.encoding.packed_tables().element_size())}
    return net, ways, fresh, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--table", type=int, default=2 ** 19)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_baked.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_render_baked.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    models_ = {mode: ways_of(mode, a, dev) for mode in ("hash", "frozen_hpd")}
    runs = [(mode, name, fn) for mode, (_, ways, _, _) in models_.items() for name, fn in ways.items()]
    for _ in range(a.warmup):
        for _, _, fn in runs:
            fn()
    ms = {(mode, name): [] for mode, name, _ in runs}
    for _ in range(a.passes):
        for mode, name, fn in runs:
            ms[(mode, name)].append(timed(fn))
    shapes = []
    for mode, (_, ways, fresh, info) in models_.items():
        info.update({name: summary(ms[(mode, name)]) for name in ways})
        info["peak"] = {name: peak_of(fn) for name, fn in fresh.items()}
        shapes.append(info)
    t = {(s["mode"], name): s[name]["median_ms"] for s in shapes for name in ("render", "module_path", "bake", "baked_render")}
    fb, hb = t[("frozen_hpd", "baked_render")], t[("hash", "baked_render")]
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_of_tree(),
           "model": {"L": 16, "F": 2, "T": a.table, "n_min": 16, "n_max": 512, "K": 4},
           "warmup_passes": a.warmup, "timed_passes": a.passes,
           "method": "HIP events around each pass, device synchronise before and after; every way of both models in one process, "
                     "one pass of each in turn per round",
           "shapes": shapes,
           "comparison": {
               "a_render_frozen_hpd_ms": t[("frozen_hpd", "render")], "b_module_path_frozen_hpd_ms": t[("frozen_hpd", "module_path")],
               "c_render_hash_ms": t[("hash", "render")], "d_baked_render_frozen_hpd_ms": fb, "d_baked_render_hash_ms": hb,
               "d_bake_frozen_hpd_ms": t[("frozen_hpd", "bake")], "d_bake_hash_ms": t[("hash", "bake")],
               "baked_frozen_hpd_below_a": bool(fb < t[("frozen_hpd", "render")]),
               "baked_frozen_hpd_over_c": fb / t[("hash", "render")],
               "baked_frozen_hpd_over_b": fb / t[("frozen_hpd", "module_path")]}}
    for k, v in res["comparison"].items():
        print(f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
