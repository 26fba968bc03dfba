#!/usr/bin/env python
"""Training from the image itself against training from the pixel list, in ONE process ("device batch sampler"):

    sampled        train.train_sampled on a data.ImageSampler (continuous positions, bilinear targets)
    sampled_pixel  the same with continuous=False (random pixel centres)
    epoch          train.train_epoch(graph=True) on permutation slices of the same batch size — the pixel list, the target list and
                   the permutation on the device, one index-select gather per batch

Headline model shape (bench.SHAPES["cfg3"]: hash mode, L = 16, F = 2, T = 2^19, n_max = 512), `--batch` pixels per step on a
`--side`^2 RGB image given by a smooth formula; each way has its own model and FusedAdam, built from the same seed.  A window is
`--calls` calls of side^2 / batch steps each (for `epoch`: one train_epoch per call), timed with HIP events around all of them; the ways
alternate window by window, so that a drift of the clock falls on all of them alike.  The data side's device bytes are recorded
both ways.

--psnr (optional): a model whose finest level is finer than the image (n_max = 4 * side) is trained both ways for the same number
of steps on a small image of the same formula and rendered on the 2x lattice; the PSNR against the FORMULA at those positions —
half of which no pixel-list batch ever contained — is recorded.  No threshold.

    python tools/time_sampler.py [--out profiles/sampler.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def formula(rows, cols, side):
    """smooth RGB in [0, 1] at pixel positions (rows, cols) (any real numbers) of a side x side image: (n, 3) float64"""
    import numpy as np
    y, x = np.asarray(rows, np.float64) / (side - 1), np.asarray(cols, np.float64) / (side - 1)
    r = 0.5 + 0.5 * np.sin(9.0 * x + 4.0 * y * y)
    g = 0.5 + 0.5 * np.cos(7.0 * y - 3.0 * x) * np.sin(5.0 * x * y + 1.0)
    b = 0.5 + 0.25 * np.sin(13.0 * (x - 0.4) ** 2 + 11.0 * (y - 0.6) ** 2) + 0.25 * np.cos(6.0 * x)
    return np.stack([r, g, b], axis=-1)


def formula_image(side):
    import numpy as np
    rr, cc = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return np.clip(np.rint(formula(rr, cc, side) * 255.0), 0, 255).astype(np.uint8)


def build(dev, c, n_max=None, T=None):
    import torch
    from collision_handling_in_instantngp_amd import models, train
    torch.manual_seed(65535)
    T = T or c["T"]
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=T, num_levels=c["L"], n_min=c["n_min"],
                                          n_max=n_max or c["n_max"], MLP_hidden_layers_widths=[64, 64],
                                          HPD_hidden_layers_widths=[32, 64, 128], HPD_out_features=T, feature_dim=c["F"],
                                          topk_k=c["K"]).to(dev)
    net.return_indices = False
    net.dense_probs = False
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    opt = train.get_optimizer(net, 1e-2, 1e-3, 1e-3, 0.0, 0.0, 1e-6)
    return net, loss_fn, opt


def pixel_list(img, dev):
    """the reference's data side on the device: coordinates, targets, permutation — 24 B per pixel for an RGB image"""
    import torch
    from collision_handling_in_instantngp_amd import data
    h, w = img.shape[:2]
    X, Y, _h, _w = data.MyDataset(image=img)[0]
    x = data.normalise_coordinates(X, w, h).to(dev).contiguous()
    shuffled, _ = data.make_permutation(h * w, torch.Generator().manual_seed(65535))
    return x, Y.to(dev).contiguous(), shuffled.to(dev)


def event_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler.json"))
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=2 ** 20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5, help="calls (of side^2 / batch steps each) per timed window")
    ap.add_argument("--ramp-windows", type=int, default=6)
    ap.add_argument("--psnr", action="store_true")
    ap.add_argument("--psnr-side", type=int, default=256)
    ap.add_argument("--psnr-steps", type=int, default=400)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from collision_handling_in_instantngp_amd import data, models, train
    if not torch.cuda.is_available():
        raise SystemExit("time_sampler.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if (a.side * a.side) % a.batch:
        raise SystemExit("--side^2 must be a multiple of --batch (train_epoch's batches are fixed slices)")
    steps = a.side * a.side // a.batch
    c = bench.SHAPES["cfg3"]
    weights = dict(l_mse=1, l_js_kl=1, l_collisions=1e-3)
    prev = models.should_use_hash_function
    models.should_use_hash_function = True
    res = {"shape": dict(c), "image": [a.side, a.side, 3], "batch": a.batch, "steps_per_window": steps * a.calls, "windows": a.windows,
           "device": torch.cuda.get_device_name(dev), "ways": {}}
    try:
        img = formula_image(a.side)
        ways, info = {}, {}
        for name, continuous in (("sampled", True), ("sampled_pixel", False)):
            net, loss_fn, opt = build(dev, c)
            s = data.ImageSampler(img, a.batch, seed=65535, continuous=continuous)
            ways[name] = (lambda net=net, loss_fn=loss_fn, opt=opt, s=s: train.train_sampled(net, loss_fn, opt, s, steps, **weights))
            info[name] = {"data_bytes": s.data_bytes(), "data_bytes_per_pixel_storage": nbytes(s.image) / (a.side * a.side), "net": net}
        net, loss_fn, opt = build(dev, c)
        x, y, perm = pixel_list(img, dev)
        ways["epoch"] = (lambda net=net, loss_fn=loss_fn, opt=opt: train.train_epoch(
            net, loss_fn, opt, x, y, a.side, a.side, 1, 1, 1e-3, batch_percentage=a.batch / (a.side * a.side), should_shuffle=True,
            shuffled_indices=perm, graph=True, slot_counts=True))
        info["epoch"] = {"data_bytes": nbytes(x, y, perm), "data_bytes_per_pixel_storage": nbytes(x, y, perm) / (a.side * a.side),
                         "net": net}
        for _ in range(a.ramp_windows):                   # capture, code objects, clock ramp
            for name in ways:
                ways[name]()
        torch.cuda.synchronize()
        ms = {name: [] for name in ways}
        for _w in range(a.windows):
            for name in ways:
                ms[name].append(event_ms(ways[name], a.calls) / (steps * a.calls))
        # the draw alone: `--calls` * 10 next() calls back to back per window (two launches each: the batch and the counter)
        for name, continuous in (("sampled", True), ("sampled_pixel", False)):
            s = data.ImageSampler(img, a.batch, seed=1, continuous=continuous)
            for _ in range(20):
                s.next()
            torch.cuda.synchronize()
            draws = [event_ms(s.next, 10 * a.calls) / (10 * a.calls) for _w in range(a.windows)]
            info[name].update(draw_ms_median=statistics.median(draws), draw_ms_windows=draws)
        for name in ways:
            net = info[name].pop("net")
            sc = net.dp.step_config
            _img, psnr, _acc = train.render_psnr(net, img)
            res["ways"][name] = dict(info[name], step_ms_median=statistics.median(ms[name]), step_ms_min=min(ms[name]),
                                     step_ms_max=max(ms[name]), step_ms_windows=ms[name], psnr_after=psnr,
                                     steps_taken=(a.ramp_windows + a.windows * a.calls) * steps, step_config=sc.signature() if sc else None)
        if a.psnr:
            side = a.psnr_side
            small = formula_image(side)
            lat = 2 * (side - 1) + 1
            rr, cc = np.meshgrid(np.arange(lat) / 2.0, np.arange(lat) / 2.0, indexing="ij")
            truth = formula(rr, cc, side).reshape(-1, 3)
            on_pixels = ((np.arange(lat)[:, None] % 2 == 0) & (np.arange(lat)[None, :] % 2 == 0)).reshape(-1)
            batch = side * side
            out = {"image": [side, side, 3], "n_max": 4 * side, "batch": batch, "steps": a.psnr_steps, "lattice": [lat, lat]}
            for name in ("sampled", "epoch"):
                net, loss_fn, opt = build(dev, c, n_max=4 * side)
                if name == "sampled":
                    s = data.ImageSampler(small, batch, seed=1)
                    train.train_sampled(net, loss_fn, opt, s, a.psnr_steps, **weights)
                else:
                    xs, ys, ps = pixel_list(small, dev)
                    for _ in range(a.psnr_steps):
                        train.train_epoch(net, loss_fn, opt, xs, ys, side, side, 1, 1, 1e-3, batch_percentage=1.0,
                                          should_shuffle=True, shuffled_indices=ps, graph=True, slot_counts=True)
                rgb = train.render(net, lat, lat, denom=2 * (side - 1)).double().cpu().numpy()

                def psnr(sel):
                    return float(10 * np.log10(1.0 / np.mean((rgb[sel] - truth[sel]) ** 2)))

                out[name] = {"psnr_2x_lattice": psnr(slice(None)), "psnr_at_pixels": psnr(on_pixels),
                             "psnr_between_pixels": psnr(~on_pixels), "psnr_image": train.render_psnr(net, small)[1]}
            res["psnr_above_image_side"] = out
    finally:
        models.should_use_hash_function = prev
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({n: {"step_ms": round(v["step_ms_median"], 4), "data_bytes": v["data_bytes"]} for n, v in res["ways"].items()}))
    if a.psnr:
        print(json.dumps(res["psnr_above_image_side"]))


if __name__ == "__main__":
    main()
