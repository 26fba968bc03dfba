"""gngf_decoder_train (forward + MSE gradient + backward in one launch) next to decoder_fwd + decoder_bwd, and the cycles of its
phases from a -DGNGF_STAMPS library.

    python tools/perf_decoder_train.py                               # the timings, production library
    python tools/perf_decoder_train.py --build-stamps 0x8181         # build the stamps library of a subset (no GPU needed)
    python tools/perf_decoder_train.py --stamps 0x8181 [--json F]    # build it if it is missing, run it, print the subset's phases
    ... --root DIR                                                   # the same for another checkout (its decoder.hip needs GNGF_STAMP_MASK)

A stamp subset is a bit mask over STAMP(k) of csrc/decoder.hip (-DGNGF_STAMP_MASK): unselected stamps compile to nothing, a
selected one holds the cycles since the previous selected stamp in program order.  The training kernel stands at 512 registers
and spills with all 16 stamps, which makes its per-phase numbers upper bounds; a subset of three or four does not.  The build
reads vgpr_count and private_segment_fixed_size of both TRAIN instantiations from the code object's metadata and refuses a
subset that spills (--allow-scratch: builds it all the same and says "fits": false in what it writes).  Subsets for the phases between the matrix runs: 0x8181 = {15, 7, 0, 8} (phases 07, 00, 08; stamp 15 holds
everything from 08 to 15), 0x1802 = {11, 1, 12} (phases 01, 12; stamp 11 holds the rest of the tile).
GNGF_LIB_PATH=...stamps.so (any -DGNGF_STAMPS library built by hand) still prints all 16 stamps."""
import argparse
import ctypes
import glob
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# --root DIR: measure another checkout (the parent commit, built in its own tree) with this tool
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
PKG = os.path.join(ROOT, "collision_handling_in_instantngp_amd")
CSRC = os.path.join(PKG, "csrc")

# by stamp index (csrc/decoder.hip, STAMP(k)), in the order the phases run.  Every VALU burst between two matrix runs has a number
# of its own.
ORDER = (0, 8, 2, 9, 10, 11, 1, 12, 3, 13, 14, 5, 4, 6, 15, 7)
NAMES = {0: "loop edge, pins", 8: "fwd: biases, split of x chunk 0", 2: "fwd: L1 run", 9: "fwd: act1 + split of L2 chunk 0",
         10: "fwd: L2 run + h1 image", 11: "fwd: act2", 1: "fwd: L3, sigmoid, rgb, d rgb", 12: "dh2 run + drain",
         3: "dh2 mask", 13: "dh1: split of chunk 0", 14: "dh1 run (+ dW2)", 5: "dh1 mask, db1", 4: "img+dW1", 6: "img+dW0",
         15: "d enc: split of chunk 0 + run", 7: "|d enc| max, db0, stores"}
MAX_VGPRS = 512


def stamps_lib(mask):
    return os.path.join(PKG, f"libgngf_hip_stamps_{mask:04x}.so")


def build_stamps(mask, allow_scratch=False):
    """decoder.hip with the subset's stamps + the production objects of the other sources -> libgngf_hip_stamps_<mask>.so and
    csrc/build/stamps_<mask>/meta.json (registers and scratch of the TRAIN instantiations, from the metadata of the code object hipcc wrote)."""
    import decoder_train_listing as listing
    out = stamps_lib(mask)
    bdir = os.path.join(CSRC, "build", f"stamps_{mask:04x}")
    meta_path = os.path.join(bdir, "meta.json")
    if os.path.isfile(out) and os.path.isfile(meta_path):
        return json.load(open(meta_path))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(bdir, exist_ok=True)
    others = [os.path.join(CSRC, os.path.basename(s)[:-4] + ".o") for s in sorted(glob.glob(os.path.join(CSRC, "*.hip")))
              if os.path.basename(s) != "decoder.hip"]
    missing = [o for o in others if not os.path.isfile(o)]
    if missing:
        raise SystemExit(f"build the production library first (make -C {CSRC}): missing {missing[0]}")
    flags = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]   # csrc/Makefile
    obj = os.path.join(bdir, "decoder.o")
    subprocess.check_call([hipcc, *flags, "-DGNGF_STAMPS", f"-DGNGF_STAMP_MASK=0x{mask:x}", "-save-temps=obj", "-c",
                           os.path.join(CSRC, "decoder.hip"), "-o", obj], cwd=CSRC)
    asm = [p for p in glob.glob(os.path.join(bdir, "*.s")) if "gfx950" in os.path.basename(p)]
    assert len(asm) == 1, asm
    lines = open(asm[0]).read().split("\n")
    meta = {name: listing.metadata(lines, key) for name, key in listing.TRAIN.items()}
    fits = all(m["vgpr_count"] <= MAX_VGPRS and m["private_segment_fixed_size"] == 0 for m in meta.values())
    # --allow-scratch: build and measure anyway, with "fits": false in every output (a kernel that stands at 512 registers
    # before any stamp is added takes one stamp without scratch and no second one)
    assert fits or allow_scratch, f"stamp subset 0x{mask:x} does not fit the training kernel: {meta} — select fewer stamps"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj, *others])
    for p in glob.glob(os.path.join(bdir, "decoder-*")) + glob.glob(os.path.join(bdir, "decoder.hip*")):     # -save-temps leaves ~200 MB
        os.remove(p)
    doc = {"mask": f"0x{mask:04x}", "stamps": [k for k in ORDER if mask >> k & 1], "fits": fits, "registers": meta}
    with open(meta_path, "w") as f:
        json.dump(doc, f, indent=1)
    return doc


def intervals(mask):
    """[(stamp, label)] in program order: what a selected stamp's cycles cover"""
    sel = [k for k in ORDER if mask >> k & 1]
    out = []
    for n, k in enumerate(sel):
        prev = sel[n - 1]
        if ORDER[ORDER.index(k) - 1] == prev:
            out.append((k, f"{k:02d} {NAMES[k]}"))
        else:
            out.append((k, f"{k:02d} everything after stamp {prev:02d} up to: {NAMES[k]}"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-stamps", type=lambda s: int(s, 0), default=None)
    ap.add_argument("--stamps", type=lambda s: int(s, 0), default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--allow-scratch", action="store_true")
    args = ap.parse_args()
    if args.build_stamps is not None:
        print(json.dumps(build_stamps(args.build_stamps, args.allow_scratch)))
        return
    built = None
    if args.stamps is not None:
        built = build_stamps(args.stamps, args.allow_scratch)
        os.environ["GNGF_LIB_PATH"] = stamps_lib(args.stamps)          # read when _lib is imported

    import torch
    from collision_handling_in_instantngp_amd import _lib
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr, query
    dev = torch.device("cuda")
    P, in_dim, out_dim = 2**20, 32, 3
    torch.manual_seed(0)
    enc = torch.randn((P, in_dim), device=dev) * 0.5
    Ws = [torch.randn((64, in_dim), device=dev) / 6, torch.randn(64, device=dev) * 0.1, torch.randn((64, 64), device=dev) / 8, torch.randn(64, device=dev) * 0.1,
          torch.randn((out_dim, 64), device=dev) / 8, torch.randn(out_dim, device=dev) * 0.1]
    target = torch.rand((P, out_dim), device=dev)
    one = torch.ones((), device=dev)
    slabs = torch.empty((query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", in_dim, out_dim),), device=dev)
    hidden = torch.empty((query("gngf_decoder_hidden_floats", P),), device=dev)
    rgb = torch.empty((P, out_dim), device=dev); denc = torch.empty_like(enc)
    def two():
        call("gngf_decoder_fwd", ptr(enc), *[ptr(w) for w in Ws], ptr(rgb), ptr(hidden), P, in_dim, out_dim, 0, stream_ptr())
        call("gngf_decoder_bwd", ptr(enc), ptr(rgb), ptr(None), ptr(target), ptr(one), ptr(Ws[0]), ptr(Ws[1]), ptr(Ws[2]), ptr(Ws[3]), ptr(Ws[4]), ptr(denc), *[ptr(None)] * 6, ptr(slabs), ptr(None), ptr(hidden), ptr(None), 0, P, in_dim, out_dim, 0, stream_ptr())
    def fused():
        call("gngf_decoder_train", ptr(enc), ptr(target), ptr(one), *[ptr(w) for w in Ws], ptr(rgb), ptr(denc), *[ptr(None)] * 6, ptr(slabs), ptr(None), ptr(None), 0, P, in_dim, out_dim, 0, stream_ptr())
    zbuf = torch.empty((16 * 2 ** 19 * 2 + 4 * 720000,), device=dev)       # the step's [table gradient | fixed-point vertex grid]: 75 MiB
    zsmall = torch.empty((4 * 720000,), device=dev)                       # the fixed-point vertex grid alone: 11 MiB
    def fused_clear(z):
        def fn():
            call("gngf_decoder_train", ptr(enc), ptr(target), ptr(one), *[ptr(w) for w in Ws], ptr(rgb), ptr(denc), *[ptr(None)] * 6, ptr(slabs), ptr(None), ptr(z), z.numel(), P, in_dim, out_dim, 0, stream_ptr())
        return fn
    runs = (("decoder_fwd + decoder_bwd", two), ("decoder_train", fused), ("decoder_train + 75 MiB clear", fused_clear(zbuf)),
            ("decoder_train + 11 MiB clear", fused_clear(zsmall)), ("decoder_train", fused))
    if args.stamps is not None:
        runs = (("decoder_train", fused), ("decoder_train", fused))     # (the last launch is the one the stamps are read from)
    doc = {"us": []}
    for name, fn in runs:
        for _ in range(60): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(30): fn()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 30 * 1e3
        doc["us"].append([name, round(us, 1)])
        print(f"{name:28s} {us:8.1f} us")
    if args.stamps is None and not os.environ.get("GNGF_LIB_PATH", "").endswith("stamps.so"):
        return
    mask = args.stamps if args.stamps is not None else 0xffff
    buf = (ctypes.c_uint64 * 16)()
    _lib.load().gngf_debug_read_stamps.argtypes = [ctypes.c_void_p]
    _lib.load().gngf_debug_read_stamps(buf)
    tot = sum(buf[k] for k in range(16) if mask >> k & 1)
    doc["cycles_per_tile"] = {}
    for k, label in intervals(mask):                                     # (workgroup 7 runs 32 tiles of the 2^20 pixels)
        doc["cycles_per_tile"][label] = round(buf[k] / 32)
        print(f"  {label:72s} {buf[k]/32:9.0f} cycles/tile  {100*buf[k]/max(tot,1):5.1f}%")
    doc["total_cycles_per_tile"] = tot / 32
    print("  total per tile", tot / 32)
    if built:
        doc.update(built)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
