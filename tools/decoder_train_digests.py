"""SHA-256 digests of everything gngf_decoder_train writes (rgb, d enc, the per-workgroup slab buffer with its max |d enc| word) at the
shapes where the kernel's tile loop can go wrong, for both TRAIN instantiations (ReLU, leaky).  The kernel has no atomics and no
memset: these bytes are a function of the inputs and of the order in which each accumulator receives its products, so a change
that only moves instructions must reproduce them exactly.

    python tools/decoder_train_digests.py OUT.json [COMMIT]     # run from a clean build of the commit the digests are to pin

tests/test_gpu_decoder_train_schedule.py holds the build under test to tests/golden/decoder_train_digests.json."""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

IN_DIM, OUT_DIM = 32, 3
# a partial first tile | lane-half boundaries | a partial last tile of a wave, a second wave | one workgroup taking a second tile |
# two and three tiles per workgroup (256 workgroups of 128 pixels), the prefetches crossing the loop edge
PIXELS = (1, 31, 33, 127, 129, 128 * 256 + 1, 128 * 257 + 5, 128 * 600 + 77)
OUTPUTS = ("rgb", "denc", "slabs")


def cases():
    return [(leaky, P) for leaky in (0, 1) for P in PIXELS]


def case_name(leaky, P):
    return f"{'leaky' if leaky else 'relu'}/P={P}"


def inputs(leaky, P, in_dim=IN_DIM):
    """Seeded numpy inputs (the seed is the case itself; another encoder width than IN_DIM joins the seed)."""
    rng = np.random.default_rng([7, leaky, P] + ([in_dim] if in_dim != IN_DIM else []))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    dims = [in_dim, 64, 64, OUT_DIM]
    ws = []
    for i in range(3):
        ws += [f(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])), f(0.1 * rng.standard_normal(dims[i + 1]))]
    return {"enc": f(0.5 * rng.standard_normal((P, in_dim))), "target": f(rng.random((P, OUT_DIM))), "gloss": f([1.25]), "ws": ws}


def _dev(inp):
    t = lambda a: torch.from_numpy(a).cuda()
    return t(inp["enc"]), t(inp["target"]), t(inp["gloss"]), [t(w) for w in inp["ws"]]


def _reduced(reduce, in_dim):
    """reduce: also hand the kernel the six gradient buffers and the max |d enc| word (the slab reduction runs in the same call)"""
    if not reduce:
        return [None] * 6, None
    shapes = ((64, in_dim), (64,), (64, 64), (64,), (OUT_DIM, 64), (OUT_DIM,))
    return [torch.full(sh, -7.0, device="cuda") for sh in shapes], torch.full((1,), -7.0, device="cuda")


def _outputs(rgb, denc, slabs, grads, absmax):
    out = {"rgb": rgb.cpu().numpy(), "denc": denc.cpu().numpy(), "slabs": slabs.cpu().numpy()}
    if absmax is not None:
        out["grads"] = [g.cpu().numpy() for g in grads]
        out["denc_absmax"] = absmax.cpu().numpy()
    return out


def run_fused(leaky, P, inp=None, reduce=False):
    """One gngf_decoder_train launch on fresh output buffers -> {name: numpy array} of everything it wrote."""
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr, query
    enc, target, gloss, ws = _dev(inp or inputs(leaky, P))
    nfl = query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", IN_DIM, OUT_DIM)
    # filled with a pattern no result equals: a word the kernel fails to write shows in the digest
    slabs = torch.full((nfl,), -7.0, device="cuda")
    rgb = torch.full((P, OUT_DIM), -7.0, device="cuda")
    denc = torch.full((P, IN_DIM), -7.0, device="cuda")
    grads, absmax = _reduced(reduce, IN_DIM)
    call("gngf_decoder_train", ptr(enc), ptr(target), ptr(gloss), *[ptr(w) for w in ws], ptr(rgb), ptr(denc), *[ptr(g) for g in grads],
         ptr(slabs), ptr(absmax), ptr(None), 0, P, IN_DIM, OUT_DIM, leaky, stream_ptr())
    torch.cuda.synchronize()
    return _outputs(rgb, denc, slabs, grads, absmax)


def run_two_kernels(leaky, P, inp=None, in_dim=IN_DIM, save_hidden=True, drgb=None, reduce=False):
    """The same quantities from gngf_decoder_fwd + gngf_decoder_bwd (all products of the forward on the fp32 pipe): equal to the
    fused kernel to fp32 rounding, not to the bit — the yardstick a mismatch is described against.
    save_hidden=False: the backward recomputes the hidden layers; drgb (P, OUT_DIM) numpy: the upstream gradient itself instead of
    target + gloss."""
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr, query
    enc, target, gloss, ws = _dev(inp or inputs(leaky, P, in_dim))
    nfl = query("gngf_decoder_bwd_slabs", P) * query("gngf_decoder_slab_floats", in_dim, OUT_DIM)
    slabs = torch.full((nfl,), -7.0, device="cuda")
    hidden = torch.empty((query("gngf_decoder_hidden_floats", P),), device="cuda") if save_hidden else None
    rgb = torch.full((P, OUT_DIM), -7.0, device="cuda")
    denc = torch.full((P, in_dim), -7.0, device="cuda")
    grads, absmax = _reduced(reduce, in_dim)
    d = None if drgb is None else torch.from_numpy(np.ascontiguousarray(drgb, dtype=np.float32)).cuda()
    call("gngf_decoder_fwd", ptr(enc), *[ptr(w) for w in ws], ptr(rgb), ptr(hidden), P, in_dim, OUT_DIM, leaky, stream_ptr())
    call("gngf_decoder_bwd", ptr(enc), ptr(rgb), ptr(d), ptr(None if d is not None else target), ptr(None if d is not None else gloss),
         *[ptr(w) for w in ws[:5]], ptr(denc), *[ptr(g) for g in grads], ptr(slabs), ptr(absmax), ptr(hidden), ptr(None), 0, P, in_dim,
         OUT_DIM, leaky, stream_ptr())
    torch.cuda.synchronize()
    return _outputs(rgb, denc, slabs, grads, absmax)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests_of(out):
    return {k: digest(out[k]) for k in OUTPUTS}


def describe_mismatch(leaky, P, out):
    """Where the fused kernel's output leaves the two-kernel path: a hazard shows as a few elements far off, a reordered sum as
    (nearly) every element off by an ulp — which the two paths are anyway, so only the far-off elements are listed."""
    ref = run_two_kernels(leaky, P)
    lines = []
    for k in OUTPUTS:
        a, b = out[k].ravel().astype(np.float64), ref[k].ravel().astype(np.float64)
        if k == "slabs":           # the max |d enc| words are bit patterns, not sums
            n = 64 * IN_DIM + 64 * 64 + OUT_DIM * 64 + 128 + OUT_DIM + 1
            keep = (np.arange(len(a)) % n) != n - 1
            a, b = a[keep], b[keep]
        scale = max(float(np.abs(b).max()), 1e-30)
        err = np.abs(a - b) / scale
        far = np.flatnonzero(~(err <= 1e-4))
        first = f"first at flat index {far[0]}: {a[far[0]]!r} vs {b[far[0]]!r}" if len(far) else "none"
        lines.append(f"{k}: {int((a != b).sum())} of {len(a)} elements differ from the two-kernel path, median relative {np.median(err):.2e}, "
                     f"{len(far)} beyond 1e-4 of the maximum ({first})")
    return "; ".join(lines)


def main():
    out_path = sys.argv[1]
    commit = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout
    doc = {"commit": commit, "hipcc": next((l for l in hipcc.splitlines() if "HIP version" in l), hipcc.splitlines()[0] if hipcc else ""),
           "device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "out_dim": OUT_DIM, "cases": {}}
    for leaky, P in cases():
        first = run_fused(leaky, P)
        again = run_fused(leaky, P)
        d = digests_of(first)
        assert d == digests_of(again), f"{case_name(leaky, P)}: two runs of one build differ"
        doc["cases"][case_name(leaky, P)] = d
        print(case_name(leaky, P), d["slabs"][:16], flush=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
