"""The per-tile loop of the two TRAIN instantiations of decoder_bwd_kernel in a `hipcc -S` listing of csrc/decoder.hip:
instruction classes, registers and scratch from the code object's metadata, and every s_waitcnt / s_nop of the loop with the
instructions around it.

  hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 --cuda-device-only -S decoder.hip -o decoder.s
  python tools/decoder_train_listing.py decoder.s [--waits] [--json out.json]

The loop is the innermost-labelled backward branch that holds the kernel's bf16 MFMAs."""
import json
import re
import sys

TRAIN = {"relu": "decoder_bwd_kernelILi32ELb0ELb1ELb0ELb1ELb1EE", "leaky": "decoder_bwd_kernelILi32ELb1ELb1ELb0ELb1ELb1EE"}


def kernel_body(lines, key):
    st = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and key in l and ":" in l)
    en = next(i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end"))      # (blocks may follow the s_endpgm)
    return lines[st:en]


def instructions(body):
    """(opcode, text) of every instruction line, labels as ('label', name)"""
    out = []
    for l in body:
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if m:
                out.append(("label", m.group(1)))
            continue
        if t.endswith(":"):
            continue
        out.append((t.split()[0], t))
    return out


def tile_loop(ins):
    labels = {t: i for i, (op, t) in enumerate(ins) if op == "label"}
    best = None
    for i, (op, t) in enumerate(ins):
        if not op.startswith("s_cbranch") and op != "s_branch":
            continue
        tgt = t.split()[-1]
        if tgt in labels and labels[tgt] < i:
            seg = ins[labels[tgt]:i + 1]
            n = sum(1 for o, _ in seg if o.startswith("v_mfma") and "bf16" in o)
            if n and (best is None or len(seg) < len(best)):
                best = seg
    if best is None:
        raise SystemExit("no loop with bf16 MFMAs found")
    return [x for x in best if x[0] != "label"]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma_bf16" if "bf16" in op else ("mfma_4x4" if "4x4" in op else "mfma_f32")
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    return "scalar"


def metadata(lines, key):
    """vgpr_count / private_segment_fixed_size of the kernel from the amdhsa.kernels metadata of the listing"""
    keep = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    start = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    cur, hit = {}, False
    for l in lines[start + 1:]:
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", l)
        if not m:
            if l and not l.startswith(" "):
                break
            continue
        if m.group(1) == "- ":                            # the next kernel's entry
            if hit:
                break
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
        hit = hit or (m.group(2) == "name" and key in m.group(3))
    if not hit:
        raise SystemExit("no metadata for " + key)
    return {k: int(cur[k]) for k in keep if k in cur}


def report(path, waits=False):
    lines = open(path).read().split("\n")
    res = {}
    for name, key in TRAIN.items():
        loop = tile_loop(instructions(kernel_body(lines, key)))
        counts = {}
        for op, _ in loop:
            counts[classify(op)] = counts.get(classify(op), 0) + 1
        counts["loop_instructions"] = len(loop)
        counts["ds_bpermute_b32"] = sum(1 for op, _ in loop if op == "ds_bpermute_b32")
        counts["v_permlane32_swap_b32"] = sum(1 for op, _ in loop if op.startswith("v_permlane32_swap"))
        counts["registers"] = metadata(lines, key)
        wl = []
        for i, (op, t) in enumerate(loop):
            if op in ("s_waitcnt", "s_nop"):
                prev = next((loop[j][0] for j in range(i - 1, -1, -1) if loop[j][0] not in ("s_waitcnt", "s_nop")), "")
                nxt = next((loop[j][1] for j in range(i + 1, len(loop)) if loop[j][0] not in ("s_waitcnt", "s_nop")), "")
                wl.append({"at": i, "what": " ".join(t.split()), "after": prev, "before": " ".join(nxt.split())})
        counts["waits"] = wl
        res[name] = counts
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    res = report(args[0])
    for name, c in res.items():
        print(name, {k: v for k, v in c.items() if k != "waits"})
        if "--waits" in sys.argv:
            for w in c["waits"]:
                print(f"  {w['at']:5d}  {w['what']:28s} after {w['after']:32s} before {w['before']}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)
