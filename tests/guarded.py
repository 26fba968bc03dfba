"""A guard-band arena: where does a kernel write?

Every buffer a test hands to a kernel is a view into ONE uint8 tensor filled with 0xFF, with at least PAD untouched bytes on each
side and a TAIL of 1 MiB behind the last one, so a store next to a buffer lands in bytes this module watches instead of in a
neighbouring tensor or in the allocator's rounding slack — and stays inside the allocation, so nothing faults.

0xFF reads as NaN in fp32 / fp16 / fp64 and as -1 in int32 / int64.  No entry point of the library produces either and the clears
write 0, so "all bytes still 0xFF" means "never written" (`unwritten`), and a kernel that reads its own output before writing it
poisons what it computes."""
import numpy as np
import torch

PAD = 4096            # untouched bytes on each side of every buffer (at least)
TAIL = 1 << 20        # untouched bytes behind the last buffer (at least)
FILL = 0xFF


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Arena:
    def __init__(self, nbytes, device="cpu"):
        """room for `nbytes` of payload and padding in front of the tail guard"""
        self.capacity = int(nbytes)
        self.buf = torch.full((self.capacity + TAIL + 16,), FILL, dtype=torch.uint8, device=device)
        self.cursor = 0               # end of the last buffer handed out
        self.regions = []             # (name, start, end) byte ranges of the payloads, ascending

    def take(self, shape, dtype, fill=None, misalign=0, name=None):
        """A contiguous view of `shape`/`dtype`: 16-byte aligned, then shifted by `misalign` bytes (a multiple of the element size).
        fill=None leaves the payload at 0xFF; any other value fills it (0: a buffer the caller zero-fills)."""
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        assert misalign % item == 0 and 0 <= misalign < 16, "misalign: a multiple of the element size below 16"
        nbytes = _numel(shape) * item
        base = self.buf.data_ptr()
        start = self.cursor + PAD
        start += (-(base + start)) % 16 + misalign
        end = start + nbytes
        if end + PAD > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes is full: {name or 'buffer'} needs [{start}, {end + PAD})")
        view = self.buf[start:end].view(dtype).view(shape)
        assert view.data_ptr() == base + start and (view.data_ptr() - misalign) % 16 == 0
        if fill is not None:
            view.fill_(fill)
        self.regions.append((name or f"buffer{len(self.regions)}", start, end))
        self.cursor = end
        return view

    def put(self, values, name=None, dtype=None, misalign=0):
        """take() of the shape and dtype of `values` (numpy array or tensor), filled with them: an input"""
        src = torch.as_tensor(values)
        if dtype is not None:
            src = src.to(dtype)
        t = self.take(tuple(src.shape), src.dtype, misalign=misalign, name=name)
        t.copy_(src)
        return t

    def damage(self):
        """[(buffer name, "before" | "after", first byte, last byte, count)] of every run of guard bytes that is no longer 0xFF.
        The byte numbers are distances from the buffer: "after" 0 = the first byte behind its end, "before" 1 = the byte in front
        of its first."""
        bad = self.buf != FILL
        for _name, s, e in self.regions:
            bad[s:e] = False
        if not bool(bad.any()):
            return []
        idx = torch.nonzero(bad).reshape(-1).cpu().numpy()
        out = []
        edges = [(None, 0, 0)] + self.regions + [(None, self.buf.numel(), self.buf.numel())]
        for (pn, _ps, pe), (nn, ns, _ne) in zip(edges[:-1], edges[1:]):
            gap = idx[(idx >= pe) & (idx < ns)]
            if not len(gap):
                continue
            # a gap between two buffers belongs in halves to its neighbours; the head has only a successor, the tail a predecessor
            mid = ns if nn is None else (pe if pn is None else (pe + ns) // 2)
            after, before = gap[gap < mid], gap[gap >= mid]
            if len(after):
                out.append((pn, "after", int(after[0] - pe), int(after[-1] - pe), int(len(after))))
            if len(before):
                out.append((nn, "before", int(ns - before[-1]), int(ns - before[0]), int(len(before))))
        return out

    def check(self):
        """every guard byte is still 0xFF"""
        found = self.damage()
        if found:
            lines = []
            for name, side, first, last, count in found:
                if side == "after":
                    lines.append(f"{count} guard byte(s) written AFTER {name}: bytes {first}..{last} past its end")
                else:
                    lines.append(f"{count} guard byte(s) written BEFORE {name}: bytes {first}..{last} in front of its start")
            raise AssertionError("store outside a buffer: " + "; ".join(lines))


def unwritten(t):
    """boolean mask, shaped like t, of the elements whose bytes are all still 0xFF"""
    item = t.element_size()
    return t.contiguous().reshape(-1).view(torch.uint8).view(-1, item).eq(FILL).all(1).view(t.shape)


def same_bytes(a, b):
    """a and b hold the same bytes (NaN payloads included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))
