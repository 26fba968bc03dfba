"""Callers of the hot path, mirrored from the reference so that parity tests read like the reference's own
training loop: Loss (utils.py:78-174), get_optimizer (functions.py:96-127), train_step
(functions.py:139-355, batching + loss assembly only; no wandb / plotting / collision diagnostics)."""
import contextlib
import math

import numpy as np
import torch

from . import models, ops
from .models import VertexDistribution


class Loss(torch.nn.Module):
    """reference utils.py:78-174.  forward(pred, labels, N, prob, collisions, min_possible_collisions)
    -> (mse, kl_divs (L,), collisions_losses).  `prob` is the dense (P,L,4,N) tensor or a VertexDistribution
    (its .pbar is the batch-mean distribution the reference computes at utils.py:138,159)."""

    def __init__(self, delta: float = 1, gamma: float = 1, epsilon: float = 0.5, should_log: bool = False) -> None:
        super().__init__()
        self._delta = delta
        self._gamma = gamma
        self._epsilon = epsilon
        self.mse = torch.nn.MSELoss()

    @staticmethod
    def _kldiv_batchmean(log_input, target):
        # torch.nn.KLDivLoss(reduction='batchmean') on (L,N) rows treated independently as 1-D inputs: /N
        return torch.xlogy(target, target).sub(target * log_input).sum(-1) / log_input.shape[-1]

    def js_kl_rows(self, pbar):
        """pbar (L,N) -> (L,) : -(gamma+eps)*JS + eps*KL per level (utils.py:122-174).  Device fp32 distributions run
        on the HIP kernels (ops.JsKlFunction); the torch expression below is the same formula for host tensors."""
        if pbar.is_cuda and pbar.dtype == torch.float32 and pbar.dim() == 2:
            return ops.js_kl_rows(pbar, self._gamma, self._epsilon)
        return self.js_kl_rows_torch(pbar)

    def js_kl_rows_torch(self, pbar):
        N = pbar.shape[-1]
        q = torch.full_like(pbar, 1.0 / N)
        lp = pbar.log()
        kl = self._kldiv_batchmean(lp, q)
        m = (pbar + q) / 2
        js = (self._kldiv_batchmean(lp, m) + self._kldiv_batchmean(q.log(), m)) / 2
        return -(self._gamma + self._epsilon) * js + self._epsilon * kl

    def _mse(self, pred, labels):
        # device tensors: the two-launch HIP kernels; host tensors (the CPU tests of the loss algebra): the torch module
        if pred.is_cuda and pred.dtype == torch.float32 and labels.dtype == torch.float32 and pred.shape == labels.shape:
            return ops.mse_loss(pred, labels)
        return self.mse(pred, labels)

    def forward(self, pred, labels, N, prob, collisions, min_possible_collisions):
        mse_loss = self._mse(pred, labels)
        if models.should_use_hash_function:
            return mse_loss, None, None
        collisions_losses = collisions / (min_possible_collisions + self._delta)
        if isinstance(prob, VertexDistribution):
            pbar = prob.pbar
            if pbar is None:
                # net.compute_pbar = False: the caller opted out of the batch-mean distribution (with a frozen HPD the
                # distribution term is a constant without gradient) — the term is not evaluated, not faked
                return mse_loss, None, collisions_losses
        else:
            pbar = prob.sum(0).sum(1) / (prob.shape[0] * prob.shape[2])          # (L,N)
        return mse_loss, self.js_kl_rows(pbar), collisions_losses


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam's update (amsgrad off; the reference's get_optimizer, functions.py:96-127) for every tensor of
    every parameter group in ONE launch of the HIP kernel behind `gngf_adam_step` (csrc/optim.hip).  State keeps
    torch.optim.Adam's layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so optimizer state dicts written by the
    reference's torch.optim.Adam load here and vice versa.  The step count is a device tensor advanced by the kernel:
    a step needs no host synchronisation and can be captured in a hipGraph together with forward and backward."""

    DTYPES = (torch.float32, torch.float16)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > 4:
            raise ValueError("at most 4 parameter groups (GNGF_ADAM_MAX_GROUPS)")
        if len({(g["betas"], g["eps"]) for g in self.param_groups}) != 1:
            raise ValueError("betas and eps are shared by all groups (as in the reference's get_optimizer)")
        self.grad_scale = 1.0        # loss scale of fp16 training: every gradient is divided by it inside the kernel
        self._step = None            # device float: steps taken
        self._table = None           # device byte tensor: the packed segment list
        self._host = None            # ring of [pinned staging buffer, event of the upload that last read it]
        self._slot = 0
        self._captured = []          # staging buffers owned by captured steps (read again at every replay)
        self._spares = []            # pinned buffers set aside for captures (no pinned allocation while capturing)
        self._table_key = None
        self._total_blocks = 0
        self._mask_source = None     # set_mask_source(): callable -> {parameter: (row map words, row_elems)} | None
        # What the moments are known to fit: True — any map (there are no moments yet); None — unknown (loaded state, a source
        # attached to existing state, dense steps taken); else the (maps, groups without weight decay) of the last masked
        # step.  A step that resolves anything else checks the moments first (_guard).
        self._fits = True
        self._masked = False         # the segment table in self._table is followed by mask records
        self._last_call = None       # the library call the last step() made (tests)

    _RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("w", "<u8"), ("n", "<i8"), ("first", "<i8"),
                        ("group", "<i4"), ("flags", "<i4")])          # csrc/optim.hip: AdamSegment (64 bytes)
    _MASK_RECORD = np.dtype([("mask", "<u8"), ("row_elems", "<i4"), ("reserved", "<i4")])      # csrc/optim.hip: AdamSegMask (16 bytes)

    @staticmethod
    def mask_record(mask_ptr, row_elems, lo):
        """(pointer, row_elems) of one segment's mask record.  A segment that starts at element `lo` of its parameter
        (_adam_range) starts at row lo / row_elems of the map: the pointer is advanced by whole 32-bit words, which needs
        lo % (32 * row_elems) == 0 — otherwise (0, 0): the record of a dense segment."""
        mask_ptr, row_elems, lo = int(mask_ptr), int(row_elems), int(lo)
        if mask_ptr == 0 or row_elems <= 0 or lo < 0 or lo % (32 * row_elems) != 0:
            return 0, 0
        return mask_ptr + (lo // row_elems // 32) * 4, row_elems

    @classmethod
    def pack_records(cls, segs, masks, block_elems):
        """Pure numpy: the bytes of the device table and its number of blocks.  segs: per segment (param, grad, exp_avg,
        exp_avg_sq, master, n, group, flags, ...) with pointers as integers; masks: None (the table gngf_adam_step reads) or
        per segment None | (mask pointer, row_elems, lo) — then the nseg 64-byte segment records are followed by nseg
        16-byte mask records (gngf_adam_step_masked's seg_masks = table + 64 * nseg)."""
        rec = np.zeros(len(segs), dtype=cls._RECORD)
        total_blocks = 0
        for i, sg in enumerate(segs):
            pp, gp, mp, vp, wp, n, gi, flags = sg[:8]
            rec[i] = (pp, gp, mp, vp, wp, n, total_blocks, gi, flags)
            total_blocks += -(-n // block_elems)
        raw = rec.view(np.uint8).reshape(-1)
        if masks is not None:
            if len(masks) != len(segs):
                raise ValueError("one mask entry (or None) per segment")
            mrec = np.zeros(len(segs), dtype=cls._MASK_RECORD)
            for i, m in enumerate(masks):
                if m is not None:
                    mrec[i] = (*cls.mask_record(*m), 0)
            raw = np.concatenate([raw, mrec.view(np.uint8).reshape(-1)])
        return raw, total_blocks

    def set_mask_source(self, source):
        """source: a callable returning {parameter: (int32 device tensor of row-map words, row_elems)} or None, asked at
        every step (get_optimizer(..., skip_unreachable_rows=True) binds net.reachable_rows).  While it gives a map, step()
        runs gngf_adam_step_masked: rows whose bit is clear are neither read nor written.  That equals the dense step bit for
        bit as long as such rows have zero moments — true for rows that never receive a gradient and an optimizer that
        starts from nothing.  Moments that were not produced under the same map — state that exists already (here, or after
        load_state_dict), steps that ran densely because the source gave None (a trainable HPD frozen later), a group whose
        weight decay was non-zero before — are checked once at the next eager step that has a map, and the source is
        dropped with a warning if they do not qualify.  None detaches."""
        self._mask_source = source
        if any("exp_avg" in st for st in self.state.values()):
            self._fits = None
        self._table_key = None

    def _resolve_masks(self, segs):
        """per segment None | (row-map words, row_elems, lo) from the mask source, or None: the dense step"""
        if self._mask_source is None:
            return None
        given = self._mask_source()
        if not given:
            return None
        out = []
        for sg in segs:
            p, lo = sg[9]
            m = given.get(p)
            if m is None:
                out.append(None)
                continue
            words, row_elems = m[0], int(m[1])
            if (words.dtype != torch.int32 or not words.is_cuda or not words.is_contiguous() or row_elems <= 0
                    or words.numel() * 32 * row_elems < p.numel()):
                raise ValueError("mask source: int32 contiguous device words, one bit per row of row_elems elements, covering the parameter")
            out.append((words, row_elems, lo) if self.mask_record(words.data_ptr(), row_elems, lo)[0] else None)
        return out if any(m is not None for m in out) else None

    @torch.no_grad()
    def _state_fits_masks(self, segs, masks):
        """One device reduction, one synchronise: exp_avg and exp_avg_sq are zero on every masked-out row of every masked segment."""
        bad = None
        for sg, m in zip(segs, masks):
            if m is None:
                continue
            (p, lo), n = sg[9], sg[5]
            words, re_, _lo = m
            if float(self.param_groups[sg[6]]["weight_decay"]) != 0.0:
                continue                                   # the kernel takes this segment densely
            st = self.state[p]
            nz = (st["exp_avg"].reshape(-1)[lo:lo + n] != 0) | (st["exp_avg_sq"].reshape(-1)[lo:lo + n] != 0)
            rows = -(-n // re_)
            if rows * re_ != n:
                nz = torch.cat([nz, nz.new_zeros(rows * re_ - n)])
            w0 = lo // re_ // 32
            w = words.reshape(-1)[w0:w0 + -(-rows // 32)]
            bits = ((w[:, None] >> torch.arange(32, device=w.device, dtype=torch.int32)) & 1).bool().reshape(-1)[:rows]
            b = (nz.reshape(rows, re_).any(1) & ~bits).any()
            bad = b if bad is None else bad | b
        return bad is None or not bool(bad.item())

    def _fit_key(self, masks):
        """what a masked step relies on: these maps, and these groups taken row by row (the others are dense in the kernel)"""
        return (tuple(None if m is None else (m[0].data_ptr(), m[1]) for m in masks),
                tuple(float(g["weight_decay"]) == 0.0 for g in self.param_groups))

    def _guard(self, segs, masks, capturing=False):
        """masks when the moments are known to fit them, else None: the dense step.  Moments of unknown origin are checked
        once, with one synchronise — never inside a capture (that step stays dense and the check waits for an eager step);
        when they do not fit, the source is dropped: dense from now on."""
        if masks is None:
            return None
        key = self._fit_key(masks)
        if self._fits is True or self._fits == key:
            self._fits = key
            return masks
        if capturing:
            return None
        if self._state_fits_masks(segs, masks):
            self._fits = key
            return masks
        import warnings
        warnings.warn("FusedAdam: the optimizer state has non-zero moments on rows outside the reachable-row map; "
                      "skipping those rows would change results — the mask source is dropped, steps stay dense")
        self._mask_source = None
        return None

    def _segments(self):
        """fp32 parameters: torch.optim.Adam's state layout.  fp16 parameters (fp16 level tables, BASELINE config 5): fp32
        moments plus `master`, the fp32 copy the update is applied to; the fp16 parameter is its rounding."""
        segs = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                grad = p.grad
                g32 = getattr(p, "grad_fp32", None) if grad is None else None      # fp16 tables: the fp32 buffer itself (ops._grad_out)
                if grad is None and g32 is None:
                    continue
                if g32 is not None:
                    if p.dtype != torch.float16 or g32.dtype != torch.float32 or g32.shape != p.shape or not p.is_cuda:
                        raise RuntimeError("grad_fp32 is the fp32 gradient of an fp16 device parameter, same shape")
                    grad = g32
                elif grad.is_sparse or p.dtype not in self.DTYPES or not p.is_cuda or grad.dtype != p.dtype:
                    raise RuntimeError("FusedAdam handles dense fp32 / fp16 device parameters (gradient of the same type)")
                half = p.dtype == torch.float16
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                    st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                if half and "master" not in st:
                    st["master"] = p.detach().float().contiguous()
                if self._step is None:
                    prev = st.get("step", 0.0)
                    self._step = torch.full((), float(prev), dtype=torch.float32, device=p.device)
                st["step"] = self._step          # one shared counter (torch keeps one equal copy per parameter)
                g = grad if grad.is_contiguous() else grad.contiguous()
                for t_ in (p, st["exp_avg"], st["exp_avg_sq"]):
                    if not t_.is_contiguous():
                        raise RuntimeError("FusedAdam needs contiguous parameters and moments")
                # data parallel, sharded optimizer state (parallel.shard_direct_levels): this rank updates elements [lo, hi) of the
                # parameter only — the others' rows arrive with the all-gather that follows the step
                lo, hi = getattr(p, "_adam_range", None) or (0, p.numel())
                if hi <= lo:
                    continue
                segs.append((p.data_ptr() + lo * p.element_size(), g.data_ptr() + lo * g.element_size(), st["exp_avg"].data_ptr() + lo * 4,
                             st["exp_avg_sq"].data_ptr() + lo * 4, (st["master"].data_ptr() + lo * 4) if half else 0, hi - lo, gi,
                             int(half) | (2 if g32 is not None else 0), g, (p, lo)))
        return segs

    def zero_grad(self, set_to_none=True):
        for group in self.param_groups:
            for p in group["params"]:
                if getattr(p, "grad_fp32", None) is not None:
                    p.grad_fp32 = None
        return super().zero_grad(set_to_none=set_to_none)

    def prepare_capture(self, steps=1):
        """Sets aside the pinned staging buffers a hipGraph capture of `steps` step() calls needs (pinned memory cannot be
        allocated while a stream captures) WITHOUT taking a step: call after one backward pass, before capturing."""
        segs = self._segments()
        capturing = torch.cuda.is_current_stream_capturing()
        masks = self._guard(segs, self._resolve_masks(segs), capturing)
        size = len(segs) * (self._RECORD.itemsize + (self._MASK_RECORD.itemsize if masks is not None else 0))
        have = [h for h in self._spares if h.numel() == size]
        for _ in range(max(0, 1 + int(steps) - len(have))):
            self._spares.append(torch.empty((size,), dtype=torch.uint8, pin_memory=True))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        import ctypes
        from ._lib import call, ptr, query, stream_ptr
        segs = self._segments()
        if not segs:
            return loss
        capturing = torch.cuda.is_current_stream_capturing()
        masks = self._guard(segs, self._resolve_masks(segs), capturing)
        if masks is None:
            self._fits = None        # a dense step: the moments it leaves are not known to fit a map that appears later
        mkey = None if masks is None else tuple(None if m is None else (m[0].data_ptr(), m[1]) for m in masks)
        key = (tuple(s_[:8] for s_ in segs), mkey)
        table, total_blocks, masked = self._table, self._total_blocks, self._masked
        if capturing or key != self._table_key:    # pointers moved (first step, new gradient buffers, loaded state)
            masked = masks is not None
            raw, total_blocks = self.pack_records(
                segs, None if masks is None else [None if m is None else (m[0].data_ptr(), m[1], m[2]) for m in masks],
                query("gngf_adam_block_elems"))
            dev = self._step.device
            # Pinned staging + asynchronous copy.  Inside a hipGraph capture (gradients allocated from the graph's pool have
            # their own addresses) the copy becomes a node of the graph, so the captured step owns a private staging buffer
            # and device table that eager steps never touch.
            if capturing:
                # pinned memory cannot be allocated while a stream captures: take one of the buffers set aside beforehand
                spare = [h for h in self._spares if h.numel() == raw.size]
                if not spare:
                    raise RuntimeError("FusedAdam: call prepare_capture() (or run one eager step()) before capturing a step in a graph")
                host = spare[0]
                self._spares.remove(host)
                host.numpy()[:] = raw
                table = torch.empty((raw.size,), dtype=torch.uint8, device=dev)
                table.copy_(host, non_blocking=True)
                self._captured.append(host)
            else:
                if self._host is None or self._host[0][0].numel() != raw.size:
                    # a ring of staging buffers: gradient buffers that alternate between two addresses re-upload the table
                    # every step, and waiting for the PREVIOUS upload would tie the host to the device each step
                    self._host = [[torch.empty((raw.size,), dtype=torch.uint8, pin_memory=True), None] for _ in range(4)]
                    self._table = torch.empty((raw.size,), dtype=torch.uint8, device=dev)
                    self._slot = 0
                    self._spares = [torch.empty((raw.size,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
                slot = self._host[self._slot]
                self._slot = (self._slot + 1) % len(self._host)
                if slot[1] is not None:
                    slot[1].synchronize()          # the upload issued four table changes ago has read this buffer
                slot[0].numpy()[:] = raw
                self._table.copy_(slot[0], non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record()
                self._table_key, self._total_blocks, self._masked, table = key, total_blocks, masked, self._table
        ng = len(self.param_groups)
        lr = (ctypes.c_float * ng)(*[float(g["lr"]) for g in self.param_groups])
        wd = (ctypes.c_float * ng)(*[float(g["weight_decay"]) for g in self.param_groups])
        b1, b2 = self.param_groups[0]["betas"]
        args = (ptr(table), len(segs), total_blocks, ptr(self._step), lr, wd, ng, float(b1), float(b2),
                float(self.param_groups[0]["eps"]), 1.0 / float(self.grad_scale))
        self._last_call = "gngf_adam_step_masked" if masked else "gngf_adam_step"
        if masked:
            # (the mask records follow the segment records in the same table: same staging, same ring, same capture rules)
            call("gngf_adam_step_masked", *args, ctypes.c_void_p(table.data_ptr() + len(segs) * self._RECORD.itemsize), stream_ptr())
        else:
            call("gngf_adam_step", *args, stream_ptr())
        return loss

    def state_dict(self):
        # torch.optim.Adam advances every parameter's `step` tensor in place: hand out one copy per parameter, not the
        # shared counter (a shared tensor would be advanced once per parameter after loading into torch's optimizer)
        sd = super().state_dict()
        sd["state"] = {k: {**v, **({"step": v["step"].detach().clone()} if "step" in v else {})} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch casts loaded state to the parameter's dtype: the fp32 moments / master copy of an fp16 parameter are put back
        from itertools import chain
        ids = list(chain.from_iterable(g["params"] for g in state_dict["param_groups"]))
        params = list(chain.from_iterable(g["params"] for g in self.param_groups))
        for i, p in zip(ids, params):
            src = state_dict["state"].get(i)
            if src is None or p.dtype != torch.float16:
                continue
            for k in ("exp_avg", "exp_avg_sq", "master"):
                if k in src:
                    self.state[p][k] = src[k].detach().to(device=p.device, dtype=torch.float32).clone()
        self._step = None                          # re-read from the loaded per-parameter `step`
        self._table_key = None
        self._fits = None                          # loaded moments: checked against the map at the next eager step that has one


def level_mask_source(net):
    """The mask source of FusedAdam.set_mask_source for a model's level tables: level l's parameter (net.dp.level_params[l], a
    (T, F) table: one row = F elements) is paired with row l of net.reachable_rows(); None while the model has no such map."""
    def source():
        rows = net.reachable_rows()
        if rows is None:
            return None
        return {p: (rows[l], int(p.shape[-1])) for l, p in enumerate(net.dp.level_params)}
    return source


def get_optimizer(net, encoding_lr, HPD_lr, MLP_lr, encoding_weight_decay, HPD_weight_decay, MLP_weight_decay,
                  betas=(0.9, 0.99), eps=1e-15, fused_kernel=None, *, skip_unreachable_rows=False):
    """reference functions.py:96-127.  On the GPU the update runs as one launch of this package's Adam kernel
    (FusedAdam: same rule and state layout as torch.optim.Adam); host tensors (CPU tests of the training algebra) and
    fused_kernel=False use torch.optim.Adam itself.
    skip_unreachable_rows (keyword-only, extension; FusedAdam only): the step visits only the level-table rows the model can
    address (net.reachable_rows(): coordinates in [0, 1]^2) — the same result bit for bit, see FusedAdam.set_mask_source."""
    groups = [{"params": list(net.encoding.parameters()), "lr": encoding_lr, "weight_decay": encoding_weight_decay}]
    if not models.should_use_hash_function:
        groups.append({"params": list(net.HPD.parameters()), "lr": HPD_lr, "weight_decay": HPD_weight_decay})
    groups.append({"params": list(net.mlp.parameters()), "lr": MLP_lr, "weight_decay": MLP_weight_decay})
    # decided from the parameters the optimizer will actually update (hash mode also owns the int64, non-trainable
    # `_prime_numbers` Parameter, which is in no group)
    grouped = [p for g_ in groups for p in g_["params"]]
    on_gpu = bool(grouped) and all(p.is_cuda and p.dtype in FusedAdam.DTYPES for p in grouped)
    if fused_kernel is None:
        fused_kernel = on_gpu
    if fused_kernel:
        opt = FusedAdam(groups, betas=betas, eps=eps)
        if skip_unreachable_rows:
            opt.set_mask_source(level_mask_source(net))
        return opt
    enc = getattr(net, "encoding", None)
    handover = getattr(enc, "grad_fp32_handover", None)
    handover = ops.FP16_TABLE_GRAD_FP32 if handover is None else handover
    if handover and any(p.dtype == torch.float16 for p in groups[0]["params"]):
        raise ValueError("fp16 level tables with the fp32 gradient hand-over (grad_fp32, no .grad) need train.FusedAdam: "
                         "torch.optim.Adam would never see a gradient for them — pass fused_kernel=True or turn the hand-over off")
    return torch.optim.Adam(groups, betas=betas, eps=eps, **({"fused": True} if on_gpu else {}))


def promised_gloss(loss_fn, l_mse):
    """The gradient that will reach the pixel-loss value when the step's total is assemble_loss(...) and backward() is seeded
    with 1: l_mse — but only when loss_fn is this package's Loss (its mse term IS MSELoss(rgb, target)) and l_mse is a plain
    number; anything else makes no promise (the decoder then runs its two-kernel path, correct for any gradient)."""
    if type(loss_fn) is Loss and isinstance(l_mse, (int, float)) and not isinstance(l_mse, bool):
        return float(l_mse)
    return None


def assemble_loss(mse, kls, colls, l_mse, l_js_kl, l_collisions):
    """reference functions.py:243-245, including the '+1 per level while previous_collisions is empty' quirk."""
    loss = mse if (isinstance(l_mse, (int, float)) and l_mse == 1) else l_mse * mse     # (x * 1 is a kernel launch of its own)
    if not models.should_use_hash_function and kls is not None:
        loss = loss + ((l_js_kl * kls) + (l_collisions * colls if colls.nelement() != 0 else 1)).sum(0)
    return loss


def _capture_guarded(body):
    """(graph, body()) with body's launches captured into a torch.cuda.CUDAGraph: the one capture of this module, for a training
    step (GraphedStep._capture) and for a body that is none (a captured score()).  Warm body up eagerly first: what it allocates
    must exist before the capture."""
    import gc
    g = torch.cuda.CUDAGraph()
    # No garbage collection while the stream captures: a collection that happens to run inside the body finalises whatever
    # cyclic garbage earlier work left behind (other models' graphs, events, blocks last used on other streams), and a
    # finaliser that touches the runtime during a capture aborts the process (seen once in round 5: "Fatal Python error:
    # Aborted ... Garbage-collecting" in the middle of a captured forward pass).  torch.cuda.graph collects once on entry;
    # what the body itself leaves behind is collected after the capture has ended.
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        # thread_local: other threads of the process (the RCCL watchdog at world > 1) may query events while we capture
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            result = body()
    finally:
        if gc_was_on:
            gc.enable()
    return g, result


def _previous(previous_collisions, previous_min_possible_collisions, dev):
    """(previous_collisions, previous_min_possible_collisions) on dev, None as the empty tensor the first epoch hands the loss
    (assemble_loss: functions.py:243-245)"""
    empty = torch.tensor([], device=dev)
    return (empty if previous_collisions is None else previous_collisions.to(dev),
            empty if previous_min_possible_collisions is None else previous_min_possible_collisions.to(dev))


class GraphedStep:
    """One optimisation step — zero_grad, net(batch), Loss, the weighted sum of functions.py:243-245, backward and
    optimizer.step() — captured ONCE into a hipGraph per batch shape and replayed for every further batch: the step is
    ~15 short kernels, so eager launch gaps and Python dispatch are a visible fraction of it (0.72 ms eager vs 0.61 ms
    replayed at 2^20 pixels).  Batches are copied into static device buffers; results come back in static buffers that
    the next replay overwrites.

        gs = GraphedStep(net, loss_fn, optimizer, l_mse, l_js_kl, l_collisions, coord_bounds=(max_row, max_col))
        r = gs(batch_x, batch_target)            # r.out (P,C), r.loss, r.mse, r.kls, r.colls, r.idx

    optimizer: a FusedAdam (its step is capturable and needs no host synchronisation) or None (forward + backward only).
    GNGF indexing with a trainable HPD, or with the dense distribution returned, needs `coord_bounds` (an upper bound of
    the coordinates of EVERY batch) so that the vertex rectangle is fixed and no device->host read happens in the step."""

    class Result:
        __slots__ = ("out", "probs", "idx", "loss", "mse", "kls", "colls")

    def __init__(self, net, loss_fn, optimizer, l_mse=1.0, l_js_kl=1.0, l_collisions=1e-3, batch_percentage=1.0,
                 coord_bounds=None, warm=2, unroll=1, cross_replay=False):
        """unroll = k > 1: ONE graph holds k consecutive steps on k batches (run_many): a replay costs ~9 us of launch latency
        on top of its kernels whatever it contains, so k steps per replay spread it over k steps.
        cross_replay: the LAST step of a replay also bins the first batch of the NEXT replay (ops.BinPipeline riders) when the caller
        names it in advance — run_many(batches, next_first=x) / gs(x, y, next_first=x) — so that no step of a steady sequence bins
        at its head, at any unroll (with unroll = 1, the data-parallel case, every step's binning rides on the step before).
        Three graphs instead of one per batch shape: `cold` (its first step bins itself) and two `steady` ones that read one of
        two binning workspaces and fill the other."""
        self.unroll = int(unroll)
        self.cross_replay = bool(cross_replay)
        if optimizer is not None and not isinstance(optimizer, FusedAdam):
            raise TypeError("GraphedStep captures FusedAdam.step(); torch.optim.Adam's step is not capturable here")
        self.net, self.loss_fn, self.optimizer = net, loss_fn, optimizer
        self.weights = (l_mse, l_js_kl, l_collisions)
        self.batch_percentage = batch_percentage
        self.warm = int(warm)
        if coord_bounds is not None:
            net.coord_bounds = (float(coord_bounds[0]), float(coord_bounds[1]))
        self._graphs = {}
        # A captured step works on static buffers anyway (every replay overwrites the previous replay's results), and _body lets
        # go of all gradients before the forward pass: the encoder may keep the table gradient in one buffer from step to step
        # (ops.PERSISTENT_TABLE_GRAD is opt-in per model: an eager loop that may keep old .grad tensors does not get it)
        if getattr(net, "dp", None) is not None:
            net.dp.persist_ok = True

    def _body(self, st, next_x=None, next_ws=None, binned_in=None):
        """next_x: the coordinate buffer of the step that FOLLOWS this one (inside the same graph, or — cross_replay — the first step
        of the next replay) — announced to the encoder, whose pixel-stage launches then carry that batch's binning
        (ops.BinPipeline), into workspace next_ws if given.  binned_in: the workspace that holds THIS step's binned pixels (filled by
        the previous replay's last step); None: found through the pipeline, or binned at the head of the step."""
        net, (l_mse, l_js_kl, l_collisions) = self.net, self.weights
        pipe = getattr(getattr(net, "dp", None), "pipeline", None)
        if pipe is not None:
            pipe.announce(next_x, next_ws)
            if binned_in is not None:
                pipe.seed(st["x"], binned_in)
        shadow = st["shadow"]
        for s_ in shadow.values():
            s_.grad = None
            if getattr(s_, "grad_fp32", None) is not None:
                s_.grad_fp32 = None
        # the step begins with zero_grad (functions.py:199): the parameters let go of the previous step's gradients as well
        # (they get this step's at the end) — a step-to-step gradient buffer (ops.PERSISTENT_TABLE_GRAD) is free to be reused
        for _name, p in st["named"]:
            p.grad = None
            if getattr(p, "grad_fp32", None) is not None:
                p.grad_fp32 = None
        # The step runs on SHADOW leaves (detached aliases of the parameters: same storage, fresh autograd identity).  An
        # autograd leaf's AccumulateGrad node is bound to the stream that was current when it was first created, and it stays
        # alive as long as any earlier graph does (a kept `loss` from an eager step on the default stream is enough): the
        # captured backward would then hop onto the legacy default stream, which cannot take part in a capture
        # (hipStreamEndCapture crashes; tools/dbg_graphed.py).  Fresh leaves get their nodes on the capturing stream.
        # the pixel loss is fused into the decoder: its gradient is formed inside the backward kernel, and its VALUE — which no
        # kernel of the step reads when it enters the total with weight 1 — runs on a parallel branch, joined at the end
        aside = isinstance(l_mse, (int, float)) and l_mse == 1 and (models.should_use_hash_function or getattr(net, "compute_pbar", True) is False)
        prev_aside, net.loss_value_aside = net.loss_value_aside, bool(aside)
        try:
            # backward() below is seeded with 1 and the total is l_mse * mse + (terms without mse): the gradient that reaches the
            # pixel loss IS l_mse — promised to the decoder, which then runs forward and backward in one launch (the promise
            # is only made for this package's own Loss: a custom loss_fn may weigh the pixel term differently)
            with net.fused_mse(st["y"], gloss=promised_gloss(self.loss_fn, l_mse)):
                out, probs, idx, _counts = torch.func.functional_call(net, shadow, (st["x"], self.batch_percentage), {"should_calc_counts": False})
        finally:
            net.loss_value_aside = prev_aside
        mse, kls, colls = self.loss_fn(out, st["y"], None if probs is None else probs.shape[-1], probs, st["pc"], st["pm"])
        loss = assemble_loss(mse, kls, colls, l_mse, l_js_kl, l_collisions)
        if loss is not mse:
            net.join_loss_value()                      # the total is computed from the value: it has to be there
        loss.backward(gradient=st["one"].to(loss.dtype))
        net.join_loss_value()
        for name, p in st["named"]:
            p.grad = shadow[name].grad             # the parameters' own .grad: what the optimizer and the caller read
            g32 = getattr(shadow[name], "grad_fp32", None)
            if g32 is not None or getattr(p, "grad_fp32", None) is not None:
                p.grad_fp32 = g32
        r = GraphedStep.Result()
        r.out, r.probs, r.idx, r.loss, r.mse, r.kls, r.colls = out.detach(), probs, idx, loss.detach(), mse.detach(), kls, colls
        return r

    def _build(self, key, bx, by, pc, pm):
        net = self.net
        if not models.should_use_hash_function and getattr(net, "coord_bounds", None) is None:
            frozen_fast = (net.hpd_is_frozen() and net.dense_probs is False and not net.compute_pbar
                           and not net._should_keep_topk_only)
            if not frozen_fast:
                raise RuntimeError("GraphedStep: GNGF indexing reads the batch's coordinate bounds on the host; pass coord_bounds= "
                                   "(an upper bound over every batch) so that the step has no device->host read")
        named = [(n, p) for n, p in net.named_parameters()]
        st = {"x": bx.detach().clone().contiguous(), "y": by.detach().clone().contiguous(), "pc": pc.detach().clone(),
              "pm": pm.detach().clone(), "one": torch.ones((), device=bx.device),
              "named": [(n, p) for n, p in named if p.requires_grad],
              "shadow": {n: p.detach().requires_grad_(p.requires_grad) for n, p in named}}
        # further batches of an unrolled graph: their own input buffers, everything else shared
        st["more"] = [dict(st, x=torch.empty_like(st["x"]), y=torch.empty_like(st["y"])) for _ in range(self.unroll - 1)]
        for m in st["more"]:
            m["x"].copy_(st["x"])
            m["y"].copy_(st["y"])
        pipe = getattr(getattr(net, "dp", None), "pipeline", None)
        if pipe is not None:
            pipe.reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, self.warm)):        # lazy initialisation (workspaces, cached tables) happens here, not in the capture
                self._body(st)
            if self.optimizer is not None:
                self.optimizer.prepare_capture(self.unroll)      # no optimizer step is taken before the first real batch
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        st["variants"] = {}
        st["pre"] = None                 # (index of the workspace that holds the next replay's first batch, identity of that batch)
        if self.cross_replay and pipe is not None and ops.BIN_PIPELINE:
            plan = ops.EncodePlan(st["x"].shape[0], net._n_ls_host, net._feature_dim)
            if plan.Ls > 0 and plan.interleaved(backward=True) and st["x"].shape[0] > 0:
                # two binning workspaces, allocated outside every capture: each steady graph reads one and fills the other
                st["W"] = [ops.TiledWorkspace(plan, st["x"], launch=False) for _ in range(2)]
                st["x_next"] = st["x"].clone()
        st["graph"], st["results"] = self._capture(st, "cold")
        st["result"] = st["results"][0]
        self._graphs[key] = st
        return st

    _VARIANTS = {"cold": (None, 0), "01": (0, 1), "10": (1, 0)}      # name -> (workspace read by the first step, filled by the last)

    def _capture(self, st, name):
        net = self.net
        pipe = getattr(getattr(net, "dp", None), "pipeline", None)
        reads, fills = self._VARIANTS[name]
        W = st.get("W")
        if self.optimizer is not None and st["variants"]:
            self.optimizer.prepare_capture(self.unroll)
        if pipe is not None:
            pipe.reset()

        def steps():
            results = []
            subs = [st] + st["more"]
            for j, sub in enumerate(subs):
                last = j + 1 == len(subs)
                # step j's pixel-stage launches bin step j + 1's batch (its own static buffer: refilled before every replay);
                # the last step's bin the first batch of the NEXT replay (cross_replay: the caller puts it into x_next beforehand)
                nx = subs[j + 1]["x"] if not last else (st["x_next"] if W is not None else None)
                results.append(self._body(sub, next_x=nx, next_ws=(W[fills] if (last and W is not None) else None),
                                          binned_in=(W[reads] if (j == 0 and W is not None and reads is not None) else None)))
                if self.optimizer is not None:
                    self.optimizer.step()
            return results

        g, results = _capture_guarded(steps)
        if pipe is not None:
            pipe.reset()
        st["variants"][name] = (g, results, self._handover(st))
        return st["variants"][name][:2]

    def _handover(self, st):
        """What a captured step leaves behind on the HOST side for its readers — the parameters' .grad / .grad_fp32, the
        encoder's one-buffer table gradient (parallel.py all-reduces it), the data-parallel bookkeeping of the deferred vertex
        stage — points into the memory pool of the graph that was captured LAST.  Each variant keeps its own set and _adopt()
        puts it back before that variant is replayed: whoever reads p.grad after a replay reads what THAT replay wrote."""
        net = self.net
        dp = getattr(net, "dp", None)
        owners = [m for m in net.modules() if hasattr(m, "_grad_base")]
        return {"grads": [(p, p.grad, getattr(p, "grad_fp32", None)) for _n, p in st["named"]],
                "bases": [(m, m._grad_base, getattr(m, "_grad_base_fp32", None)) for m in owners],
                "dp": None if dp is None else (dp.deferred, dp.tables_reduced)}

    def _adopt(self, handover):
        for p, g, g32 in handover["grads"]:
            p.grad = g
            if g32 is not None or getattr(p, "grad_fp32", None) is not None:
                p.grad_fp32 = g32
        for m, base, base32 in handover["bases"]:
            m._grad_base = base
            if base32 is not None or getattr(m, "_grad_base_fp32", None) is not None:
                m._grad_base_fp32 = base32
        dp = getattr(self.net, "dp", None)
        if dp is not None and handover["dp"] is not None:
            dp.deferred, dp.tables_reduced = handover["dp"]

    def _variant(self, st, use):
        if use not in st["variants"]:
            self._capture(st, use)
        g, results, handover = st["variants"][use]
        self._adopt(handover)
        return g, results

    @staticmethod
    def _ident(t):
        return (id(t), t.data_ptr(), t._version, tuple(t.shape))

    def _replay(self, st, batches, pc, pm, next_first):
        """copies the batches in, picks the graph (steady when the previous call announced exactly batches[0][0]), announces the
        next replay's first batch, replays"""
        use = "cold"
        pre = st.get("pre")
        if "W" in st and pre is not None and batches is not None and pre[2] is batches[0][0] and pre[1] == self._ident(batches[0][0]):
            use = "01" if pre[0] == 0 else "10"
        if batches is not None:
            for sub, (bx, by) in zip([st] + st["more"], batches):
                sub["x"].copy_(bx)
                sub["y"].copy_(by)
        if pc is not None and pc.numel():
            st["pc"].copy_(pc)
            st["pm"].copy_(pm)
        st["pre"] = None
        if "W" in st and next_first is not None and tuple(next_first.shape) == tuple(st["x"].shape):
            st["x_next"].copy_(next_first)
            # (the tensor itself is kept: while it is alive no other tensor can take its id and allocator block — ADVICE r4)
            st["pre"] = (self._VARIANTS[use][1], self._ident(next_first), next_first)
        g, results = self._variant(st, use)
        g.replay()
        return results

    def run_many(self, batches, previous_collisions=None, previous_min_possible_collisions=None, next_first=None):
        """unroll consecutive steps in ONE replay: batches = [(x, target)] * unroll (same shapes).  Returns the list of results.
        next_first (cross_replay): the coordinates of the first batch of the NEXT call — pass that very tensor, unmodified, as its
        batches[0][0] and no step of that replay bins at its head."""
        if len(batches) != self.unroll:
            raise ValueError(f"run_many needs exactly unroll = {self.unroll} batches")
        (x0, y0) = batches[0]
        pc, pm = _previous(previous_collisions, previous_min_possible_collisions, x0.device)
        key = (tuple(x0.shape), tuple(y0.shape), tuple(pc.shape), tuple(pm.shape), bool(models.should_use_hash_function))
        st = self._graphs.get(key)
        if st is None:
            st = self._build(key, x0, y0, pc, pm)
        return self._replay(st, batches, pc, pm, next_first)

    def replay_only(self, key=None):
        """Replays the (only, or the named) captured step on the batch already in its static buffers (benchmarks)."""
        st = self._graphs[key] if key is not None else next(iter(self._graphs.values()))
        g, results = self._variant(st, "cold")
        g.replay()
        return results[0]

    def replay_steady(self, key=None):
        """Benchmarks, cross_replay: replays the steady graph on the batches already in the static buffers (x_next holds the first
        batch again), alternating between the two binning workspaces.  Needs one run_many(..., next_first=batches[0][0]) before."""
        st = self._graphs[key] if key is not None else next(iter(self._graphs.values()))
        pre = st.get("pre")
        if "W" not in st or pre is None:
            return self.replay_only(key)
        use = "01" if pre[0] == 0 else "10"
        g, results = self._variant(st, use)
        st["pre"] = (self._VARIANTS[use][1], *pre[1:])
        g.replay()
        return results[0]

    def __call__(self, batch_x, batch_target, previous_collisions=None, previous_min_possible_collisions=None, next_first=None):
        if self.unroll != 1:
            raise ValueError("an unrolled GraphedStep takes its batches through run_many()")
        return self.run_many([(batch_x, batch_target)], previous_collisions, previous_min_possible_collisions, next_first)[0]


def _graphed_step_for(net, loss_fn, optimizer, weights, batch_percentage, rest, coord_bounds):
    """The GraphedStep (cross_replay) of this net and configuration, cached on net._graphed_step: built anew when the loss, the
    optimizer, the weights (l_mse, l_js_kl, l_collisions), batch_percentage or `rest` — what else the caller's steps depend on
    — differ from the cached one's.  coord_bounds: called only when a step is built (train_epoch's reads the device)."""
    gs = getattr(net, "_graphed_step", None)
    cfg = (id(loss_fn), id(optimizer), *weights, batch_percentage, *rest)
    if gs is None or gs._cfg != cfg:
        gs = GraphedStep(net, loss_fn, optimizer, *weights, batch_percentage, coord_bounds=coord_bounds(), cross_replay=True)
        gs._cfg = cfg
        net._graphed_step = gs
    return gs


def _eager_step(net, loss_fn, optimizer, bx, by, pc, pm, weights, one, batch_percentage=1.0, should_calc_counts=False):
    """One optimisation step launch by launch: zero_grad -> net -> Loss -> weighted sum -> backward -> step (functions.py:199-250).
    one: the seed of backward(), d loss / d loss = 1 as a device scalar — no fill per batch.
    Returns (out, idx, loss, mse, kls, colls, counts)."""
    optimizer.zero_grad()
    by = by.contiguous()
    with (net.fused_mse(by, gloss=promised_gloss(loss_fn, weights[0])) if hasattr(net, "fused_mse") else contextlib.nullcontext()):
        out, probs, idx, counts = net(bx, batch_percentage, should_calc_counts=should_calc_counts)
    mse, kls, colls = loss_fn(out, by, None if probs is None else probs.shape[-1], probs, pc, pm)
    loss = assemble_loss(mse, kls, colls, *weights)
    loss.backward(gradient=one.to(loss.dtype))
    optimizer.step()
    return out, idx, loss, mse, kls, colls, counts


def train_epoch(net, loss_fn, optimizer, x, target, w, h, l_mse, l_js_kl, l_collisions, batch_percentage=1.0,
                should_shuffle=True, shuffled_indices=None, previous_collisions=None, previous_min_possible_collisions=None,
                should_calc_counts=False, graph=False, image=None, slot_counts=False):
    """The batch loop of the reference's train_step (functions.py:183-281): ceil(1/batch_percentage) mini-batches of
    zero_grad -> net -> Loss -> weighted sum -> backward -> step.  graph=True replays each step from a hipGraph
    (GraphedStep, cached on the net per batch shape).  Returns a dict of per-batch device tensors and the outputs /
    indices in batch order; nothing is read back to the host inside the loop.  image: an EpochImage that receives every
    batch's outputs (one launch after the step, outside any graph) — the epoch's image, accuracy and PSNR on the device.
    slot_counts: when the forward passes track the slots they use, rec["used"] is the device (K | 1, L) int32 count of distinct
    slots (net.tracked_slot_counts()) and rec["collisions"], which needs a host read in hash mode, is not formed."""
    net.train()
    shape = w * h
    if image is not None:
        if image.P != shape or (image.perm is not None) != bool(should_shuffle):
            raise ValueError("image= was built for another image size, or with / without the permutation this epoch uses")
        image.begin()
    num_batches = int(np.ceil(shape / (shape * batch_percentage)))
    step = int(batch_percentage * shape)
    dev = x.device
    pc, pm = _previous(previous_collisions, previous_min_possible_collisions, dev)
    weights = (l_mse, l_js_kl, l_collisions)
    outputs = torch.zeros((shape, target.shape[1]), device=dev)     # (the reference leaves unvisited rows uninitialised)
    indices = None
    rec = {"loss": [], "mse": [], "kls": [], "colls": [], "counts": []}
    one = torch.ones((), device=dev)                 # seed of backward(): the same d loss / d loss = 1, without a fill per batch
    # the reference's collision statistic (functions.py:327) without the index tensor: when the model does not return indices the
    # forward passes mark the slots their batches use (models.start_collision_tracking) and train_step reads the maps
    # (a dense_levels model cannot track — the marking kernel serves the spatial hash only: the statistic comes from its indices)
    tracked = (hasattr(net, "start_collision_tracking") and not getattr(net, "return_indices", True) and not should_calc_counts
               and not models.should_batchnorm_data and not getattr(net, "_dense_levels", False))
    if tracked:
        net.start_collision_tracking()
    elif hasattr(net, "stop_collision_tracking"):
        net.stop_collision_tracking()
    rec["tracked"] = tracked
    gs = None
    if graph:
        gs = _graphed_step_for(net, loss_fn, optimizer, weights, batch_percentage, (tracked,), lambda: (
            None if models.should_use_hash_function else (float(x[:, 0].max()), float(x[:, 1].max()))))

    def batch(b):
        lo_, hi_ = b * step, (b + 1) * step
        sel = shuffled_indices[lo_:hi_].long() if should_shuffle else slice(lo_, hi_)
        return x[sel].contiguous(), target[sel]

    pipe = getattr(getattr(net, "dp", None), "pipeline", None)
    upcoming = batch(0) if num_batches > 0 else None
    for b in range(num_batches):
        lo, hi = b * step, (b + 1) * step
        bx, by = upcoming
        # the batches are fixed slices of one permutation (functions.py:186-194): the next one is materialised a step ahead and
        # announced, so that this step's pixel-stage launches bin it (ops.BinPipeline; eager steps only — a replayed step
        # copies its batch into static buffers)
        upcoming = batch(b + 1) if b + 1 < num_batches else None
        if pipe is not None:
            pipe.announce(upcoming[0] if (upcoming is not None and gs is None and upcoming[0].shape == bx.shape and bx.shape[0] > 0) else None)
        if bx.shape[0] == 0:
            continue
        if gs is not None and not should_calc_counts:
            # (the next slice is named a step ahead: this replay's launches bin it, the next replay starts on binned pixels)
            nf = upcoming[0] if (upcoming is not None and upcoming[0].shape == bx.shape) else None
            r = gs(bx, by, pc, pm, next_first=nf)
            out, idx, loss, mse, kls, colls, counts = r.out, r.idx, r.loss, r.mse, r.kls, r.colls, []
        else:
            out, idx, loss, mse, kls, colls, counts = _eager_step(net, loss_fn, optimizer, bx, by, pc, pm, weights, one,
                                                                  batch_percentage, should_calc_counts)
        outputs[lo:lo + out.shape[0]] = out.detach()
        if image is not None:
            image.add(out.detach(), lo)
        if idx is not None:
            if indices is None:
                indices = torch.zeros((shape, *idx.shape[1:]), dtype=idx.dtype, device=dev)
            indices[lo:lo + idx.shape[0]] = idx
        rec["loss"].append(loss.detach().clone())
        rec["mse"].append(mse.detach().clone())
        if kls is not None:
            rec["kls"].append(kls.detach().clone())
            rec["colls"].append(colls.detach().clone() if colls.nelement() != 0 else torch.ones_like(kls.detach()))
        rec["counts"].append(counts)
    rec["outputs"], rec["indices"] = outputs, indices
    if tracked:
        if slot_counts:
            rec["used"] = net.tracked_slot_counts()
        else:
            rec["collisions"] = net.tracked_hash_collisions()
        net.stop_collision_tracking()
    return rec


def train_sampled(net, loss_fn, optimizer, sampler, steps, *, l_mse, l_js_kl, l_collisions, graph=True, previous_collisions=None,
                  previous_min_possible_collisions=None):
    """`steps` optimisation steps on batches a data.ImageSampler draws on the device from the image itself (random positions, or
    random pixel centres) — no coordinate tensor, no target tensor, no permutation.  Batch k + 1 is drawn before step k runs and
    named to it, so a replayed step (graph=True: GraphedStep with the sampler's coord_bounds and cross_replay, cached on the net)
    bins its successor's pixels and none but the first bins at its head; an eager step (graph=False) is train_epoch's.  The call
    advances sampler.draw by steps + 1: the batch drawn ahead of the last step is not trained on (the next call draws its own).
    Returns {"loss": (steps,), "mse": (steps,)} fp32 device tensors; nothing is read back to the host.  Scoring: score(net,
    sampler) on the device (fit_sampled builds the epoch loop on both).  Hash, dense_levels and GNGF models (frozen or trainable HPD); not should_batchnorm_data (the
    sampler's coordinates are the unit square's) and not with a data-parallel exchange (the ranks would draw the same batches)."""
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    if models.should_batchnorm_data:
        raise ValueError("train_sampled: should_batchnorm_data moves the coordinates out of the unit square the sampler draws in")
    dp = getattr(net, "dp", None)
    if dp is not None and (dp.active or dp.defer_vertex or dp.world > 1 or dp.zero is not None):
        raise ValueError("train_sampled: every rank of a data-parallel exchange would draw the same batches; sharded draws are not built")
    if sampler.buffers < 2:
        raise ValueError("train_sampled draws batch k + 1 while batch k is in use: the sampler needs buffers >= 2")
    net.train()
    dev = sampler.image.device
    pc, pm = _previous(previous_collisions, previous_min_possible_collisions, dev)
    weights = (l_mse, l_js_kl, l_collisions)
    losses = torch.zeros((steps,), device=dev)
    mses = torch.zeros((steps,), device=dev)
    if steps == 0:
        return {"loss": losses, "mse": mses}
    if hasattr(net, "stop_collision_tracking"):
        net.stop_collision_tracking()
    gs = None
    if graph:
        gs = _graphed_step_for(net, loss_fn, optimizer, weights, 1.0, (False, "sampled", tuple(sampler.coord_bounds)),
                               lambda: sampler.coord_bounds)
    one = torch.ones((), device=dev)
    pipe = getattr(dp, "pipeline", None)
    upcoming = sampler.next()
    for k in range(steps):
        bx, by = upcoming
        upcoming = sampler.next()                    # batch k + 1, in the other buffer pair: batch k stays as it is
        if gs is not None:
            r = gs(bx, by, pc, pm, next_first=upcoming[0])
            loss, mse = r.loss, r.mse
        else:
            if pipe is not None:
                pipe.announce(upcoming[0] if k + 1 < steps else None)
            _out, _idx, loss, mse, _kls, _colls, _counts = _eager_step(net, loss_fn, optimizer, bx, by, pc, pm, weights, one)
        losses[k].copy_(loss.detach())
        mses[k].copy_(mse.detach())
    return {"loss": losses, "mse": mses}


def train_step(net, loss_fn, optimizer, x, target, w, h, hash_table_size, topk_k, l_mse, l_js_kl, l_collisions,
               batch_percentage=1, num_levels=4, should_bw=False, should_calc_counts=False, should_shuffle=True,
               shuffled_indices=None, reordered_indices=None, previous_collisions=None,
               previous_min_possible_collisions=None, *, graph=False, image=None):
    """reference functions.py:139-355 — same positional signature and the same 9-tuple:
        (loss, to_show_img (h,w,3) int32 numpy, collisions, min_possible_collisions, counts_per_level, mse,
         kl_div_losses (L,) | None, collisions_losses (L,) | None, indices_per_level)
    Differences, all in host-side bookkeeping: values are read back once per epoch instead of per batch; pixels that no
    batch visits (int(batch_percentage * w * h) * num_batches < w * h) show as zeros where the reference shows
    uninitialised memory; collision statistics are taken over each pixel's own top-K indices (the reference allocates
    topk_k / batch_size index slots per pixel and fills topk_k of them, so its statistic is partly uninitialised memory —
    SURVEY.md §8f.3).  graph=True (keyword-only, extension) replays every step from a hipGraph.  image= (keyword-only,
    extension): an EpochImage that collects the epoch's image on the device; position 1 of the tuple is then None — no gather,
    cast or host copy of the outputs — and the caller reads image.psnr(), image.accuracy() and, when wanted, image.image()."""
    import collections
    import functools
    import operator
    rec = train_epoch(net, loss_fn, optimizer, x, target, w, h, l_mse, l_js_kl, l_collisions, batch_percentage=batch_percentage,
                      should_shuffle=should_shuffle, shuffled_indices=shuffled_indices, previous_collisions=previous_collisions,
                      previous_min_possible_collisions=previous_min_possible_collisions, should_calc_counts=should_calc_counts,
                      graph=graph, image=image)
    hash_mode = bool(models.should_use_hash_function)
    loss_item = float(torch.stack(rec["loss"]).double().mean().item())            # np.mean over batches (functions.py:286)
    mse_loss = float(torch.stack(rec["mse"]).double().mean().item())
    no_dist = hash_mode or not rec["kls"]
    kl_div_losses = None if no_dist else torch.stack(rec["kls"]).double().mean(0).cpu().numpy()
    collisions_losses = None if no_dist else torch.stack(rec["colls"]).double().mean(0).cpu().numpy()
    outputs, indices = rec["outputs"], rec["indices"]
    if should_shuffle and (image is None or indices is not None):
        ro = reordered_indices
        if ro is None:                                  # inverse permutation (main.py:55-58)
            ro = torch.empty_like(shuffled_indices)
            ro[shuffled_indices.long()] = torch.arange(shuffled_indices.numel(), device=shuffled_indices.device, dtype=ro.dtype)
        ro = ro.long().to(outputs.device)
        outputs = outputs[ro] if image is None else None
        indices = indices[ro] if indices is not None else None
    indices_per_level = []
    if should_calc_counts and indices is not None:
        flat = indices.permute(1, 0, *range(2, indices.dim())).reshape(indices.shape[1], -1).cpu().numpy()
        indices_per_level = [dict(zip(*np.unique(level, return_counts=True))) for level in flat]
    if indices is not None:
        collisions, min_possible_collisions = net.calc_hash_collisions(indices)
    elif rec.get("collisions") is not None:             # return_indices = False: the slot maps the forward passes marked
        collisions, min_possible_collisions = rec["collisions"]
    else:
        collisions, min_possible_collisions = torch.tensor([]), torch.tensor([])
    to_show_img = None
    if image is None:
        to_show_img = (outputs * 255).reshape((h, w, 3) if not should_bw else (h, w)).int().detach().cpu().numpy()
    counts_per_level = [
        dict(functools.reduce(operator.add, map(collections.Counter, [c[i] for c in rec["counts"]])))
        for i in range(num_levels) if should_calc_counts
    ]
    return (loss_item, to_show_img, collisions, min_possible_collisions, counts_per_level, mse_loss, kl_div_losses,
            collisions_losses, indices_per_level)


def calc_psnr(pred: np.ndarray, target: np.ndarray) -> float:
    """reference functions.py:134-136 (peak = max(target))."""
    mse = np.square(pred - target).mean()
    return 20 * np.log10(np.max(target)) - 10 * np.log10(mse)


def calc_accuracy(predicted: np.ndarray, target: np.ndarray, size: int) -> float:
    """reference functions.py:130-131: the share of equal elements, in percent."""
    return (np.equal(predicted, target).sum() / size) * 100


def psnr_from_sums(sse, n, peak_term):
    """calc_psnr from the integer sum of squared differences over n elements: peak_term = 20 * np.log10(np.max(target)) as
    numpy evaluates it on the caller's array (a float16 for a uint8 image), the mean formed in float64 as np.mean does.  inf
    at sse == 0, as numpy gives."""
    with np.errstate(divide="ignore"):
        return peak_term - 10 * np.log10(np.float64(sse) / n)


class EpochImage:
    """The epoch's image and its two statistics on the device (reference functions.py:308, 332-335, 690-692): begin() once
    per epoch, add(out, lo) per batch, then accuracy() / psnr() read 16 bytes; image() is the only bulk copy, on demand.
    og_image: the array the caller would hand to calc_psnr, (h,w,3) or (h,w), whole values 0..255.  shuffled_indices: the
    epoch's permutation (batch row lo + i is pixel shuffled_indices[lo + i]); None: batches are consecutive pixels."""

    def __init__(self, og_image, shuffled_indices=None, device="cuda"):
        og = np.asarray(og_image)
        if og.ndim not in (2, 3) or og.size == 0 or (og.ndim == 3 and not 1 <= og.shape[2] <= 4):
            raise ValueError(f"og_image must be (h,w) or (h,w,C) with C <= 4, got {og.shape}")
        self.h, self.w = int(og.shape[0]), int(og.shape[1])
        self.C = 1 if og.ndim == 2 else int(og.shape[2])
        self.shape = tuple(og.shape)
        self.P = self.h * self.w
        self.n_elems = self.P * self.C
        t8 = og.astype(np.uint8)
        if not np.array_equal(t8, og):
            raise ValueError("og_image must hold whole values in 0..255")
        # exactly calc_psnr's expression on the array as passed: numpy rounds it to float16 for a uint8 image, and every PSNR
        # computed by calc_psnr carries that rounding
        self.peak_term = 20 * np.log10(np.max(og_image))
        dev = torch.device(device)
        self.perm = None
        if shuffled_indices is not None:
            perm = torch.as_tensor(shuffled_indices).reshape(-1)
            if perm.numel() != self.P or perm.dtype.is_floating_point:
                raise ValueError(f"shuffled_indices must be {self.P} integers")
            if int(perm.min()) < 0 or int(perm.max()) >= self.P:      # the kernel trusts it: a bad index would be a stray write
                raise ValueError(f"shuffled_indices must lie in [0, {self.P})")
            self.perm = perm.to(device=dev, dtype=torch.int32).contiguous()
        self.target = torch.from_numpy(np.ascontiguousarray(t8).reshape(-1)).to(dev)
        self.img = torch.zeros((self.P, self.C), dtype=torch.int32, device=dev)
        self._sums = torch.zeros((2,), dtype=torch.int64, device=dev)
        self._workspace = ops.image_metrics_workspace(self.n_elems, dev)

    def begin(self):
        """zeroes the image: pixels no batch visits stay 0, as in train_epoch's outputs buffer"""
        self.img.zero_()

    def add(self, out, lo):
        """one batch's decoder output (n,C) fp32 contiguous, whose first row is batch-order row lo of the epoch"""
        if out.dim() != 2 or out.shape[1] != self.C:
            raise ValueError(f"out must be (n, {self.C}), got {tuple(out.shape)}")
        if lo < 0 or lo + out.shape[0] > self.P:
            raise ValueError(f"rows [{lo}, {lo + out.shape[0]}) leave the image's {self.P} pixels")
        ops.image_scatter(out, self.perm, self.img, lo)

    def sums(self):
        """device int64 pair (#equal elements, sum of squared differences); no synchronisation.  Integers: a data-parallel
        caller can all-reduce them."""
        return ops.image_metrics(self.img, self.target, self._sums, self._workspace)

    def accuracy(self):
        eq = self.sums().cpu().numpy()[0]
        return float((eq / self.n_elems) * 100)

    def psnr(self):
        sse = self.sums().cpu().numpy()[1]
        return float(psnr_from_sums(sse, self.n_elems, self.peak_term))

    def image_tensor(self):
        """device int32 (h,w,C) / (h,w) view of the image"""
        return self.img.view(self.shape)

    def image(self):
        return self.image_tensor().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# The epoch loop (reference functions.py:639-814): early stopping, the zero-collision stop, keeping the best model.

class EarlyStopping:
    """reference utils.py:177-205, branch for branch (quirks included: an equal loss resets the counter, should_reset=False
    never moves best_loss, a NaN loss becomes best_loss and then every call resets)."""

    def __init__(self, tolerance: int = 5, min_delta: int = 0, should_reset: bool = True):
        self.tolerance = tolerance
        self.min_delta = min_delta
        self.best_loss = np.inf
        self.counter = 0
        self.early_stop = False
        self._should_reset = should_reset

    def __call__(self, loss):
        if abs(self.best_loss - loss) < self.min_delta and (loss < self.best_loss):
            self.counter += 1
        elif abs(self.best_loss - loss) > self.min_delta and (loss > self.best_loss):
            self.counter += 1
        else:
            if not self._should_reset:
                if self.counter <= 0:
                    self.counter = 0
                else:
                    self.counter -= 1
            else:
                self.counter = 0
                self.best_loss = loss
        if self.counter >= self.tolerance:
            self.early_stop = True


# csrc/epoch.hip: EpochState (128 bytes)
EPOCH_STATE = np.dtype([("take", "<i4"), ("last", "<i4"), ("finished", "<i4"), ("stop", "<i4"), ("reason", "<i4"), ("cause", "<i4"),
                        ("zero_checks", "<i4"), ("zero_all", "<i4"), ("epoch", "<i8"), ("counter", "<i8"), ("best_sse", "<i8"),
                        ("best_epoch", "<i8"), ("last_epoch", "<i8"), ("best_loss", "<f8"), ("reserved", "<i8", (6,))])
STOP_REASONS = {0: None, 1: "epochs", 2: "early_stopping", 3: "zero_collisions"}
# the integer save rule (sse <= best_sse) is the reference's float rule (train_psnr >= best_psnr) while adjacent sums give
# distinct PSNRs: shown for sse <= 2^44 in DESIGN.md §3 (at 2^50 about one adjacent pair in five rounds to the same PSNR)
SSE_ORDER_LIMIT = 1 << 44


def sse_limit0(n, peak_term):
    """The largest integer sse with psnr_from_sums(sse, n, peak_term) >= 0 — the reference's `best_psnr = 0` start
    (functions.py:650) as a bound on the sum of squared differences; -1 when not even sse = 0 qualifies.  Bisection with
    psnr_from_sums itself, which does not increase with sse."""
    def ok(s):
        return bool(psnr_from_sums(s, n, peak_term) >= 0)
    if not ok(0):
        return -1
    lo, hi = 0, 1 << 62                      # ok(lo), not ok(hi)
    if ok(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


def new_epoch_state(best_sse0):
    """the state record gngf_epoch_tail starts from, as a numpy record"""
    st = np.zeros((), dtype=EPOCH_STATE)
    st["zero_all"] = 1
    st["best_sse"] = best_sse0
    st["best_epoch"] = st["last_epoch"] = -1
    st["best_loss"] = np.inf
    return st


def epoch_state_tensor(best_sse0, device):
    """new_epoch_state's record as gngf_epoch_tail takes it: 128 bytes on the device"""
    return torch.from_numpy(new_epoch_state(best_sse0).reshape(1).view(np.uint8).copy()).to(device)


def levels_free_of_collisions(used, nverts, hash_source):
    """The check of functions.py:684 on the distinct-slot counts used (Kc, L): are the last two levels (the one level when
    L = 1) free of collisions?  Hash source: nverts - used == 0; GNGF: mean over k clamped at 0 equals 0, i.e. the integer
    sum over k is <= 0 (models.py:597-607)."""
    used = np.asarray(used, dtype=np.int64).reshape(-1, len(nverts))
    diff = np.asarray(nverts, dtype=np.int64)[None, :] - used
    last2 = diff[:, -2:]
    return bool((last2[0] == 0).all()) if hash_source else bool((last2.sum(0) <= 0).all())


def replay_epoch_decisions(losses, sses, zeros, *, epochs, tolerance, min_delta, should_reset=True, sse_limit):
    """The decisions of the reference's epoch loop (functions.py:650, 681-688, 761-801) on the host, from the per-epoch
    train_loss, the image's sse and — zeros, or None when the rule is off — whether the last two levels were free of
    collisions.  What gngf_epoch_tail computes on the device; tests hold both to the reference's recorded runs."""
    stopper = EarlyStopping(tolerance=tolerance, min_delta=min_delta, should_reset=should_reset)
    best_sse, best_epoch, last_epoch, reason, cause = int(sse_limit), -1, -1, None, 0
    checks = []
    saved, fired, zero_stop, counter = [], [], [], []
    for e in range(min(int(epochs), len(losses))):
        zs = False
        if zeros is not None and e != 0 and len(checks) < 10:
            checks.append(bool(zeros[e]))
            if len(checks) == 10 and all(checks):
                zs = True
                stopper.early_stop = True
                cause = cause or 3
        take = int(sses[e]) <= best_sse
        if take:
            best_sse, best_epoch = int(sses[e]), e
        f = False
        if stopper.early_stop:
            last_epoch, reason = e, STOP_REASONS[cause]
        else:
            if e != 0:
                stopper(losses[e])
                f = bool(stopper.early_stop)
                if f:
                    cause = cause or 2
            if e == epochs - 1:
                last_epoch, reason = e, "epochs"
        saved.append(take), fired.append(f), zero_stop.append(zs), counter.append(int(stopper.counter))
        if last_epoch >= 0:
            break
    return {"saved": saved, "fired": fired, "zero_stop": zero_stop, "counter": counter, "best_epoch": best_epoch,
            "last_epoch": last_epoch, "stop_reason": reason, "epochs_run": len(saved)}


def state_tensors(net, optimizer=None):
    """name -> tensor of everything a checkpoint holds: 'model.<key>' for every entry of net.state_dict() (BatchNorm buffers
    included) and 'optimizer.<i>.<key>' for every tensor of the state of the optimizer's i-th parameter (exp_avg, exp_avg_sq,
    master, step; i counts through the parameter groups as optimizer.state_dict() does)."""
    out = {f"model.{k}": v for k, v in net.state_dict().items()}
    if optimizer is not None:
        i = 0
        for group in optimizer.param_groups:
            for p in group["params"]:
                for k, v in optimizer.state.get(p, {}).items():
                    if torch.is_tensor(v):
                        out[f"optimizer.{i}.{k}"] = v
                i += 1
    return out


class DeviceSnapshot:
    """Shadows of a set of device tensors and a predicated copy into them: take_if(flag) copies every tensor when the device
    int32 `flag` is non-zero (one launch of gngf_snapshot_if, no synchronisation), restore() copies the shadows back,
    tensors() hands them out by name.  "Save the best model" without a file: tensors = state_tensors(net, optimizer), built
    once the optimizer's state exists.  Tensors that share memory (FusedAdam's one step counter) share their shadow."""

    _RECORD = np.dtype([("src", "<u8"), ("dst", "<u8"), ("bytes", "<i8"), ("first", "<i8")])      # csrc/epoch.hip: SnapshotRecord

    @classmethod
    def pack_records(cls, pairs, block_bytes):
        """Pure numpy: (table bytes, records, blocks) for pairs of (src pointer, dst pointer, bytes); pairs of 0 bytes
        are left out, first_block is the running sum of ceil(bytes / block_bytes)."""
        pairs = [(int(s), int(d), int(n)) for s, d, n in pairs if int(n) > 0]
        rec = np.zeros(len(pairs), dtype=cls._RECORD)
        total_blocks = 0
        for i, (s, d, n) in enumerate(pairs):
            rec[i] = (s, d, n, total_blocks)
            total_blocks += -(-n // block_bytes)
        return rec.view(np.uint8).reshape(-1), len(pairs), total_blocks

    def __init__(self, tensors):
        from ._lib import query
        named = dict(tensors) if isinstance(tensors, dict) else {i: t for i, t in enumerate(tensors)}
        for name, t in named.items():
            if not torch.is_tensor(t) or not t.is_cuda:
                raise ValueError(f"DeviceSnapshot: {name!r} does not live on the device — a snapshot is a device-to-device copy. "
                                 "A torch.optim.Adam that is not capturable keeps its step counter on the host: use "
                                 "train.FusedAdam (get_optimizer's choice on the GPU), whose whole state is on the device")
            if not t.is_contiguous():
                raise ValueError(f"DeviceSnapshot: {name!r} is not contiguous")
        self._live, self._shadow = named, {}          # (the copy tables hold raw pointers: both sides are kept alive here)
        by_memory, pairs = {}, []
        for name, t in named.items():
            key = (t.data_ptr(), t.numel() * t.element_size(), t.dtype, tuple(t.shape))
            if key not in by_memory or t.numel() == 0:
                by_memory[key] = torch.empty_like(t)
                pairs.append((t.data_ptr(), by_memory[key].data_ptr(), key[1]))
            self._shadow[name] = by_memory[key]
        self.bytes = sum(n for _s, _d, n in pairs)
        dev = next(iter(named.values())).device if named else torch.device("cuda")
        block = query("gngf_snapshot_block_bytes")
        raw, self._nrec, self._blocks = self.pack_records(pairs, block)
        back, _n, _b = self.pack_records([(d, s, n) for s, d, n in pairs], block)
        self._take = torch.from_numpy(raw.copy()).to(dev)
        self._back = torch.from_numpy(back.copy()).to(dev)
        self._one = torch.ones((1,), dtype=torch.int32, device=dev)

    def take_if(self, flag):
        ops.snapshot_if(self._take, self._nrec, self._blocks, flag)

    def restore(self):
        """the live tensors get the shadows' contents back, in place (a raw copy: autograd's version counters do not move)"""
        ops.snapshot_if(self._back, self._nrec, self._blocks, self._one)

    def tensors(self):
        return dict(self._shadow)


class FitResult:
    """What fit() returns.  log: per recorded epoch, numpy arrays read from the device once — loss, mse (float64), kls,
    colls_loss (epochs, L; NaN in hash mode), eq, sse (int64), used (epochs, Kc, L), counter, saved, stopper_fired,
    zero_stop, and psnr, accuracy derived as EpochImage derives them.  last_epoch: the epoch of the reference's `break` (or
    epochs - 1); best_epoch: the last epoch whose state was saved (-1: none); stop_reason: 'epochs', 'early_stopping' or
    'zero_collisions'; best: the DeviceSnapshot of best_epoch; issued: epochs enqueued (past last_epoch when a poll came
    late); restored: the live state was put back to last_epoch's."""

    def __init__(self, log, last_epoch, best_epoch, stop_reason, best, issued, restored):
        self.log, self.last_epoch, self.best_epoch, self.stop_reason = log, last_epoch, best_epoch, stop_reason
        self.best, self.issued, self.restored = best, issued, restored


def _refuse_host_state(optimizer):
    if isinstance(optimizer, FusedAdam):
        return
    if not all(bool(g.get("capturable", False)) for g in optimizer.param_groups):
        raise ValueError("fit() keeps the best and the final state in device snapshots and never waits for the host: an optimizer "
                         "whose state lives on the host (the step counter of a torch.optim.Adam that is not capturable) cannot take "
                         "part — use train.FusedAdam (get_optimizer's choice on the GPU)")


class _EpochLoop:
    """The device side of an epoch loop, shared by fit() and fit_sampled() (whose "epochs" are rounds): the state record of
    gngf_epoch_tail and its take / last / finished words, the pinned word a poll reads, the two logs, the `best` and `final`
    snapshots, and the count of rounds issued.  Per round the caller runs its steps and then calls tail(), then stop(); after its
    loop, result().  n_elems, peak_term: what the PSNR is formed with; limit: the number of rounds at most; hash_source, tolerance,
    min_delta, should_reset: gngf_epoch_tail's."""

    def __init__(self, net, optimizer, dev, *, limit, n_elems, peak_term, poll_every, exact_final, **tail):
        self.net, self.optimizer, self.dev, self.limit, self.tail_kw = net, optimizer, dev, limit, tail
        self.n_elems, self.peak_term, self.poll_every, self.exact_final = n_elems, peak_term, poll_every, exact_final
        self.L = net._num_levels
        self.nverts = torch.from_numpy(np.asarray(net._level_vertex_counts(), dtype=np.int64)).to(dev)
        self.state = epoch_state_tensor(sse_limit0(n_elems, peak_term), dev)
        flags = self.state.view(torch.int32)
        self.take, self.last, self.finished = flags[0:1], flags[1:2], flags[2:3]
        self.polled = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
        self.logf = self.logi = self.best = self.final = None
        self.Kc = self.issued = 0

    def tail(self, loss, mse, kls, colls, sums, used):
        """after a round's steps: one launch of gngf_epoch_tail on the round's per-step loss / mse (kls, colls: None or per step),
        the image's sums and the distinct-slot counts used (Kc, L) | None, then the predicated copies into the snapshots"""
        if self.best is None:
            # the optimizer's state exists now (the first step has run): the shadows are allocated once, here
            tensors = state_tensors(self.net, self.optimizer)
            self.best = DeviceSnapshot(tensors)
            self.final = DeviceSnapshot(tensors) if self.exact_final else None
            self.Kc = 0 if used is None else int(used.shape[0])
            self.logf = torch.full((self.limit, 2 + 2 * self.L), float("nan"), dtype=torch.float64, device=self.dev)
            self.logi = torch.zeros((self.limit, 6 + self.Kc * self.L), dtype=torch.int64, device=self.dev)
        ops.epoch_tail(self.state, self.logf, self.logi, loss, mse, kls, colls, sums, used, self.nverts, epochs=self.limit, **self.tail_kw)
        self.best.take_if(self.take)
        if self.final is not None:
            self.final.take_if(self.last)
        self.issued += 1

    def stop(self):
        """every poll_every rounds, and after the last: one word read back — the loop's only synchronisation.  True: the device
        has finished, issue no more."""
        if self.issued % self.poll_every != 0 and self.issued != self.limit:
            return False
        self.polled.copy_(self.finished, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return int(self.polled[0]) != 0

    def result(self):
        """the FitResult; rounds issued past the device's last one are undone from the `final` snapshot"""
        st = self.state.cpu().numpy().view(EPOCH_STATE)[0]
        last_epoch, best_epoch = int(st["last_epoch"]), int(st["best_epoch"])
        restored = False
        if self.issued > last_epoch + 1 and self.final is not None:
            self.final.restore()
            restored = True
        n, L = last_epoch + 1, self.L
        lf, li = self.logf[:n].cpu().numpy(), self.logi[:n].cpu().numpy()
        log = {"loss": lf[:, 0], "mse": lf[:, 1], "kls": lf[:, 2:2 + L], "colls_loss": lf[:, 2 + L:2 + 2 * L], "eq": li[:, 0],
               "sse": li[:, 1], "counter": li[:, 2], "saved": li[:, 3].astype(bool), "stopper_fired": li[:, 4].astype(bool),
               "zero_stop": li[:, 5].astype(bool), "used": li[:, 6:].reshape(n, self.Kc, L)}
        log["psnr"] = np.array([float(psnr_from_sums(s, self.n_elems, self.peak_term)) for s in log["sse"]], dtype=np.float64)
        log["accuracy"] = np.array([float((q / self.n_elems) * 100) for q in log["eq"]], dtype=np.float64)
        return FitResult(log, last_epoch, best_epoch, STOP_REASONS[int(st["reason"])], self.best, self.issued, restored)


def fit(net, loss_fn, optimizer, x, target, w, h, og_image, *, epochs, tolerance, min_delta, should_reset=True, l_mse, l_js_kl,
        l_collisions, batch_percentage=1.0, should_shuffle=True, shuffled_indices=None, graph=True, poll_every=16,
        exact_final=True, after_epoch=None):
    """The reference's epoch loop (functions.py:639-814) around train_epoch, with every decision taken on the device: per
    epoch the steps, the image's sums (EpochImage), one launch of gngf_epoch_tail (early stopping as utils.EarlyStopping,
    the zero-collision stop of functions.py:681-688, `train_psnr >= best_psnr`) and a predicated copy of the whole state
    into the `best` snapshot.  The host only enqueues; every poll_every epochs it reads one word (`finished`) — the only
    synchronisation.  Epochs enqueued after the reference's `break` record nothing; exact_final keeps the state of the last
    epoch in a second snapshot and puts it back, so that after fit() model and optimizer are the reference's at its break
    (False: they have taken the extra steps, up to poll_every - 1 epochs).  after_epoch(e): called once the launches of epoch e
    are enqueued; it must not synchronise if the loop is to stay free of host waits.  should_calc_counts is always False.
    Single process: a model whose data-parallel exchange is enabled is refused."""
    dp = getattr(net, "dp", None)
    if dp is not None and (dp.exchange is not None or dp.world > 1 or dp.zero is not None):
        raise ValueError("fit() runs in one process: this model's data-parallel exchange is enabled")
    _refuse_host_state(optimizer)
    epochs, poll_every = int(epochs), max(1, int(poll_every))
    if epochs < 1:
        raise ValueError("epochs must be at least 1")
    dev = x.device
    if should_shuffle:
        shuffled_indices = torch.as_tensor(shuffled_indices).to(dev)
    image = EpochImage(og_image, shuffled_indices if should_shuffle else None, device=dev)
    if image.n_elems * 255 ** 2 > SSE_ORDER_LIMIT:
        raise ValueError(f"fit(): {image.n_elems} image elements — the integer save rule is shown to equal the reference's float "
                         f"PSNR comparison for n * 255^2 <= 2^44 only (DESIGN.md §3)")
    hash_mode = bool(models.should_use_hash_function)
    L = net._num_levels
    loop = _EpochLoop(net, optimizer, dev, limit=epochs, n_elems=image.n_elems, peak_term=image.peak_term, poll_every=poll_every,
                      exact_final=exact_final, hash_source=hash_mode, tolerance=tolerance, min_delta=min_delta, should_reset=should_reset)
    nverts_f = loop.nverts.to(torch.float32)
    nverts_host = np.asarray(net._level_vertex_counts(), dtype=np.int64)
    min_possible = torch.from_numpy(np.maximum(nverts_host - net._hash_table_size, 0)).to(dev)
    pc = pm = None
    for e in range(epochs):
        rec = train_epoch(net, loss_fn, optimizer, x, target, w, h, l_mse, l_js_kl, l_collisions, batch_percentage=batch_percentage,
                          should_shuffle=should_shuffle, shuffled_indices=shuffled_indices, previous_collisions=pc,
                          previous_min_possible_collisions=pm, should_calc_counts=False, graph=graph, image=image, slot_counts=True)
        used = rec.get("used")
        if used is None and rec["indices"] is not None:
            used = net._distinct_slot_counts(rec["indices"], L, net._hash_table_size)
        no_dist = hash_mode or not rec["kls"]
        loop.tail(torch.stack(rec["loss"]).float(), torch.stack(rec["mse"]).float(),
                  None if no_dist else torch.stack(rec["kls"]).float(), None if no_dist else torch.stack(rec["colls"]).float(),
                  image.sums(), used)
        if used is not None and not hash_mode:
            # the next epoch's previous_collisions (functions.py:678-679; models.py:597-607), formed on the device
            pc = (nverts_f[None, :] - used.to(torch.float32)).mean(0).clamp_min_(0)
            pm = min_possible
        if after_epoch is not None:
            after_epoch(e)
        if loop.stop():
            break
    return loop.result()


# ------------------------------------------------------------------------------------------------------------------------
# Rendering: the picture a model encodes, on any pixel lattice, in one forward-only launch (csrc/render.inc).

LATTICE_EXACT = 1 << 24      # pixel indices up to here are exact in fp32: the kernel forms coordinates from them


def _check_lattice(rows, cols, denom, origin):
    rows, cols, r0, c0 = int(rows), int(cols), int(origin[0]), int(origin[1])
    if rows < 1 or cols < 1:
        raise ValueError(f"a lattice has at least one row and one column, got {rows} x {cols}")
    if not np.float32(denom) > 0:
        raise ValueError(f"denom must be positive, got {denom}")
    if min(r0, c0) < -LATTICE_EXACT or r0 + rows > LATTICE_EXACT or c0 + cols > LATTICE_EXACT:
        raise ValueError(f"pixel indices must lie in [-2^24, 2^24] (exact in float32), got origin {(r0, c0)} and {rows} x {cols}")
    return rows, cols, r0, c0


def lattice_coordinates(rows, cols, denom, origin=(0, 0)):
    """Host float32 (rows * cols, 2): the (row, col) coordinate of every lattice point, rows outermost —
    ((origin[0] + r) / denom, (origin[1] + c) / denom), each one float32 division, which is what the render kernel computes
    per pixel and, for denom = max(w, h) - 1, what data.normalise_coordinates gives for data.pixel_grid.  For callers and
    tests: render() itself never builds coordinates."""
    rows, cols, r0, c0 = _check_lattice(rows, cols, denom, origin)
    d = np.float32(denom)
    rr = (np.arange(r0, r0 + rows, dtype=np.int64).astype(np.float32) / d).astype(np.float32)
    cc = (np.arange(c0, c0 + cols, dtype=np.int64).astype(np.float32) / d).astype(np.float32)
    return np.stack([np.repeat(rr, cols), np.tile(cc, rows)], axis=1)


_GENERAL_PATH = " — evaluate net(x) on explicit coordinates instead"


def _check_render_model(net, who):
    """What the render kernel holds, for render() and bake(): the decoder's output width C, or ValueError naming net(x)."""
    general = _GENERAL_PATH
    if models.should_batchnorm_data:
        raise ValueError(f"{who}: should_batchnorm_data normalises coordinates with batch statistics, a lattice has none" + general)
    widths = [tuple(seq[0].weight.shape) for seq in net.mlp]
    L, F = net._num_levels, net._feature_dim
    if len(widths) != 3 or widths[0] != (64, L * F) or widths[1] != (64, 64) or widths[2][1] != 64 or widths[2][0] > 4:
        raise ValueError(f"{who}: the render kernel holds a decoder with hidden widths [64, 64] and at most 4 outputs, this one is "
                         f"{[w[::-1] for w in widths]}" + general)
    if L * F > 64:
        raise ValueError(f"{who}: L * F = {L * F} encoder features, the render kernel holds at most 64" + general)
    if F not in (1, 2, 4):
        raise ValueError(f"{who}: feature_dim = {F}, the render kernel gathers rows of 1, 2 or 4 features" + general)
    return widths[2][0]


def _check_unit_square(rows, cols, r0, c0, denom, why):
    d = np.float32(denom)
    hi = max(np.float32(r0 + rows - 1) / d, np.float32(c0 + cols - 1) / d)
    if r0 < 0 or c0 < 0 or hi > 1:
        raise ValueError(f"{why} over [0, 1]^2; this lattice spans [{r0 / float(d):g}, {float(hi):g}]" + _GENERAL_PATH)


def _index_source(net):
    """the ops.MODE_* a model's encoder runs with"""
    if not net._hash_mode:
        return ops.MODE_VERTEX_TABLE
    return ops.MODE_DENSE_HASH if getattr(net, "_dense_levels", False) else ops.MODE_HASH


def _render_setup(net, rows, cols, denom, origin):
    """Validation shared by render(): (rows, cols, r0, c0, denom, C) or ValueError naming net(x) as the general path."""
    if denom is None:
        denom = max(int(rows), int(cols)) - 1           # data.normalise_coordinates: the longer side spans [0, 1]
    rows, cols, r0, c0 = _check_lattice(rows, cols, denom, origin)
    C = _check_render_model(net, "render()")
    why = _unit_square_why(net, "render()")
    if why is not None:
        _check_unit_square(rows, cols, r0, c0, denom, why)
    return rows, cols, r0, c0, float(np.float32(denom)), C


def _forward_outputs(lead, C, dev, rgb, image, out_rgb, out_image, who):
    """The (out_rgb, out_image) a forward-only call writes — None where not asked for — new tensors on dev unless given: rgb
    (prod(lead), C) float32, image (*lead, C) int32 — (*lead) for one channel; lead = (rows, cols) of a render, (P,) of a query.
    ValueError for a buffer of the wrong kind or size."""
    rgb, image = bool(rgb) or out_rgb is not None, bool(image) or out_image is not None
    if not (rgb or image):
        raise ValueError(f"{who}: ask for rgb, image or both")
    n = math.prod(lead)
    for name, t, dt in (("out_rgb", out_rgb, torch.float32), ("out_image", out_image, torch.int32)):
        if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() != n * C):
            raise ValueError(f"{name} must be a contiguous device {dt} tensor of {' x '.join(str(s) for s in (*lead, C))} elements")
    if rgb and out_rgb is None:
        out_rgb = torch.empty((n, C), dtype=torch.float32, device=dev)
    if image and out_image is None:
        out_image = torch.empty((*lead, C) if C != 1 else tuple(lead), dtype=torch.int32, device=dev)
    return out_rgb, out_image


def _asked_for(out_rgb, out_image):
    """what a forward-only call returns: the pair, or whichever was asked for"""
    if out_rgb is not None and out_image is not None:
        return out_rgb, out_image
    return out_rgb if out_rgb is not None else out_image


def _unit_square_why(net, who):
    """why `who` needs its coordinates inside [0, 1]^2 with this model's index source — None for plain hash indexing, which is
    defined on the whole plane"""
    if not net._hash_mode:
        return f"{who}: GNGF indexing looks vertices up in the table"
    if getattr(net, "_dense_levels", False):
        return f"{who}: a dense level clamps a vertex outside its grid, so the model is defined"
    return None


@torch.no_grad()
def _render_vertex_table(net):
    """(vert_idx, vert_w, vstride) over the (n_max + 2)^2 vertices of [0, 1]^2 for the CURRENT HPD weights.  A frozen HPD: the
    model's own cached table (keyed on the parameters' data_ptr / _version, models._frozen_vertex_table).  A trainable HPD is
    updated through raw pointers (FusedAdam, DeviceSnapshot.restore) that move no version counter, so no key can vouch for a
    cached table: it is evaluated anew for every render, the same two calls as the cached one."""
    blend = ops.BLEND_CODES[models.should_softmax_topk_features]
    if net.hpd_is_frozen():
        _tv, ti, w, vstride, _NV, _order = net._frozen_vertex_table(blend)
        return ti, w, vstride
    vstride = net._n_max + 2
    tv, ti, _, _ = ops.HpdVertexFunction.apply(vstride * vstride, vstride, net._topk_k, None, False, models.HPD_CHUNK_BYTES, None,
                                               *net.HPD.flat_params())
    return ti, ops.BlendFunction.apply(tv, blend), vstride


@torch.no_grad()
def _forward_model(net, tables):
    """The model as the forward-only ops calls take it, once the caller has validated its own arguments (a trainable HPD is
    evaluated here): ((tables, n_ls, decoder parameters), keywords) — tables = net.encoding.packed_tables(), the level
    resolutions on their device, the six detached decoder tensors; vert_idx / vert_w / vstride (the vertex table of the current
    HPD weights under GNGF indexing: _render_vertex_table), leaky and mode."""
    ti, w, vstride = (None, None, 0) if net._hash_mode else _render_vertex_table(net)
    return ((tables, net._n_ls_flat(tables.device), [p.detach() for p in net._decoder_params()]),
            dict(vert_idx=ti, vert_w=w, vstride=vstride, leaky=net._leaky, mode=_index_source(net)))


@torch.no_grad()
def render(net, rows, cols, denom=None, origin=(0, 0), *, rgb=True, image=False, out_rgb=None, out_image=None):
    """The picture the model encodes NOW, on the lattice ((origin[0] + r) / denom, (origin[1] + c) / denom), r < rows,
    c < cols: one launch of gngf_render — no coordinate tensor, no binning, no (P, L F) encoding in memory, none of the
    reference-shaped index / probability outputs.  denom None: max(rows, cols) - 1, the training normalisation
    (data.normalise_coordinates), so render(net, h, w) is the trained image itself.  An integer upscale by s of an h x w image:
    rows = (h - 1) s + 1, cols = (w - 1) s + 1, denom = (max(w, h) - 1) s — the original pixels are lattice points.
    Returns what was asked for: rgb (rows * cols, C) float32, image (rows, cols, C) int32 — (rows, cols) for a should_bw model —
    = (rgb * 255).int(), or the pair (rgb, image).  out_rgb / out_image: buffers to write instead of new tensors (each
    implies its output); with every requested output given, a hash-mode or frozen-HPD render allocates nothing and never
    synchronises, so it may be captured in a graph.  GNGF indexing reads the per-vertex table of the current HPD weights
    (_render_vertex_table; a trainable HPD is evaluated per call) and needs the lattice inside [0, 1]^2.
    ValueError: should_batchnorm_data, a decoder other than [64, 64] with at most 4 outputs, L * F > 64, F not in {1, 2, 4} —
    net(x) is the general path."""
    rows, cols, r0, c0, denom, C = _render_setup(net, rows, cols, denom, origin)
    tables = net.encoding.packed_tables()
    out_rgb, out_image = _forward_outputs((rows, cols), C, tables.device, rgb, image, out_rgb, out_image, "render()")
    model, kw = _forward_model(net, tables)
    ops.render_lattice(*model, rows, cols, denom, (r0, c0), out_rgb=out_rgb, out_image=out_image, **kw)
    return _asked_for(out_rgb, out_image)


def _check_query_coordinates(xy, who, unit_square_why):
    """check=True of query(): one min / max reduction, one host read.  ValueError for a non-finite coordinate; with
    unit_square_why (the sources that clamp a vertex), for a coordinate outside [0, 1]^2, worded as render()'s refusal."""
    if xy.numel() == 0:
        return
    lo, hi = (float(v) for v in torch.stack(torch.aminmax(xy)).tolist())        # (NaN propagates through both)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{who}: xy holds non-finite coordinates (min {lo:g}, max {hi:g})")
    if unit_square_why is not None and (lo < 0 or hi > 1):
        raise ValueError(f"{unit_square_why} over [0, 1]^2; these coordinates span [{lo:g}, {hi:g}]" + _GENERAL_PATH)


@torch.no_grad()
def query(net, xy, *, rgb=True, image=False, out_rgb=None, out_image=None, check=True):
    """The model as it is NOW at the coordinates xy — a contiguous device float32 (P, 2) tensor of (row, column) coordinates, the
    order of a training batch (a sampler's x is a valid xy) and of lattice_coordinates — in one launch of gngf_ext3_query: no
    binning, no (P, L F) encoding in memory, none of the reference-shaped index / probability outputs.  Row p is, bit for bit,
    what render() gives a lattice point with the same float32 coordinate.
    Returns what was asked for, as render() does: rgb (P, C) float32, image (P, C) int32 — (P,) for a should_bw model —
    = (rgb * 255).int(), or the pair.  out_rgb / out_image: buffers to write instead of new tensors (each implies its output).
    check=True: one min / max reduction of xy and one host read — ValueError for non-finite coordinates, and for coordinates
    outside [0, 1]^2 where the index source clamps a vertex (GNGF indexing, dense levels): the value there is not the model's.
    Hash indexing is defined on the whole plane.  check=False reads nothing back: with every requested output given, a
    hash-mode or frozen-HPD call allocates nothing and never synchronises, so it may be captured in a graph; out-of-range
    coordinates then read a clamped vertex (never outside a buffer), non-finite ones give unspecified values.
    ValueError for what render() refuses — should_batchnorm_data, a decoder other than [64, 64] with at most 4 outputs,
    L * F > 64, F not in {1, 2, 4}: net(x) is the general path — and for an xy of another kind."""
    C = _check_render_model(net, "query()")
    P = ops.check_query_xy("query()", xy)
    out_rgb, out_image = _forward_outputs((P,), C, xy.device, rgb, image, out_rgb, out_image, "query()")
    if check:
        _check_query_coordinates(xy, "query()", _unit_square_why(net, "query()"))
    tables = net.encoding.packed_tables()
    if tables.device != xy.device:
        raise ValueError(f"query(): xy is on {xy.device}, the model on {tables.device}")
    model, kw = _forward_model(net, tables)
    ops.query_points(*model, xy, out_rgb=out_rgb, out_image=out_image, **kw)
    return _asked_for(out_rgb, out_image)


def _score_render(render_image, out_dim, og_image):
    """render_psnr of the model and of a BakedGrid: render_image(h, w) -> int32 device image, scored against og_image."""
    og = np.asarray(og_image)
    if og.ndim not in (2, 3) or og.size == 0 or (og.ndim == 3 and not 1 <= og.shape[2] <= 4):
        raise ValueError(f"og_image must be (h,w) or (h,w,C) with C <= 4, got {og.shape}")
    t8 = og.astype(np.uint8)
    if not np.array_equal(t8, og):
        raise ValueError("og_image must hold whole values in 0..255")
    h, w = int(og.shape[0]), int(og.shape[1])
    C = 1 if og.ndim == 2 else int(og.shape[2])
    if out_dim != C:
        raise ValueError(f"og_image has {C} channel(s), the model {out_dim}")
    img = render_image(h, w)
    dev = img.device
    n = h * w * C
    sums = ops.image_metrics(img, torch.from_numpy(np.ascontiguousarray(t8).reshape(-1)).to(dev),
                             torch.zeros((2,), dtype=torch.int64, device=dev), ops.image_metrics_workspace(n, dev))
    eq, sse = sums.cpu().numpy()
    return img.view(og.shape), float(psnr_from_sums(sse, n, 20 * np.log10(np.max(og_image)))), float((eq / n) * 100)


def render_psnr(net, og_image):
    """Renders the model at og_image's own lattice — (h,w,3) or (h,w), whole values 0..255, what calc_psnr would be handed — and
    scores it: (image int32 device tensor of og_image's shape, psnr, accuracy), the numbers formed as EpochImage.psnr() /
    .accuracy() form them (integer sums on the device — gngf_image_metrics — floats on the host).  After fit():
    `res.best.restore(); image, psnr, acc = render_psnr(net, og_image)` is the best model's picture and score."""
    return _score_render(lambda h, w: render(net, h, w, rgb=False, image=True), net.mlp[-1][0].weight.shape[0], og_image)


# ------------------------------------------------------------------------------------------------------------------------
# Scoring: the model against the uint8 image it is trained on, in one render launch that writes no picture (csrc/render.inc:
# the scoring form; include/gngf_ext2.h), and the epoch loop of fit() on batches a data.ImageSampler draws.

def scored_elements(h, w, C, step=1):
    """n of score(): the elements of the pixels (i step, j step) of an (h,w,C) image — ceil(h / step) ceil(w / step) C"""
    h, w, C, step = int(h), int(w), int(C), int(step)
    if h < 1 or w < 1 or C < 1 or step < 1:
        raise ValueError(f"scored_elements: h, w, C and step are at least 1, got {(h, w, C, step)}")
    return (-(-h // step)) * (-(-w // step)) * C


def sse_order_refusal(n, who="fit_sampled()"):
    """None, or the text of the refusal when n scored elements are too many for the integer save rule (n * 255^2 must not exceed
    SSE_ORDER_LIMIT: DESIGN.md §3) — with the remedy a scored loop has, a coarser lattice"""
    if int(n) * 255 ** 2 <= SSE_ORDER_LIMIT:
        return None
    return (f"{who}: {int(n)} scored elements — the integer save rule is shown to equal the reference's float PSNR comparison for "
            f"n * 255^2 <= 2^44 only (DESIGN.md §3); score a coarser lattice: raise step (score_step)")


def psnr_accuracy_from_sums(eq, sse, n, image_max):
    """(psnr, accuracy) of score()'s two sums over n elements, as EpochImage forms them: psnr_from_sums with the peak term
    20 * np.log10(np.max(image)) of the WHOLE uint8 image (numpy evaluates it in float16 for a uint8 maximum, and so does this),
    accuracy = eq / n * 100."""
    peak_term = 20 * np.log10(np.uint8(image_max))
    return float(psnr_from_sums(int(sse), int(n), peak_term)), float((int(eq) / int(n)) * 100)


def _score_image(image, denom):
    """(uint8 device tensor (h,w,C), denom) of what score() was handed: a data.ImageSampler (its image and denom) or a tensor"""
    from .data import ImageSampler
    if isinstance(image, ImageSampler):
        return image.image, (image.denom if denom is None else denom)
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("score(): image must be a contiguous device uint8 tensor (h,w) / (h,w,C) or a data.ImageSampler")
    if image.dim() == 2:
        image = image.unsqueeze(-1)
    if image.dim() != 3 or image.numel() == 0:
        raise ValueError(f"score(): image must be (h,w) or (h,w,C), got {tuple(image.shape)}")
    if denom is None:
        denom = max(int(image.shape[0]), int(image.shape[1])) - 1
        if denom < 1:
            raise ValueError("score(): a 1 x 1 image has no default denom (max(h, w) - 1 = 0): pass denom")
    return image, denom


def _score_setup(net, image, step, denom, who):
    """Validation shared by score() and fit_sampled(), render()'s: (image (h,w,C), denom, step) or ValueError naming net(x)."""
    img, denom = _score_image(image, denom)
    h, w, Ci = (int(s) for s in img.shape)
    _check_lattice(h, w, denom, (0, 0))
    step = int(step)
    if step < 1:
        raise ValueError(f"{who}: step must be >= 1, got {step}")
    C = _check_render_model(net, who)
    if Ci != C:
        raise ValueError(f"{who}: the image has {Ci} channel(s), the model {C}" + _GENERAL_PATH)
    why = _unit_square_why(net, who)
    if why is not None:
        _check_unit_square(h, w, 0, 0, denom, why)
    return img, float(np.float32(denom)), step


@torch.no_grad()
def score(net, image, *, step=1, denom=None, out=None):
    """The model NOW against the image it is trained on: (2,) int64 on the device, [eq, sse] — the number of equal elements and
    the sum of squared differences between (rgb * 255).int() of the model at the pixels (i step, j step) and the uint8 image
    there, over n = scored_elements(h, w, C, step) elements.  One launch of the render kernel's scoring form and a one-workgroup
    launch behind it: no int32 image, no upload, no synchronisation.  The integers are those of
    ops.image_metrics(render(net, h, w, denom, image=True)[::step, ::step], image[::step, ::step]) — a scored pixel sees the
    coordinate a full render gives it, and a pixel-centre training batch.
    image: a device uint8 (h,w) / (h,w,C) tensor (denom None: max(h, w) - 1, render()'s default) or a data.ImageSampler (its image
    and its denom); a 1 x 1 tensor image has no default and needs denom.  out: the (2,) int64 device tensor to write; with it, and the workspace cached on the net by an earlier
    call, a hash-mode or frozen-HPD call allocates nothing and may be captured in a graph (a trainable HPD evaluates its vertex
    table per call, as render() does).
    ValueError: what render() refuses (should_batchnorm_data, a decoder other than [64, 64] with at most 4 outputs, L * F > 64,
    F not in {1, 2, 4}, a GNGF or dense_levels model outside [0, 1]^2), a channel count other than the model's, step < 1 —
    net(x) is the general path."""
    img, denom, step = _score_setup(net, image, step, denom, "score()")
    tables = net.encoding.packed_tables()
    dev = tables.device
    if out is None:
        out = torch.empty((2,), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous() or out.numel() != 2:
        raise ValueError("score(): out must be a contiguous device int64 tensor of 2 elements")
    ws = getattr(net, "_score_workspace", None)
    if ws is None or ws.device != dev:
        ws = net._score_workspace = ops.render_score_workspace(dev)
    model, kw = _forward_model(net, tables)
    ops.render_score(*model, img, denom=denom, step=step, sums=out, workspace=ws, **kw)
    return out


def score_psnr(net, image, *, step=1, denom=None):
    """(psnr, accuracy) of the model against the image as host floats — score()'s sums read back (the one synchronisation),
    formed by psnr_from_sums exactly as EpochImage forms them (psnr_accuracy_from_sums): the peak term comes from the WHOLE
    image's maximum, n = scored_elements(h, w, C, step).  denom: score()'s (a 1 x 1 tensor image needs one)."""
    img, denom = _score_image(image, denom)
    eq, sse = score(net, image, step=step, denom=denom).cpu().numpy()
    h, w, C = (int(s) for s in img.shape)
    return psnr_accuracy_from_sums(eq, sse, scored_elements(h, w, C, step), int(img.max()))


def fit_sampled(net, loss_fn, optimizer, sampler, *, rounds, steps_per_round, tolerance, min_delta, should_reset=True, l_mse,
                l_js_kl, l_collisions, score_step=1, graph=True, poll_every=16, exact_final=True, after_round=None):
    """fit() for batches a data.ImageSampler draws: a round is steps_per_round steps of train_sampled, then score(net, sampler,
    step=score_step), then one launch of gngf_epoch_tail — handed the round's per-step loss / mse and the score's sums, with
    kls = colls = used = None — and the predicated copies into the `best` (and, exact_final, the `final`) snapshot: what fit()
    does per epoch, with every decision on the device.  The host only enqueues; every poll_every rounds it reads one word.
    The log's "epochs" are rounds; kls / colls_loss are NaN and used is empty.  The zero-collision stop is OFF: sampled training
    tracks no indices, so there are no distinct-slot counts to check (stop_reason is 'epochs' or 'early_stopping').
    after_round(r, rec): called once the launches of round r are enqueued, with train_sampled's {"loss", "mse"} of the round;
    it must not synchronise if the loop is to stay free of host waits.
    ValueError: what train_sampled refuses (should_batchnorm_data, a data-parallel exchange, a sampler with fewer than 2
    buffers) and fit() refuses (an optimizer whose state lives on the host, rounds < 1), steps_per_round < 1, a model the render
    kernel does not hold (score()'s refusals), and n * 255^2 > SSE_ORDER_LIMIT for the n = scored_elements(h, w, C, score_step)
    scored elements — raise score_step."""
    dp = getattr(net, "dp", None)
    if dp is not None and (dp.exchange is not None or dp.active or dp.defer_vertex or dp.world > 1 or dp.zero is not None):
        raise ValueError("fit_sampled() runs in one process: this model's data-parallel exchange is enabled")
    if models.should_batchnorm_data:
        raise ValueError("fit_sampled(): should_batchnorm_data moves the coordinates out of the unit square the sampler draws in")
    if sampler.buffers < 2:
        raise ValueError("fit_sampled(): train_sampled draws batch k + 1 while batch k is in use: the sampler needs buffers >= 2")
    _refuse_host_state(optimizer)
    rounds, steps_per_round, poll_every = int(rounds), int(steps_per_round), max(1, int(poll_every))
    if rounds < 1 or steps_per_round < 1:
        raise ValueError("fit_sampled(): rounds and steps_per_round must be at least 1")
    img, _denom, score_step = _score_setup(net, sampler, score_step, None, "fit_sampled()")
    n_elems = scored_elements(img.shape[0], img.shape[1], img.shape[2], score_step)
    refusal = sse_order_refusal(n_elems)
    if refusal is not None:
        raise ValueError(refusal)
    dev = img.device
    peak_term = 20 * np.log10(np.uint8(int(img.max())))          # (one read, before the loop)
    loop = _EpochLoop(net, optimizer, dev, limit=rounds, n_elems=n_elems, peak_term=peak_term, poll_every=poll_every,
                      exact_final=exact_final, hash_source=net._hash_mode, tolerance=tolerance, min_delta=min_delta,
                      should_reset=should_reset)
    sums = torch.zeros((2,), dtype=torch.int64, device=dev)
    for r in range(rounds):
        rec = train_sampled(net, loss_fn, optimizer, sampler, steps_per_round, l_mse=l_mse, l_js_kl=l_js_kl,
                            l_collisions=l_collisions, graph=graph)
        score(net, sampler, step=score_step, out=sums)
        loop.tail(rec["loss"], rec["mse"], None, None, sums, None)
        if after_round is not None:
            after_round(r, rec)
        if loop.stop():
            break
    return loop.result()


# ------------------------------------------------------------------------------------------------------------------------
# Baking: once training stops, sum_k w[v, k] table[l, idx[v, k]] is a constant of the (level, vertex) — the vertex grid of a
# training step, over all L levels.  A BakedGrid holds that grid and a copy of the decoder: the picture without the model.

baked_level_offsets = ops.baked_level_offsets       # (offsets, vtot) of a baked grid: the one statement of its layout in Python


class BakedGrid:
    """A model baked for inference (bake()): `grid` (vtot, F) fp32 in baked_level_offsets' layout, `decoder` — COPIES of the
    six decoder tensors [W0, b0, W1, b1, W2, b2] — and the level resolutions (`n_ls` int32 on the grid's device, `n_ls_host`
    the same as a list), with L, F, out_dim, leaky and nbytes (grid + decoder).  It holds no reference to the model, its HPD
    or its tables; data.save_baked / load_baked store and read exactly these fields.
    A SNAPSHOT: nothing ties it to the weights it was baked from — bake again (bake(net, out=baked)) after they change."""

    FIELDS = ("grid", "decoder", "n_ls_host", "L", "F", "out_dim", "leaky")

    def __init__(self, grid, decoder, n_ls_host, leaky, n_ls=None):
        n_ls_host = [int(n) for n in n_ls_host]
        L, vtot = len(n_ls_host), baked_level_offsets(n_ls_host)[1]
        decoder = list(decoder)
        if grid.dim() != 2 or grid.shape[0] != vtot or grid.shape[1] not in (1, 2, 4) or grid.dtype != torch.float32:
            raise ValueError(f"grid must be float32 ({vtot}, F) with F in (1, 2, 4) for resolutions {n_ls_host}, "
                             f"got {grid.dtype} {tuple(grid.shape)}")
        F = int(grid.shape[1])
        shapes = [tuple(t.shape) for t in decoder]
        C = shapes[4][0] if len(shapes) == 6 and len(shapes[4]) == 2 else 0
        if not 0 < L <= 32 or L * F > 64 or not 1 <= C <= 4 or shapes != [(64, L * F), (64,), (64, 64), (64,), (C, 64), (C,)] \
                or any(t.dtype != torch.float32 or t.device != grid.device for t in decoder):
            raise ValueError(f"decoder must be float32 [W0 (64, {L * F}), b0, W1 (64, 64), b1, W2 (C, 64), b2] with C <= 4 on "
                             f"{grid.device}, got {shapes}")
        self.grid, self.decoder = grid.contiguous(), [t.contiguous() for t in decoder]
        self.n_ls_host = n_ls_host
        self.n_ls = n_ls if n_ls is not None else torch.tensor(n_ls_host, dtype=torch.int32, device=grid.device)
        self.L, self.F, self.out_dim, self.leaky = L, F, C, bool(leaky)
        self.nbytes = sum(t.numel() * t.element_size() for t in [self.grid, *self.decoder])

    @torch.no_grad()
    def render(self, rows, cols, denom=None, origin=(0, 0), *, rgb=True, image=False, out_rgb=None, out_image=None):
        """train.render's contract, return shapes and output validation, from the baked grid: one launch of gngf_render_grid,
        no allocation when every requested output is given.  The lattice must lie inside [0, 1]^2 whatever the model's index
        source was — a baked hash model has no rows beyond its grids."""
        if denom is None:
            denom = max(int(rows), int(cols)) - 1
        rows, cols, r0, c0 = _check_lattice(rows, cols, denom, origin)
        _check_unit_square(rows, cols, r0, c0, denom, "BakedGrid.render(): a baked model holds the vertices of its levels")
        out_rgb, out_image = _forward_outputs((rows, cols), self.out_dim, self.grid.device, rgb, image, out_rgb, out_image,
                                              "BakedGrid.render()")
        ops.render_grid(self.grid, self.n_ls, self.n_ls_host, self.decoder, rows, cols, float(np.float32(denom)), (r0, c0),
                        leaky=self.leaky, out_rgb=out_rgb, out_image=out_image)
        return _asked_for(out_rgb, out_image)

    @torch.no_grad()
    def query(self, xy, *, rgb=True, image=False, out_rgb=None, out_image=None, check=True):
        """train.query's contract, return shapes and validation, from the baked grid: one launch of gngf_ext3_query_grid, row p
        bit for bit what render() gives a lattice point with the same float32 coordinate.  check=True refuses non-finite
        coordinates and coordinates outside [0, 1]^2 whatever the model's index source was — a baked hash model has no rows
        beyond its grids; check=False reads nothing back (capturable with the outputs given) and clamps."""
        P = ops.check_query_xy("BakedGrid.query()", xy)
        if xy.device != self.grid.device:
            raise ValueError(f"BakedGrid.query(): xy is on {xy.device}, the grid on {self.grid.device}")
        out_rgb, out_image = _forward_outputs((P,), self.out_dim, xy.device, rgb, image, out_rgb, out_image, "BakedGrid.query()")
        if check:
            _check_query_coordinates(xy, "BakedGrid.query()", "BakedGrid.query(): a baked model holds the vertices of its levels")
        ops.query_grid_points(self.grid, self.n_ls, self.n_ls_host, self.decoder, xy, leaky=self.leaky, out_rgb=out_rgb,
                              out_image=out_image)
        return _asked_for(out_rgb, out_image)

    def render_psnr(self, og_image):
        """train.render_psnr of the baked picture: (image, psnr, accuracy)."""
        return _score_render(lambda h, w: self.render(h, w, rgb=False, image=True), self.out_dim, og_image)


@torch.no_grad()
def bake(net, *, out=None):
    """The model as it is NOW, baked: BakedGrid with grid[offsets[l] + gy (N_l + 2) + gx] = sum_k w[v, k] table[l, idx[v, k]]
    — one launch of gngf_vertex_grid_fwd over all L levels, from the vertex table of the current HPD weights
    (_render_vertex_table: the cached table of a frozen HPD, a fresh evaluation of a trainable one) or, in hash mode, from the
    hashed rows themselves — and copies of the decoder tensors.  out: a BakedGrid of the same shape to refresh in place (grid
    and decoder copies; no allocation).
    A bake is a snapshot.  FusedAdam and DeviceSnapshot.restore() write weights through raw pointers, so nothing can vouch for
    its freshness: the caller bakes again after the weights change.
    ValueError for what render() refuses: should_batchnorm_data, a decoder other than [64, 64] with at most 4 outputs,
    L * F > 64, F not in {1, 2, 4} — net(x) is the general path."""
    C = _check_render_model(net, "bake()")
    tables = net.encoding.packed_tables()
    dev = tables.device
    L, T, F = tables.shape
    n_ls_host = list(net._n_ls_host)
    if out is None:
        out = BakedGrid(torch.empty((baked_level_offsets(n_ls_host)[1], F), dtype=torch.float32, device=dev),
                        [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in net._decoder_params()], n_ls_host,
                        net._leaky)
    elif not isinstance(out, BakedGrid) or out.n_ls_host != n_ls_host or (out.F, out.out_dim, out.leaky) != (F, C, net._leaky) \
            or out.grid.device != dev:
        raise ValueError("bake(): out must be a BakedGrid of this model's shape (resolutions, F, outputs, activation) on its device")
    (_, _, dec), kw = _forward_model(net, tables)
    ti = kw["vert_idx"]
    NV, K = (0, 0) if ti is None else (int(ti.shape[0]), int(ti.shape[1]))
    ops.bake_vertex_grid(tables, out.n_ls, n_ls_host, ti, kw["vert_w"], kw["vstride"], NV, F, T, K, out=out.grid, mode=kw["mode"])
    for d, s in zip(out.decoder, dec):
        d.copy_(s)
    return out
