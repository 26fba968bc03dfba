"""CPU: the host side of the row-masked Adam step (train.FusedAdam.pack_records / mask_record) on fake pointers, and a
numpy restatement of the reachable-row map (csrc/stats.hip: gngf_mark_reachable_rows) that tests/test_gpu_adam_masked.py
compares the kernel against."""
import numpy as np
import pytest

from oracle import gngf_oracle as orc


# ------------------------------------------------------------------------------------------------ the expected map, in numpy
def level_vertices(n):
    """(gx, gy) int32 of the (n + 2)^2 vertices 0 <= gx, gy <= n + 1 of a level of resolution n (row-major in gy)."""
    g = np.arange(int(n) + 2, dtype=np.int32)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    return gx.reshape(-1), gy.reshape(-1)


def set_bits(words, slots):
    slots = np.asarray(slots, dtype=np.int64).reshape(-1)
    np.bitwise_or.at(words, slots >> 5, (np.uint32(1) << (slots & 31).astype(np.uint32)).astype(np.uint32))


def expected_hash_row_map(n_ls, T):
    """(L, ceil(T/32)) uint32: bit (slot & 31) of word [l, slot >> 5] for slot = _fast_hash(gx, gy) % T (the oracle's
    spatial_hash) of every vertex of level l."""
    out = np.zeros((len(n_ls), (T + 31) // 32), dtype=np.uint32)
    for l, n in enumerate(n_ls):
        gx, gy = level_vertices(n)
        grid = np.stack([gx, gy], axis=1)[:, :, None, None]              # (P, 2, 1, 1)
        set_bits(out[l], orc.spatial_hash(grid, T)[:, 0, 0])
    return out


def expected_table_row_map(n_ls, T, vert_idx, vstride):
    """the same for a per-vertex table vert_idx (NV, K): the union over k of the rows of vertex gy * vstride + gx"""
    vert_idx = np.asarray(vert_idx)
    out = np.zeros((len(n_ls), (T + 31) // 32), dtype=np.uint32)
    for l, n in enumerate(n_ls):
        gx, gy = level_vertices(n)
        vid = gy.astype(np.int64) * vstride + gx
        vid = vid[(gx < vstride) & (vid < vert_idx.shape[0])]
        rows = vert_idx[vid].reshape(-1)
        set_bits(out[l], rows[(rows >= 0) & (rows < T)])
    return out


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def unpack_rows(words, T):
    """(T,) bool from ceil(T/32) uint32 words"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:T].astype(bool)


def test_expected_map_is_self_consistent():
    L, T = 3, 64
    n_ls = orc.level_resolutions(2, 16, L)
    m = expected_hash_row_map(n_ls, T)
    assert m.shape == (L, 2) and m.dtype == np.uint32
    for l, n in enumerate(n_ls):
        pc = popcount(m[l])
        assert 0 < pc <= min(T, (int(n) + 2) ** 2), (l, pc)
        # one bit per distinct slot, nothing else
        gx, gy = level_vertices(n)
        slots = orc.spatial_hash(np.stack([gx, gy], axis=1)[:, :, None, None], T)[:, 0, 0]
        assert pc == len(np.unique(slots))
        assert np.array_equal(np.flatnonzero(unpack_rows(m[l], T)), np.unique(slots))
    # T no multiple of 32: the last word is partial and no bit at or above T is set
    T2 = 50
    m2 = expected_hash_row_map(n_ls, T2)
    assert m2.shape == (L, 2)
    full = np.unpackbits(m2.view(np.uint8), bitorder="little").reshape(L, 64)
    assert not full[:, T2:].any()
    assert all(popcount(m2[l]) <= min(T2, (int(n) + 2) ** 2) for l, n in enumerate(n_ls))
    # the finest level (18^2 = 324 vertices on 64 rows) saturates the table
    assert popcount(m[2]) == T


def test_expected_table_map_is_the_union_over_k():
    n_ls = np.array([1, 2], dtype=np.int32)
    vstride, K, T = 4, 2, 40
    vert_idx = (np.arange(vstride * vstride * K, dtype=np.int32).reshape(-1, K) * 7) % T
    m = expected_table_row_map(n_ls, T, vert_idx, vstride)
    for l, n in enumerate(n_ls):
        want = set()
        for gy in range(n + 2):
            for gx in range(n + 2):
                want |= set(int(r) for r in vert_idx[gy * vstride + gx])
        assert set(np.flatnonzero(unpack_rows(m[l], T)).tolist()) == want


# ------------------------------------------------------------------------------------------------ record packing
def _train():
    from collision_handling_in_instantngp_amd import train
    return train


def fake_segment(i, n, group=0, flags=0):
    base = 0x7f0000000000 + i * 0x10000000
    return (base, base + 0x1000000, base + 0x2000000, base + 0x3000000, (base + 0x4000000) if flags & 1 else 0, n, group, flags)


def test_mask_record_layout_is_16_bytes():
    FA = _train().FusedAdam
    d = FA._MASK_RECORD
    assert d.itemsize == 16
    assert [(n, d.fields[n][1], d.fields[n][0].itemsize) for n in d.names] == [("mask", 0, 8), ("row_elems", 8, 4), ("reserved", 12, 4)]
    assert FA._RECORD.itemsize == 64


def test_pack_without_masks_is_the_dense_table():
    FA = _train().FusedAdam
    segs = [fake_segment(0, 5000), fake_segment(1, 2048, group=1), fake_segment(2, 1, group=1, flags=3)]
    raw, blocks = FA.pack_records(segs, None, 2048)
    assert raw.dtype == np.uint8 and raw.size == 3 * 64 and blocks == 3 + 1 + 1
    rec = raw.view(FA._RECORD)
    assert rec["first"].tolist() == [0, 3, 4] and rec["n"].tolist() == [5000, 2048, 1]
    assert rec["group"].tolist() == [0, 1, 1] and rec["flags"].tolist() == [0, 0, 3]
    assert rec["p"].tolist() == [s[0] for s in segs] and rec["w"].tolist() == [s[4] for s in segs]


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_pack_with_masks_row_elems_and_offsets(F):
    FA = _train().FusedAdam
    T = 4096
    mask = 0x7e0000001000
    # a whole table; the upper half of one (_adam_range = (T*F/2, T*F)); a decoder tensor without a map
    segs = [fake_segment(0, T * F), fake_segment(1, T * F // 2), fake_segment(2, 64 * 35, group=1)]
    masks = [(mask, F, 0), (mask + 0x100000, F, T * F // 2), None]
    raw, blocks = FA.pack_records(segs, masks, 2048)
    assert raw.size == 3 * 64 + 3 * 16
    dense_raw, dense_blocks = FA.pack_records(segs, None, 2048)
    assert blocks == dense_blocks and np.array_equal(raw[:3 * 64], dense_raw)       # the segment records are untouched
    mrec = raw[3 * 64:].view(FA._MASK_RECORD)
    assert mrec["row_elems"].tolist() == [F, F, 0] and mrec["reserved"].tolist() == [0, 0, 0]
    assert int(mrec["mask"][0]) == mask
    # lo = T*F/2 elements = T/2 rows = T/64 words further on
    assert int(mrec["mask"][1]) == mask + 0x100000 + (T // 2 // 32) * 4
    assert int(mrec["mask"][2]) == 0


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_misaligned_range_takes_the_dense_record(F):
    FA = _train().FusedAdam
    mask = 0x7e0000001000
    assert FA.mask_record(mask, F, 32 * F) == (mask + 4, F)
    assert FA.mask_record(mask, F, 64 * F * 5) == (mask + 40, F)
    for lo in (F, 16 * F, 32 * F + 1, 31 * F, 32 * F - F):
        if lo % (32 * F) == 0:
            continue
        assert FA.mask_record(mask, F, lo) == (0, 0), lo
    segs = [fake_segment(0, 1000), fake_segment(1, 1000)]
    raw, _ = FA.pack_records(segs, [(mask, F, 16 * F), (mask, F, 0)], 2048)
    mrec = raw[2 * 64:].view(FA._MASK_RECORD)
    assert (int(mrec["mask"][0]), int(mrec["row_elems"][0])) == (0, 0)
    assert (int(mrec["mask"][1]), int(mrec["row_elems"][1])) == (mask, F)
    # no map at all, or a nonsensical row width: dense as well
    assert FA.mask_record(0, F, 0) == (0, 0) and FA.mask_record(mask, 0, 0) == (0, 0)
    with pytest.raises(ValueError):
        FA.pack_records(segs, [None], 2048)


def test_get_optimizer_keyword_is_keyword_only_and_off_by_default():
    import inspect
    sig = inspect.signature(_train().get_optimizer)
    p = sig.parameters["skip_unreachable_rows"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_state_guard_checks_whenever_the_moments_were_not_produced_under_the_same_map():
    """FusedAdam._guard, driven without a device: the moments are checked (once) whenever a step resolves a map they are not
    known to fit — after dense steps, after load_state_dict / set_mask_source on existing state, after a group's weight decay
    went to 0 — never while capturing, and not again while consecutive masked steps use the same maps."""
    import torch
    from collision_handling_in_instantngp_amd.train import FusedAdam

    class Words:
        def __init__(self, addr):
            self.addr = addr

        def data_ptr(self):
            return self.addr

    p = torch.nn.Parameter(torch.zeros(4, 2))
    opt = FusedAdam([{"params": [p], "weight_decay": 0.0}, {"params": [torch.nn.Parameter(torch.zeros(3))], "weight_decay": 1e-6}])
    checks, verdict = [], [True]
    opt._state_fits_masks = lambda segs, masks: (checks.append(1), verdict[0])[1]
    opt._mask_source = object()
    a, b = [(Words(4096), 2, 0), None], [(Words(8192), 2, 0), None]
    assert opt._fits is True
    assert opt._guard([], a) is a and not checks                       # no moments yet: any map fits
    assert opt._guard([], a) is a and not checks                       # the same maps again
    assert opt._guard([], b) is b and len(checks) == 1                 # other maps: checked
    assert opt._guard([], None) is None and len(checks) == 1
    opt._fits = None                                                   # what a dense step (or load_state_dict) leaves behind
    assert opt._guard([], b, capturing=True) is None and len(checks) == 1 and opt._fits is None     # dense, the check waits
    assert opt._guard([], b) is b and len(checks) == 2
    assert opt._guard([], b, capturing=True) is b and len(checks) == 2
    opt.param_groups[1]["weight_decay"] = 0.0                          # that group was dense in the kernel until now
    assert opt._guard([], b) is b and len(checks) == 3
    assert opt._guard([], b) is b and len(checks) == 3
    verdict[0] = False
    opt._fits = None
    with pytest.warns(UserWarning, match="reachable-row map"):
        assert opt._guard([], b) is None
    assert opt._mask_source is None and len(checks) == 4
