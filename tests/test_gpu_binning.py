"""Every reachable form of the pixel binning (csrc/encode_tiled.hip, "binning") against ONE numpy model of the counting sort:
tile = clamp(int(x * TS)), clamp(int(y * TS)) with the cast truncating, bincount, exclusive prefix sums, the work items enumerated
tile by tile.  Exact integers throughout: no tolerances.  The order of the pixels inside a tile is free (it is whatever the atomics
make it); everything else is determined."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (P, tile_shift, NB, chunk): the smallest shapes at which each piece can still go wrong
SHAPES = [
    (1, 0, 1, 1024),          # one pixel, one tile
    (5000, 0, 3, 1024),       # one tile split into five items; block 2 is partial (per_block = 2048)
    (8193, 2, 1, 4096),       # one block, one pixel past a whole (8 pixels per thread x 1024 threads) trip
    (20001, 3, 4, 256),       # most tiles empty (y < 0.3), both clamps run (coordinates at 1.0 and just outside [0, 1])
    (70000, 6, 9, 1024),      # 4096 tiles, more than the workgroup has threads: four consecutive tiles per thread in the scan
]
FORMS = ["four_launch", "prepare_four_launch", "prepare_zero_fill", "prepare_counters", "reserving"]

# the vertex riders of the prepare forms: spatial-hash source, L = 2, F = 2, T = 64, resolutions [4, 8]
N_LS, F, T = [4, 8], 2, 64
VTOT = sum((n + 2) ** 2 for n in N_LS)
ZERO_FLOATS = 4 * (2 * 4096 + 5)          # three zero-fill rider blocks, the last one partial


def _coords(P, seed, strip=False):
    rng = np.random.default_rng(seed)
    xy = rng.random((P, 2), dtype=np.float32)
    if strip:
        xy[:, 1] *= np.float32(0.3)
        edge = np.array([1.0, 1.0, -1e-3, 1.0 + 1e-3, -0.25, 1.5], np.float32)
        where = rng.choice(P, size=2 * edge.size, replace=False)
        xy[where[:edge.size], 0] = edge
        xy[where[edge.size:], 1] = edge
    return xy


def _model(xy, tile_shift, chunk):
    TS = 1 << tile_shift
    ntiles = TS * TS
    cell = np.clip(np.trunc(xy * np.float32(TS)).astype(np.int64), 0, TS - 1)       # (the product is exact: TS is a power of two)
    tile = cell[:, 1] * TS + cell[:, 0]
    counts = np.bincount(tile, minlength=ntiles)
    nit = -(-counts // chunk)
    tile_off = np.concatenate([[0], np.cumsum(counts)])
    tile_item_base = np.concatenate([[0], np.cumsum(nit)])
    rows = [(tile_off[t] + j * chunk, min(chunk, counts[t] - j * chunk), t, nit[t]) for t in np.flatnonzero(counts) for j in range(nit[t])]
    return types.SimpleNamespace(counts=counts, tile_off=tile_off, tile_item_base=tile_item_base,
                                 items=np.array(rows, np.int64).reshape(-1, 4), ids_by_tile=np.argsort(tile, kind="stable"))


@functools.lru_cache(maxsize=None)
def _case(shape, second=False):
    """coordinates and model of a shape, computed once; `second`: another batch of the same shape"""
    P, tile_shift, NB, chunk = shape
    xy = _coords(P, 1000 * SHAPES.index(shape) + (7 if second else 0), strip=(P == 20001))
    xy.setflags(write=False)
    return xy, _model(xy, tile_shift, chunk)


class _Buffers:
    """the outputs of one binning job, pre-filled with values no correct run leaves behind"""

    def __init__(self, shape):
        P, tile_shift, NB, chunk = shape
        ntiles = 1 << (2 * tile_shift)
        self.max_items = -(-P // chunk) + ntiles
        i32 = dict(dtype=torch.int32, device=DEV)
        self.blockhist = torch.full((ntiles * (NB + 1),), -7, **i32)
        self.tile_off = torch.full((ntiles + 1,), -7, **i32)
        self.tile_item_base = torch.full((ntiles + 1,), -7, **i32)
        self.items = torch.full((self.max_items, 4), -7, **i32)
        self.n_items = torch.full((4,), 7, **i32)
        self.sorted = torch.full((P, 4), float("nan"), dtype=torch.float32, device=DEV)

    def pointers(self, lib):
        return [lib.ptr(b) for b in (self.tile_off, self.tile_item_base, self.items, self.n_items, self.sorted)]


def _check(buf, xy, m):
    P = xy.shape[0]
    assert np.array_equal(buf.tile_off.cpu().numpy(), m.tile_off)                   # (closing entry included)
    assert np.array_equal(buf.tile_item_base.cpu().numpy(), m.tile_item_base)
    n_items = buf.n_items.cpu().numpy()
    assert n_items[0] == len(m.items) and np.all(n_items[1:] == 0), n_items
    assert np.array_equal(buf.items.cpu().numpy()[:n_items[0]], m.items)            # start, count, tile, items of the tile
    srt = buf.sorted.cpu().numpy()
    ids = srt[:, 2].copy().view(np.int32)
    assert np.array_equal(np.sort(ids), np.arange(P))                               # every pixel exactly once
    assert np.array_equal(srt[:, :2], xy[ids])                                      # coordinates travel with their index
    assert np.all(srt[:, 3] == 0)
    segment = np.repeat(np.arange(m.counts.size), m.counts)                         # the tile that owns each place of `sorted`
    assert np.array_equal(ids[np.lexsort((ids, segment))], m.ids_by_tile)           # per tile, the model's set of pixels


@pytest.fixture(scope="module")
def lib():
    from collision_handling_in_instantngp_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def vertex(lib):
    """level tables of the riders' vertex stage and the vertex grid gngf_vertex_grid_fwd makes of them"""
    rng = np.random.default_rng(5)
    v = types.SimpleNamespace(tables=torch.as_tensor(rng.standard_normal((len(N_LS), T, F)).astype(np.float32)).to(DEV),
                              n_ls=torch.tensor(N_LS, dtype=torch.int32, device=DEV), n_ls_c=(ctypes.c_int32 * len(N_LS))(*N_LS))
    v.G = torch.full((VTOT, F), float("nan"), dtype=torch.float32, device=DEV)
    lib.call("gngf_vertex_grid_fwd", lib.ptr(v.tables), 0, None, None, lib.ptr(v.n_ls), v.n_ls_c, lib.ptr(v.G), len(N_LS), F, T, 0, 0, 0, 0,
             lib.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(v.G).any()
    return v


def _counters(kind, ntiles):
    from collision_handling_in_instantngp_amd import ops
    owner = types.SimpleNamespace(bin_ws={})           # counters of this test alone, zero as at their first use
    return ops._bin_workspace(torch.device(DEV, torch.cuda.current_device()), ntiles, owner, kind=kind)


def _prepare(lib, vertex, shape, xy_dev, buf, words, zero_fill=None, counters=None):
    """gngf_encode_tiled_prepare with the vertex riders on; returns (G, dG_zero) as the call left them"""
    P, tile_shift, NB, chunk = shape
    G = torch.full((VTOT, F), float("nan"), dtype=torch.float32, device=DEV)
    dG_zero = torch.full((VTOT * F * words + (4 if words == 2 else 0),), float("nan"), dtype=torch.float32, device=DEV)
    lib.call("gngf_encode_tiled_prepare", lib.ptr(xy_dev), P, tile_shift, NB, chunk, lib.ptr(buf.blockhist), *buf.pointers(lib),
             lib.ptr(vertex.tables), 0, None, None, lib.ptr(vertex.n_ls), vertex.n_ls_c, lib.ptr(G), lib.ptr(dG_zero), words, len(N_LS), F, T,
             0, 0, 0, 0, lib.ptr(zero_fill), 0 if zero_fill is None else zero_fill.numel(), lib.ptr(counters), None, lib.stream_ptr())
    torch.cuda.synchronize()
    return G, dG_zero


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "P%d_ts%d_NB%d_chunk%d" % s)
@pytest.mark.parametrize("form", FORMS)
def test_binning_form_equals_the_counting_sort_model(lib, vertex, form, shape):
    P, tile_shift, NB, chunk = shape
    ntiles = 1 << (2 * tile_shift)
    xy, m = _case(shape)
    xy_dev = torch.tensor(xy, device=DEV)

    if form == "four_launch":
        buf = _Buffers(shape)
        lib.call("gngf_bin_pixels", lib.ptr(xy_dev), P, tile_shift, NB, chunk, lib.ptr(buf.blockhist), *buf.pointers(lib), lib.stream_ptr())
        torch.cuda.synchronize()
        _check(buf, xy, m)
        return

    if form == "reserving":
        # two different batches back to back on one set of counters: the cursors run on from the first job into the second
        pws = _counters("reserve", ntiles)
        total = np.zeros(ntiles, np.int64)
        for second in (False, True):
            xy_b, m_b = _case(shape, second)
            xy_b_dev = torch.tensor(xy_b, device=DEV)
            buf = _Buffers(shape)
            job = lib.BinJob(lib.ptr(xy_b_dev), P, tile_shift, NB, chunk, lib.ptr(buf.blockhist), lib.ptr(pws), *buf.pointers(lib))
            lib.call("gngf_bin_pixels2", ctypes.byref(job), None, 0, lib.stream_ptr())
            torch.cuda.synchronize()
            _check(buf, xy_b, m_b)
            w = pws.cpu().numpy()
            total += m_b.counts
            assert np.array_equal(w[:ntiles], total)                                # cursors = every pixel ever reserved in the tile
            assert np.array_equal(w[ntiles:2 * ntiles], w[:ntiles])                 # start == cursors: where the next job begins
            assert w[2 * ntiles + 2] == 0                                           # the count ticket
        return

    zero_fill = torch.full((ZERO_FLOATS,), float("nan"), dtype=torch.float32, device=DEV) if form == "prepare_zero_fill" else None
    counters = _counters("prepare", ntiles) if form == "prepare_counters" else None
    for words in (1, 2):                               # (prepare_counters: the second call finds the counters as the first left them)
        buf = _Buffers(shape)
        if zero_fill is not None:
            zero_fill.fill_(float("nan"))
        G, dG_zero = _prepare(lib, vertex, shape, xy_dev, buf, words, zero_fill, counters)
        _check(buf, xy, m)
        assert torch.equal(G, vertex.G)                                             # bit for bit
        assert torch.all(dG_zero == 0)                                              # (words = 2: the two trailing 64-bit words too)
        if zero_fill is not None:
            assert torch.all(zero_fill == 0)
        if counters is not None:
            assert torch.all(counters == 0)
