"""CPU: ops.vertex_flat_list — the static item list of the flat vertex backward (gngf_vertex_grid_bwd_flat) — against a direct numpy
enumeration: every (level, vertex, k) exactly once, sorted by dest with gi ascending inside a run, gi / w / dest as include/gngf.h
defines them; a table the kernel must not gather through is refused on the host."""
import numpy as np
import pytest
import torch

N_LS, VSTRIDE, K, T = (16, 23, 33), 35, 4, 64


def _table(seed=0):
    rng = np.random.default_rng(seed)
    NV = VSTRIDE * VSTRIDE
    return rng.integers(0, T, size=(NV, K)).astype(np.int32), rng.random((NV, K), dtype=np.float32)


def test_list_holds_every_level_vertex_k_once_sorted_by_dest():
    from collision_handling_in_instantngp_amd import ops
    vi, w = _table()
    lst = ops.vertex_flat_list(torch.as_tensor(vi), torch.as_tensor(w), list(N_LS), VSTRIDE, T)
    vtot = sum((n + 2) ** 2 for n in N_LS)
    assert vtot == 2174 and lst.n == 8696 and (lst.Ls, lst.T, lst.vtot) == (3, T, vtot)
    gi, ww, dest = lst.gi.numpy(), lst.w.numpy(), lst.dest.numpy()
    assert gi.dtype == np.int32 and dest.dtype == np.int32 and ww.dtype == np.float32 and gi.shape == ww.shape == dest.shape == (8696,)
    assert bool((np.diff(dest) >= 0).all())                                            # sorted by dest ...
    same = np.diff(dest) == 0
    assert bool((np.diff(gi)[same] >= 0).all())                                        # ... stably: gi ascends inside a run
    assert gi.min() == 0 and gi.max() == vtot - 1 and dest.min() >= 0 and dest.max() < len(N_LS) * T
    # the direct enumeration, as a multiset of (gi, dest, w) — k does not show in the list, (gi, dest, w) triples do
    want = []
    goff = 0
    for l, n in enumerate(N_LS):
        gw = n + 2
        for gy in range(gw):
            for gx in range(gw):
                vid = gy * VSTRIDE + gx
                for k in range(K):
                    want.append((goff + gy * gw + gx, l * T + int(vi[vid, k]), float(w[vid, k])))
        goff += gw * gw
    assert sorted(want) == sorted(zip(gi.tolist(), dest.tolist(), ww.tolist()))
    assert np.array_equal(np.bincount(gi, minlength=vtot), np.full(vtot, K))            # every vertex of every level: K items


def test_out_of_range_slot_and_short_table_are_refused():
    from collision_handling_in_instantngp_amd import ops
    vi, w = _table(1)
    for bad in (T, -1):
        v2 = vi.copy()
        v2[17 * VSTRIDE + 3, 2] = bad                                                  # a vertex of level 1's and level 2's grids
        with pytest.raises(ValueError, match="outside the table"):
            ops.vertex_flat_list(torch.as_tensor(v2), torch.as_tensor(w), list(N_LS), VSTRIDE, T)
    v3 = vi.copy()
    v3[VSTRIDE * VSTRIDE - 1, 0] = T + 5                                               # the last vertex of level 2's grid
    with pytest.raises(ValueError):
        ops.vertex_flat_list(torch.as_tensor(v3), torch.as_tensor(w), list(N_LS), VSTRIDE, T)
    with pytest.raises(ValueError, match="does not fit"):                              # a grid wider than the table's stride
        ops.vertex_flat_list(torch.as_tensor(vi), torch.as_tensor(w), [16, 23, 40], VSTRIDE, T)
    with pytest.raises(ValueError, match="does not fit"):                              # ... or longer than the table
        ops.vertex_flat_list(torch.as_tensor(vi[:-VSTRIDE]), torch.as_tensor(w[:-VSTRIDE]), list(N_LS), VSTRIDE, T)


def test_no_list_above_the_cap_and_lists_follow_their_table():
    from collision_handling_in_instantngp_amd import ops
    vi, w = _table(2)
    tvi, tw = torch.as_tensor(vi), torch.as_tensor(w)
    prev = ops.VERTEX_BWD_FLAT_MAX_ITEMS
    try:
        ops.VERTEX_BWD_FLAT_MAX_ITEMS = 8695
        assert ops.vertex_flat_list(tvi, tw, list(N_LS), VSTRIDE, T) is None
        ops.VERTEX_BWD_FLAT_MAX_ITEMS = 8696
        assert ops.vertex_flat_list(tvi, tw, list(N_LS), VSTRIDE, T).n == 8696
    finally:
        ops.VERTEX_BWD_FLAT_MAX_ITEMS = prev
    # the headline shape stays well below the cap, and its list below the tables it serves
    from oracle import gngf_oracle as orc
    items = sum((int(n) + 2) ** 2 for n in orc.level_resolutions(16, 512, 16)) * 4
    assert items == 2866176 <= ops.VERTEX_BWD_FLAT_MAX_ITEMS and items * 12 < 16 * 2 ** 19 * 2 * 4
    order = torch.arange(8)
    assert ops.attach_flat_lists(order, tvi, tw, list(N_LS), VSTRIDE, T) is order and ops.attach_flat_lists(None, tvi, tw, list(N_LS), VSTRIDE, T) is None
    lists = order.flat_lists
    a = lists.get(2, tvi, tw, T)
    assert a.Ls == 2 and a.n == (18 ** 2 + 25 ** 2) * K and lists.get(2, tvi, tw, T) is a          # built once per level count
    assert lists.get(3, tvi, tw, T).n == 8696
    assert lists.get(2, tvi.clone(), tw, T) is None and lists.get(2, tvi, tw, T + 1) is None       # another table: no list
