"""CPU: the crossing-row table of the row-owning flat vertex backward (ops.flat_crossing_rows: the dest of every run that touches
more than one block of 1024 items, the rows gngf_ext3_vertex_grid_bwd_flat_owned adds to instead of storing) against a numpy
model that walks the runs one by one, on hand-made dest arrays; and StepConfig: the owned configuration is the parent's chain."""
import numpy as np
import pytest
import torch

BLOCK = 1024


def model(dest, block=BLOCK):
    """run by run: [start, end) touches blocks start // block .. (end - 1) // block"""
    dest = np.asarray(dest)
    out = []
    start = 0
    for i in range(1, len(dest) + 1):
        if i == len(dest) or dest[i] != dest[start]:
            if start // block != (i - 1) // block:
                out.append(int(dest[start]))
            start = i
    return np.array(out, dtype=np.int32)


def runs(*lengths, first=3, step=2):
    return np.concatenate([np.full(n, first + step * k, dtype=np.int64) for k, n in enumerate(lengths)])


CASES = {
    "run_ends_on_item_1023_next_starts_on_1024": runs(500, 524, 700, 300),
    "run_spans_four_blocks": runs(1000, 2500, 100),
    "exactly_1024_items": runs(300, 724),
    "exactly_4096_items_boundaries_on_blocks": runs(1024, 1024, 1024, 1024),
    "exactly_4096_items_crossing": runs(1000, 1100, 900, 1096),
    "ragged_last_block": runs(700, 700, 700, 19),
    "single_run_over_the_whole_list": runs(5000),
    "single_run_of_one_block": runs(1024),
    "all_runs_of_length_one": np.arange(3000, dtype=np.int64) * 3 + 1,
    "short_list": runs(5, 6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_crossing_rows_equal_the_run_by_run_model(name):
    from collision_handling_in_instantngp_amd import ops
    assert ops.FLAT_BLOCK_ITEMS == BLOCK
    dest = CASES[name]
    assert bool((np.diff(dest) >= 0).all())
    got = ops.flat_crossing_rows(torch.as_tensor(dest))
    want = model(dest)
    assert got.dtype == torch.int32 and got.is_contiguous()
    assert np.array_equal(got.numpy(), want), (name, got.numpy(), want)
    assert len(want) <= max(0, (len(dest) - 1) // BLOCK)                   # at most one row per block boundary
    assert np.array_equal(np.unique(want), want)                           # each row once, ascending


def test_the_named_cases_are_what_they_say():
    d = CASES["run_ends_on_item_1023_next_starts_on_1024"]
    assert d[1023] != d[1024] and len(model(d)) == 0
    d = CASES["run_spans_four_blocks"]
    assert np.array_equal(model(d), [5]) and len({i // BLOCK for i in np.nonzero(d == 5)[0]}) == 4
    assert len(CASES["exactly_1024_items"]) == 1024 and len(model(CASES["exactly_1024_items"])) == 0
    assert len(CASES["exactly_4096_items_boundaries_on_blocks"]) == 4096 and len(model(CASES["exactly_4096_items_boundaries_on_blocks"])) == 0
    assert len(CASES["exactly_4096_items_crossing"]) == 4096 and len(model(CASES["exactly_4096_items_crossing"])) == 2
    assert len(CASES["ragged_last_block"]) % BLOCK != 0 and len(model(CASES["ragged_last_block"])) == 2
    assert np.array_equal(model(CASES["single_run_over_the_whole_list"]), [3])
    assert len(model(CASES["all_runs_of_length_one"])) == 0


def test_another_block_size_is_honoured():
    from collision_handling_in_instantngp_amd import ops
    dest = runs(3, 6, 2, 5)
    for block in (2, 4, 8, 16):
        assert np.array_equal(ops.flat_crossing_rows(torch.as_tensor(dest), block).numpy(), model(dest, block))


def test_vertex_flat_list_carries_the_crossing_rows():
    from collision_handling_in_instantngp_amd import ops
    rng = np.random.default_rng(5)
    n_ls, K, T = (16, 23, 33), 4, 64
    vstride = max(n_ls) + 2
    vi = torch.as_tensor(rng.integers(0, T, size=(vstride * vstride, K)).astype(np.int32))
    vw = torch.as_tensor(rng.random((vstride * vstride, K), dtype=np.float32))
    lst = ops.vertex_flat_list(vi, vw, list(n_ls), vstride, T)
    assert lst.n == 8696
    want = model(lst.dest.numpy())
    assert len(want) > 0 and np.array_equal(lst.cross.numpy(), want)
    assert int(lst.cross.min()) >= 0 and int(lst.cross.max()) < len(n_ls) * T


def _plan(Ls=16, interleaved=True):
    import types
    return types.SimpleNamespace(Ls=Ls, interleaved=lambda backward: interleaved)


def _choose(owned, **kw):
    from collision_handling_in_instantngp_amd import ops
    args = dict(L=16, T=2 ** 19, F=2, P=2 ** 20, mode=ops.MODE_VERTEX_TABLE, fp32_tables=True, needs_grad=True, link_defer_zero=True,
                link_zero_hidden=True, exchange=False, persist_ok=True, persist_alloc_ok=True, have_reserve_ws=True)
    args.update(kw)
    plan = _plan(args.pop("Ls", 16))
    return ops.StepConfig.choose(plan, args["L"], args["T"], args["F"], args["P"], args["mode"], args["fp32_tables"], args["needs_grad"],
                                 args["link_defer_zero"], args["link_zero_hidden"], args["exchange"], args["persist_ok"],
                                 args["persist_alloc_ok"], args["have_reserve_ws"], flat_list=True, owned_rows=owned)


def test_the_owned_configuration_is_the_parents_chain_with_a_marker():
    parent, owned = _choose(False), _choose(True)
    assert parent.vertex_bwd_flat and owned.vertex_bwd_flat and owned.owned_rows and not parent.owned_rows
    assert owned.chain() == parent.chain() == "vertex_table tiled bin=pipeline vfwd=fused px=interleaved sink=dG64 dE=block/decoder direct=none"
    assert owned.signature() == parent.signature() + " rows=owned"
    assert " rows=owned" not in parent.signature() and parent.signature().endswith(" vbwd=flat")


def test_owned_rows_is_taken_on_the_fused_single_rank_chain_without_direct_levels_only():
    from collision_handling_in_instantngp_amd import ops
    assert _choose(True).owned_rows
    assert not _choose(True, exchange=True).owned_rows                      # an exchange is set up
    assert not _choose(True, Ls=12).owned_rows                              # direct levels add to rows of their own
    assert not _choose(True, mode=ops.MODE_HASH).owned_rows                 # no vertex table
    assert not _choose(True, have_reserve_ws=False).owned_rows              # not the fused chain
    assert not _choose(True, fp32_tables=False).owned_rows
    assert ops.VERTEX_BWD_OWNED == 1 and "vertex_bwd_flat_owned" in ops.STEP_CHAIN_SIGNATURE
