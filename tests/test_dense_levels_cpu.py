"""CPU: the dense-where-it-fits index source (GNGF_MODE_DENSE_HASH = 2, dense_levels=True) — what can be checked without a device:
the enum and its Python mirror, what every mode-accepting entry point answers BEFORE any launch, the constructor's refusals, the
(N_l + 2)^2 <= T boundary, StepConfig's chain for the new source, and the rounding-zone cap of the render rule for the oracle
values tests/test_gpu_dense_levels.py compares against.

gngf_vertex_grid_fwd / _bwd, gngf_encode_tiled_prepare and gngf_render have no launch-free path on which mode 2 answers
differently from any other value (without buffers they refuse every mode, with buffers they launch): nothing is asserted about
them here; tests/test_gpu_dense_levels.py runs each of them in mode 2."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1          # hipErrorInvalidValue


def test_enum_value_and_python_mirror():
    from collision_handling_in_instantngp_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "gngf.h")).read()
    assert re.search(r"GNGF_MODE_HASH = 0\b.*GNGF_MODE_VERTEX_TABLE = 1\b.*GNGF_MODE_DENSE_HASH = 2\b", header, re.S)
    assert "#define GNGF_ABI_VERSION 15" in header and _lib.ABI_VERSION == 15         # additive: no version of its own
    assert (ops.MODE_HASH, ops.MODE_VERTEX_TABLE, ops.MODE_DENSE_HASH) == (0, 1, 2)
    assert ops.index_source(None) == 0 and ops.index_source(object()) == 1 and ops.index_source(None, 2) == 2
    for bad in ((None, 1), (object(), 2), (object(), 0), (None, 3)):
        with pytest.raises(ValueError):
            ops.index_source(*bad)


def test_entry_points_answer_before_any_launch():
    from collision_handling_in_instantngp_amd import _lib
    lib = _lib.load()
    n = None

    def encode_fwd(mode, P=0):            # xy tables dt vidx vw n_ls enc P L F T K mode vstride NV l0 l1 order stream
        return lib.gngf_encode_fwd(n, n, 0, n, n, n, n, P, 4, 2, 512, 0, mode, 0, 0, 0, 4, n, n)

    def encode_bwd(mode, P=0):            # xy tables dt vidx vw n_ls genc dtables dvw P L F T K mode vstride NV l0 l1 stream
        return lib.gngf_encode_bwd(n, n, 0, n, n, n, n, n, n, P, 4, 2, 512, 0, mode, 0, 0, 0, 4, n)

    # an empty batch is success for every index source there is, and only for those
    assert [encode_fwd(m) for m in (0, 1, 2, 3, -1)] == [0, 0, 0, INVALID, INVALID]
    assert [encode_bwd(m) for m in (0, 1, 2, 3, -1)] == [0, 0, 0, INVALID, INVALID]
    # ... and a batch without buffers is refused before the launch
    assert encode_fwd(2, P=5) == INVALID and encode_bwd(2, P=5) == INVALID

    def fused(mode):                      # sorted items n_items max_items n_ls n_ls_host tables dt vidx vw enc L Ls F T K mode ...
        return lib.gngf_encode_tiled_fwd_fused(n, n, n, 0, n, n, n, 0, n, n, n, 4, 4, 2, 512, 0, mode, 0, 0, 2, 4096, n, n)
    assert fused(0) == 0 and fused(2) == INVALID               # the fused vertex forward keeps rejecting the new source


def test_constructor_refusals_and_the_table_boundary():
    from collision_handling_in_instantngp_amd import models, ops, parallel

    def make(T=484, **kw):
        return models.GeneralNeuralGaugeFields(2, T, 4, 8, 32, [64, 64], [32, 64, 128], T, 2, 4, **kw)
    prev = (models.should_use_hash_function, models.should_batchnorm_data)
    try:
        models.should_use_hash_function, models.should_batchnorm_data = False, False
        with pytest.raises(ValueError, match="should_use_hash_function"):
            make(dense_levels=True)
        models.should_use_hash_function, models.should_batchnorm_data = True, True
        with pytest.raises(ValueError, match="should_batchnorm_data"):
            make(dense_levels=True)
        models.should_batchnorm_data = False
        # N = 8, 12, 20, 32: T = 484 = 22^2 holds the N = 20 grid, 483 does not
        net = make(484, dense_levels=True)
        assert net.dense_level_mask == [True, True, True, False] and net._n_ls_host == [8, 12, 20, 32]
        assert make(483, dense_levels=True).dense_level_mask == [True, True, False, False]
        assert make(64, dense_levels=True).dense_level_mask == [False] * 4
        assert make(2048, dense_levels=True).dense_level_mask == [True] * 4
        assert make(2048).dense_level_mask == [False] * 4 and make(2048)._dense_levels is False
        assert ops.dense_level_mask([20], 484) == [True] and ops.dense_level_mask([20], 483) == [False]
        # the keyword comes after table_dtype, and the state dict is what it was
        import inspect
        names = list(inspect.signature(models.GeneralNeuralGaugeFields.__init__).parameters)
        assert names[-2:] == ["table_dtype", "dense_levels"]
        assert set(net.state_dict()) == set(make(484).state_dict())
        # no data-parallel exchange, no collision tracking
        with pytest.raises(ValueError, match="dense_levels"):
            parallel.enable_vertex_grid_exchange(net, 2)
        assert net.dp.exchange is None and net.dp.world == 1
        parallel.enable_vertex_grid_exchange(net, 1)
        with pytest.raises(RuntimeError, match="dense_levels"):
            net.start_collision_tracking()
        # the indices of the return contract: the dense rows, built in torch
        import torch
        x = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.5, 0.26]])
        n_ls = torch.tensor(net._n_ls_host, dtype=torch.int32)
        idx = torch.full((3, 4, 4), -7, dtype=torch.int64)
        net._dense_rows_into(idx, x, n_ls)
        assert idx[0, 0].tolist() == [0, 1, 10, 11] and idx[1, 0].tolist() == [8 * 10 + 8, 8 * 10 + 9, 9 * 10 + 8, 9 * 10 + 9]
        assert idx[2, 2].tolist() == [5 * 22 + 10, 5 * 22 + 11, 6 * 22 + 10, 6 * 22 + 11] and (idx[:, 3] == -7).all()
    finally:
        models.should_use_hash_function, models.should_batchnorm_data = prev


def test_step_config_of_the_new_source():
    """the chain of the issue: vertex riders build G, the pixel stage fills the grid gradient (dG64 on the interleaved kernels, fp32 on
    the generic ones), gngf_vertex_grid_bwd finishes; direct levels add with atomics; no exchange"""
    from collision_handling_in_instantngp_amd import ops
    n16 = [int(n) for n in __import__("oracle.gngf_oracle", fromlist=["x"]).level_resolutions(16, 512, 16)]
    plan = ops.EncodePlan(2 ** 20, n16, 2)
    args = (plan, 16, 2 ** 19, 2, 2 ** 20, ops.MODE_DENSE_HASH, True, True, True, True, False, True, True, True)
    sc = ops.StepConfig.choose(*args)
    assert (sc.source, sc.staged, sc.direct, sc.binning, sc.vertex_fwd) == ("dense_hash", 16, 0, "prepare", "riders")
    assert (sc.pixel, sc.grad_sink, sc.table_grad, sc.clear, sc.direct_bwd, sc.exchange) == (
        "interleaved", "dG64", "alloc", "decoder", "none", False)
    assert sc.chain().startswith("dense_hash tiled ")
    ng = ops.StepConfig.choose(plan, 16, 2 ** 19, 2, 2 ** 20, ops.MODE_DENSE_HASH, True, False, False, False, False, False, True, True)
    assert (ng.vertex_fwd, ng.grad_sink, ng.table_grad) == ("riders", "none", "none")
    plan4 = ops.EncodePlan(2 ** 20, n16, 4)
    g4 = ops.StepConfig.choose(plan4, 16, 2 ** 19, 4, 2 ** 20, ops.MODE_DENSE_HASH, True, True, False, False, False, False, True, True)
    assert (g4.pixel, g4.grad_sink, g4.clear) == ("generic", "fp32_grid", "riders")
    direct = ops.StepConfig.choose(ops.EncodePlan(100, n16, 2), 16, 2 ** 19, 2, 100, ops.MODE_DENSE_HASH, True, True, False, False, False,
                                   False, True, True)
    assert (direct.staged, direct.direct, direct.direct_bwd, direct.table_grad) == (0, 16, "atomics", "alloc")
    with pytest.raises(ValueError, match="exchange"):
        ops.StepConfig.choose(plan, 16, 2 ** 19, 2, 2 ** 20, ops.MODE_DENSE_HASH, True, True, False, False, True, False, True, True)


def test_oracle_values_keep_the_rounding_zone_small():
    """tests/test_gpu_dense_levels.py::test_render_and_bake_vs_module_forward applies tests/test_gpu_render.py's integer-image rule on
    the 61 x 67 lattice: from the oracle values of its configurations alone, the rounding zone is under 5 % of the elements, and the
    picture is more than three adjacent integers"""
    import test_gpu_render as tr
    from collision_handling_in_instantngp_amd import train
    import dense_levels_helpers as td
    x = train.lattice_coordinates(61, 67, 66)
    for T, F, fp16 in [(512, 2, False), (483, 2, False), (2048, 4, False), (500, 1, False), (512, 2, True)]:
        c = td.cfg(T, F, fp16)
        p = tr.render_params(c)
        if fp16:
            p["tables"] = p["tables"].astype(np.float16).astype(np.float32)
        idx, want = td.oracle_model(p, x, T)
        assert want.shape == (61 * 67, 3) and tr.rounding_zone(want).mean() < 0.05
        q = np.floor(want.astype(np.float64) * 255.0)
        assert all(np.unique(q[:, k]).size > 3 for k in range(3))
        # and the rule itself: three dense levels at T = 512, rows inside the level's grid
        for l, n in enumerate(td.N_LS):
            if (n + 2) ** 2 <= T:
                assert idx[:, l].min() >= 0 and idx[:, l].max() < (n + 2) ** 2
            else:
                assert idx[:, l].max() < T
