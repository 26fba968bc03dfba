"""CPU: bench.py's launcher contract — `--gpus N` is what runs, or the run is refused (no GPU call before the decision)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_must_agree_with_gpus_flag():
    import bench
    a = bench.parse_args(["--gpus", "1"])
    assert bench.resolve_world(a, {}) == ("run", 1)
    assert bench.resolve_world(bench.parse_args(["--gpus", "4"]), {}) == ("spawn", 4)          # bare `python bench.py --gpus 4`
    assert bench.resolve_world(bench.parse_args(["--gpus", "4"]), {"WORLD_SIZE": "4"}) == ("run", 4)
    with pytest.raises(SystemExit) as e:
        bench.resolve_world(a, {"WORLD_SIZE": "2"})
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        bench.resolve_world(bench.parse_args(["--gpus", "8"]), {"WORLD_SIZE": "1"})


def test_gpus_1_under_world_size_2_refuses_before_touching_the_gpu():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert "refusing" in r.stderr and r.stdout.strip() == ""


def test_bare_gpus_n_starts_n_rank_processes(monkeypatch):
    """the spawn path hands the same argv to torch.distributed.run with --nproc-per-node N (the child processes are not run here)"""
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    rc = bench.spawn_ranks(2, ["--gpus", "2", "--backend", "gloo", "--steps", "3"])
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "2", "--backend", "gloo", "--steps", "3"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_ab_switches_and_unroll_list_parse():
    """--set NAME=VALUE (same-box A/B of ops switches) and --unrolls a,b,c (steps per replayed graph)"""
    import bench
    a = bench.parse_args(["--set", "DG64=0", "--set", "HASH_VERTEX_FUSION=1", "--unrolls", "10,4,2"])
    assert a.set == ["DG64=0", "HASH_VERTEX_FUSION=1"] and a.unrolls == (10, 4, 2)
    assert bench.parse_args([]).set == [] and 4 in bench.parse_args([]).unrolls


def test_plain_run_is_lean_and_full_is_opt_in():
    """--full (side measurements) is off by default; --dump-outputs names the folder of the last step's outputs"""
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """small arrays in full, large ones as the same seeded sample from run to run (a share of the byte budget in proportion to
    their size), float32 on disk unless float64, never more than the limit"""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 7 * 2 ** 20)          # 1.75 Mi elements: rgb whole, the gradients ~half
    g = torch.Generator().manual_seed(0)
    arrays = {"rgb": torch.rand((2 ** 18, 3), generator=g), "grad.also_big": torch.rand((2 ** 18, 3), generator=g), "loss": torch.tensor(0.25),
              "grad.big": torch.rand((2 ** 19, 2), generator=g).half(), "grad.small": torch.rand((64, 3), generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name in arrays:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= bench.DUMP_BUDGET_BYTES
    assert np.load(tmp_path / "a" / "grad.small.npy").dtype == np.float64
    assert np.load(tmp_path / "a" / "grad.small.npy").shape == (64, 3) and np.load(tmp_path / "a" / "loss.npy").shape == ()
    assert np.array_equal(np.load(tmp_path / "a" / "rgb.npy"), arrays["rgb"].numpy())      # the step's output comes first
    for name in ("grad.also_big", "grad.big"):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        flat = arrays[name].reshape(-1)
        assert got.ndim == 1 and 0.4 * flat.numel() < got.size < 0.6 * flat.numel(), (name, got.size)
        pos = bench.dump_positions(flat.numel(), got.size)
        assert np.array_equal(got, flat[torch.from_numpy(pos)].float().numpy()), name
    bench.dump_outputs(str(tmp_path / "c"), {"grad.big": arrays["grad.big"]})       # one array that fits: written whole, in its shape
    assert np.array_equal(np.load(tmp_path / "c" / "grad.big.npy"), arrays["grad.big"].float().numpy())
