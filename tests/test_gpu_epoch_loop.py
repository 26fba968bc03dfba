"""GPU: the epoch loop on the device (csrc/epoch.hip, train.fit).  gngf_epoch_tail against the runs of the reference's own
loop recorded in tests/golden/G20_epoch_loop.npz and against the host restatement train.replay_epoch_decisions (held to the
same runs on the CPU, tests/test_epoch_loop_cpu.py); gngf_snapshot_if byte for byte with guard words; train.fit end to end
at the smallest shapes, every check made within one run (training is not reproducible from run to run: float atomics)."""
import os

import numpy as np
import pytest
import torch

from test_epoch_loop_cpu import G20, loop_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", G20 + ".npz")
LOOP_NAMES = [str(n) for n in np.load(GOLDEN_FILE, allow_pickle=False)["loop_names"]]


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _device_state(train, limit):
    return train.epoch_state_tensor(limit, DEV)


def _host_state(train, state):
    return state.cpu().numpy().view(train.EPOCH_STATE)[0]


def _run_tail(train, ops, *, epochs, tolerance, min_delta, should_reset, limit, losses, mses, sums, used, nverts, hash_source,
              kls=None, colls=None, calls=None):
    """feeds gngf_epoch_tail epoch by epoch (losses: (E, nb) fp32); returns the per-call (take, last, finished), both logs
    and the state after every call"""
    L = len(nverts)
    Kc = 0 if used is None else used.shape[1]
    state = _device_state(train, limit)
    logf = torch.full((epochs, 2 + 2 * L), -7.0, dtype=torch.float64, device=DEV)
    logi = torch.full((epochs, 6 + Kc * L), -7, dtype=torch.int64, device=DEV)
    nv = _t(nverts, torch.int64)
    flags, states, logs = [], [], []
    for e in range(len(losses) if calls is None else calls):
        i = min(e, len(losses) - 1)                        # calls past the planted epochs repeat the last inputs
        ops.epoch_tail(state, logf, logi, _t(losses[i], torch.float32), _t(mses[i], torch.float32),
                       None if kls is None else _t(kls[i], torch.float32), None if colls is None else _t(colls[i], torch.float32),
                       _t(sums[i], torch.int64), None if used is None else _t(used[i], torch.int32), nv, hash_source=hash_source,
                       tolerance=tolerance, min_delta=min_delta, should_reset=should_reset, epochs=epochs)
        st = _host_state(train, state)
        flags.append((int(st["take"]), int(st["last"]), int(st["finished"])))
        states.append(st.copy())
        logs.append((logf.cpu().numpy(), logi.cpu().numpy()))
    return flags, states, logs


@pytest.mark.parametrize("name", LOOP_NAMES)
def test_epoch_tail_equals_the_reference_loop(golden, name):
    from collision_handling_in_instantngp_amd import ops, train
    c = loop_case(golden(G20), name)
    run, epochs = int(c["epochs_run"]), int(c["epochs"])
    extra = 3
    E = len(c["losses"])
    flags, states, logs = _run_tail(
        train, ops, epochs=epochs, tolerance=int(c["tolerance"]), min_delta=float(c["min_delta"]), should_reset=True,
        limit=c["sse_limit"], losses=c["losses"].astype(np.float32).reshape(E, 1), mses=c["losses"].astype(np.float32).reshape(E, 1),
        sums=np.stack([c["eq"], c["sse"]], 1), used=c["used"][:, None, :], nverts=c["nverts"], hash_source=True, calls=run + extra)
    with np.errstate(invalid="ignore"):
        host = train.replay_epoch_decisions(c["losses"], c["sse"], c["zeros"], epochs=epochs, tolerance=int(c["tolerance"]),
                                            min_delta=float(c["min_delta"]), sse_limit=c["sse_limit"])
    saved = c["saved_epochs"].tolist()
    print(f"{name}: take/last/finished per call {flags}; golden saved {saved}, run {run}, reason {str(c['stop_reason'])}")
    # flags, call by call: take at the golden's saving epochs, last and finished at the golden's last epoch, nothing afterwards
    for e in range(run + extra):
        assert flags[e] == (int(e in saved and e < run), int(e == run - 1), int(e >= run - 1)), (name, e, flags[e])
    st = states[run - 1]
    assert int(st["last_epoch"]) == run - 1 and int(st["epoch"]) == run
    assert train.STOP_REASONS[int(st["reason"])] == str(c["stop_reason"]) == host["stop_reason"]
    assert int(st["best_epoch"]) == (saved[-1] if saved else -1) == host["best_epoch"]
    # the log: rows [0, run) hold the epochs, the rows behind them were never written
    logf, logi = logs[run - 1]
    assert np.array_equal(logf[:run, 0], c["losses"][:run], equal_nan=True) and np.array_equal(logf[:run, 1], c["losses"][:run], equal_nan=True)
    assert np.isnan(logf[:run, 2:]).all()                                  # no kls / colls were given
    assert np.array_equal(logi[:run, 0], c["eq"][:run]) and np.array_equal(logi[:run, 1], c["sse"][:run])
    assert logi[:run, 2].tolist() == host["counter"]
    assert logi[:run, 3].astype(bool).tolist() == host["saved"] == [e in saved for e in range(run)]
    assert logi[:run, 4].astype(bool).tolist() == host["fired"]
    assert logi[:run, 5].astype(bool).tolist() == host["zero_stop"]
    assert np.array_equal(logi[:run, 6:], c["used"][:run])
    assert (logf[run:] == -7.0).all() and (logi[run:] == -7).all()
    # the calls after the last epoch change nothing but take = last = 0
    for e in range(run, run + extra):
        assert np.array_equal(logs[e][0], logf, equal_nan=True) and np.array_equal(logs[e][1], logi)
        a, b = states[e].copy(), st.copy()
        a["take"] = a["last"] = b["take"] = b["last"] = 0
        assert a.tobytes() == b.tobytes(), (name, e)


ES_NAMES = [str(n) for n in np.load(GOLDEN_FILE, allow_pickle=False)["es_names"]]


@pytest.mark.parametrize("name", ES_NAMES)
def test_epoch_tail_stopper_equals_the_reference_traces(golden, name):
    """the stopper inside the kernel, call by call, against the traces of the reference's class — should_reset=False, NaN and
    inf included (the reference's loop only ever builds the default stopper).  Epoch 0 is not shown to the stopper, so call
    i of the trace is epoch i + 1; the trace is followed up to the call that fires (one epoch later the run ends)."""
    from collision_handling_in_instantngp_amd import ops, train
    g = golden(G20)
    t = {k: g[f"es/{name}/{k}"] for k in ("tolerance", "min_delta", "should_reset", "losses", "counter", "best_loss", "early_stop")}
    fired = np.flatnonzero(t["early_stop"])
    ncalls = int(fired[0]) + 1 if fired.size else len(t["losses"])
    losses = np.concatenate([[123.0], t["losses"][:ncalls]]).astype(np.float32).reshape(-1, 1)
    assert np.array_equal(losses[1:, 0].astype(np.float64), t["losses"][:ncalls], equal_nan=True)      # planted as fp32 values
    E = len(losses)
    sums = np.stack([np.zeros(E, np.int64), np.full(E, 5, np.int64)], 1)
    _flags, states, logs = _run_tail(train, ops, epochs=100, tolerance=int(t["tolerance"]), min_delta=float(t["min_delta"]),
                                     should_reset=bool(t["should_reset"]), limit=10 ** 6, losses=losses, mses=losses, sums=sums, used=None,
                                     nverts=np.array([81, 289]), hash_source=False)
    assert int(states[0]["counter"]) == 0 and np.isinf(states[0]["best_loss"]) and int(states[0]["stop"]) == 0
    for i in range(ncalls):
        st = states[i + 1]
        want = t["best_loss"][i]
        assert int(st["counter"]) == int(t["counter"][i]), (name, i)
        assert int(st["stop"]) == int(t["early_stop"][i]), (name, i)
        assert (np.isnan(st["best_loss"]) and np.isnan(want)) or st["best_loss"] == want, (name, i, st["best_loss"], want)
    logi = logs[-1][1]
    assert logi[1:E, 2].tolist() == t["counter"][:ncalls].tolist() and logi[1:E, 4].astype(bool).tolist() == t["early_stop"][:ncalls].tolist()
    assert int(states[-1]["finished"]) == 0                                # the break comes an epoch after the stopper fired


def test_epoch_tail_means_are_numpy_means_bit_for_bit():
    from collision_handling_in_instantngp_amd import ops, train
    rng = np.random.default_rng(11)
    E, nb, L = 6, 3, 5
    # (big, -big, small): the in-order sum keeps `small`, any other order rounds it to big's grid
    big = (3e9 * (1 + rng.random(E))).astype(np.float32)
    losses = np.stack([big, -big, rng.random(E).astype(np.float32)], 1)
    mses = rng.random((E, nb)).astype(np.float32)
    bigk = (1e9 * (1 + rng.random((E, L)))).astype(np.float32)
    kls = np.stack([bigk, -bigk, rng.standard_normal((E, L)).astype(np.float32)], 1)
    colls = rng.random((E, nb, L)).astype(np.float32)
    sums = np.stack([np.arange(E), 1000 - np.arange(E)], 1)
    _flags, _states, logs = _run_tail(train, ops, epochs=E, tolerance=99, min_delta=0.0, should_reset=True, limit=10 ** 6, losses=losses,
                                      mses=mses, sums=sums, used=None, nverts=np.arange(1, L + 1), hash_source=False, kls=kls, colls=colls)
    logf = logs[-1][0]
    for e in range(E):
        want = np.concatenate([[np.mean(losses[e].astype(np.float64)), np.mean(mses[e].astype(np.float64))],
                               np.mean(kls[e].astype(np.float64), axis=0), np.mean(colls[e].astype(np.float64), axis=0)])
        assert logf[e].tobytes() == want.tobytes(), (e, logf[e], want)
    different = sum(np.mean(losses[e].astype(np.float64)) != np.mean(losses[e][::-1].astype(np.float64)) for e in range(E))
    assert different > 0                                                   # (the order of the sum is visible in these inputs)


@pytest.mark.parametrize("broken_at", [None, 4])
def test_epoch_tail_zero_collision_rule_gngf_form(broken_at):
    """K = 4 ranks with mixed-sign nverts - used at the last two levels: free of collisions iff the sum over the ranks is <= 0"""
    from collision_handling_in_instantngp_amd import ops, train
    nverts = np.array([81, 289, 625, 1089], dtype=np.int64)
    E, K = 13, 4
    rng = np.random.default_rng(5)
    used = np.tile(nverts, (E, K, 1)).astype(np.int64)
    used[:, :, :2] -= rng.integers(1, 50, size=(E, K, 2))                  # the first levels collide: they do not count
    for e in range(E):
        d = rng.integers(-3, 4, size=(K, 2))
        d[0] -= d.sum(0) + rng.integers(0, 2, size=2)                      # nverts - used sums to 0 or -1 over the ranks
        used[e, :, 2:] -= d
    assert (np.abs(nverts[None, None, 2:] - used[:, :, 2:]).max(1) > 0).all()         # no rank-wise zeros: signs are mixed
    if broken_at is not None:
        used[broken_at, 1, 3] -= 2                                         # sums to +1 or +2 in that epoch
    zeros = [train.levels_free_of_collisions(u, nverts, False) for u in used]
    assert all(zeros) == (broken_at is None)
    losses = np.linspace(1.0, 0.5, E).astype(np.float32).reshape(E, 1)
    sums = np.stack([np.zeros(E, np.int64), 500 - np.arange(E)], 1)
    flags, states, logs = _run_tail(train, ops, epochs=E, tolerance=99, min_delta=1e-4, should_reset=True, limit=10 ** 6, losses=losses,
                                    mses=losses, sums=sums, used=used.astype(np.int32), nverts=nverts, hash_source=False)
    host = train.replay_epoch_decisions(losses[:, 0].astype(np.float64), sums[:, 1], zeros, epochs=E, tolerance=99, min_delta=1e-4,
                                        sse_limit=10 ** 6)
    run = host["epochs_run"]
    assert run == (11 if broken_at is None else E)
    st = states[run - 1]
    assert train.STOP_REASONS[int(st["reason"])] == host["stop_reason"] == ("zero_collisions" if broken_at is None else "epochs")
    assert int(st["last_epoch"]) == run - 1 and flags[run - 1][1:] == (1, 1)
    logi = logs[-1][1]
    assert logi[:run, 5].astype(bool).tolist() == host["zero_stop"]
    assert np.array_equal(logi[:run, 6:].reshape(run, K, 4), used[:run])


# ------------------------------------------------------------------------------------------------ gngf_snapshot_if
def _snapshot_cases(block):
    sizes = [1, 3, 4, 5, 15, 16, 17]
    out = []
    for dtype, item in ((torch.float32, 4), (torch.float16, 2), (torch.int64, 8)):
        per_block = block // item
        for n in sizes + [per_block - 1, per_block, per_block + 1, 2 ** 20 + 3]:
            for src_off, dst_off in ((0, 0), (4, 4), (4, 0), (0, 4)):
                out.append((dtype, n * item, src_off, dst_off))
    return out


def test_snapshot_if_copies_exactly_its_bytes_or_nothing():
    from collision_handling_in_instantngp_amd import _lib, ops, train
    block = _lib.query("gngf_snapshot_block_bytes")
    cases = _snapshot_cases(block)
    GUARD = 64

    def layout(offsets):
        pos, at = GUARD, []
        for nbytes, off in offsets:
            pos = -(-pos // 16) * 16 + off               # 16-byte aligned, or 4 bytes past it
            at.append(pos)
            pos += nbytes + GUARD
        return at, pos + 16
    src_at, src_size = layout([(nb, so) for _d, nb, so, _do in cases])
    dst_at, dst_size = layout([(nb, do) for _d, nb, _so, do in cases])
    g = torch.Generator(device=DEV).manual_seed(7)
    src = torch.randint(0, 256, (src_size,), dtype=torch.uint8, device=DEV, generator=g)
    before = torch.randint(0, 256, (dst_size,), dtype=torch.uint8, device=DEV, generator=g)
    dst = before.clone()
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    pairs = [(src.data_ptr() + s, dst.data_ptr() + d, nb) for (_t_, nb, _so, _do), s, d in zip(cases, src_at, dst_at)]
    pairs.insert(5, (src.data_ptr(), dst.data_ptr(), 0))                  # an empty tensor among them: left out by the packer
    for (s, d, nb), (_t_, _nb, so, do) in zip([p for p in pairs if p[2]], cases):
        assert s % 16 == so and d % 16 == do and s + nb <= src.data_ptr() + src_size and d + nb <= dst.data_ptr() + dst_size
    raw, nrec, blocks = train.DeviceSnapshot.pack_records(pairs, block)
    assert nrec == len(cases)
    table = torch.from_numpy(raw.copy()).to(DEV)
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ops.snapshot_if(table, nrec, blocks, flag)
    assert torch.equal(dst, before)                                        # flag 0: destination and guards untouched
    want = before.clone()
    for (_t_, nb, _so, _do), s, d in zip(cases, src_at, dst_at):
        want[d:d + nb] = src[s:s + nb]
    assert not torch.equal(want, before)
    flag.fill_(1)
    ops.snapshot_if(table, nrec, blocks, flag)
    bad = (dst != want).nonzero()
    assert bad.numel() == 0, f"first differing byte at {int(bad[0])} of {dst_size}"
    # typed views of three of the copies, as a caller sees them
    for i in (0, len(cases) // 2, len(cases) - 4):
        dtype, nb, so, do = cases[i]
        if so % dtype.itemsize or do % dtype.itemsize:
            continue
        a = src[src_at[i]:src_at[i] + nb].view(dtype)
        b = dst[dst_at[i]:dst_at[i] + nb].view(dtype)
        assert a.view(torch.uint8).equal(b.view(torch.uint8))


def test_device_snapshot_take_if_and_restore():
    from collision_handling_in_instantngp_amd import train
    g = torch.Generator(device=DEV).manual_seed(3)
    step = torch.full((), 5.0, device=DEV)
    live = {"a": torch.rand((257, 3), device=DEV, generator=g), "h": torch.rand((33,), device=DEV, generator=g).half(),
            "n": torch.arange(7, device=DEV), "empty": torch.zeros((0, 4), device=DEV), "step0": step, "step1": step}
    snap = train.DeviceSnapshot(live)
    first = {k: v.clone() for k, v in live.items()}
    assert snap.tensors()["step0"] is snap.tensors()["step1"]             # shared memory, one shadow
    assert snap.bytes == 257 * 3 * 4 + 33 * 2 + 7 * 8 + 4
    flag = torch.ones((1,), dtype=torch.int32, device=DEV)
    snap.take_if(flag)
    for k, v in live.items():
        v.add_(1)
    flag.zero_()
    snap.take_if(flag)                                                     # not taken: the shadows keep the first state
    for k in live:
        assert torch.equal(snap.tensors()[k], first[k]) and snap.tensors()[k].dtype == live[k].dtype, k
    snap.restore()
    for k in live:
        assert torch.equal(live[k], first[k]), k
    with pytest.raises(ValueError, match="FusedAdam"):
        train.DeviceSnapshot({"step": torch.tensor(3.0)})


# ------------------------------------------------------------------------------------------------ train.fit, end to end
W_, H_ = 24, 20


def _problem():
    from collision_handling_in_instantngp_amd import data
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(H_, W_, 3)).astype(np.uint8)
    X = data.normalise_coordinates(torch.from_numpy(data.pixel_grid(H_, W_)).float(), W_, H_).to(DEV)
    Y = torch.tensor(img.reshape(-1, 3) / 255).float().to(DEV)
    shuffled, _ = data.make_permutation(H_ * W_, torch.Generator().manual_seed(4))
    return img, X, Y, shuffled


def _model(source):
    """L = 4, T = 2^8, F = 2, n 8..32 (K = 4); hash / frozen GNGF: the forward passes track their slots (no index tensor);
    learning GNGF: the model's defaults (index tensor returned, dense distribution)"""
    from collision_handling_in_instantngp_amd import models, train
    models.should_use_hash_function = source == "hash"
    torch.manual_seed(6)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=256, num_levels=4, n_min=8, n_max=32,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=256, feature_dim=2, topk_k=4)
    if source != "gngf_learning":
        net.return_indices = False
        net.dense_probs = False
    if source == "gngf_frozen":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
    return net, train.Loss(delta=1, gamma=-2, epsilon=1), train.get_optimizer(net, 1e-3, 1e-3, 1e-3, 0, 1e-6, 1e-6)


EPOCHS, TOLERANCE, MIN_DELTA = 40, 6, 1.0      # a falling loss moves by less than min_delta: a stall at every call, stop in epoch 7


@pytest.mark.parametrize("source,batch_percentage,poll_every", [
    ("hash", 1.0, 7), ("hash", 1 / 3, 7), ("hash", 1 / 3, 1), ("gngf_frozen", 1.0, 7), ("gngf_frozen", 1 / 3, 7),
    ("gngf_learning", 1.0, 7), ("gngf_learning", 1 / 3, 7), ("gngf_learning", 1.0, 1)])
def test_fit_end_to_end(source, batch_percentage, poll_every, monkeypatch, tmp_path):
    from collision_handling_in_instantngp_amd import data, models, train
    img, X, Y, shuffled = _problem()
    made = []

    class Recording(train.EpochImage):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(train, "EpochImage", Recording)
    try:
        net, loss_fn, opt = _model(source)
        clones, seen = [], []

        def after_epoch(e):
            clones.append({k: v.clone() for k, v in train.state_tensors(net, opt).items()})
            seen.append((made[0].psnr(), made[0].accuracy()))

        res = train.fit(net, loss_fn, opt, X, Y, W_, H_, img, epochs=EPOCHS, tolerance=TOLERANCE, min_delta=MIN_DELTA, l_mse=1, l_js_kl=1,
                        l_collisions=1e-3, batch_percentage=batch_percentage, should_shuffle=True, shuffled_indices=shuffled, graph=True,
                        poll_every=poll_every, after_epoch=after_epoch)
        log = res.log
        n = res.last_epoch + 1
        print(f"{source} bp {batch_percentage:.3f} poll {poll_every}: issued {res.issued}, last {res.last_epoch}, best {res.best_epoch}, "
              f"{res.stop_reason}, restored {res.restored}; loss {log['loss'].tolist()}; sse {log['sse'].tolist()}; "
              f"counter {log['counter'].tolist()}; used[-1] {log['used'][-1].tolist()}; snapshot {res.best.bytes} bytes")
        assert len(made) == 1 and len(clones) == res.issued and all(len(v) == n for v in log.values())
        assert res.issued == min(EPOCHS, -(-n // poll_every) * poll_every)
        # the logged sequence, replayed through the host restatement of the reference's loop, gives the same decisions
        L = 4
        nverts = net._level_vertex_counts()
        zeros = [train.levels_free_of_collisions(u, nverts, source == "hash") for u in log["used"]]
        assert log["used"].shape == (n, 1 if source == "hash" else 4, L) and (log["used"] > 0).all()
        host = train.replay_epoch_decisions(log["loss"], log["sse"], zeros, epochs=EPOCHS, tolerance=TOLERANCE, min_delta=MIN_DELTA,
                                            sse_limit=train.sse_limit0(img.size, made[0].peak_term))
        assert (host["last_epoch"], host["best_epoch"], host["stop_reason"]) == (res.last_epoch, res.best_epoch, res.stop_reason)
        assert host["saved"] == log["saved"].tolist() and host["fired"] == log["stopper_fired"].tolist()
        assert host["zero_stop"] == log["zero_stop"].tolist() and host["counter"] == log["counter"].tolist()
        # this run stops early, by the stopper, and poll_every = 7 has issued epochs past the last one
        assert res.stop_reason == "early_stopping" and res.last_epoch < EPOCHS - 1 and res.best_epoch >= 0
        assert res.restored == (res.issued > n) and (poll_every == 1) == (res.issued == n)
        # the state: best is the state after best_epoch, the live state the one after last_epoch, bit for bit
        held = res.best.tensors()
        assert set(held) == set(clones[0]) and any(k.endswith(".exp_avg") for k in held) and any(k.endswith(".step") for k in held)
        for k, v in held.items():
            assert torch.equal(v, clones[res.best_epoch][k]), k
        live = train.state_tensors(net, opt)
        for k, v in live.items():
            assert torch.equal(v, clones[res.last_epoch][k]), k
        if res.issued > n:
            assert any(not torch.equal(clones[res.issued - 1][k], clones[res.last_epoch][k]) for k in live)      # the extra epochs did train
        assert float(live["optimizer.0.step"]) == n * int(np.ceil(1 / batch_percentage))
        # psnr and accuracy as EpochImage gives them
        assert [p for p, _a in seen[:n]] == log["psnr"].tolist() and [a for _p, a in seen[:n]] == log["accuracy"].tolist()
        if source == "hash":
            assert np.array_equal(log["mse"], log["loss"])                 # l_mse = 1 and no other term
        assert np.isnan(log["kls"]).all() == (source != "gngf_learning")
        # the five checkpoint files from the snapshot load into a fresh model and optimizer
        folder = str(tmp_path / "best")
        paths = data.save_snapshot(res.best, net, opt, folder)
        assert sorted(os.path.basename(p) for p in paths.values()) == sorted(data.CHECKPOINT_FILES.values())
        net2, _loss2, opt2 = _model(source)
        data.load_checkpoint(net2, folder, optimizer=opt2, parts=("model",))
        for k, v in net2.state_dict().items():
            assert torch.equal(v, held[f"model.{k}"]), k
        loaded = opt2.state_dict()["state"]
        wanted = {k: v for k, v in held.items() if k.startswith("optimizer.")}
        assert len(wanted) == sum(len([x for x in st.values() if torch.is_tensor(x)]) for st in loaded.values())
        for i, st in loaded.items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    assert torch.equal(v.to(DEV), wanted[f"optimizer.{i}.{k}"]), (i, k)
        net3, _l3, _o3 = _model(source)
        data.load_checkpoint(net3, folder, parts=("encoding", "mlp") + (() if source == "hash" else ("HPD",)))
        for k, v in net3.encoding.state_dict().items():
            assert torch.equal(v, held[f"model.encoding.{k}"]), k
    finally:
        models.should_use_hash_function = False


def test_fit_refuses_a_data_parallel_model():
    from collision_handling_in_instantngp_amd import models, train
    img, X, Y, shuffled = _problem()
    try:
        net, loss_fn, opt = _model("hash")
        net.dp.world = 2
        with pytest.raises(ValueError, match="one process"):
            train.fit(net, loss_fn, opt, X, Y, W_, H_, img, epochs=3, tolerance=2, min_delta=1e-4, l_mse=1, l_js_kl=1, l_collisions=1e-3,
                      shuffled_indices=shuffled)
    finally:
        models.should_use_hash_function = False
