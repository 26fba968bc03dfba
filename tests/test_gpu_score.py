"""GPU: train.score / ops.render_score / gngf_ext2_render_score — the model scored against its uint8 image in one render launch
that writes no picture — and train.fit_sampled, the epoch loop on sampled batches built on it.

Every comparison is on integers and exact.  The reference is the two-call way of the parent: render(net, h, w, denom, image=True)
(gngf_render, held to the oracle by tests/test_gpu_render.py) and ops.image_metrics (gngf_image_metrics, held by
tests/test_gpu_epoch_image.py), and the same two sums formed in numpy from that rendered image.

Set-up of every case: parameters from test_gpu_render.render_params (tables uniform in [-1, 1): the picture varies); the target
is the model's own rendered image clipped to 0..255 with a fixed pseudo-random perturbation in {-2..2} on about half the
elements, clipped again — so 0 < eq < n by construction, which every case asserts."""
import numpy as np
import pytest
import torch

import guarded
import test_gpu_render as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"

ENTRY = "gngf_ext2_render_score"
INVALID = 1          # hipErrorInvalidValue


def entry_points():
    """the entry points of include/gngf_ext2.h with a guard-band case here (tests/test_ext2_abi_cpu.py keeps the ledger)"""
    return [ENTRY]


MODELS = {
    "hash-L16F2": tr.cfg(tr.FIRST, "hash", 4096),                        # exact 32-feature form
    "hash-L4F2": tr.cfg(tr.NARROW, "hash", 4096),                        # narrower form
    "hash-L16F4": tr.cfg(tr.WIDE, "hash", 4096),                         # 64-feature form
    "hash-L10F4": tr.cfg(dict(L=10, F=4, n_min=8, n_max=64), "hash", 4096),   # narrower 64-feature form
    "hash-fp16": tr.cfg(tr.FIRST, "hash", 4096, fp16=True),
    "hash-leaky": tr.cfg(tr.FIRST, "hash", 4096, leaky=True),
    "gngf-frozen-K4": tr.cfg(tr.FIRST, "gngf", 256, K=4),
    "gngf-frozen-K1": tr.cfg(tr.NARROW, "gngf", 256, K=1),
    "gngf-trainable": tr.cfg(tr.FIRST, "gngf", 256, K=4),
    "dense-levels": tr.cfg(tr.NARROW, "hash", 512),                      # (N_l + 2)^2 <= 512: three dense levels, one hashed
    "hash-bw": tr.cfg(tr.FIRST, "hash", 4096, bw=True),                  # C = 1
    "hash-C4": tr.cfg(tr.FIRST, "hash", 4096),                           # C = 4: the last layer replaced below
    "gngf-bw": tr.cfg(tr.FIRST, "gngf", 256, K=4, bw=True),              # C = 1 / C = 4 through the vertex-table source ...
    "gngf-C4": tr.cfg(tr.FIRST, "gngf", 256, K=4),
    "wide-bw": tr.cfg(tr.WIDE, "hash", 4096, bw=True),                   # ... and through the 64-feature form
    "wide-C4": tr.cfg(tr.WIDE, "hash", 4096),
}
SINGLE_LINE_ONLY = ("hash-bw", "hash-C4", "gngf-bw", "gngf-C4", "wide-bw", "wide-C4")
SHAPES_ALL = [(19, 21)]
SHAPES_FEW = [(8, 16), (200, 300)]
FEW = ["hash-L16F2", "gngf-frozen-K4", "hash-L16F4"]


def build(name):
    """(net on the device, its configuration); call inside tr.switches(MODELS[name])"""
    from collision_handling_in_instantngp_amd import models
    c = MODELS[name]
    if name == "dense-levels":
        p = tr.render_params(c)
        net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=c["T"], num_levels=c["L"], n_min=c["n_min"],
                                              n_max=c["n_max"], MLP_hidden_layers_widths=[64, 64],
                                              HPD_hidden_layers_widths=[32, 64, 128], HPD_out_features=c["T"], feature_dim=c["F"],
                                              topk_k=c["K"], dense_levels=True)
        sd = net.state_dict()
        new = {f"encoding._hash_tables.{l}.weight": p["tables"][l] for l in range(c["L"])}
        for i in range(3):
            new[f"mlp.{i}.0.weight"], new[f"mlp.{i}.0.bias"] = p["dec_w"][i], p["dec_b"][i]
        net.load_state_dict({k: (torch.from_numpy(new[k]).to(v.dtype) if k in new else v) for k, v in sd.items()})
    else:
        net = tr.build_net(c, freeze_hpd=name != "gngf-trainable")
    if name.endswith("-C4"):
        rng = np.random.default_rng(44)
        last = torch.nn.Linear(64, 4)
        with torch.no_grad():
            last.weight.copy_(torch.from_numpy(rng.uniform(-0.125, 0.125, (4, 64)).astype(np.float32)))
            last.bias.copy_(torch.from_numpy(rng.uniform(-0.125, 0.125, (4,)).astype(np.float32)))
        net.mlp[-1][0] = last
    return net.to(DEV), c


def perturbed(rendered, seed=5):
    """the target of a case from the parent's rendered int32 image (numpy): uint8, about half the elements moved by -2..2"""
    rng = np.random.default_rng(seed)
    base = np.clip(rendered, 0, 255).astype(np.int64)
    delta = rng.integers(-2, 3, size=base.shape) * (rng.random(base.shape) < 0.5)
    return np.clip(base + delta, 0, 255).astype(np.uint8)


def numpy_sums(rendered, img):
    d = rendered.astype(np.int64) - img.astype(np.int64)
    return np.array([int((d == 0).sum()), int((d * d).sum())], dtype=np.int64)


def two_call_way(net, h, w, denom, C):
    """(rendered int32 numpy (h,w,C), the uint8 target numpy (h,w,C)) — the parent's render, once per case"""
    from collision_handling_in_instantngp_amd import train
    rendered = train.render(net, h, w, denom, rgb=False, image=True)
    torch.cuda.synchronize()
    r = rendered.cpu().numpy().reshape(h, w, C)
    return rendered, r, perturbed(r)


def check_equal_to_two_calls(net, h, w, C, denom=None):
    from collision_handling_in_instantngp_amd import ops, train
    dn = denom if denom is not None else max(h, w) - 1
    rendered, r, img = two_call_way(net, h, w, dn, C)
    n = h * w * C
    want = numpy_sums(r, img)
    assert 0 < want[0] < n, (want, n)
    target = torch.from_numpy(img).to(DEV)
    metrics = ops.image_metrics(rendered, target.reshape(-1), torch.zeros((2,), dtype=torch.int64, device=DEV),
                                ops.image_metrics_workspace(n, DEV))
    got = train.score(net, target if C != 1 else target.reshape(h, w), step=1, denom=denom)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.shape == (2,) and got.is_cuda
    assert np.array_equal(metrics.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 1. equality with the two-call way
@pytest.mark.parametrize("name", [m for m in MODELS if m not in SINGLE_LINE_ONLY])
def test_score_equals_render_then_metrics_every_model(name):
    """19 x 21 x 3 (ragged in both block dimensions), every form the render kernel has"""
    c = MODELS[name]
    with tr.switches(c):
        net, _ = build(name)
        for h, w in SHAPES_ALL:
            check_equal_to_two_calls(net, h, w, 3)


@pytest.mark.parametrize("shape", SHAPES_FEW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FEW)
def test_score_equals_render_then_metrics_other_shapes(name, shape):
    """8 x 16: exactly one block; 200 x 300: 469 blocks over 256 workgroups — some walk two blocks, the last trip is ragged"""
    c = MODELS[name]
    with tr.switches(c):
        net, _ = build(name)
        check_equal_to_two_calls(net, shape[0], shape[1], 3)


@pytest.mark.parametrize("name,h,w,C,denom", [("hash-L16F2", 1, 1, 3, 7.0), ("gngf-frozen-K4", 1, 1, 3, 7.0),
                                              ("hash-L16F4", 1, 1, 3, 7.0),
                                              ("hash-bw", 1, 40, 1, None), ("hash-C4", 40, 1, 4, None),
                                              ("gngf-bw", 1, 40, 1, None), ("gngf-C4", 40, 1, 4, None),
                                              ("wide-bw", 1, 40, 1, None), ("wide-C4", 40, 1, 4, None)],
                         ids=["1x1x3-hash", "1x1x3-gngf", "1x1x3-wide", "1x40x1-hash", "40x1x4-hash", "1x40x1-gngf", "40x1x4-gngf",
                              "1x40x1-wide", "40x1x4-wide"])
def test_score_smallest_and_single_line_images(name, h, w, C, denom):
    """the smallest image, a single row (C = 1) and a single column (C = 4): each through the exact hash form, a vertex-table form
    and a 64-feature form — one column or one row of a block is live, nbx or nby is 1, the texel loop runs 1 or 4 wide"""
    c = MODELS[name]
    with tr.switches(c):
        net, _ = build(name)
        check_equal_to_two_calls(net, h, w, C, denom=denom)


# ------------------------------------------------------------------------------------------------ 2. step
def test_score_on_a_coarser_lattice():
    """37 x 50 x 3, step in {2, 3, 7}: the sums over rendered[::step, ::step] against img[::step, ::step]; a step past both sides
    scores pixel (0, 0) alone.  The full render uses the same denom, so the strided pixels carry the same coordinates."""
    from collision_handling_in_instantngp_amd import train
    h, w, C = 37, 50, 3
    for name in ("hash-L16F2", "gngf-frozen-K4"):
        c = MODELS[name]
        with tr.switches(c):
            net, _ = build(name)
            _rendered, r, img = two_call_way(net, h, w, max(h, w) - 1, C)
            target = torch.from_numpy(img).to(DEV)
            for step in (1, 2, 3, 7, 50, 51, 1 << 40):
                want = numpy_sums(r[::step, ::step], img[::step, ::step])
                n = train.scored_elements(h, w, C, step)
                assert n == r[::step, ::step].size
                if step <= 7:
                    assert 0 < want[0] < n
                got = train.score(net, target, step=step).cpu().numpy()
                assert np.array_equal(got, want), (name, step, got, want)


# ------------------------------------------------------------------------------------------------ 3. guard band
def raw_model(name):
    """the arguments of ops.render_score for a model: (tables, n_ls, decoder parameters, keywords)"""
    from collision_handling_in_instantngp_amd import train
    net, c = build(name)
    (tables, n_ls, dec), kw = train._forward_model(net, net.encoding.packed_tables())
    return net, tables, n_ls, dec, kw


@pytest.mark.parametrize("name", ["hash-L16F2", "gngf-frozen-K4", "hash-L16F4"])
def test_render_score_guarded(name):
    """image at misalignments 0, 1 and 3 bytes, sums 8-byte but not 16-byte aligned, a workspace larger than the size query:
    stores stay inside sums and the queried words of the workspace; sums is fully written; the words beyond are unwritten"""
    from collision_handling_in_instantngp_amd import _lib, ops, train
    c = MODELS[name]
    words = _lib.query("gngf_ext2_render_score_workspace_words")
    extra = 64
    with tr.switches(c):
        net, tables, n_ls, dec, kw = raw_model(name)
        for (h, w), step in (((19, 21), 1), ((200, 300), 1), ((37, 50), 3)):
            denom = float(max(h, w) - 1)
            _rendered, r, img = two_call_way(net, h, w, denom, 3)
            want = numpy_sums(r[::step, ::step], img[::step, ::step])
            for misalign in (0, 1, 3):
                arena = guarded.Arena(img.size + 8 * (words + extra) + 16 + 8 * guarded.PAD, device=DEV)
                image = arena.put(img, name="image", misalign=misalign)
                sums = arena.take((2,), torch.int64, misalign=8, name="sums")
                workspace = arena.take((words + extra,), torch.int64, name="workspace")
                assert image.data_ptr() % 4 == misalign and sums.data_ptr() % 16 == 8
                ops.render_score(tables, n_ls, dec, image, denom=denom, step=step, sums=sums, workspace=workspace, **kw)
                torch.cuda.synchronize()
                arena.check()
                assert not bool(guarded.unwritten(sums).any())
                assert bool(guarded.unwritten(workspace[words:]).all())
                assert np.array_equal(image.cpu().numpy(), img)
                assert np.array_equal(sums.cpu().numpy(), want), (name, h, w, step, misalign)


# ------------------------------------------------------------------------------------------------ 4. rejections
def test_invalid_arguments_are_rejected_before_any_launch():
    """every rejection of include/gngf_ext2.h gives hipErrorInvalidValue and leaves sums as it was"""
    from collision_handling_in_instantngp_amd import _lib
    c = MODELS["gngf-frozen-K4"]
    with tr.switches(c):
        net, tables, n_ls, dec, kw = raw_model("gngf-frozen-K4")
        h, w, C = 19, 21, 3
        image = torch.zeros((h, w, C), dtype=torch.uint8, device=DEV)
        buf = torch.full((4,), -77, dtype=torch.int64, device=DEV)
        ws = torch.empty((_lib.query("gngf_ext2_render_score_workspace_words") + 1,), dtype=torch.int64, device=DEV)
        L, T, F = tables.shape
        NV, K = kw["vert_idx"].shape
        good = dict(tables=tables.data_ptr(), feat_dtype=0, vert_idx=kw["vert_idx"].data_ptr(), vert_w=kw["vert_w"].data_ptr(),
                    n_ls=n_ls.data_ptr(), W0=dec[0].data_ptr(), b0=dec[1].data_ptr(), W1=dec[2].data_ptr(), b1=dec[3].data_ptr(),
                    W2=dec[4].data_ptr(), b2=dec[5].data_ptr(), L=L, F=F, T=T, K=K, mode=1, vstride=kw["vstride"], NV=NV, out_dim=C,
                    leaky=0, image=image.data_ptr(), h=h, w=w, C=C, denom=20.0, step=1, sums=buf.data_ptr(),
                    workspace=ws.data_ptr(), stream=None)
        lib = _lib.load()

        def rc(**change):
            a = dict(good, **change)
            return lib.gngf_ext2_render_score(*[a[k] for k in good])

        bad = [dict(C=4), dict(out_dim=4), dict(out_dim=5, C=5), dict(h=0), dict(w=0), dict(h=(1 << 24) + 1), dict(w=(1 << 24) + 1),
               dict(step=0), dict(step=-3), dict(image=None), dict(sums=None), dict(workspace=None),
               dict(sums=buf.data_ptr() + 4), dict(workspace=ws.data_ptr() + 4), dict(denom=0.0), dict(denom=float("nan")),
               # what gngf_render rejects of the model
               dict(L=0), dict(F=3), dict(L=17, F=4), dict(T=0), dict(mode=3), dict(feat_dtype=2), dict(tables=None),
               dict(tables=tables.data_ptr() + 4), dict(n_ls=None), dict(W0=None), dict(b2=None), dict(vert_idx=None),
               dict(vert_w=None), dict(K=0), dict(K=129), dict(vstride=0), dict(NV=0), dict(NV=(1 << 31) // K + 1)]
        for change in bad:
            assert rc(**change) == INVALID, change
        torch.cuda.synchronize()
        assert bool((buf == -77).all())
        assert rc() == 0                                    # the unchanged arguments are accepted
        torch.cuda.synchronize()
        assert bool((buf[:2] >= 0).all()) and bool((buf[2:] == -77).all())


# ------------------------------------------------------------------------------------------------ 5. capture
def test_captured_score_follows_the_tables():
    """a hash-mode score(..., out=buf) captured once and replayed twice, a table row changed in between: the sums of two eager
    calls.  Captured with the guard of GraphedStep._capture (train._capture_guarded); nothing is allocated inside."""
    from collision_handling_in_instantngp_amd import train
    c = MODELS["hash-L16F2"]
    h, w, C = 19, 21, 3
    with tr.switches(c):
        net, _ = build("hash-L16F2")
        _rendered, r, img = two_call_way(net, h, w, max(h, w) - 1, C)
        target = torch.from_numpy(img).to(DEV)
        buf = torch.zeros((2,), dtype=torch.int64, device=DEV)
        first = train.score(net, target, out=buf).clone()           # eager: the library is loaded, the workspace is cached
        tables = net.encoding.packed_tables()
        saved = tables[:, :64].clone()
        changed = saved * -1.0 + 0.25
        with torch.no_grad():
            tables[:, :64] = changed
        second = train.score(net, target).clone()
        with torch.no_grad():
            tables[:, :64] = saved
        torch.cuda.synchronize()
        assert not torch.equal(first, second)
        assert np.array_equal(first.cpu().numpy(), numpy_sums(r, img))

        def body():
            before = torch.cuda.memory_allocated()
            out = train.score(net, target, out=buf)
            assert torch.cuda.memory_allocated() == before
            return out

        buf.zero_()
        g, out = train._capture_guarded(body)
        torch.cuda.synchronize()
        assert out is buf and bool((buf == 0).all())                # capturing launches nothing
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, first)
        with torch.no_grad():
            tables[:, :64] = changed
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, second)


# ------------------------------------------------------------------------------------------------ 6. fit_sampled
FIT = dict(h=48, w=64, C=3, batch=2048, steps=4, rounds=12, poll=5, seed=21)
LRS = dict(encoding=1e-2, other=1e-3)


def smooth_image(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127.5 + 110 * np.sin(x / 9.0) * np.cos(y / 7.0), 255.0 * x / (w - 1), 255.0 * (y / (h - 1)) ** 2], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def fit_setup(mode):
    from collision_handling_in_instantngp_amd import data, models, train
    torch.manual_seed(7)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=1024 if mode == "hash" else 256, num_levels=4, n_min=8,
                                          n_max=32, MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=1024 if mode == "hash" else 256, feature_dim=2, topk_k=4).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    if mode != "hash":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    opt = train.get_optimizer(net, LRS["encoding"], LRS["other"], LRS["other"], 0.0, 0.0, 1e-6)
    sampler = data.ImageSampler(smooth_image(FIT["h"], FIT["w"]), FIT["batch"], seed=FIT["seed"], continuous=False)
    return net, loss_fn, opt, sampler


# min_delta 1.0: a round whose loss improves on the best by less than 1.0 — every improving round of this task — counts against the
# patience, so tolerance 2 fires after two improving rounds in a row (asserted below); tolerance 1000 cannot fire in 12 rounds
MIN_DELTA = 1.0


def mean_in_order(values):
    """csrc/epoch.hip: the float32 values summed in float64 in order, one division (np.mean of fewer than 8 float64 values)"""
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s / np.float64(len(values))


@pytest.mark.parametrize("mode,graph,tolerance", [("hash", True, 2), ("hash", True, 1000), ("gngf_frozen", True, 1000),
                                                  ("hash", False, 2)],
                         ids=["hash-graph-stops", "hash-graph-runs-out", "gngf-frozen", "hash-eager-stops"])
def test_fit_sampled_decides_as_the_replay(mode, graph, tolerance):
    from collision_handling_in_instantngp_amd import models, train
    f = FIT
    models.should_use_hash_function = mode == "hash"
    try:
        net, loss_fn, opt, sampler = fit_setup(mode)
        steps_seen = []

        def hook(r, rec):
            steps_seen.append((rec["loss"].clone(), rec["mse"].clone()))

        res = train.fit_sampled(net, loss_fn, opt, sampler, rounds=f["rounds"], steps_per_round=f["steps"], tolerance=tolerance,
                                min_delta=MIN_DELTA, l_mse=1, l_js_kl=1, l_collisions=1e-3, graph=graph, poll_every=f["poll"],
                                exact_final=True, after_round=hook)
        torch.cuda.synchronize()
        log = res.log
        n = res.last_epoch + 1
        assert len(log["loss"]) == n and res.issued == len(steps_seen) and res.issued >= n
        # the logged loss / mse of a round: the mean fit() forms of the per-step values
        for r in range(n):
            for key, col in (("loss", 0), ("mse", 1)):
                vals = steps_seen[r][col].cpu().numpy()
                assert vals.dtype == np.float32 and len(vals) == f["steps"]
                assert log[key][r] == mean_in_order(vals) == np.mean(vals.astype(np.float64)), (key, r)
        n_elems = train.scored_elements(f["h"], f["w"], f["C"], 1)
        peak = 20 * np.log10(np.max(smooth_image(f["h"], f["w"])))
        want = train.replay_epoch_decisions(log["loss"], log["sse"], None, epochs=f["rounds"], tolerance=tolerance, min_delta=MIN_DELTA,
                                            should_reset=True, sse_limit=train.sse_limit0(n_elems, peak))
        assert list(log["saved"]) == want["saved"] and list(log["stopper_fired"]) == want["fired"]
        assert list(log["counter"]) == want["counter"] and not log["zero_stop"].any()
        assert (res.last_epoch, res.best_epoch, res.stop_reason) == (want["last_epoch"], want["best_epoch"], want["stop_reason"])
        if tolerance == 2:
            assert res.stop_reason == "early_stopping" and res.last_epoch < f["rounds"] - 1
            # polled every 5 rounds: rounds were issued past the break unless it fell on a poll, and exact_final put the state back
            assert res.restored == (res.issued > n)
            assert res.issued == min(f["rounds"], -(-n // f["poll"]) * f["poll"])
        else:
            assert res.stop_reason == "epochs" and res.last_epoch == f["rounds"] - 1 and not res.restored
        assert 0 < log["eq"][-1] < n_elems and res.best_epoch >= 0
        assert np.array_equal(log["psnr"], [float(train.psnr_from_sums(s, n_elems, peak)) for s in log["sse"]])
        # the live state is last_epoch's
        live = train.score(net, sampler).cpu().numpy()
        assert (live[0], live[1]) == (log["eq"][res.last_epoch], log["sse"][res.last_epoch])
        # and the snapshot best_epoch's
        res.best.restore()
        best = train.score(net, sampler).cpu().numpy()
        assert (best[0], best[1]) == (log["eq"][res.best_epoch], log["sse"][res.best_epoch])
        assert log["sse"][res.best_epoch] == log["sse"][:n].min()
        psnr, acc = train.score_psnr(net, sampler)
        assert psnr == log["psnr"][res.best_epoch] and acc == log["accuracy"][res.best_epoch]
    finally:
        models.should_use_hash_function = False


# ------------------------------------------------------------------------------------------------ 7. Python-side refusals
def test_score_and_fit_sampled_refuse_what_they_cannot_serve():
    from collision_handling_in_instantngp_amd import data, models, train
    models.should_use_hash_function = True
    try:
        net, loss_fn, opt, sampler = fit_setup("hash")
        img3 = sampler.image
        kw = dict(rounds=2, steps_per_round=1, tolerance=5, min_delta=0.0, l_mse=1, l_js_kl=1, l_collisions=1e-3)
        models.should_batchnorm_data = True
        try:
            with pytest.raises(ValueError, match="should_batchnorm_data"):
                train.score(net, img3)
            with pytest.raises(ValueError, match="should_batchnorm_data"):
                train.fit_sampled(net, loss_fn, opt, sampler, **kw)
        finally:
            models.should_batchnorm_data = False
        narrow = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=1024, num_levels=4, n_min=8, n_max=32,
                                                 MLP_hidden_layers_widths=[32, 32], HPD_hidden_layers_widths=[32, 64, 128],
                                                 HPD_out_features=1024, feature_dim=2, topk_k=4).to(DEV)
        nopt = train.get_optimizer(narrow, 1e-2, 1e-3, 1e-3, 0.0, 0.0, 1e-6)
        with pytest.raises(ValueError, match=r"net\(x\)"):
            train.score(narrow, img3)
        with pytest.raises(ValueError, match=r"net\(x\)"):
            train.fit_sampled(narrow, loss_fn, nopt, sampler, **kw)
        gray = data.ImageSampler(smooth_image(48, 64)[:, :, 0], 256, continuous=False)
        with pytest.raises(ValueError, match="channel"):
            train.score(net, gray)
        with pytest.raises(ValueError, match="channel"):
            train.score(net, img3[:, :, 0].contiguous())
        with pytest.raises(ValueError, match="channel"):
            train.fit_sampled(net, loss_fn, opt, gray, **kw)
        with pytest.raises(ValueError, match="step"):
            train.score(net, img3, step=0)
        with pytest.raises(ValueError, match="step"):
            train.fit_sampled(net, loss_fn, opt, sampler, score_step=0, **kw)
        # over the SSE limit at step 1: 9511 x 9511 x 3 elements times 255^2 > 2^44 (the image is never touched: a broadcast view
        # of one row would do, but the sampler wants a contiguous image — 271 MB of zeros)
        side = 9511
        assert side * side * 3 * 255 ** 2 > train.SSE_ORDER_LIMIT
        big = data.ImageSampler(torch.zeros((side, side, 3), dtype=torch.uint8, device=DEV), 256, continuous=False)
        with pytest.raises(ValueError, match="step"):
            train.fit_sampled(net, loss_fn, opt, big, **kw)
        # ... and a coarser lattice is the remedy the message names: the same call is past that check with score_step = 2
        assert train.sse_order_refusal(train.scored_elements(side, side, 3, 2)) is None
        # what train_sampled and fit refuse
        single = data.ImageSampler(smooth_image(48, 64), 256, continuous=False, buffers=1)
        with pytest.raises(ValueError, match="buffers"):
            train.fit_sampled(net, loss_fn, opt, single, **kw)
        with pytest.raises(ValueError, match="at least 1"):
            train.fit_sampled(net, loss_fn, opt, sampler, **dict(kw, rounds=0))
        host_opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        with pytest.raises(ValueError, match="host"):
            train.fit_sampled(net, loss_fn, host_opt, sampler, **kw)
    finally:
        models.should_use_hash_function = False
