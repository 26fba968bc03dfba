"""GPU: the device batch sampler (csrc/sample.hip: gngf_ext_sample_pixels, data.ImageSampler, train.train_sampled) against the
numpy restatement tests/sampler_reference.py.  Every buffer the kernel writes is a view into a tests/guarded.py arena: after each
call the guard bytes are intact, every output element is written and `draw` is the old value plus one.  xy and pixel-mode targets
are bit-identical; continuous targets are within 1e-6 of the float64 bilinear value of the same fp32 position.  The bound is
derived, not observed: fr and fc are exact; a term t w carries at most five roundings (t = texel / 255, 1 - fr, 1 - fc, their
product, t w), each a relative 2^-24, and the terms sum to at most 1; the three additions add 2^-24 each on partial sums in
[0, 1]: 8 * 2^-24 = 4.8e-7 < 1e-6."""
import numpy as np
import pytest
import torch

import guarded
import sampler_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

ENTRY = "gngf_ext_sample_pixels"
BATCHES = [1, 255, 257, 4099]                       # one lane; one short of, one over a workgroup; 17 workgroups, ragged
IMAGES = [(1, 1), (2, 2), (3, 1000), (61, 67)]      # (1, 1): pixel centres only — nothing to interpolate between
CHANNELS = [1, 3, 4]
CASE_TABLE = [(ENTRY, f"{h}x{w}x{C}-{'continuous' if cont else 'pixel'}", dict(h=h, w=w, C=C, continuous=cont))
              for (h, w) in IMAGES for C in CHANNELS for cont in (False, True) if not (cont and min(h, w) < 2)]
CONTINUOUS_ATOL = 1e-6


def entry_points():
    """the entry points of include/gngf_ext.h with a guard-band case here (tests/test_ext_abi_cpu.py keeps the ledger)"""
    return sorted({c[0] for c in CASE_TABLE})


def image_of(h, w, C):
    return np.random.default_rng(1000 * h + 10 * w + C).integers(0, 256, size=(h, w, C), dtype=np.uint8)


def bits_equal(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def check_batch(x, target, want, continuous):
    x, target = x.cpu().numpy(), target.cpu().numpy()
    assert bits_equal(x, want["xy"]), "xy differs from the restatement"
    if continuous:
        err = np.abs(target.astype(np.float64) - want["target64"]).max()
        assert err <= CONTINUOUS_ATOL, f"continuous target {err:.3e} from the float64 bilinear value"
    else:
        assert bits_equal(target, want["target"]), "pixel-mode target differs from the restatement"


@pytest.mark.parametrize("case", CASE_TABLE, ids=[c[1] for c in CASE_TABLE])
def test_sample_pixels_guarded(case):
    """P in BATCHES x outputs aligned / both shifted by 4 bytes, on one image: stores stay inside xy, target and draw"""
    from collision_handling_in_instantngp_amd import ops
    _entry, _label, kw = case
    h, w, C, continuous = kw["h"], kw["w"], kw["C"], kw["continuous"]
    img = image_of(h, w, C)
    texel = ref.array_texel(img)
    denom = float(max(h, w, 2) - 1)
    for n, P in enumerate(BATCHES):
        for misalign in (0, 4):
            arena = guarded.Arena(P * (2 + C) * 4 + h * w * C + 8 * guarded.PAD, device=DEV)
            image = arena.put(img, name="image")
            d0, seed = 3 * n + misalign // 4, (-7 if misalign else 12345) + n
            draw = arena.take((1,), torch.int64, fill=d0, name="draw")
            xy = arena.take((P, 2), torch.float32, misalign=misalign, name="xy")
            target = arena.take((P, C), torch.float32, misalign=misalign, name="target")
            ops.sample_pixels(image, seed, draw, xy, target, denom=denom, continuous=continuous)
            torch.cuda.synchronize()
            arena.check()
            assert not bool(guarded.unwritten(xy).any()) and not bool(guarded.unwritten(target).any())
            assert int(draw.item()) == d0 + 1
            assert np.array_equal(image.cpu().numpy(), img)
            check_batch(xy, target, ref.sample(texel, h, w, C, denom, seed, d0, P, continuous), continuous)


def test_empty_batch_launches_nothing():
    from collision_handling_in_instantngp_amd import ops
    arena = guarded.Arena(8 * guarded.PAD, device=DEV)
    image = arena.put(image_of(2, 2, 3), name="image")
    draw = arena.take((1,), torch.int64, fill=9, name="draw")
    xy, target = torch.empty((0, 2), device=DEV), torch.empty((0, 3), device=DEV)
    ops.sample_pixels(image, 0, draw, xy, target, denom=1.0, continuous=True)
    torch.cuda.synchronize()
    arena.check()
    assert int(draw.item()) == 9


BIG = (36000, 36000, 4)            # 5.18e9 texel bytes: offsets pass 2^31 for 59 % of the samples and 2^32 for 17 %


def big_texel(r, c, k):
    """the large image by formula, on int64 index arrays (numpy) — fill_big evaluates the same on the device"""
    return ((r * 3 + c * 5 + k * 7 + ((r * c) >> 10)) & 255).astype(np.uint8)


def fill_big(h, w, C):
    image = torch.empty((h, w, C), dtype=torch.uint8, device=DEV)
    c = torch.arange(w, dtype=torch.int32, device=DEV).view(1, w, 1)
    k = torch.arange(C, dtype=torch.int32, device=DEV).view(1, 1, C)
    for lo in range(0, h, 1000):
        r = torch.arange(lo, min(h, lo + 1000), dtype=torch.int32, device=DEV).view(-1, 1, 1)        # r c < 2^31
        image[lo:lo + r.shape[0]] = ((r * 3 + c * 5 + k * 7 + ((r * c) >> 10)) & 255).to(torch.uint8)
    return image


def test_texel_offsets_are_64_bit():
    """h w C > 2^32: an offset formed in 32 bits, signed or not, reads another texel.  The image is an input (a const pointer) and
    lives outside the arena — a guarded 5 GB buffer would be compared byte by byte; the outputs are guarded as everywhere.  One
    image, filled once, serves both modes."""
    from collision_handling_in_instantngp_amd import ops
    h, w, C = BIG
    P = 4099
    image = fill_big(h, w, C)
    for continuous in (False, True):
        arena = guarded.Arena(P * (2 + C) * 4 + 8 * guarded.PAD, device=DEV)
        draw = arena.take((1,), torch.int64, fill=2, name="draw")
        xy = arena.take((P, 2), torch.float32, name="xy")
        target = arena.take((P, C), torch.float32, name="target")
        ops.sample_pixels(image, 77, draw, xy, target, denom=float(h - 1), continuous=continuous)
        torch.cuda.synchronize()
        arena.check()
        assert not bool(guarded.unwritten(xy).any()) and not bool(guarded.unwritten(target).any()) and int(draw.item()) == 3
        want = ref.sample(big_texel, h, w, C, float(h - 1), 77, 2, P, continuous)
        rows, cols = (want["r0"], want["c0"]) if continuous else (want["r"], want["c"])
        offsets = (rows * w + cols) * C
        assert (offsets >= 2 ** 31).sum() > P // 3 and (offsets >= 2 ** 32).sum() > P // 10
        check_batch(xy, target, want, continuous)
    del image


@pytest.mark.parametrize("continuous", [False, True], ids=["pixel", "continuous"])
def test_image_sampler_draws_in_sequence_and_keeps_the_previous_batch(continuous):
    """three next() calls are draws d, d + 1, d + 2 of the restatement; the batch of call k is untouched by call k + 1 (two rotating
    pairs); next() allocates nothing; state_dict / load_state_dict continue the sequence"""
    from collision_handling_in_instantngp_amd import data
    h, w, C, P = 61, 67, 3, 257
    img = image_of(h, w, C)
    texel = ref.array_texel(img)
    s = data.ImageSampler(img, P, seed=42, continuous=continuous)
    assert s.image.dtype == torch.uint8 and s.image.is_cuda and s.denom == 66.0
    assert s.coord_bounds == (float(np.float32(60) / np.float32(66)), 1.0)
    s.load_state_dict({"seed": 42, "draw": 5, "batch": P, "mode": "continuous" if continuous else "pixel"})
    torch.cuda.synchronize()
    kept = []
    for k in range(3):
        before = torch.cuda.memory_allocated()
        x, t = s.next()
        assert torch.cuda.memory_allocated() == before
        assert x.shape == (P, 2) and t.shape == (P, C) and x.is_contiguous() and t.is_contiguous()
        if kept:
            px, pt, cx, ct = kept[-1]
            assert x.data_ptr() != px.data_ptr() and guarded.same_bytes(px, cx) and guarded.same_bytes(pt, ct)      # batch k - 1 stands
        check_batch(x, t, ref.sample(texel, h, w, C, 66.0, 42, 5 + k, P, continuous), continuous)
        kept.append((x, t, x.clone(), t.clone()))
    assert s.draw == 8
    assert s.state_dict() == {"seed": 42, "draw": 8, "batch": P, "mode": "continuous" if continuous else "pixel"}
    with pytest.raises(ValueError):
        s.load_state_dict({"seed": 42, "draw": 0, "batch": P + 1, "mode": "pixel"})
    gray = data.ImageSampler(img[:, :, 0], 8, continuous=False)                # (h, w): one channel
    x, t = gray.next()
    check_batch(x, t, ref.sample(ref.array_texel(img[:, :, :1]), h, w, 1, 66.0, 0, 0, 8, False), False)
    dev = data.ImageSampler(torch.from_numpy(img).to(DEV), 8, seed=1)          # a device tensor is taken as it is
    x, t = dev.next()
    check_batch(x, t, ref.sample(texel, h, w, C, 66.0, 1, 0, 8, True), True)


def test_captured_next_draws_a_new_batch_on_every_replay():
    from collision_handling_in_instantngp_amd import data
    h, w, C, P = 61, 67, 3, 4099
    img = image_of(h, w, C)
    texel = ref.array_texel(img)
    s = data.ImageSampler(img, P, seed=9)
    s.next()                                           # draw 0, eager: the library is loaded, nothing lazy is left for the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        before = torch.cuda.memory_allocated()
        x, t = s.next()
        assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert s.draw == 1                                 # capturing launches nothing
    got = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got.append((x.clone(), t.clone()))
    assert s.draw == 3
    assert not guarded.same_bytes(got[0][0], got[1][0])
    for k, (gx, gt) in enumerate(got):
        check_batch(gx, gt, ref.sample(texel, h, w, C, 66.0, 9, 1 + k, P, True), True)


# ------------------------------------------------------------------------------------------------ train_sampled
TRAIN = dict(h=61, w=67, C=3, P=1027, steps=3, seed=11)
LRS = dict(encoding=1e-4, other=1e-3)
_BY_HAND = {}


def _net(models, mode):
    torch.manual_seed(3)
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=256, num_levels=4, n_min=8, n_max=32,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=256, feature_dim=2, topk_k=4).to(DEV)
    net.return_indices = False
    net.dense_probs = False
    if mode != "hash":
        for p in net.HPD.parameters():
            p.requires_grad = False
        net.compute_pbar = False
    return net


def _setup(mode):
    from collision_handling_in_instantngp_amd import models, train
    net = _net(models, mode)
    loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
    opt = train.get_optimizer(net, LRS["encoding"], LRS["other"], LRS["other"], 0.0, 0.0, 1e-6)
    return net, loss_fn, opt


def restated_batches(continuous=True):
    c = TRAIN
    texel = ref.array_texel(image_of(c["h"], c["w"], c["C"]))
    return [ref.sample(texel, c["h"], c["w"], c["C"], 66.0, c["seed"], d, c["P"], continuous) for d in range(c["steps"] + 1)]


def by_hand(mode):
    """the existing GraphedStep driven by hand on the restated batches, once per mode: {name: parameter after three steps}"""
    if mode not in _BY_HAND:
        from collision_handling_in_instantngp_amd import train
        net, loss_fn, opt = _setup(mode)
        bounds = (float(np.float32(60) / np.float32(66)), 1.0)
        gs = train.GraphedStep(net, loss_fn, opt, 1, 1, 1e-3, coord_bounds=bounds, cross_replay=True)
        batches = [(torch.from_numpy(b["xy"]).to(DEV), torch.from_numpy(b["target"]).to(DEV)) for b in restated_batches()]
        for k in range(TRAIN["steps"]):
            gs(batches[k][0], batches[k][1], next_first=batches[k + 1][0])
        torch.cuda.synchronize()
        _BY_HAND[mode] = {k: p.detach().clone() for k, p in net.named_parameters()}
    return _BY_HAND[mode]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", ["hash", "gngf_frozen"])
def test_train_sampled_is_graphed_step_on_the_restated_batches(mode, graph):
    """three steps on the 61 x 67 image (L = 4, F = 2, T = 256): the batches the steps received are the restatement's draws 0..3,
    draw ends at steps + 1, and the parameters equal those of GraphedStep driven by hand on the restated batches — to the bounds of
    tests/test_gpu_model.py::test_three_training_steps_match_reference: rtol 1e-2 (its third step) and atol 0.02 lr (its bound on a
    parameter's update: lr 1e-4 for the level tables, 1e-3 elsewhere)."""
    from collision_handling_in_instantngp_amd import data, models, train
    c = TRAIN
    models.should_use_hash_function = mode == "hash"
    try:
        want = by_hand(mode)
        net, loss_fn, opt = _setup(mode)
        sampler = data.ImageSampler(image_of(c["h"], c["w"], c["C"]), c["P"], seed=c["seed"])
        seen, inner = [], sampler.next

        def recording_next():
            x, t = inner()
            seen.append((x.clone(), t.clone()))
            return x, t

        sampler.next = recording_next
        rec = train.train_sampled(net, loss_fn, opt, sampler, c["steps"], l_mse=1, l_js_kl=1, l_collisions=1e-3, graph=graph)
        torch.cuda.synchronize()
        assert sampler.draw == c["steps"] + 1 and len(seen) == c["steps"] + 1
        gs = getattr(net, "_graphed_step", None)
        assert (isinstance(gs, train.GraphedStep) and gs.cross_replay and len(gs._graphs) == 1) if graph else gs is None
        for (x, t), b in zip(seen, restated_batches()):
            check_batch(x, t, b, True)
        assert rec["loss"].shape == (c["steps"],) and rec["mse"].shape == (c["steps"],) and rec["loss"].is_cuda
        assert bool(torch.isfinite(rec["loss"]).all()) and bool((rec["mse"] > 0).all())
        moved = 0
        for name, p in net.named_parameters():
            if not p.requires_grad or not p.dtype.is_floating_point:
                assert torch.equal(p.detach(), want[name]), name
                continue
            lr = LRS["encoding"] if "hash_tables" in name else LRS["other"]
            np.testing.assert_allclose(p.detach().cpu().numpy(), want[name].cpu().numpy(), rtol=1e-2, atol=0.02 * lr, err_msg=name)
            moved += 1
        assert moved >= 7                                  # four level tables... and the decoder's tensors
    finally:
        models.should_use_hash_function = False


@pytest.mark.parametrize("kind", ["dense_levels", "gngf_learning"])
def test_train_sampled_runs_the_other_model_kinds(kind):
    """a dense_levels model (T = 512: three dense levels, one hashed) and GNGF indexing with a TRAINABLE HPD, three replayed steps:
    the batches are the restatement's, draw ends at steps + 1, the losses are finite and every trainable tensor moved.  (What a step
    computes on these models is held elsewhere; here: that the loop serves them.)"""
    from collision_handling_in_instantngp_amd import data, models, train
    c = TRAIN
    models.should_use_hash_function = kind == "dense_levels"
    try:
        torch.manual_seed(3)
        net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=512 if kind == "dense_levels" else 256, num_levels=4,
                                              n_min=8, n_max=32, MLP_hidden_layers_widths=[64, 64],
                                              HPD_hidden_layers_widths=[32, 64, 128],
                                              HPD_out_features=512 if kind == "dense_levels" else 256, feature_dim=2, topk_k=4,
                                              dense_levels=(kind == "dense_levels")).to(DEV)
        net.return_indices = False
        loss_fn = train.Loss(delta=1, gamma=-2, epsilon=1)
        opt = train.get_optimizer(net, LRS["encoding"], LRS["other"], LRS["other"], 0.0, 0.0, 1e-6)
        # the level tables, the decoder and, where it is used, the HPD (not the BatchNorm of should_batchnorm_data: it is not run)
        used = ("_hash_tables.", "mlp.") + (("HPD.",) if kind == "gngf_learning" else ())
        before = {k: p.detach().clone() for k, p in net.named_parameters()
                  if p.requires_grad and p.dtype.is_floating_point and any(u in k for u in used)}
        sampler = data.ImageSampler(image_of(c["h"], c["w"], c["C"]), c["P"], seed=c["seed"])
        seen, inner = [], sampler.next

        def recording_next():
            x, t = inner()
            seen.append((x.clone(), t.clone()))
            return x, t

        sampler.next = recording_next
        rec = train.train_sampled(net, loss_fn, opt, sampler, c["steps"], l_mse=1, l_js_kl=1, l_collisions=1e-3, graph=True)
        torch.cuda.synchronize()
        assert sampler.draw == c["steps"] + 1
        for (x, t), b in zip(seen, restated_batches()):
            check_batch(x, t, b, True)
        assert bool(torch.isfinite(rec["loss"]).all()) and bool(torch.isfinite(rec["mse"]).all()) and bool((rec["mse"] > 0).all())
        after = dict(net.named_parameters())
        assert len(before) >= 10
        for k, p0 in before.items():
            assert bool(torch.isfinite(after[k]).all()) and not torch.equal(after[k].detach(), p0), k
    finally:
        models.should_use_hash_function = False


def test_train_sampled_refuses_a_single_buffer_pair():
    from collision_handling_in_instantngp_amd import data, models, train
    models.should_use_hash_function = True
    try:
        net, loss_fn, opt = _setup("hash")
        s = data.ImageSampler(image_of(61, 67, 3), 64, buffers=1)
        with pytest.raises(ValueError, match="buffers"):
            train.train_sampled(net, loss_fn, opt, s, 1, l_mse=1, l_js_kl=1, l_collisions=1e-3)
    finally:
        models.should_use_hash_function = False
