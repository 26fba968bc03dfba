"""GPU: the epoch image, train_accuracy and train_psnr on the device (train.EpochImage over csrc/metrics.hip) against what the
tree computes on the host — data.reassemble_image, train.calc_psnr, train.calc_accuracy.  Integer statistics of an integer
image: every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 3), (7, 5, 1), (61, 67, 3), (256, 257, 3)]


def _planted():
    """0, 1, k/255 for several k — the values where (x * 255) lands on or next to a whole number — and the floats one ulp
    either side of each"""
    ks = np.array([0, 1, 2, 3, 5, 17, 64, 85, 127, 128, 170, 200, 254, 255], dtype=np.float32)
    base = np.concatenate([ks / np.float32(255), np.array([0.0, 1.0], dtype=np.float32)]).astype(np.float32)
    lo = np.nextafter(base, np.float32(-np.inf), dtype=np.float32)
    hi = np.nextafter(base, np.float32(np.inf), dtype=np.float32)
    return np.concatenate([base, lo, hi])


def _outputs(rng, P, C):
    out = rng.random((P, C), dtype=np.float32)
    planted = _planted()
    flat = out.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, 4 * planted.size)]
    flat[pos] = planted[np.arange(pos.size) % planted.size]
    return out


def _batches(P, nb):
    """train_epoch's slices: nb batches of int(P / nb) rows (rows beyond them are never visited)"""
    step = P if nb == 1 else int(P / nb)
    return [(b * step, step) for b in range(nb)]


def _run_epoch(ep, out_dev, P, nb):
    ep.begin()
    assembled = torch.zeros_like(out_dev)
    for lo, n in _batches(P, nb):
        if n == 0:                                  # as train_epoch skips an empty batch
            continue
        ep.add(out_dev[lo:lo + n].contiguous(), lo)
        assembled[lo:lo + n] = out_dev[lo:lo + n]
    return assembled


@functools.lru_cache(maxsize=None)
def _case(shape, shuffled, nb):
    """inputs and the host reference of one case, computed once"""
    from collision_handling_in_instantngp_amd import data, train
    h, w, C = shape
    P = h * w
    rng = np.random.default_rng(1000 * P + 10 * nb + int(shuffled))
    out = _outputs(rng, P, C)
    gen = torch.Generator().manual_seed(P + nb)
    shuf, reordered = data.make_permutation(P, gen) if shuffled else (None, None)
    out_dev = torch.tensor(out, device=DEV)
    assembled = torch.zeros_like(out_dev)
    for lo, n in _batches(P, nb):
        assembled[lo:lo + n] = out_dev[lo:lo + n]
    want_img = data.reassemble_image(assembled if C == 3 else assembled.reshape(-1), reordered, h, w, should_bw=(C == 1),
                                     should_shuffle=shuffled)
    # a target that shares about a third of its elements with the prediction, so that the count is not trivially 0
    target = rng.integers(0, 256, size=want_img.shape)
    hit = rng.random(want_img.shape) < 0.35
    target[hit] = np.clip(want_img[hit], 0, 255)
    target = target.astype(np.uint8)
    if target.max() == 0:
        target.flat[0] = 9                          # (log10 of a zero peak is not a case of interest)
    want = {"img": want_img,
            "eq": int(np.equal(want_img, target).sum()),
            "sse": int(np.square(want_img.astype(np.int64) - target.astype(np.int64)).sum()),
            "psnr": train.calc_psnr(want_img, target),
            "acc": train.calc_accuracy(want_img, target, want_img.size)}
    return out_dev, shuf, reordered, target, want


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_image_and_statistics_are_exact(shape, shuffled, nb):
    from collision_handling_in_instantngp_amd import data, train
    h, w, C = shape
    P = h * w
    out_dev, shuf, reordered, target, want = _case(shape, shuffled, nb)
    ep = train.EpochImage(target if C == 3 else target.reshape(h, w), shuf, device=DEV)
    assembled = _run_epoch(ep, out_dev, P, nb)
    got_img = ep.image()
    assert got_img.dtype == np.int32 and got_img.shape == want["img"].shape
    assert np.array_equal(got_img, want["img"])
    assert np.array_equal(ep.image_tensor().cpu().numpy(), want["img"])
    sums = ep.sums()
    assert sums.is_cuda and sums.dtype == torch.int64 and tuple(sums.shape) == (2,)
    eq, sse = (int(v) for v in sums.cpu().numpy())
    print(f"shape {shape} shuffled {shuffled} nb {nb}: eq {eq} (want {want['eq']}), sse {sse} (want {want['sse']}), "
          f"psnr {ep.psnr()!r} (want {want['psnr']!r}), accuracy {ep.accuracy()!r} (want {want['acc']!r})")
    assert (eq, sse) == (want["eq"], want["sse"])
    assert 0 < want["eq"] < want["img"].size or P == 1
    assert ep.psnr() == want["psnr"]
    assert ep.accuracy() == want["acc"]
    dev_img = data.reassemble_image_device(assembled if C == 3 else assembled.reshape(-1), reordered, h, w,
                                           should_bw=(C == 1), should_shuffle=shuffled)
    assert dev_img.is_cuda and dev_img.dtype == torch.int32
    assert np.array_equal(dev_img.cpu().numpy(), want["img"])


def test_scatter_beyond_one_grid_sweep():
    """420 x 421 x 3 = 530 460 elements in one batch: more than the 2048 x 256 lanes of the scatter's largest grid, so its
    grid-stride loop takes a second trip (the four shapes above fit in one)"""
    test_image_and_statistics_are_exact((420, 421, 3), True, 1)


def test_unvisited_pixel_reads_zero_and_counts_in_both_sums():
    """P = 61 * 67 = 4087 in three batches of 1362 rows: pixel shuffled[4086] is never visited"""
    from collision_handling_in_instantngp_amd import train
    shape = (61, 67, 3)
    P = 61 * 67
    out_dev, shuf, reordered, target, want = _case(shape, True, 3)
    assert 3 * int(P / 3) == P - 1
    target = target.copy()
    pix = int(shuf[P - 1])
    target.reshape(P, 3)[pix] = (0, 7, 0)                   # two elements equal the unvisited zeros, one differs by 7
    ep = train.EpochImage(target, shuf, device=DEV)
    _run_epoch(ep, out_dev + 0.5, P, 3)                     # (every visited pixel is >= 127: the zeros are the unvisited ones)
    img = ep.image()
    assert np.array_equal(img.reshape(P, 3)[pix], (0, 0, 0))
    assert int((img.reshape(P, 3) == 0).all(1).sum()) == 1
    eq, sse = (int(v) for v in ep.sums().cpu().numpy())
    assert eq == int(np.equal(img, target).sum())
    assert sse == int(np.square(img.astype(np.int64) - target.astype(np.int64)).sum())
    # without the unvisited pixel the sums are smaller by exactly its share: 2 equal elements, 49 of squared difference
    rest = np.ones(P, bool)
    rest[pix] = False
    assert eq - int(np.equal(img.reshape(P, 3)[rest], target.reshape(P, 3)[rest]).sum()) == 2
    assert sse - int(np.square(img.reshape(P, 3)[rest].astype(np.int64) - target.reshape(P, 3)[rest].astype(np.int64)).sum()) == 49


def test_second_epoch_on_the_same_object_depends_on_that_epoch_only():
    from collision_handling_in_instantngp_amd import train
    shape = (61, 67, 3)
    P = 61 * 67
    out_dev, shuf, reordered, target, want = _case(shape, True, 3)
    ep = train.EpochImage(target, shuf, device=DEV)
    _run_epoch(ep, 1.0 - out_dev, P, 1)                     # first epoch: other outputs, and it visits EVERY pixel
    first = (ep.image(), ep.sums().clone())
    assert not np.array_equal(first[0], want["img"])
    _run_epoch(ep, out_dev, P, 3)                           # second: begin() must clear the pixel this epoch does not visit
    assert np.array_equal(ep.image(), want["img"])
    a = ep.sums().clone()
    b = ep.sums().clone()
    assert torch.equal(a, b)
    assert tuple(int(v) for v in a.cpu().numpy()) == (want["eq"], want["sse"])
    assert ep.psnr() == want["psnr"] and ep.accuracy() == want["acc"]


def test_values_outside_0_1_are_not_clamped():
    from collision_handling_in_instantngp_amd import train
    h, w = 9, 11
    P = h * w
    rng = np.random.default_rng(5)
    out = rng.random((P, 3), dtype=np.float32)
    out[3] = (-0.5, 3.0, 0.25)
    out[P - 1] = (3.0, -0.5, -0.5)
    target = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    ep = train.EpochImage(target, None, device=DEV)
    _run_epoch(ep, torch.tensor(out, device=DEV), P, 1)
    img = ep.image()
    assert tuple(img.reshape(P, 3)[3]) == (-127, 765, 63)
    assert tuple(img.reshape(P, 3)[P - 1]) == (765, -127, -127)
    want_img = (torch.tensor(out) * 255).int().numpy().reshape(h, w, 3)
    assert np.array_equal(img, want_img)
    eq, sse = (int(v) for v in ep.sums().cpu().numpy())
    assert eq == int(np.equal(want_img, target).sum())
    assert sse == int(np.square(want_img.astype(np.int64) - target.astype(np.int64)).sum())
    assert ep.psnr() == train.calc_psnr(want_img, target)


def test_bad_permutation_and_cpu_tensors_are_rejected():
    from collision_handling_in_instantngp_amd import _lib, train
    target = np.full((4, 5, 3), 200, dtype=np.uint8)
    P = 20
    good = torch.randperm(P, generator=torch.Generator().manual_seed(0)).int()
    for bad_value in (P, -1, 2 ** 31 - 1):
        bad = good.clone()
        bad[7] = bad_value
        with pytest.raises(ValueError):
            train.EpochImage(target, bad, device=DEV)
    with pytest.raises(ValueError):
        train.EpochImage(target, good[:-1], device=DEV)
    ep = train.EpochImage(target, good, device=DEV)
    ep.begin()
    with pytest.raises(_lib.GngfLibraryError):
        ep.add(torch.zeros((P, 3)), 0)
    with pytest.raises(ValueError):
        ep.add(torch.zeros((P, 3), device=DEV), 1)          # rows [1, 21) leave the image
    assert int(ep.image_tensor().abs().max()) == 0           # nothing was written


# ------------------------------------------------------------------------------------------------ end to end, cfg1
def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _cfg1(golden):
    """BASELINE configs[0] on the strawberry golden (as tests/test_gpu_model.py builds it): L = 4, T = 2^8, K = 4"""
    from collision_handling_in_instantngp_amd import models, train
    g7 = golden("G7_end_to_end_gngf")
    models.should_use_hash_function = False
    net = models.GeneralNeuralGaugeFields(input_dim=2, hash_table_size=256, num_levels=4, n_min=8, n_max=32,
                                          MLP_hidden_layers_widths=[64, 64], HPD_hidden_layers_widths=[32, 64, 128],
                                          HPD_out_features=256, feature_dim=2, topk_k=4)
    sd = net.state_dict()
    net.load_state_dict({k: (_t(g7["init_" + k.replace(".", "_")]) if "init_" + k.replace(".", "_") in g7 else v)
                         for k, v in sd.items()})
    return net, train.Loss(delta=1, gamma=-2, epsilon=1), train.get_optimizer(net, 1e-4, 1e-3, 1e-3, 0, 1e-6, 1e-6)


@pytest.mark.parametrize("graph", [False, True])
def test_cfg1_epoch_through_train_epoch_and_train_step(golden, graph):
    from collision_handling_in_instantngp_amd import data, train
    g = golden("G8_train_curve")
    img = golden("strawberry_rgb")["img"]
    h, w = img.shape[:2]
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    X = (torch.tensor(np.stack([rows, cols], -1).reshape(-1, 2)).float() / (max(w, h) - 1)).to(DEV)
    Y = torch.tensor(img.reshape(-1, 3) / 255).float().to(DEV)
    shuffled = _t(g["shuffled"].astype(np.int64))
    reordered = torch.empty_like(shuffled)
    reordered[shuffled] = torch.arange(shuffled.numel(), device=DEV)

    net, loss_fn, opt = _cfg1(golden)
    ep = train.EpochImage(img, g["shuffled"], device=DEV)
    rec = train.train_epoch(net, loss_fn, opt, X, Y, w, h, 1, 1, 1e-3, batch_percentage=1 / 3, should_shuffle=True,
                            shuffled_indices=shuffled, graph=graph, image=ep)
    want_img = data.reassemble_image(rec["outputs"], reordered, h, w)
    assert np.array_equal(ep.image(), want_img)
    psnr = ep.psnr()
    print(f"graph={graph}: device PSNR {psnr!r}, host {train.calc_psnr(want_img, img)!r}, reference {float(g['psnr'][0])!r}; "
          f"accuracy {ep.accuracy()!r}")
    assert psnr == train.calc_psnr(want_img, img)
    assert ep.accuracy() == train.calc_accuracy(want_img, img, want_img.size)
    assert abs(psnr - float(g["psnr"][0])) < 0.01

    results = []
    ep2 = train.EpochImage(img, g["shuffled"], device=DEV)
    for extra in ({"image": ep2}, {}):
        net, loss_fn, opt = _cfg1(golden)
        results.append(train.train_step(net, loss_fn, opt, X, Y, w, h, 256, 4, 1, 1, 1e-3, 1 / 3, 4, False, False, True, shuffled,
                                        reordered, None, None, graph=graph, **extra))
    with_image, without = results
    assert len(with_image) == len(without) == 9
    assert with_image[1] is None
    assert without[1].shape == (h, w, 3) and without[1].dtype == np.int32
    print(f"graph={graph}: train_step(image=) PSNR {ep2.psnr()!r}; image equal to the run without image=: "
          f"{np.array_equal(ep2.image(), without[1])}; loss {with_image[0]!r} / {without[0]!r}, mse {with_image[5]!r} / {without[5]!r}")
    assert ep2.image().shape == (h, w, 3) and ep2.image().dtype == np.int32
    assert abs(ep2.psnr() - float(g["psnr"][0])) < 0.01
    assert abs(ep2.psnr() - train.calc_psnr(without[1], img)) < 0.01
    for pos in (0, 5):                                                      # loss, mse: floats
        np.testing.assert_allclose(with_image[pos], without[pos], rtol=2e-3, atol=0, err_msg=f"position {pos}")
    for pos in (2, 3, 6, 7):                                                # collisions, minimum, JS/KL rows, collision losses
        a, b = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64) for v in (with_image[pos], without[pos]))
        assert a.shape == b.shape, pos
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=0, err_msg=f"position {pos}")
    assert with_image[4] == without[4] == [] and with_image[8] == without[8] == []
