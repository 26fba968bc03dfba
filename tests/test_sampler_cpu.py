"""CPU: the device batch sampler (include/gngf_ext.h: gngf_ext_sample_pixels) without a device — what the entry point and its
Python wrappers reject before any device work, and the properties of the numpy restatement (tests/sampler_reference.py) that
tests/test_gpu_sampler.py holds the kernel to: indices in range at the smallest and largest image sides, positions inside the image,
pixel-mode batches equal to the reference's data path bit for bit, uniform draws, no sample shared between draws."""
import numpy as np
import pytest
import torch

import sampler_reference as ref

SIDES = [1, 2, 3, 1000, 1 << 24]
EDGE_U = np.array([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], dtype=np.uint64)


def rejected(h=4, w=4, C=3, denom=3.0, continuous=0, P=5):
    from collision_handling_in_instantngp_amd import _lib
    return _lib.load().gngf_ext_sample_pixels(None, h, w, C, denom, 0, None, continuous, None, None, P, None)


def test_rejected_arguments_return_invalid_value_before_any_launch():
    """all pointers NULL: whatever is accepted here would have launched"""
    assert rejected() == 1                                    # NULL pointers with P > 0
    assert rejected(P=0) == 0                                 # P == 0: success, no launch, nothing read
    assert rejected(P=-1) == 1
    for C in (0, 5, -1):
        assert rejected(C=C, P=0) == 1
    for denom in (0.0, -1.0, float("nan")):
        assert rejected(denom=denom, P=0) == 1
    for side in (0, -1, (1 << 24) + 1):
        assert rejected(h=side, P=0) == 1 and rejected(w=side, P=0) == 1
    assert rejected(h=1 << 24, w=1 << 24, P=0) == 0
    assert rejected(h=1, w=1, P=0) == 0                       # one pixel: fine for pixel centres ...
    for h, w in ((1, 4), (4, 1), (1, 1)):
        assert rejected(h=h, w=w, continuous=1, P=0) == 1     # ... no cell to interpolate in
    assert rejected(h=2, w=2, continuous=1, P=0) == 0
    assert rejected(continuous=2, P=0) == 1


def test_wrapper_validates_before_any_device_work():
    """CPU tensors: a ValueError names the argument before the binding looks at a pointer; valid arguments get as far as the
    binding, which has no CPU path"""
    from collision_handling_in_instantngp_amd import _lib, data, ops
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    draw = torch.zeros((), dtype=torch.int64)
    xy, tg = torch.zeros((7, 2)), torch.zeros((7, 3))
    bad = [dict(image=torch.zeros((4, 5), dtype=torch.uint8)), dict(image=torch.zeros((4, 5, 5), dtype=torch.uint8)),
           dict(denom=0.0), dict(denom=float("nan")), dict(xy=torch.zeros((7, 3))), dict(target=torch.zeros((7, 1))),
           dict(target=torch.zeros((6, 3))), dict(draw=torch.zeros((2,), dtype=torch.int64)),
           dict(image=torch.zeros((1, 5, 3), dtype=torch.uint8), continuous=True)]
    for kw in bad:
        a = dict(image=img, seed=0, draw=draw, xy=xy, target=tg, denom=4.0, continuous=False)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.sample_pixels(a["image"], a["seed"], a["draw"], a["xy"], a["target"], denom=a["denom"], continuous=a["continuous"])
    with pytest.raises(_lib.GngfLibraryError):
        ops.sample_pixels(img, 0, draw, xy, tg, denom=4.0, continuous=False)
    with pytest.raises(TypeError):
        data.ImageSampler(np.zeros((4, 4, 3), np.float32), 8)
    with pytest.raises(ValueError):
        data.ImageSampler(np.zeros((4, 4, 5), np.uint8), 8)
    with pytest.raises(ValueError):
        data.ImageSampler(np.zeros((1, 4), np.uint8), 8, continuous=True)
    with pytest.raises(ValueError):
        data.ImageSampler(np.zeros((1, 1), np.uint8), 8, continuous=False)          # max(h, w) - 1 = 0 is no denominator


def test_train_sampled_refuses_what_it_does_not_serve():
    from collision_handling_in_instantngp_amd import models, train

    class Sampler:
        buffers = 2

    assert hasattr(models, "should_batchnorm_data")
    prev = models.should_batchnorm_data
    models.should_batchnorm_data = True
    try:
        with pytest.raises(ValueError, match="should_batchnorm_data"):
            train.train_sampled(object(), None, None, Sampler(), 1, l_mse=1, l_js_kl=1, l_collisions=1e-3)
    finally:
        models.should_batchnorm_data = prev

    class Net:
        class dp:
            active, defer_vertex, world, zero = True, False, 2, None

    with pytest.raises(ValueError, match="data-parallel"):
        train.train_sampled(Net(), None, None, Sampler(), 1, l_mse=1, l_js_kl=1, l_collisions=1e-3)


def test_generator_is_the_stated_one():
    """sample 0 of draw 0 with seed 0 is splitmix64's first output — the published test vector of that generator"""
    assert int(ref.bits(0, 0, 1)[0]) == 0xE220A8397B1DCDAF
    z = ref.bits(12345, 3, 1000)
    assert np.array_equal(z[5:8], ref.bits(12345, 3, 1000, i=[5, 6, 7]))
    assert np.array_equal(ref.bits(7, 2, 10), ref.bits(7, 0, 10, i=np.arange(20, 30)))       # the counter is d P + i + 1
    assert np.array_equal(ref.bits(-1, 0, 4), ref.bits((1 << 64) - 1, 0, 4))                  # the seed's 64 bits, signed or not
    u, v = ref.uv(1, 0, 1 << 12)
    assert u.max() < (1 << 24) and v.max() < (1 << 24)


@pytest.mark.parametrize("h", SIDES)
@pytest.mark.parametrize("w", SIDES)
def test_indices_are_in_range(h, w):
    """at the ends of the 24-bit range and over a draw: pixel indices inside the image, the bilinear cell and its + 1 neighbours
    inside it, fractions in [0, 1], positions at most h - 1"""
    u = np.concatenate([EDGE_U, ref.uv(3, 0, 1 << 14)[0]])
    v = np.concatenate([EDGE_U[::-1], ref.uv(3, 0, 1 << 14)[1]])
    r, c = ref.pixel_indices(u, v, h, w)
    assert r.min() >= 0 and r.max() <= h - 1 and c.min() >= 0 and c.max() <= w - 1
    assert r[len(EDGE_U) - 1] == h - 1 and r[0] == 0
    if h < 2 or w < 2:
        return
    pr, pc = ref.positions(u, v, h, w)
    assert pr.dtype == np.float32 and pr.min() >= 0 and pc.min() >= 0
    assert pr.max() <= np.float32(h - 1) and pc.max() <= np.float32(w - 1)
    r0, fr, c0, fc = ref.cells(pr, pc, h, w)
    assert r0.min() >= 0 and r0.max() + 1 <= h - 1 and c0.min() >= 0 and c0.max() + 1 <= w - 1
    assert fr.min() >= 0 and fr.max() <= 1 and fc.min() >= 0 and fc.max() <= 1
    # (1 - 2^-24) (h - 1) rounds below h - 1 (the decrement is more than half an ulp): the min() of the cell is a belt, never taken
    assert pr.max() < np.float32(h - 1) and np.array_equal(r0, np.floor(pr).astype(np.int64))
    assert pc.max() < np.float32(w - 1) and np.array_equal(c0, np.floor(pc).astype(np.int64))


@pytest.mark.parametrize("shape", [(61, 67, 3), (5, 9, 1), (40, 17, 3)])
def test_pixel_mode_is_the_reference_data_path_bit_for_bit(shape):
    """xy = normalise_coordinates(pixel_grid)[r * w + c] and target = MyDataset's Y[r * w + c]; and for all 256 texel values
    float32(t / 255 in float64), MyDataset's arithmetic, equals (float)t / 255.0f, the kernel's"""
    from collision_handling_in_instantngp_amd import data
    t = np.arange(256)
    assert np.array_equal((t.astype(np.float64) / 255).astype(np.float32), t.astype(np.float32) / np.float32(255.0))
    h, w, C = shape
    rng = np.random.default_rng(h * w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    X, Y, hh, ww = data.MyDataset(image=img, should_bw=(C == 1))[0]
    assert (hh, ww) == (h, w) and Y.shape == (h * w, C)
    Xn = data.normalise_coordinates(X, w, h).numpy()
    used = data.to_grayscale(img)[:, :, None] if C == 1 else img
    for seed, draw in ((0, 0), (5, 2)):
        s = ref.sample(ref.array_texel(used), h, w, C, max(h, w) - 1, seed, draw, 4099, continuous=False)
        flat = s["r"] * w + s["c"]
        assert s["xy"].dtype == np.float32 and s["target"].dtype == np.float32
        assert np.array_equal(s["xy"].view(np.uint32), Xn[flat].view(np.uint32))
        assert np.array_equal(s["target"].view(np.uint32), Y.numpy()[flat].view(np.uint32))
        assert len(np.unique(flat)) > 0.5 * min(4099, h * w)


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("draw", [0, 1, 7])
def test_draws_are_uniform_over_16_by_16_cells(seed, draw):
    """2^20 samples of one draw, binned by the top four bits of u and v: each of the 256 counts is Binomial(2^20, 1/256), mean 4096,
    sigma = sqrt(4096 * 255/256) = 63.9; 5 sigma = 320 (the generator stays within 3.7 sigma at these seeds and draws)"""
    u, v = ref.uv(seed, draw, 1 << 20)
    cell = ((u >> np.uint64(20)) * np.uint64(16) + (v >> np.uint64(20))).astype(np.int64)
    counts = np.bincount(cell, minlength=256)
    assert counts.sum() == 1 << 20 and len(counts) == 256
    assert np.abs(counts - 4096).max() <= 320, np.abs(counts - 4096).max()


def test_two_consecutive_draws_share_no_sample():
    for seed, d, P in ((0, 0, 4099), (1, 6, 1 << 16)):
        a, b = ref.bits(seed, d, P), ref.bits(seed, d + 1, P)
        assert len(np.intersect1d(a, b)) == 0
        assert len(np.unique(np.concatenate([a, b]))) == 2 * P            # (the finaliser is a bijection of distinct counters)
        ua, va = ref.uv(seed, d, P)
        ub, vb = ref.uv(seed, d + 1, P)
        assert len(np.intersect1d((ua << np.uint64(24)) | va, (ub << np.uint64(24)) | vb)) == 0


def test_float64_value_bounds_the_fp32_value():
    """the restatement's own fp32 target stays within the bound tests/test_gpu_sampler.py holds the kernel to"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(61, 67, 3), dtype=np.uint8)
    s = ref.sample(ref.array_texel(img), 61, 67, 3, 66, 0, 0, 1 << 16, continuous=True)
    assert np.abs(s["target"].astype(np.float64) - s["target64"]).max() <= 1e-6
    assert s["target64"].min() >= 0 and s["target64"].max() <= 1
