"""The guard-band arena of tests/guarded.py on CPU tensors: it must bite, name what it bit, and stay quiet otherwise."""
import pytest
import torch

import guarded

DTYPES = [torch.float32, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8]


def arena3():
    a = guarded.Arena(1 << 16)
    x = a.take((5, 3), torch.float32, name="x")
    y = a.take(7, torch.int32, fill=0, misalign=4, name="y")
    z = a.take((2, 2), torch.float16, name="z")
    return a, x, y, z


def region(a, name):
    return next(r for r in a.regions if r[0] == name)


def test_layout_alignment_padding_and_tail():
    a, x, y, z = arena3()
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 4 and z.data_ptr() % 16 == 0
    assert x.is_contiguous() and tuple(x.shape) == (5, 3) and tuple(y.shape) == (7,)
    prev_end = 0
    for _name, s, e in a.regions:
        assert s - prev_end >= guarded.PAD
        prev_end = e
    assert a.buf.numel() - prev_end >= guarded.TAIL >= 1 << 20
    assert bool(guarded.unwritten(x).all()) and bool((y == 0).all())
    assert bool(torch.isnan(x).all()) and bool(torch.isnan(z).all())          # 0xFF reads as NaN ...
    assert int(a.take(1, torch.int64, name="i")[0]) == -1                      # ... and as -1
    a.check()
    with pytest.raises(MemoryError):
        guarded.Arena(3 * guarded.PAD).take(guarded.PAD + 1, torch.uint8)


def test_a_full_in_bounds_write_passes():
    a, x, y, z = arena3()
    x.fill_(1.5)
    y.fill_(3)
    z.fill_(-2.0)
    a.check()
    assert a.damage() == []
    assert not bool(guarded.unwritten(x).any()) and not bool(guarded.unwritten(z).any())


def test_one_byte_before_a_buffer_is_caught_and_named():
    a, x, y, z = arena3()
    _n, s, _e = region(a, "y")
    a.buf[s - 1] = 0
    assert a.damage() == [("y", "before", 1, 1, 1)]
    with pytest.raises(AssertionError, match=r"1 guard byte\(s\) written BEFORE y: bytes 1\.\.1 in front"):
        a.check()


def test_one_byte_after_a_buffer_is_caught_and_named():
    a, x, y, z = arena3()
    _n, _s, e = region(a, "x")
    a.buf[e] = 7
    assert a.damage() == [("x", "after", 0, 0, 1)]
    with pytest.raises(AssertionError, match=r"1 guard byte\(s\) written AFTER x: bytes 0\.\.0 past its end"):
        a.check()


def test_a_run_of_bytes_reports_first_last_and_count():
    a, x, y, z = arena3()
    _n, _s, e = region(a, "x")
    a.buf[e + 4:e + 8] = 0            # the four bytes of the float one element past x's end ...
    a.buf[e + 12] = 0                 # ... and one more, 0x00 0xFF-s in between
    assert a.damage() == [("x", "after", 4, 12, 5)]
    # both sides of one buffer, and a second buffer
    _n, s, _e = region(a, "z")
    a.buf[s - 16:s] = 1
    assert a.damage() == [("x", "after", 4, 12, 5), ("z", "before", 1, 16, 16)]


def test_the_far_end_of_the_tail_guard_is_caught():
    a, x, y, z = arena3()
    _n, _s, e = region(a, "z")
    last = a.buf.numel() - 1
    a.buf[last] = 0
    assert a.damage() == [("z", "after", last - e, last - e, 1)]
    with pytest.raises(AssertionError, match="AFTER z"):
        a.check()
    # in front of the first buffer
    b, x, y, z = arena3()
    b.buf[0] = 0
    assert b.damage() == [("x", "before", region(b, "x")[1], region(b, "x")[1], 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_unwritten_finds_a_single_skipped_element(dtype):
    a = guarded.Arena(1 << 16)
    t = a.take((6, 5), dtype, name="t")
    assert bool(guarded.unwritten(t).all())
    t.fill_(0)
    assert not bool(guarded.unwritten(t).any())
    t.reshape(-1).view(torch.uint8).fill_(guarded.FILL)
    t[:4].fill_(3)
    t[4, :3].fill_(3)
    t[4, 4] = 3
    t[5].fill_(3)
    want = torch.zeros((6, 5), dtype=torch.bool)
    want[4, 3] = True
    assert torch.equal(guarded.unwritten(t), want)
    # an element with one byte changed counts as written
    if t.element_size() > 1:
        u = a.take(3, dtype, name="u")
        u.view(torch.uint8)[u.element_size()] = 0
        assert guarded.unwritten(u).tolist() == [True, False, True]
    a.check()


def test_put_copies_an_input_and_same_bytes_compares_nan_payloads():
    a = guarded.Arena(1 << 16)
    src = torch.arange(12, dtype=torch.float32).view(3, 4)
    t = a.put(src, name="in", misalign=4)
    assert torch.equal(t, src) and t.data_ptr() % 16 == 4
    n = a.take(4, torch.float32, name="nan")
    assert guarded.same_bytes(n, n.clone()) and not guarded.same_bytes(n, torch.full((4,), float("nan")))
    a.check()
