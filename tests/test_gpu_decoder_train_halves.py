"""The training decoder's output layer sums two partials per pixel and channel: lane half h of a wave holds the hidden units j with
(j >> 2) & 1 == h, and the two halves exchange their partials with v_permlane32_swap (no LDS).  The digests of
test_gpu_decoder_train_schedule.py would report a swap in the wrong direction only as "differs"; here the weights say which half
failed: W2 is non-zero only on the hidden units ONE half holds, so every rgb value is that half's partial plus an exact zero from
the other — a half that receives the wrong partner value (its own again, another channel's, or nothing) misses decoder_fwd's rgb
by the whole pre-activation.

Pixel counts: a single pixel, the lane-half boundary of a wave (31, 32, 33), two waves (64), a partial and a full first tile plus
one pixel (127, 129), and a workgroup's second trip through the tile loop (128 * 256 + 1).  The bound on rgb is the one
test_fused_decoder_training_kernel_equals_forward_plus_backward holds the fused kernel to (5e-7 absolute: the two kernels run the
hidden layers on different matrix pipes)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import decoder_train_digests as dtd  # noqa: E402

pytestmark = pytest.mark.gpu

PIXELS = (1, 31, 32, 33, 64, 127, 129, 128 * 256 + 1)


def _inputs(leaky, P, half):
    inp = dtd.inputs(leaky, P)
    held = ((np.arange(64) >> 2) & 1) == half               # csrc/decoder_common.inc: crow(r, h) = (r & 3) + 8 (r >> 2) + 4 h
    w2 = inp["ws"][4].copy()
    w2[:, ~held] = 0.0
    inp["ws"][4] = w2
    return inp


def _forward_rgb(leaky, P, inp):
    import torch
    from collision_handling_in_instantngp_amd._lib import call, ptr, stream_ptr
    t = lambda a: torch.from_numpy(a).cuda()
    enc, ws = t(inp["enc"]), [t(w) for w in inp["ws"]]
    rgb = torch.full((P, dtd.OUT_DIM), -7.0, device="cuda")
    call("gngf_decoder_fwd", ptr(enc), *[ptr(w) for w in ws], ptr(rgb), ptr(None), P, dtd.IN_DIM, dtd.OUT_DIM, leaky, stream_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy()


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("leaky", (0, 1))
def test_output_layer_with_weights_on_one_lane_half(leaky, P, half):
    inp = _inputs(leaky, P, half)
    want = _forward_rgb(leaky, P, inp)
    first = dtd.run_fused(leaky, P, inp)["rgb"]
    again = dtd.run_fused(leaky, P, inp)["rgb"]
    err = np.abs(first.astype(np.float64) - want.astype(np.float64))
    print(f"leaky={leaky} P={P} half={half}: max |rgb - decoder_fwd| = {err.max():.3e}")
    assert first.tobytes() == again.tobytes(), "rgb differs between two runs of the same build on the same inputs"
    assert np.isfinite(first).all()
    # the weights must matter: with W2 = 0 every rgb value would be sigmoid(b2)
    b2 = inp["ws"][5].astype(np.float64)
    assert np.abs(want - 1.0 / (1.0 + np.exp(-b2))[None, :]).max() > 1e-3
    worst = np.unravel_index(int(err.argmax()), err.shape)
    assert err.max() <= 5e-7, (f"weights on lane half {half} only: pixel {worst[0]} channel {worst[1]} is {first[worst]!r}, "
                               f"decoder_fwd gives {want[worst]!r}")
