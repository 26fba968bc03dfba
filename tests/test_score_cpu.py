"""CPU: the host side of train.score / train.fit_sampled — what needs no device: the count of scored elements, the floats formed
from the two integer sums, and the arithmetic of the SSE-limit refusal."""
import numpy as np
import pytest


def test_scored_elements_is_the_size_of_the_strided_image():
    from collision_handling_in_instantngp_amd import train
    sides = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 37, 50, 64]
    for h in sides:
        for w in sides:
            for step in (1, 2, 3, 4, 7, 8, 16, 49, 50, 51, 1000):
                for C in (1, 3, 4):
                    want = np.zeros((h, w, C), dtype=np.uint8)[::step, ::step].size
                    assert train.scored_elements(h, w, C, step) == want, (h, w, C, step)
    assert train.scored_elements(1 << 24, 1 << 24, 4, 1) == 1 << 50           # Python integers: no overflow
    assert train.scored_elements(1 << 24, 1 << 24, 3, 1 << 40) == 3
    for bad in ((0, 4, 3, 1), (4, 0, 3, 1), (4, 4, 0, 1), (4, 4, 3, 0), (4, 4, 3, -2)):
        with pytest.raises(ValueError):
            train.scored_elements(*bad)


def test_psnr_and_accuracy_from_sums_are_epoch_images():
    """score_psnr's floats: psnr_from_sums with the peak term numpy gives for the whole uint8 image (float16 arithmetic for a
    uint8 maximum — EpochImage.peak_term), accuracy = eq / n * 100 — and calc_psnr / calc_accuracy of the reference on the
    images the sums came from"""
    from collision_handling_in_instantngp_amd import train
    rng = np.random.default_rng(3)
    for top in (255, 254, 200, 17, 1):
        og = rng.integers(0, top + 1, size=(13, 11, 3)).astype(np.uint8)
        og[0, 0, 0] = top
        pred = np.clip(og.astype(np.int64) + rng.integers(-3, 4, size=og.shape), 0, 255).astype(np.int32)
        pred[1, 1, 1] = og[1, 1, 1] + 1
        d = pred.astype(np.int64) - og.astype(np.int64)
        eq, sse, n = int((d == 0).sum()), int((d * d).sum()), og.size
        psnr, acc = train.psnr_accuracy_from_sums(eq, sse, n, int(og.max()))
        peak_term = 20 * np.log10(np.max(og))
        assert peak_term.dtype == np.float16
        assert psnr == float(train.psnr_from_sums(sse, n, peak_term))
        assert acc == float((eq / n) * 100) == float(train.calc_accuracy(pred, og, n))
        assert psnr == float(train.calc_psnr(pred, og))
    psnr, acc = train.psnr_accuracy_from_sums(12, 0, 12, 255)
    assert psnr == float("inf") and acc == 100.0


def test_sse_limit_refusal_arithmetic():
    """refused exactly when n * 255^2 > SSE_ORDER_LIMIT = 2^44; the message names the remedy"""
    from collision_handling_in_instantngp_amd import train
    assert train.SSE_ORDER_LIMIT == 1 << 44
    edge = train.SSE_ORDER_LIMIT // 255 ** 2                  # the largest n that passes
    assert edge * 255 ** 2 <= train.SSE_ORDER_LIMIT < (edge + 1) * 255 ** 2
    assert train.sse_order_refusal(edge) is None and train.sse_order_refusal(1) is None
    msg = train.sse_order_refusal(edge + 1)
    assert isinstance(msg, str) and "step" in msg and "2^44" in msg
    # the sizes the sampler exists for: 2048^2 x 3 passes, 16384^2 x 3 does not at step 1 and does at step 2
    assert train.sse_order_refusal(train.scored_elements(2048, 2048, 3, 1)) is None
    assert train.sse_order_refusal(train.scored_elements(16384, 16384, 3, 1)) is not None
    assert train.sse_order_refusal(train.scored_elements(16384, 16384, 3, 2)) is None
    # every sum a passing image can reach is below the limit the save rule is shown for
    assert edge * 255 ** 2 <= train.SSE_ORDER_LIMIT


def test_the_new_names_are_part_of_the_modules():
    from collision_handling_in_instantngp_amd import ops, train
    import inspect
    for name in ("score", "score_psnr", "scored_elements", "fit_sampled", "_capture_guarded"):
        assert callable(getattr(train, name)), name
    sig = inspect.signature(train.fit_sampled)
    for kw in ("rounds", "steps_per_round", "tolerance", "min_delta", "should_reset", "l_mse", "l_js_kl", "l_collisions", "score_step",
               "graph", "poll_every", "exact_final", "after_round"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw
    assert (sig.parameters["score_step"].default, sig.parameters["poll_every"].default) == (1, 16)
    sig = inspect.signature(ops.render_score)
    assert [p for p in sig.parameters][:4] == ["tables", "n_ls", "decoder_params", "image"]
    for kw in ("denom", "step", "sums", "workspace", "vert_idx", "vert_w", "vstride", "leaky", "mode"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw
    assert "zero-collision stop" in train.fit_sampled.__doc__.lower()       # the docstring says that the rule is off
