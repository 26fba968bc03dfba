"""The training decoder's instruction schedule may change; what it computes may not, not by a bit.

gngf_decoder_train has no atomics and no memset: everything it writes (rgb, d enc, the per-workgroup slabs of weight and bias
gradients with the max |d enc| word) is a function of the inputs and of the order in which each accumulator receives its
products.  tests/golden/decoder_train_digests.json holds the SHA-256 of those bytes as the commit named in it produced them
(tools/decoder_train_digests.py, which also defines the cases: both TRAIN instantiations, and the pixel counts at which the tile
loop can go wrong — a partial first tile, the lane-half boundary, a partial last tile, a workgroup's second tile, two and three
tiles per workgroup with the prefetches crossing the loop edge).  No tolerance, no quantile."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import decoder_train_digests as dtd  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "decoder_train_digests.json")) as _f:
    GOLDEN = json.load(_f)


def test_golden_covers_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(dtd.case_name(leaky, P) for leaky, P in dtd.cases())
    assert (GOLDEN["in_dim"], GOLDEN["out_dim"]) == (dtd.IN_DIM, dtd.OUT_DIM)


@pytest.mark.parametrize("leaky,P", dtd.cases(), ids=[dtd.case_name(leaky, P) for leaky, P in dtd.cases()])
def test_training_decoder_writes_the_pinned_bytes(leaky, P):
    first = dtd.run_fused(leaky, P)
    again = dtd.run_fused(leaky, P)          # same process, fresh buffers: a stale register crossing the tile loop would show
    got, want = dtd.digests_of(first), GOLDEN["cases"][dtd.case_name(leaky, P)]
    print(dtd.case_name(leaky, P), got)
    for k in dtd.OUTPUTS:
        assert first[k].tobytes() == again[k].tobytes(), f"{k}: two runs of the same build on the same inputs differ"
    if got != want:
        bad = [k for k in dtd.OUTPUTS if got[k] != want[k]]
        pytest.fail(f"{bad} differ from commit {GOLDEN['commit'][:12]} ({GOLDEN['hipcc']}).  Against the two-kernel path — "
                    + dtd.describe_mismatch(leaky, P, first))
