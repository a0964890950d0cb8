"""The bits of the regtile engine's results did not move.

A change that only re-expresses the kernels' arithmetic (the same operations in the same order on other instructions) must leave every bit of
`forward` and `loss_grad` where it was; the tolerance tests against the oracle cannot see a last-bit difference, this file sees nothing else.
ENGINE_REGTILE at 40 columns (one full 32-column tile and a ragged 8: both 16-column halves of the forward kernel, the `valid` masks, a
half-empty tile) x 3 frames x 2 sub-steps, MPP physics and mish, weights / 1e2 and weights / 4 (pre-activations of order 0.1 and 1, so that the
activation arithmetic reaches the result), both matrix arithmetics.  Checked: two rounds on one handle are bit-identical, and the SHA-256
digests of `sol` and of the result vector [gradient; loss terms; total] equal tests/golden/regtile_bits.json.

The fixture was recorded on one MI355X from the build of the PARENT commit of the change that added this file.  It changes only together with
an intended change of the engine's arithmetic: then regenerate it with `python tests/golden/make_regtile_bits.py` on the new build and say so
in that commit.  Correctness stays with the oracle tests (tests/test_gpu_parity.py, tests/test_gpu_z1_tape_record.py)."""
import json

import numpy as np
import pytest

from tests.golden import make_regtile_bits as R

pytestmark = pytest.mark.gpu

with open(R.PATH) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(R.key(d, ma) for d in R.WEIGHT_DIVISORS for ma in R.ARITHMETICS)


@pytest.mark.parametrize("ma", R.ARITHMETICS)
@pytest.mark.parametrize("divisor", R.WEIGHT_DIVISORS)
def test_bits_against_recorded_digests(divisor, ma):
    (sol1, res1), (sol2, res2) = R.run(divisor, ma, calls=2)
    assert np.isfinite(sol1).all() and np.isfinite(res1).all()
    assert sol1.tobytes() == sol2.tobytes(), "forward is not run-to-run bit-identical"
    assert res1.tobytes() == res2.tobytes(), "loss_grad is not run-to-run bit-identical"
    got, want = R.record(sol1, res1), GOLDEN[R.key(divisor, ma)]
    print("div %g %s: loss %.9e (recorded %.9e), |gradient| %.9e (recorded %.9e)" % (divisor, ma, got["loss_total"], want["loss_total"],
                                                                                     got["gradient_norm"], want["gradient_norm"]))
    assert got["sol_sha256"] == want["sol_sha256"], "sol moved"
    assert got["result_sha256"] == want["result_sha256"], (got["loss_total"], want["loss_total"], got["gradient_norm"], want["gradient_norm"])
