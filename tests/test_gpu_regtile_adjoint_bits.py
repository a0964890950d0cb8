"""The bits of every instantiation of the regtile adjoint did not move, and do not move from call to call.

tests/test_gpu_regtile_bits.py holds mish, MPP and the Z1 tape.  This file holds what it leaves out of rt_adjoint_kernel<ACT, ZT, SPLIT>: all six
activations, both matrix arithmetics, and COLNDE_RT_ZTAPE unset and = 0 (a fresh handle each, so that <ACT, false, false> — the adjoint that
recomputes layer 1 from the stage tape — runs).  ENGINE_REGTILE at 33 columns (a full tile and a tile of one column), 3 frames x 2 sub-steps
(a save-point injection between stages, a step boundary inside an interval) and 2 frames x 1 sub-step (one step: the first and the last stage
of the loop; its frames lie half as far apart, so that both sizes take the time step 1/576 — RK4 is not stable on this closure with a longer
one).  Checked per case: the SHA-256 digests of `sol` and of the result vector [gradient; loss terms; total] equal
tests/golden/regtile_adjoint_bits.json, three loss_grad calls on one handle are bit-identical, everything is finite.

The run-to-run identity is what catches a tape load that is consumed before it has landed: a change that only moves where the adjoint's loads
are issued and waited for must pass it, and its digests are the parent's.

The fixture was recorded on one MI355X from the build of the PARENT commit of the change that added this file.  It changes only together with
an intended change of the engine's arithmetic: then regenerate it with `python tests/golden/make_regtile_adjoint_bits.py` on the new build and
say so in that commit."""
import json

import numpy as np
import pytest

from tests.golden import make_regtile_adjoint_bits as R

pytestmark = pytest.mark.gpu

with open(R.PATH) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(R.key(*c) for c in R.CASES)
    assert len(R.CASES) == 6 * 2 * 2 * 2


@pytest.mark.parametrize("frames,substeps", R.SIZES)
@pytest.mark.parametrize("z1_tape", R.Z1_TAPE)
@pytest.mark.parametrize("ma", R.ARITHMETICS)
@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_adjoint_bits_against_recorded_digests(act, ma, z1_tape, frames, substeps):
    sol, (res1, res2, res3) = R.run(act, ma, z1_tape, frames, substeps, calls=3)
    assert np.isfinite(sol).all() and np.isfinite(res1).all() and np.isfinite(res2).all() and np.isfinite(res3).all()
    assert res1.tobytes() == res2.tobytes() == res3.tobytes(), "loss_grad is not run-to-run bit-identical"
    got, want = R.record(sol, res1), GOLDEN[R.key(act, ma, z1_tape, frames, substeps)]
    print("%s: loss %.9e (recorded %.9e), |gradient| %.9e (recorded %.9e)" % (R.key(act, ma, z1_tape, frames, substeps), got["loss_total"],
                                                                             want["loss_total"], got["gradient_norm"], want["gradient_norm"]))
    assert got["sol_sha256"] == want["sol_sha256"], "sol moved"
    assert got["result_sha256"] == want["result_sha256"], (got["loss_total"], want["loss_total"], got["gradient_norm"], want["gradient_norm"])
