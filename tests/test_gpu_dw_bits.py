"""The bits of loss_grad did not move on any way through the taped weight-gradient GEMM (csrc/engine_dwgemm.hip) and its plan (csrc/dw_plan.h).

One case per path (tests/golden/make_dw_bits.py names the existing test each configuration is taken from):
  tile16/lds, /l2stream, /split     tile16's taped adjoint at 21 columns (two tiles, one ragged): the LDS-staged f32 kernel, the L2-streaming one
                                    (COLNDE_T16_DWLDS=0) and the bf16 split kernel
  fc32/<arithmetic>                 the free-convection engine at Nz = 32, one 32-column tile
  wide/<arithmetic>                 3 x (96-400-400-31) at 16 columns and one save interval: the records do not fit the LDS — split passes over chunks of
                                    the 400 x 400 matrices, or the f32 kernel streaming from L2
  ensemble/<arithmetic>             K = 2 wind-mixing models at 8 columns (model index in the launch grid, per-model strides)
Checked per case: the SHA-256 digests of `sol` and of the result (gradient, loss terms, total) equal tests/golden/dw_bits.json, two loss_grad calls
on one handle are bit-identical, everything is finite.

The fixture was recorded on one MI355X from the build of the PARENT commit of the change that added this file (the dW GEMM moved to its own
translation unit with no kernel changed, the plan moved to the host header).  It changes only together with an intended change of the arithmetic or of
the plan's slice counts (the reduction order): then regenerate it with `python tests/golden/make_dw_bits.py` on the new build and say so in that commit."""
import json

import numpy as np
import pytest

from tests.golden import make_dw_bits as R

pytestmark = pytest.mark.gpu

with open(R.PATH) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(R.CASES) and len(R.CASES) == 9
    # the three tile16 kernels and the two arithmetics did run different code: the same solution, different sums
    assert len({GOLDEN[k]["sol_sha256"] for k in ("tile16/lds", "tile16/l2stream", "tile16/split")}) == 1
    assert len({GOLDEN[k]["result_sha256"] for k in GOLDEN}) == len(GOLDEN)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_dw_bits_against_recorded_digests(name):
    sol, (res1, res2) = R.run(name, calls=2)
    assert np.isfinite(sol).all() and np.isfinite(res1).all() and np.isfinite(res2).all()
    assert res1.tobytes() == res2.tobytes(), "loss_grad is not run-to-run bit-identical"
    got, want = R.record(sol, res1), GOLDEN[name]
    print("%s: loss %.9e (recorded %.9e), |gradient| %.9e (recorded %.9e)" % (name, got["loss_total"], want["loss_total"], got["gradient_norm"],
                                                                             want["gradient_norm"]))
    assert got["sol_sha256"] == want["sol_sha256"], "sol moved"
    assert got["result_sha256"] == want["result_sha256"], (got["loss_total"], want["loss_total"], got["gradient_norm"], want["gradient_norm"])
