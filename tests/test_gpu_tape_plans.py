"""The tape planners decide what they decided, and the gradient computes what it computed, on the plans tests/test_gpu_dw_bits.py does not reach: more
than one column block or time segment, the optional tapes, the ensembles' per-model plans (tests/golden/make_tape_plans.py lists the cases).

Checked per case against tests/golden/tape_plans.json: the eight integers of colnde_plan after the first loss_grad, the colnde_describe string, the
SHA-256 digests of `sol` and of loss_grad's result; two loss_grad calls on one handle are bit-identical; everything is finite.

The fixture was recorded on one MI355X from the build of the PARENT commit of the change that added this file (the planners' decisions moved to
csrc/tape_plan.h, fc32 and tile16 kept one planner each for single handles and ensembles; no kernel changed).  It changes only together with an intended
change of a plan or of the arithmetic: then regenerate it with `python tests/golden/make_tape_plans.py` on the new build and say so in that commit."""
import json

import numpy as np
import pytest

from tests.golden import make_tape_plans as R

pytestmark = pytest.mark.gpu

with open(R.PATH) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case_and_plans_reorder_sums():
    assert sorted(GOLDEN) == sorted(R.CASES) and len(R.CASES) == 25
    alone = ["wide/ztape", "fc32/convadj_seg2", "ens_wm/schedule", "ens_conv/seg2"]      # a problem (or a time axis) of their own
    assert sorted([k for g in R.PLAN_GROUPS.values() for k in g] + alone) == sorted(R.CASES)
    for group, names in R.PLAN_GROUPS.items():
        # one problem, one arithmetic: the same solution, and distinct plans gave at least two distinct gradients
        assert len({GOLDEN[k]["sol_sha256"] for k in names}) == 1, group
        assert len({json.dumps(GOLDEN[k]["plan"]) + GOLDEN[k]["describe"] for k in names}) == len(names), group
        assert len({GOLDEN[k]["result_sha256"] for k in names}) >= 2, group
    # the plans the fixture is there for
    plan = {k: GOLDEN[k]["plan"] for k in GOLDEN}
    assert plan["tile16/block16"][1:3] == [16, 2] and plan["netsplit/block16"][1:3] == [16, 2] and plan["regtile/block32"][1:3] == [32, 2]
    assert plan["tile16/inreg"][1:6] == [0, 0, 0, 0, 0] and plan["netsplit/rich"][6] == 7 and plan["netsplit/plain"][6] == 3
    assert plan["regtile/default"][3] == 1 and plan["regtile/ztape0"][3] == 0 and "activation_rows=global_memory" in GOLDEN["wide/ztape"]["describe"]
    assert [plan[k][3] for k in ("fc32/whole", "fc32/seg1", "fc32/seg3", "fc32/block32_seg2", "fc32/convadj_seg2")] == [0, 4, 2, 2, 2]
    assert plan["fc32/block32"][1:3] == [32, 2] and plan["fc32/block32_seg2"][1:3] == [32, 2]
    assert plan["conv/whole"][3] == 0 and plan["conv/seg2"][3] == 2 and plan["conv/seg2"][6] == 3
    assert plan["ens_wm/rich"][6] == 7 and plan["ens_wm/plain"][6] == 3 and "schedule=9/4" in GOLDEN["ens_wm/schedule"]["describe"]
    assert plan["ens_fc/whole"][3] == 0 and plan["ens_fc/seg2"][3] == 2 and plan["ens_conv/seg2"][3] == 2 and plan["ens_conv/seg2"][6] == 3


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_plan_and_bits_against_the_recorded(name):
    sol, (res1, res2), plan, desc = R.run(name, calls=2)
    assert np.isfinite(sol).all() and np.isfinite(res1).all() and np.isfinite(res2).all()
    assert res1.tobytes() == res2.tobytes(), "loss_grad is not run-to-run bit-identical"
    got, want = R.record(sol, res1, plan, desc), GOLDEN[name]
    print("%s: plan %s (recorded %s)\n  %s" % (name, got["plan"], want["plan"], got["describe"]))
    assert got["plan"] == want["plan"]
    assert got["describe"] == want["describe"]
    assert got["sol_sha256"] == want["sol_sha256"], "sol moved"
    assert got["result_sha256"] == want["result_sha256"], "the gradient or the loss moved"
