"""Records tests/golden/regtile_adjoint_bits.json: SHA-256 digests of what the regtile engine computes on the cases of
tests/test_gpu_regtile_adjoint_bits.py, from the build that is in the tree when this runs (one MI355X).

    python tests/golden/make_regtile_adjoint_bits.py    # rewrites tests/golden/regtile_adjoint_bits.json

regtile_bits.json holds mish with the Z1 tape only.  This one holds the instantiations of rt_adjoint_kernel it leaves out: every activation,
both matrix arithmetics, and the adjoint that recomputes layer 1 from the stage tape (COLNDE_RT_ZTAPE=0: rt_adjoint_kernel<ACT, false, false>).

Run it on the PARENT of a change that must not move the bits, commit the file with the change, and the test holds the change to it.
Run it again only with a change that is meant to alter the arithmetic (and say so in that commit)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import colnde                                                # noqa: E402
from colnde import synthetic                                 # noqa: E402
from colnde.nde import ENGINE_REGTILE                        # noqa: E402

N_COLUMNS = 33                                               # one full 32-column tile and a tile of one column
# (frames, sub-steps): 3 x 2 has a save-point injection between stages and a step boundary inside an interval; 2 x 1 is one step, whose four
# stages are the first and the last of the loop at once.  Both take the same time step, 1/576: RK4 is not stable on this closure with a longer
# one (colnde_min_substeps), so the frames of the one-sub-step case lie half as far apart.
SIZES = ((3, 2), (2, 1))
FRAMES_TOTAL = {2: 289, 1: 577}                              # sub-steps -> frames per unit of time + 1
WEIGHT_DIVISOR = 4.0                                         # pre-activations of order 1: the activation arithmetic reaches the result
ACTIVATIONS = ("identity", "relu", "mish", "swish", "tanh", "leakyrelu")
ARITHMETICS = ("bf16x3_exact", "f32_mfma")
Z1_TAPE = (True, False)                                      # COLNDE_RT_ZTAPE unset / = 0
SCALINGS = (1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3)
PATH = os.path.join(HERE, "regtile_adjoint_bits.json")
CASES = [(a, ma, z, f, s) for a in ACTIVATIONS for ma in ARITHMETICS for z in Z1_TAPE for f, s in SIZES]


def key(act, ma, z1_tape, frames, substeps):
    return "%s/%s/%s/%dx%d" % (act, ma, "z1_tape" if z1_tape else "recompute", frames, substeps)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def run(act, ma, z1_tape, frames, substeps, calls=1):
    """(sol, [result vector [gradient; terms(6); total] of each of `calls` loss_grad calls]) on one fresh handle.  The Z1-tape switch is read
    when the handle plans its tapes, so it is set around the handle's whole life and put back."""
    p = synthetic.wind_mixing_problem(N_COLUMNS, n_frames=frames, substeps=substeps, weight_divisor=WEIGHT_DIVISOR,
                                      n_frames_total=FRAMES_TOTAL[substeps], activations=(act, act, "identity"))
    before = os.environ.get("COLNDE_RT_ZTAPE")
    if z1_tape:
        os.environ.pop("COLNDE_RT_ZTAPE", None)
    else:
        os.environ["COLNDE_RT_ZTAPE"] = "0"
    try:
        with colnde.ColumnNDE(p.cfg, p.n_columns, engine=ENGINE_REGTILE, matrix_arithmetic=ma) as nde:
            assert nde.engine == ENGINE_REGTILE and nde.matrix_arithmetic == ma
            nde.set_problem(p.x0, p.bcs)
            truth = nde.forward(p.weights_truth)
            nde.set_problem(p.x0, p.bcs, truth)
            sol = nde.forward(p.weights)
            res = []
            for _ in range(calls):
                tot, terms, g = nde.loss_grad(p.weights, SCALINGS)
                res.append(np.concatenate([g, terms, [tot]]).astype(np.float32))
            plan = nde.plan()
            assert plan["z1_taped"] == z1_tape and plan["bf16x3_adjoint"] == (z1_tape and ma == "bf16x3_exact"), plan
    finally:
        if before is None:
            os.environ.pop("COLNDE_RT_ZTAPE", None)
        else:
            os.environ["COLNDE_RT_ZTAPE"] = before
    return sol, res


def record(sol, res):
    n = res.size - 7
    return {"sol_sha256": sha(sol), "result_sha256": sha(res), "loss_total": float(res[-1]),
            "gradient_norm": float(np.linalg.norm(res[:n].astype(np.float64)))}


if __name__ == "__main__":
    fixture = {}
    for case in CASES:
        sol, (res,) = run(*case)
        assert np.isfinite(sol).all() and np.isfinite(res).all(), case
        fixture[key(*case)] = record(sol, res)
    with open(PATH, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(fixture, indent=1, sort_keys=True))
