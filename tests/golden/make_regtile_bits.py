"""Records tests/golden/regtile_bits.json: SHA-256 digests of what the regtile engine computes on the cases of
tests/test_gpu_regtile_bits.py, from the build that is in the tree when this runs (one MI355X).

    python tests/golden/make_regtile_bits.py            # rewrites tests/golden/regtile_bits.json

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

N_COLUMNS, N_FRAMES, SUBSTEPS = 40, 3, 2                     # one full 32-column tile and a ragged 8; 2 x 2 x 4 = 16 stages per tile, 32 in all
WEIGHT_DIVISORS = (1e2, 4.0)                                 # pre-activations of order 0.1 and of order 1: the activation arithmetic shows
ARITHMETICS = ("bf16x3_exact", "f32_mfma")
SCALINGS = (1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3)
PATH = os.path.join(HERE, "regtile_bits.json")


def key(divisor, ma):
    return "div%g/%s" % (divisor, ma)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def run(divisor, ma, calls=1):
    """[(sol, result vector [gradient; terms(6); total])] of `calls` forward + loss_grad rounds on one handle."""
    p = synthetic.wind_mixing_problem(N_COLUMNS, n_frames=N_FRAMES, substeps=SUBSTEPS, weight_divisor=divisor)
    out = []
    with colnde.ColumnNDE(p.cfg, p.n_columns, engine=ENGINE_REGTILE, matrix_arithmetic=ma) as nde:
        assert nde.engine == ENGINE_REGTILE and nde.matrix_arithmetic == ma
        nde.set_problem(p.x0, p.bcs)
        truth = nde.forward(p.weights_truth)
        nde.set_problem(p.x0, p.bcs, truth)
        for _ in range(calls):
            sol = nde.forward(p.weights)
            tot, terms, g = nde.loss_grad(p.weights, SCALINGS)
            out.append((sol, np.concatenate([g, terms, [tot]]).astype(np.float32)))
    return out


def record(sol, res):
    n = res.size - 7
    return {"sol_sha256": sha(sol), "result_sha256": sha(res), "loss_total": float(res[-1]),
            "gradient_norm": float(np.linalg.norm(res[:n].astype(np.float64)))}


if __name__ == "__main__":
    fixture = {key(d, ma): record(*run(d, ma)[0]) for d in WEIGHT_DIVISORS for ma in ARITHMETICS}
    with open(PATH, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(fixture, indent=1, sort_keys=True))
