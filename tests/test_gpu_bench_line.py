"""bench.py end to end on the GPU (VERDICT r4 task 1): stdout is ONE line, it parses as strict JSON, it is far below 8 KB and carries `roofline` and
`cpu_baseline` — with --full and the side configs on (the block that made round 4's line 25 KB), at a reduced size so that the test stays short.
A plain run (no --full) carries the same contract keys with nothing measured beyond the headline, and --dump-outputs writes what its last timed
step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_compact_parsable_line(tmp_path):
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--columns", "4096", "--frames", "33", "--full"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    assert len(lines[0]) < 8192
    line = json.loads(lines[0], parse_constant=lambda c: pytest.fail("non-strict JSON constant %s" % c))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["dtype"] == "f32"
    assert line["config"]["columns_per_gpu"] == 4096 and line["config"]["frames"] == 33
    rf, cb = line["roofline"], line["cpu_baseline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and rf["avg_launch_ms"] > 0 and rf["launches"] == 2 and rf["unit"] == "TFLOP/s"
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "oracle/colnde_ref.c" in cb["sample"]
    assert line["self_check"]["ok"] is True
    sc = line["side_configs_ms"]
    assert sc["errors"] is None and sc["config4_shard_ms"] > 0 and sc["config3_8sim_ms"] > 0 and sc["wide_wind_mixing_4096x32steps_ms"] > 0
    # the full record went to a file, not to stdout / stderr
    full = json.load(open(os.path.join(ROOT, "gpurun_out", "bench_full.json")))
    assert "configs" in full and len(json.dumps(full)) > len(lines[0])
    assert len(r.stderr) < 16384


def test_plain_run_measures_only_the_headline_and_dumps_its_last_timed_step(tmp_path):
    import torch
    import colnde
    from colnde import synthetic
    dump = tmp_path / "dump"
    ncol, frames, steps = 1024, 17, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--columns", str(ncol), "--frames", str(frames),
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    line = json.loads(lines[0], parse_constant=lambda c: pytest.fail("non-strict JSON constant %s" % c))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == 1 and line["roofline"]["launches"] == steps and line["ms_per_step"] > 0
    # value is the column-timesteps of one step over the milliseconds of one timed step (both rounded to 6 digits on the line)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (ncol * 2 * (frames - 1)) - 1) < 1e-4
    assert line["cpu_baseline"] is None and line["opt_out"] is None and line["self_check"] is None and line["full_record"] is None
    assert line["roofline"]["clock"] is None and "side_configs_ms" not in line
    assert sorted(os.listdir(dump)) == ["gradient.npy", "loss_terms.npy", "loss_total.npy"]
    g, terms, tot = (np.load(dump / (n + ".npy")) for n in ("gradient", "loss_terms", "loss_total"))
    assert g.dtype == terms.dtype == tot.dtype == np.float32 and terms.shape == (6,) and tot.shape == (1,)
    # the same seeded inputs through a handle of this process: what the bench's timed step hands its caller
    dev = torch.device("cuda", 0)
    p = synthetic.wind_mixing_problem(ncol, n_frames=frames, substeps=2, seed=synthetic.SEED)
    wp = synthetic.wind_mixing_problem(1, n_frames=2, seed=synthetic.SEED)
    x0, bcs = torch.from_numpy(p.x0).to(dev), torch.from_numpy(p.bcs).to(dev)
    w, wt = torch.from_numpy(wp.weights).to(dev), torch.from_numpy(wp.weights_truth).to(dev)
    with colnde.ColumnNDE(p.cfg, ncol) as nde:
        nde.set_global_columns(ncol)
        nde.set_problem(x0, bcs)
        truth = nde.forward(wt)
        nde.set_problem(x0, bcs, truth)
        res = nde.loss_grad(w, [1.0, 1.0, 1.0, 5e-3, 5e-3, 5e-3]).cpu().numpy()
    npar = p.cfg.n_params
    assert g.shape == (npar,) and np.isfinite(g).all() and tot[0] > 0
    np.testing.assert_allclose(terms, res[npar:npar + 6], rtol=1e-6, atol=0)
    np.testing.assert_allclose(tot, res[npar + 6:npar + 7], rtol=1e-6, atol=0)
    assert np.linalg.norm(g.astype(np.float64) - res[:npar]) <= 1e-6 * np.linalg.norm(res[:npar].astype(np.float64))
