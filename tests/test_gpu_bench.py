"""bench.py end to end on the GPU, the way the driver runs it: a plain run prints the result line for exactly the steps it was given,
and --dump-outputs writes what the timed path returned in its last step -- the same arrays in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    d = 1024   # the default workload: the north star, full-rank (mu, C) -> params_len = d + d^2
    lines = [_bench(tmp_path / k, 30, 3) for k in ("a", "b")]
    for line in lines:
        assert line["metric"] == "ELBO-grad-estimates/sec" and line["unit"] == "estimates/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 30 and line["warmup"] == 3
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-4)
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["also"] is None   # the non-headline legs are --full only
    out = [{n: np.load(tmp_path / k / (n + ".npy")) for n in ("value", "grad")} for k in ("a", "b")]
    for o in out:
        assert o["value"].dtype == np.float32 and o["value"].shape == (1,)
        assert o["grad"].dtype == np.float32 and o["grad"].shape == (d + d * d,)
        assert np.isfinite(o["value"]).all() and np.isfinite(o["grad"]).all() and np.linalg.norm(o["grad"]) > 0
    # same arguments -> same estimate indices -> the same last estimate (to rounding)
    assert abs(float(out[0]["value"][0]) - float(out[1]["value"][0])) <= 1e-6 * abs(float(out[1]["value"][0]))
    assert np.linalg.norm(out[0]["grad"].astype(np.float64) - out[1]["grad"]) <= 1e-6 * np.linalg.norm(out[1]["grad"].astype(np.float64))
