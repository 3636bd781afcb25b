"""`python bench.py` at N = 1 as a driver runs it: the plain line holds the headline and nothing that takes runs of its own
(those are --full), --steps is the number of timed steps, and --dump-outputs writes what the last timed step returned --
the same fit a caller makes on the same seeded cloud."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(capi, tmp_path):
    from misc3d_amd import synth

    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--points", "200000", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["unit"] == "hypotheses/s"
    assert d["ms_per_step"] > 0 and np.isclose(d["value"], 10_000 * 1e3 / d["ms_per_step"], rtol=1e-9)
    for k in ("metric", "higher_is_better", "dtype", "roofline"):
        assert k in d
    for k in ("cold", "without_kernel_timing_events", "fp64_only", "plane_bound", "setup_ms", "oneshot_ms", "cpu_baseline"):
        assert k not in d, k
    assert "attainable" not in d["roofline"]

    got = {n: np.load(out / f"{n}.npy") for n in ("params", "inliers", "summary")}
    assert all(v.dtype == np.float64 for v in got.values())
    # the bench's workload (C2: plane, 10 000 hypotheses, threshold 0.01, probability 1, sampler seed 11) fitted here directly
    pts = synth.plane_cloud_c2(200000, seed=2)
    with capi.Cloud(pts) as cloud:
        r = cloud.fit(0, 0.01, 10_000, 1.0, seed=11)
    st = r.stats
    assert got["summary"].tolist() == [r.ret, st["best_index"], st["n_inliers"], st["count"], st["iterations"]]
    assert np.array_equal(got["inliers"], r.inliers.astype(np.float64))
    assert np.allclose(got["params"], r.params, rtol=0, atol=1e-12)
    assert d["result"]["best_index"] == st["best_index"] and d["result"]["n_inliers"] == len(r.inliers)
