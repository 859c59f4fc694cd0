"""bench.py --dump-outputs: after the timed steps the verdict and transcript digest of the LAST timed step are written as
float32 .npy files, and two runs with the same arguments write the same arrays (the inputs come from the seed alone), so
that two builds of the project can be compared output for output.  A run without --full measures the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, detail):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--participants", "4096",
           "--threshold", "64", "--cpu-sample", "0", "--wb-shares", "0", "--registered-keys", "0", "--ec-boxes", "0", "--lone-boxes", "0",
           "--host-boxes", "0", "--config-boxes", "0", "--drop-in-threads", "0", "--steady-steps", "0", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, MPVSS_BENCH_DETAIL=str(detail)))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{\"metric\"")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_of_the_last_timed_step_are_reproducible(tmp_path):
    dumps = []
    for k in range(2):
        res = _bench(tmp_path / f"run{k}", tmp_path / f"detail{k}.json")
        assert res["steps"] == 5 and res["ms_per_step"] > 0
        assert res["value"] == pytest.approx(4096 * 1e3 / res["ms_per_step"], rel=1e-4)
        assert sorted(os.listdir(tmp_path / f"run{k}")) == ["digest.npy", "verdict.npy"]
        verdict = np.load(tmp_path / f"run{k}" / "verdict.npy")
        digest = np.load(tmp_path / f"run{k}" / "digest.npy")
        assert verdict.dtype == np.float32 and verdict.tolist() == [1.0]
        assert digest.dtype == np.float32 and digest.shape == (32,)
        assert np.all((digest >= 0) & (digest <= 255) & (digest == np.round(digest))) and digest.any()
        dumps.append(digest)
    assert np.array_equal(dumps[0], dumps[1])


def test_a_plain_run_measures_the_headline_only(tmp_path):
    """Without --full every secondary leg stays off even with its own options at their defaults: no object of those legs in
    the result, no steady state, no issue-rate probe, and the roofline read from the overlapped launches of the timed steps."""
    detail = tmp_path / "detail.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--participants", "4096",
           "--threshold", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, MPVSS_BENCH_DETAIL=str(detail)))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.load(open(detail))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["value"] == pytest.approx(4096 * 1e3 / res["ms_per_step"], rel=1e-4)
    for leg in ("verify_share", "extract_shares", "distribute", "cpu_baseline", "configs", "strong", "host_buffers", "one_call",
                "drop_in", "registered_keys", "ec", "secondary_error"):
        assert leg not in res, leg
    assert res["value_steady_state"] is None and res["compute"]["sustained_probe"] is None
    assert res["roofline"]["kernel_ms_is"] == "overlapped launch (timed region)"
