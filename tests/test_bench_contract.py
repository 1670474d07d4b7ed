"""bench.py keeps the driver's JSON contract (one line on rank 0 with the metric,
roofline and CPU-baseline objects) — tiny runs on the GPU box: one with --full (every leg),
one plain (the timed steps only) that also writes its outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--batch", "128", "--steps", "2",
                        "--warmup", "1", "--cpu-seconds", "0.5", "--cpu-threads", "2", "--parity-seqs", "4"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k, t in [("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int),
                 ("warmup", int), ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str),
                 ("dtype", str), ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)]:
        assert isinstance(d[k], t), k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["value"] > 0 and "vs_baseline" in d
    assert "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert rf["achieved"] > 0 and rf["peak"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert "traffic" in rf
    ps = d["parity_sampled"]
    assert ps["sequences"] == 4 and ps["frames"] == 4 * 4 and ps["mismatches"] == 0, ps
    hf = d["host_fed"]
    assert 0 < hf["value"] < d["value"] and hf["upload_GBps"] > 0
    c = d["counts_per_seq_step"]
    assert c["S_p"] > 0 and c["S_l"] > 0 and c["M_p"] > 0 and c["M_o"] >= c["S_p"]
    assert d["roofline"]["window"] and "traffic_note" in d["roofline"]
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """Without --full: the headline fields only (no leg of its own), D distinct sequences (512, at most
    a chunk: 256 at this batch) copied on the device over a batch that is no multiple of D, and
    --dump-outputs: float arrays within 64 MB in which a sequence and its copies (b, b + D, ...)
    computed the same record."""
    B, D, out = 1200, 256, str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", "2",
                        "--warmup", "1", "--dump-outputs", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert d["metric"] and d["unit"] == "stereo frames/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - B * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("cpu_baseline", "host_fed", "latency_b1", "detection"):
        assert d[k] is None, k
    assert d["parity_sampled"]["sequences"] == 0 and d["cut_search"]["proven_leg"] is None
    assert d["host"]["distinct_sequences_per_rank"] == D and d["host"]["chunk_sequences"] == D
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    n = len(arrs["seq"])
    assert n == 256 and len(set(arrs["seq"])) == n and arrs["Tfw"].shape == (n, 4, 4)
    assert np.isfinite(arrs["Tfw"]).all() and (arrs["n_pt"] > 0).all() and (arrs["n_inliers"] > 0).all()
    assert arrs["pt_P"].shape[1:] == (2048, 3) and arrs["pdesc"].dtype == np.float32
    rec = arrs["step_records"]
    assert rec.shape == (B, 24) and rec.any()
    for s0 in range(D, B, D):
        assert (rec[s0:s0 + D] == rec[:min(D, B - s0)]).all(), s0
    assert len(np.unique(rec[:D], axis=0)) > 1
