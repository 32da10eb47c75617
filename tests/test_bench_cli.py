"""bench.py's command line: a plain run times the steps and nothing else, --full adds the passes of their own, --dump-outputs
writes what the last timed step returned.  The GPU cases run the benchmark itself (a fresh process each) on a corpus of 3000
short documents."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import SCORE_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "p50_ms", "p90_ms")
FULL_ONLY = ("repeat_ms_per_step", "value_device_io", "stages_ms", "roofline", "roofline_by_kernel", "cpu_baseline", "parity_vs_cpu")
# odd batch, documents shorter than a tile, more candidates than n_full_scores
SMALL = dict(docs=3000, doc_len=32, batch=5, qlen=32, topk=10, nfull=64, nprobe=4, steps=3, warmup=2)


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
    for k, v in SMALL.items():
        cmd += ["--" + k.replace("_", "-"), str(v)]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "stdout carries exactly one line"
    return json.loads(lines[0])


def test_dump_outputs_formats(tmp_path):
    """ids and counts leave as float64 (exact up to 2^53), scores as float32, under the names of what fp_search returns"""
    sys.path.insert(0, ROOT)
    import bench
    pids = np.array([[7, 2**40 + 1, -1]], dtype=np.int64)
    scores = np.array([[1.5, 0.25, 0.0]], dtype=np.float32)
    counts = np.array([2], dtype=np.int32)
    d = tmp_path / "a" / "b"   # (created on demand)
    bench._dump_outputs(str(d), (pids[:, :3], scores, counts))
    assert sorted(os.listdir(d)) == ["counts.npy", "pids.npy", "scores.npy"]
    got = {n: np.load(d / (n + ".npy")) for n in ("pids", "scores", "counts")}
    assert got["pids"].dtype == np.float64 and np.array_equal(got["pids"].astype(np.int64), pids)
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"], scores)
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"].astype(np.int32), counts)


def test_options_exist(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    """a plain run prints the headline fields and none of --full's; what it dumps is what fp_search returns for the query batch of
    the last timed step (the inputs are seeded: rebuilt here from the same arguments)"""
    out = _bench("--dump-outputs", str(tmp_path / "o"))
    for k in HEADLINE:
        assert k in out, k
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["steps"] == SMALL["steps"] and out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(SMALL["batch"] / (out["ms_per_step"] * 1e-3), rel=1e-9)
    got = {n: np.load(tmp_path / "o" / (n + ".npy")) for n in ("pids", "scores", "counts")}
    assert got["pids"].shape == got["scores"].shape == (SMALL["batch"], SMALL["topk"]) and got["counts"].shape == (SMALL["batch"],)

    import fast_plaid_amd as fp
    R = fp.fast_plaid_rust
    C = fp.synth.default_num_centroids(SMALL["docs"] * SMALL["doc_len"])
    spec = fp.synth.SynthSpec(n_docs=SMALL["docs"], doc_len=SMALL["doc_len"], n_centroids=C, dim=128, nbits=4, seed=42)
    cent, bw = fp.synth.centroids(spec), fp.synth.bucket_weights(spec)
    index = R.construct_synthetic_index(spec, "cuda:0", centroids=cent, bucket_weights=bw)
    q = fp.synth.make_queries(spec, cent, SMALL["batch"], SMALL["qlen"], seed=1000 + SMALL["warmup"] + SMALL["steps"] - 1)
    pids, scores, counts = R.search_arrays(index, q, R.SearchParameters(2000, SMALL["nfull"], SMALL["topk"], SMALL["nprobe"]))
    assert np.array_equal(got["counts"], counts) and counts.min() > 0
    assert np.array_equal(got["pids"], pids)
    assert np.abs(got["scores"] - scores).max() <= SCORE_TOL


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements():
    out = _bench("--full")
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert len(out["repeat_ms_per_step"]) == 5 and out["stages_ms"]["S6+S7 maxsim"] > 0
    assert out["parity_vs_cpu"]["queries"] == SMALL["batch"] and out["parity_vs_cpu"]["max_abs_score_diff"] <= SCORE_TOL
