"""fp_centroid_outliers, the device operator behind the update policy's outlier step, against its numpy restatement
(tests/update_policy_model.py): the outlier rows, the squared distances (as uint32 words) and the nearest centroids equal bit for
bit on every path -- the MFMA narrowing with ragged tiles, the exact kernel, an overflowing candidate list, degenerate sizes,
unnormalised data, chunk boundaries -- then the thresholds' edges, the error codes and determinism.  Inputs: tests/outliers_worker.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import outliers_worker as W
import update_policy_model as M
from fptest_env import with_test_opts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL = {}


def _model(name):
    """the model's answer for a case at the case's threshold: computed once, shared by the tests, never modified"""
    if name not in _MODEL:
        cent, x, thr = W.case(name)
        _MODEL[name] = M.outliers(cent, x, thr)
    return _MODEL[name]


def _same(name, rows, sqdist, nearest, want=None):
    want_rows, want_sq, want_near = _model(name) if want is None else want
    print(f"{name}: outliers {rows.shape[0]} (model {want_rows.shape[0]}) of {want_sq.shape[0]}, sqdist words that differ "
          f"{int((sqdist.view(np.uint32) != want_sq.view(np.uint32)).sum())}, nearest that differ {int((nearest != want_near).sum())}")
    assert np.array_equal(nearest, want_near), name
    assert np.array_equal(sqdist.view(np.uint32), want_sq.view(np.uint32)), name
    assert rows.dtype == np.int64 and np.array_equal(rows, want_rows), name


@pytest.fixture(scope="module")
def fp():
    import fast_plaid_amd
    from fast_plaid_amd import _native
    assert _native.lib().fp_device_count() >= 1, "no MI355X visible"
    return fast_plaid_amd


@pytest.mark.parametrize("name", ["n128", "n64", "e48", "e128", "cap", "t1", "c1", "t0", "big"])
def test_bit_identical_to_the_model(fp, name):
    cent, x, thr = W.case(name)
    want_rows, want_sq, want_near = _model(name)
    T = x.shape[0]
    if T >= 20:   # on the model alone: neither "all" nor "none" can pass (t1 and t0 have no room for a fraction)
        assert 0.05 * T <= want_rows.shape[0] <= 0.60 * T, (name, want_rows.shape[0], T)
    rc, rows, sqdist, nearest = W.call(cent, x, thr)
    assert rc == 0, (name, fp._native.last_error())
    _same(name, rows, sqdist, nearest)
    c = W.last_counts()
    print(name, c)
    if name == "t0":
        assert c["chunks"] == 0
    elif name in ("e48", "e128", "c1"):
        assert (c["chunks"], c["narrowed_chunks"], c["fallback_chunks"]) == (1, 0, 0)
    elif name == "cap":
        assert (c["chunks"], c["narrowed_chunks"], c["fallback_chunks"]) == (1, 1, 1)
    else:
        assert (c["chunks"], c["narrowed_chunks"], c["fallback_chunks"]) == (1, 1, 0)
    if name == "cap":    # the 12 identical centroids: everything they attract goes to the first
        assert (want_near == 0).sum() >= 100 and not ((want_near > 0) & (want_near < 12)).any()
    if name == "big":
        assert np.linalg.norm(x.astype(np.float32), axis=1).mean() > 250
    # only the rows and the count: the optional outputs may be absent
    rc, rows2, _, _ = W.call(cent, x, thr, want_all=False)
    assert rc == 0 and np.array_equal(rows2, want_rows)


def test_chunk_boundaries(fp, tmp_path):
    """FP_TEST=outlier_chunk=1000 with T = 2500: three chunks, the last one short; the compaction's offsets carry across them"""
    out = str(tmp_path / "chunk.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "outliers_worker.py"), out, "chunk", "cap"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=with_test_opts(dict(os.environ), outlier_chunk=1000), timeout=600)
    assert p.returncode == 0 and "OUTLIERS_WORKER_OK" in p.stdout, p.stdout[-4000:]
    z = np.load(out)
    want_rows = _model("chunk")[0]
    assert 0.05 * 2500 <= want_rows.shape[0] <= 0.60 * 2500
    assert ((want_rows >= 1000) & (want_rows < 2000)).any() and (want_rows >= 2000).any()   # every chunk contributes
    _same("chunk", z["rows_chunk"], z["sqdist_chunk"], z["nearest_chunk"])
    assert z["counts_chunk"].tolist() == [3, 3, 0], z["counts_chunk"]
    _same("cap", z["rows_cap"], z["sqdist_cap"], z["nearest_cap"])                            # one chunk of 1000: the knob's edge
    assert z["counts_cap"].tolist() == [1, 1, 1], z["counts_cap"]


def test_threshold_edges(fp):
    cent, x, _ = W.case("n128")
    _, sq, near = _model("n128")
    order = np.argsort(sq, kind="stable")
    i = next(i for i in range(order.shape[0] // 2, order.shape[0] - 1) if sq[order[i + 1]] > sq[order[i]])
    row, succ = int(order[i]), int(order[i + 1])
    want = (np.flatnonzero(sq > sq[row]).astype(np.int64), sq, near)
    assert row not in want[0] and succ in want[0]
    rc, rows, sqdist, nearest = W.call(cent, x, sq[row])        # the compare is strict: the chosen row stays out, its successor is in
    assert rc == 0
    _same("n128@row", rows, sqdist, nearest, want)
    assert row not in rows and succ in rows
    rc, rows, sqdist, nearest = W.call(cent, x, np.float32(sq.max()))   # at the largest distance: nothing is above it
    assert rc == 0 and rows.shape[0] == 0
    rc, rows, sqdist, nearest = W.call(cent, x, np.float32(np.inf))
    assert rc == 0 and rows.shape[0] == 0 and np.array_equal(sqdist.view(np.uint32), sq.view(np.uint32))
    # threshold 0 on points half of which ARE centroids (their distance is zero or a few ulps off it, as the model has it)
    cent, x, thr = W.case("zero")
    want = _model("zero")
    assert thr == 0 and 0.05 * x.shape[0] <= want[0].shape[0] <= 0.60 * x.shape[0] and (want[1] <= 0).sum() >= 100
    rc, rows, sqdist, nearest = W.call(cent, x, thr)
    assert rc == 0
    _same("zero", rows, sqdist, nearest)


def test_domain_errors(fp):
    cent, x, thr = W.case("e48")
    assert W.call(cent, x, np.nan)[0] == -1 and "threshold" in fp._native.last_error()                  # FP_EINVAL
    assert W.call(cent, x, -1.0)[0] == -1
    bad = x.copy()
    bad[123, 17] = np.inf
    assert W.call(cent, bad, thr)[0] == -1 and "embeddings" in fp._native.last_error()
    assert W.last_counts() == {}
    cent_n, x_n, _ = W.case("n64")                                                                       # ... met by the narrowing too
    bad_n = x_n.copy()
    bad_n[77, 5] = -np.inf
    assert W.call(cent_n, bad_n, thr)[0] == -1 and "embeddings" in fp._native.last_error()
    badc = cent.copy()
    badc[5, 3] = np.inf
    assert W.call(badc, x, thr)[0] == -1 and "centroids" in fp._native.last_error()
    badc[5, 3] = np.nan
    assert W.call(badc, x, thr)[0] == -1
    assert W.call(np.zeros((4, 300), np.float16), np.zeros((10, 300), np.float16), thr)[0] == -4        # FP_EUNSUPPORTED: dim
    assert W.call(cent, x, thr, n_centroids=0)[0] == -1
    rc, rows, sqdist, nearest = W.call(cent, x, thr)                                                     # and the next call is right
    assert rc == 0
    _same("e48", rows, sqdist, nearest)


def test_deterministic_and_nearest_is_assign_l2s(fp):
    from fast_plaid_amd import _native as N, maintain
    for name in ("n128", "e48", "cap"):
        cent, x, thr = W.case(name)
        a, b = W.call(cent, x, thr), W.call(cent, x, thr)
        assert a[0] == 0 and b[0] == 0 and all(p.tobytes() == q.tobytes() for p, q in zip(a[1:], b[1:])), name
        hn = M.half_norms(cent)
        lab = np.zeros(x.shape[0], np.int64)
        N.check(N.lib().fp_assign_l2(0, cent.ctypes.data, hn.ctypes.data, cent.shape[0], cent.shape[1], x.ctypes.data, x.shape[0], lab.ctypes.data))
        assert np.array_equal(lab, a[3]) and np.array_equal(lab, _model(name)[2]), name
    # the Python wrapper: threshold -> float32(threshold^2)
    cent, x, _ = W.case("n64")
    rows, sqdist, nearest = maintain.centroid_outliers(cent, x, 0.37)
    _same("n64@0.37", rows, sqdist, nearest, M.outliers(cent, x, M.threshold_sq(0.37)))
