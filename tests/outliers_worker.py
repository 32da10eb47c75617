"""Inputs of tests/test_centroid_outliers_gpu.py, the raw fp_centroid_outliers call, and -- run as a program -- the GPU worker of
its chunk-boundary case: FP_TEST=outlier_chunk=.. is read inside the library, so the setting is one run of this file:
    outliers_worker.py OUT.npz CASE [CASE ..]      (the test sets FP_TEST)
writes rows_<case> / sqdist_<case> / nearest_<case> / counts_<case> and prints OUTLIERS_WORKER_OK.

Every case is clustered points (a centroid plus noise of a scale drawn per token, so the distances straddle the threshold) with
planted far points."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _clustered(rng, cent32, T, lo, hi, far):
    """T points: centroid + noise of norm uniform in [lo, hi]; a fraction `far` of them replaced by fresh directions of the
    centroids' typical norm"""
    C, dim = cent32.shape
    noise = _unit(rng.standard_normal((T, dim), dtype=np.float32)) * rng.uniform(lo, hi, (T, 1)).astype(np.float32)
    x = cent32[rng.integers(0, C, T)] + noise
    planted = rng.random(T) < far
    scale = float(np.linalg.norm(cent32, axis=1).mean())
    x[planted] = _unit(rng.standard_normal((int(planted.sum()), dim), dtype=np.float32)) * scale
    return x


def case(name):
    """-> (centroids fp16 [C, dim], embeddings fp16 [T, dim], threshold_sq float32)"""
    rng = np.random.default_rng(sum(name.encode()) + 2000)
    shapes = dict(n128=(128, 300, 1000),    # the MFMA narrowing, ragged tiles on both axes
                  n64=(64, 256, 129),       # ... at its smallest table
                  e48=(48, 70, 333),        # the exact kernel: a dim the narrowing is not built for
                  e128=(128, 64, 200),      # ... and a table below 256 centroids
                  cap=(128, 300, 1000),     # 12 identical centroids: more than ASSIGN_CAP = 8 candidates
                  t1=(128, 300, 1), c1=(128, 1, 100), t0=(128, 300, 0),
                  big=(128, 300, 700),      # unnormalised values, |x| about 300
                  zero=(64, 256, 400),      # threshold 0: half of the points ARE centroids
                  chunk=(64, 256, 2500))    # under outlier_chunk=1000: three chunks, the last one short
    dim, C, T = shapes[name]
    if name == "big":
        cent = rng.uniform(-45, 45, (C, dim)).astype(np.float32)
        x = _clustered(rng, cent, T, 20.0, 220.0, 0.1)
        thr = np.float32(140.0 ** 2)
    else:
        cent = _unit(rng.standard_normal((C, dim), dtype=np.float32))
        if name == "cap":
            cent[:12] = cent[0]
        x = _clustered(rng, cent, T, 0.05, 0.9, 0.1)
        if name == "cap":                    # a fifth of the points sit close to the 12 twins
            near = rng.random(T) < 0.2
            x[near] = cent[0] + 0.05 * _unit(rng.standard_normal((int(near.sum()), dim), dtype=np.float32))
        if name == "c1":                     # one centroid: everything else is far
            x = _clustered(rng, cent, T, 0.05, 0.9, 0.3)
        thr = np.float32(0.5 ** 2)
        if name == "zero":
            thr = np.float32(0.0)
    cent16 = np.ascontiguousarray(cent.astype(np.float16))
    x16 = np.ascontiguousarray(x.astype(np.float16))
    if name == "zero":
        same = rng.random(T) < 0.5
        x16[same] = cent16[rng.integers(0, C, int(same.sum()))]
    return cent16, x16, thr


def call(cent, emb, threshold_sq, device=0, want_all=True, n_centroids=None, dim=None):
    """fp_centroid_outliers through the binding -> (return code, rows i64, sqdist f32 [T], nearest i64 [T])"""
    from fast_plaid_amd import _native as N
    cent = np.ascontiguousarray(cent, np.float16)
    emb = np.ascontiguousarray(emb, np.float16)
    T = emb.shape[0]
    rows = np.full(max(T, 1), -7, np.int64)
    sqdist = np.full(max(T, 1), np.nan, np.float32)
    nearest = np.full(max(T, 1), -7, np.int64)
    count = np.full(1, -7, np.int64)
    vp = lambda a: a.ctypes.data  # noqa: E731
    rc = N.lib().fp_centroid_outliers(device, vp(cent), cent.shape[0] if n_centroids is None else n_centroids,
                                      cent.shape[1] if dim is None else dim, vp(emb), T, float(threshold_sq), vp(rows), vp(count),
                                      vp(sqdist) if want_all else None, vp(nearest) if want_all else None)
    n = int(count[0])
    assert rows[n:].tolist() == [-7] * (rows.shape[0] - n) or rc != 0, "rows past *out_count were written"
    return rc, rows[:max(n, 0)].copy(), sqdist[:T], nearest[:T]


def last_counts():
    from fast_plaid_amd import maintain
    return maintain.last_outlier_counts()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    out = {}
    for name in sys.argv[2:]:
        cent, x, thr = case(name)
        rc, rows, sqdist, nearest = call(cent, x, thr)
        assert rc == 0, (name, rc)
        c = last_counts()
        out[f"rows_{name}"], out[f"sqdist_{name}"], out[f"nearest_{name}"] = rows, sqdist, nearest
        out[f"counts_{name}"] = np.array([c["chunks"], c["narrowed_chunks"], c["fallback_chunks"]])
    np.savez(sys.argv[1], **out)
    print("OUTLIERS_WORKER_OK")
