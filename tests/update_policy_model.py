"""numpy restatement of fp_centroid_outliers (include/fastplaid.h states the arithmetic; this file restates exactly that and nothing
of the product's code -- the product must not import it):

  hn[c]      = 0.5f * ascending-d fp32 chain of cent[c][d]^2                       (kmeans_model.prepare, fp_kmeans step 2)
  score[t,c] = fl32(chain(t, c) - hn[c]), chain = ascending-d fp32 sum of x[t][d] * cent[c][d]
  nearest[t] = argmax_c score[t,c], ties -> lowest c;  s[t] = score[t, nearest[t]]
  x2[t]      = ascending-d fp32 chain of x[t][d]^2
  sqdist[t]  = fl32(x2[t] - 2 s[t])                                                (2 s is exact)
  rows       = ascending t with sqdist[t] > threshold_sq, a strict fp32 compare

and the centroid count an update_centroids call appends (update.py:161-162, fast_plaid.py:109-122 with one-row documents).
"""
import math

import numpy as np

import kmeans_model as KM


def half_norms(cent16: np.ndarray) -> np.ndarray:
    return KM.prepare(np.asarray(cent16, np.float16).astype(np.float32))[1]


def distances(cent16: np.ndarray, x16: np.ndarray):
    """-> (sqdist f32 [T], nearest i64 [T], hn f32 [C])"""
    c = np.asarray(cent16, np.float16).astype(np.float32)
    x = np.asarray(x16, np.float16).astype(np.float32)
    hn = half_norms(cent16)
    T = x.shape[0]
    acc = np.zeros((T, c.shape[0]), np.float32)
    x2 = np.zeros(T, np.float32)
    for d in range(x.shape[1]):
        acc += x[:, d, None] * c[None, :, d]      # fp32: the product of two fp16 values is exact, the addition rounds once
        x2 = x2 + x[:, d] * x[:, d]
    score = acc - hn[None, :]
    nearest = np.argmax(score, axis=1).astype(np.int64) if T else np.zeros(0, np.int64)   # first maximal value = lowest index
    s = score[np.arange(T), nearest]
    sqdist = (x2 - np.float32(2.0) * s).astype(np.float32)
    return sqdist, nearest, hn


def outliers(cent16: np.ndarray, x16: np.ndarray, threshold_sq):
    """-> (rows i64 ascending, sqdist f32 [T], nearest i64 [T])"""
    sqdist, nearest, _ = distances(cent16, x16)
    return np.flatnonzero(sqdist > np.float32(threshold_sq)).astype(np.int64), sqdist, nearest


def threshold_sq(threshold) -> np.float32:
    """what maintain.centroid_outliers passes for a cluster threshold"""
    return np.float32(float(threshold) ** 2)


def k_update(n_out: int, max_points_per_centroid: int = 256) -> int:
    return max(1, 4 * math.ceil(n_out / max_points_per_centroid))


def appended(n_out: int, max_points_per_centroid: int = 256) -> int:
    """centroids appended for n_out outlier rows: K = min(k_update, rows in the sample) and every row is sampled while
    1 + 16 sqrt(120 n) >= n, i.e. for every n_out below about 30 000"""
    if n_out == 0:
        return 0
    assert 1 + int(16 * math.sqrt(120 * n_out)) >= n_out
    return min(k_update(n_out, max_points_per_centroid), n_out)
