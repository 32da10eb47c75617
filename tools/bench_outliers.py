#!/usr/bin/env python3
"""Outliers of a centroid table (the update policy's hot step), the device operator against the only other route to the same
answer, on the same seeded input:

    native   maintain.centroid_outliers: fp_centroid_outliers -- the embeddings go up in chunks, MFMA-narrowed assignment, distance
             and ordered compaction on the device, the outlier rows come back
    host     kmeans.assign_l2 (fp_assign_l2: the exact kernel, the labels come back), then distance and threshold in numpy

One run = both paths at one shape, one after the other in one process (the same input, the same machine):

    python tools/bench_outliers.py --shape small      2^20 tokens x 2^13 centroids, dim 128
    python tools/bench_outliers.py --shape large      2^22 tokens x 2^16 centroids, dim 128

Prints one JSON line: wall seconds of each path (after a tiny warm-up call that loads the library and the device), the outlier
counts of both, and for the native path the HIP-event split of its device time (upload + data check / assignment / distance +
compaction / download, summed over the chunks) with each part's share of the call's wall time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"small": (1 << 20, 1 << 13, 128), "large": (1 << 22, 1 << 16, 128), "tiny": (1 << 15, 1 << 9, 128)}


def sample(n, c, dim, seed):
    """unit-norm fp16 centroids, and tokens around them with noise of a scale drawn per token (so the distances straddle the
    threshold) -- a tenth of the tokens are fresh directions, the drift"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((c, dim), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    out = np.empty((n, dim), np.float16)
    step = 1 << 18
    for i in range(0, n, step):
        m = min(step, n - i)
        noise = rng.standard_normal((m, dim), dtype=np.float32) * (rng.uniform(0.05, 0.9, (m, 1)).astype(np.float32) / np.sqrt(dim))
        x = cent[rng.integers(0, c, m)] + noise
        far = rng.random(m) < 0.1
        x[far] = rng.standard_normal((int(far.sum()), dim), dtype=np.float32)
        out[i: i + m] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return cent.astype(np.float16), out


def host_route(cent, emb, threshold):
    from fast_plaid_amd import kmeans
    labels = kmeans.assign_l2(cent, emb)
    c32 = cent.astype(np.float32)
    c2 = np.einsum("ij,ij->i", c32, c32)
    thr = np.float32(threshold) ** 2
    rows = []
    step = 1 << 18
    for i in range(0, emb.shape[0], step):
        x = emb[i: i + step].astype(np.float32)
        lab = labels[i: i + step]
        d = np.einsum("ij,ij->i", x, x) + c2[lab] - 2.0 * np.einsum("ij,ij->i", x, c32[lab])
        rows.append(i + np.flatnonzero(d > thr))
    return np.concatenate(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from fast_plaid_amd import maintain
    n, c, dim = SHAPES[args.shape]
    t0 = time.perf_counter()
    cent, emb = sample(n, c, dim, args.seed)
    t_gen = time.perf_counter() - t0
    maintain.centroid_outliers(cent[:256], emb[:2048], args.threshold, rows_only=True)
    host_route(cent[:256], emb[:2048], args.threshold)
    t0 = time.perf_counter()
    rows, _, _ = maintain.centroid_outliers(cent, emb, args.threshold, rows_only=True)
    wall_native = time.perf_counter() - t0
    counts = maintain.last_outlier_counts()
    t0 = time.perf_counter()
    rows_host = host_route(cent, emb, args.threshold)
    wall_host = time.perf_counter() - t0
    dev = {k: round(counts[k] / 1000.0, 3) for k in ("upload_us", "assign_us", "outlier_us", "download_us")}
    res = dict(tool="bench_outliers", shape=args.shape, n=n, c=c, dim=dim, threshold=args.threshold, seed=args.seed, gen_s=round(t_gen, 2),
               native_wall_s=round(wall_native, 4), host_wall_s=round(wall_host, 4), speedup=round(wall_host / wall_native, 2),
               outliers_native=int(rows.shape[0]), outliers_host=int(rows_host.shape[0]),
               rows_only_in_one=int(np.setxor1d(rows, rows_host).shape[0]),   # numpy's distance rounds elsewhere: the edge may differ
               chunks=counts["chunks"], narrowed_chunks=counts["narrowed_chunks"], fallback_chunks=counts["fallback_chunks"],
               device_ms={k[:-3]: v for k, v in dev.items()},
               device_ms_per_chunk={k[:-3]: round(v / max(counts["chunks"], 1), 3) for k, v in dev.items()},
               share_of_wall={k[:-3]: round(v / 1000.0 / wall_native, 4) for k, v in dev.items()},
               assign_ns_per_point=round(counts["assign_us"] * 1000.0 / n, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
