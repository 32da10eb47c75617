#!/usr/bin/env python3
"""k-means for index creation, host loop against the native trainer, on the same seeded input:

    kmeans.lloyd         the host loop: per iteration the sample goes up, fp_assign_l2 (exact kernel), labels come back, numpy update
    kmeans.lloyd_device  fp_kmeans: one upload, every iteration on the device (MFMA-narrowed assignment, exact integer sums)

One run = one path at one shape (run them one at a time, each under its own time limit):

    python tools/bench_kmeans.py --shape small --path host        n = 2^21, k = 2^13, dim 128
    python tools/bench_kmeans.py --shape large --path native      n = 2^23, k = 2^16, dim 128

Prints one JSON line: wall seconds of the call (after a tiny warm-up call that loads the library and the device), and for the native
path the HIP-event split of the device time (upload / assign / index / sum / finalise, summed over the iterations)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"small": (1 << 21, 1 << 13, 128), "large": (1 << 23, 1 << 16, 128), "tiny": (1 << 15, 1 << 9, 128)}


def sample(n, k, dim, seed):
    """unit-norm fp16 points around k / 8 random directions (a token sample is clustered, not uniform on the sphere)"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((max(k // 8, 1), dim), dtype=np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    out = np.empty((n, dim), np.float16)
    step = 1 << 18
    for i in range(0, n, step):
        m = min(step, n - i)
        x = centers[rng.integers(0, centers.shape[0], m)] + (0.7 / np.sqrt(dim)) * rng.standard_normal((m, dim), dtype=np.float32)
        out[i: i + m] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--path", choices=["host", "native"], required=True)
    ap.add_argument("--niter", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from fast_plaid_amd import kmeans
    n, k, dim = SHAPES[args.shape]
    t0 = time.perf_counter()
    data = sample(n, k, dim, args.seed)
    t_gen = time.perf_counter() - t0
    warm = data[:2048]
    run = (lambda d, kk, it: kmeans.lloyd(d, kk, it, np.random.default_rng(args.seed), "cuda:0", None)) if args.path == "host" else \
          (lambda d, kk, it: kmeans.lloyd_device(d, kk, it, np.random.default_rng(args.seed), args.seed, "cuda:0", None))
    run(warm, 256, 1)
    t0 = time.perf_counter()
    cent = run(data, k, args.niter)
    wall = time.perf_counter() - t0
    res = dict(tool="bench_kmeans", path=args.path, shape=args.shape, n=n, k=k, dim=dim, niter=args.niter, seed=args.seed,
               wall_s=round(wall, 4), s_per_iter=round(wall / max(args.niter, 1), 4), gen_s=round(t_gen, 2),
               centroid_norm_mean=round(float(np.linalg.norm(cent, axis=1).mean()), 6))
    if args.path == "native":
        res["device_ms"] = {kk: (round(v, 3) if kk != "iterations" else v) for kk, v in kmeans.last_device_timings().items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
