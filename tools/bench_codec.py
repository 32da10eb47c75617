#!/usr/bin/env python3
"""Codec training (create.train_codec with its cluster threshold), the host path against the native one, on the same seeded
input in one process:

    host     fp_compress for the codes, then numpy: the residuals, a sort of n * dim floats, a per-dim mean, einsum norms
    native   fp_residual_stats: residuals, exact histogram, exact per-dim sums and norms on the device; the host reads the order
             statistics from a cumulative sum and sorts n norms

    python tools/bench_codec.py --tokens 50000 --dim 128 --centroids 4096
    python tools/bench_codec.py --tokens 1048576 --dim 128 --centroids 4096 --nbits 2

Prints one JSON line: wall seconds of both paths (each after a small warm-up call that loads the library and the device; both
calls end in a device synchronise), their ratio, and the worst relative differences.  Asserts what the tests assert: cutoffs and
weights equal, avg_residual within 2e-3, the threshold within (2 dim + 4) 2^-24."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sample(n, c, dim, seed):
    """unit-norm fp16 centroids and tokens around them"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((c, dim), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    out = np.empty((n, dim), np.float16)
    step = 1 << 16
    for i in range(0, n, step):
        m = min(step, n - i)
        x = cent[rng.integers(0, c, m)] + 0.3 * rng.standard_normal((m, dim), dtype=np.float32) / np.sqrt(dim)
        out[i: i + m] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return cent.astype(np.float16), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, required=True)
    ap.add_argument("--dim", type=int, required=True)
    ap.add_argument("--centroids", type=int, required=True)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls of each path, alternating; the least wall time is reported")
    args = ap.parse_args()
    from fast_plaid_amd import create
    cent, emb = sample(args.tokens, args.centroids, args.dim, args.seed)
    for native in (False, True):
        create.train_codec(emb[:2048], cent, args.nbits, "cuda:0", with_threshold=True, native=native)
    wall, out = {False: [], True: []}, {}
    for _ in range(args.repeat):
        for native in (False, True):
            t0 = time.perf_counter()
            out[native] = create.train_codec(emb, cent, args.nbits, "cuda:0", with_threshold=True, native=native)
            wall[native].append(time.perf_counter() - t0)
    (cut, wts, avg, thr), (ncut, nwts, navg, nthr) = out[False], out[True]
    assert np.array_equal(ncut, cut) and np.array_equal(nwts, wts)
    avg_rel = float(np.max(np.abs(navg - avg) / np.abs(avg)))
    thr_rel = float(abs(float(nthr) - float(thr)) / float(thr))
    assert avg_rel <= 2e-3 and thr_rel <= (2 * args.dim + 4) * 2.0 ** -24, (avg_rel, thr_rel)
    print(json.dumps(dict(tool="bench_codec", tokens=args.tokens, dim=args.dim, centroids=args.centroids, nbits=args.nbits, seed=args.seed,
                          host_wall_s=round(min(wall[False]), 4), native_wall_s=round(min(wall[True]), 4),
                          host_wall_all_s=[round(w, 4) for w in wall[False]], native_wall_all_s=[round(w, 4) for w in wall[True]],
                          speedup=round(min(wall[False]) / min(wall[True]), 2), cutoffs_and_weights_equal=True, avg_max_rel=avg_rel,
                          threshold_rel=thr_rel)))


if __name__ == "__main__":
    main()
