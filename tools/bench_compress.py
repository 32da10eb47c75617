"""Throughput of fp_compress (exact nearest-centroid assignment + residual packing) at index-build sizes.
    bench_compress.py                                     dim 128, C = 2^13 and 2^17, T = 2^18 (one timed call each)
    bench_compress.py --dim 96 --centroids 8192 --tokens 262144 [--repeat 5] [--dump OUT.npz]
With a shape given it also prints the chunk counts and device times of fp_compress_last_counts.  FP_TEST=assign_exact=1 forces
the all-VALU kernel, FP_TEST=assign_sliced=1 sends dim 64 / 128 through the K-sliced MFMA kernel."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import fast_plaid_amd as fp
from fast_plaid_amd import create as CR

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--centroids", type=int, default=0)
ap.add_argument("--tokens", type=int, default=1 << 18)
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--dump", default="")
a = ap.parse_args()
D = a.dim
for C, T in ((a.centroids, a.tokens),) if a.centroids else ((8192, a.tokens), (131072, a.tokens)):
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((C, D), dtype=np.float32); cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    emb = cent[rng.integers(0, C, T)] + 0.03 * rng.standard_normal((T, D), dtype=np.float32)
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float16)
    cut = np.linspace(-0.05, 0.05, 15).astype(np.float16)
    CR.compress(cent, cut, emb[:4096], 4)
    for _ in range(a.repeat):
        t = time.perf_counter(); codes, res = CR.compress(cent, cut, emb, 4); dt = time.perf_counter() - t
        print("C=%d T=%d: %.3f s  %.2f Mtok/s  %.1f TFLOP/s useful (2 T C D / time; FP_TEST=assign_exact=1 forces the all-VALU kernel)" % (C, T, dt, T / dt / 1e6, 2.0 * T * C * D / dt / 1e12))
        if a.centroids:
            n = CR.last_compress_counts()
            if n:
                print("  dim=%d chunks=%d narrowed=%d fallback=%d assign_us=%d pack_us=%d  %.1f TFLOP/s useful over the assignment; candidates per token "
                      "mean %.3f max %d (FP_TEST=assign_stats=1, else 0)" % (D, n["chunks"], n["narrowed_chunks"], n["fallback_chunks"], n["assign_us"],
                      n["pack_us"], 2.0 * T * C * D / max(n["assign_us"], 1) / 1e6, n["cand_sum"] / T, n["cand_max"]))
    if a.dump:
        np.savez(a.dump, codes=codes, res=res)
