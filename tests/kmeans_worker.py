"""Inputs of tests/test_kmeans_gpu.py, the raw fp_kmeans call, and -- run as a program -- the GPU worker of its chunk-boundary
case: FP_TEST=kmeans_chunk=.. is read inside the library, so the setting is one run of this file:
    kmeans_worker.py OUT.npz CASE [CASE ..]      (the test sets FP_TEST)
writes cent<niter>_<case> / counts<niter>_<case> for every niter of NITERS and prints KMEANS_WORKER_OK."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NITERS = (0, 1, 4)


def _unit(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)


def case(name):
    """-> (data fp16 [n, dim], k, init_rows int64 [k], seed)"""
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    if name in ("mfma128", "mfma64"):                  # MFMA narrowing, ragged tiles: neither n nor k is a multiple of 128
        data, k = _unit(rng, 5003, 128 if name == "mfma128" else 64), 300
        init = rng.permutation(5003)[:k]
    elif name == "exact48":                            # the exact kernel: a dim the narrowing is not built for
        data, k = _unit(rng, 2003, 48), 37
        init = rng.permutation(2003)[:k]
    elif name == "exact128":                           # ... and a table below 256 centroids
        data, k = _unit(rng, 2003, 128), 100
        init = rng.permutation(2003)[:k]
    elif name == "ties":                               # equal scores: the first index wins, the twin cluster is empty and reseeded
        data, k = _unit(rng, 3001, 64), 260
        data[100:120] = data[0:20]                     # duplicate data rows
        init = rng.permutation(np.arange(200, 3001))[:k]
        init[0] = init[1] = 250                        # the same row named twice
        init[2], init[3] = 7, 107                      # two rows with the same values
        init[4], init[5] = 111, 11
    elif name in ("cap", "chunkcap"):                  # 20 identical initial centroids: more than ASSIGN_CAP = 8 candidates
        n, dim, k = (3001, 128, 300) if name == "cap" else (2500, 64, 256)
        data = _unit(rng, n, dim)
        data[0:20] = data[0]
        init = rng.permutation(np.arange(20, n))[:k]
        init[:20] = np.arange(20)
    elif name == "big":                                # unnormalised values up to about 300
        data, k = rng.uniform(-300, 300, (3001, 128)).astype(np.float16), 300
        init = rng.permutation(3001)[:k]
    elif name == "chunk":                              # n = 2500 under kmeans_chunk=1000: three chunks, the last one short
        data, k = _unit(rng, 2500, 64), 256
        init = rng.permutation(2500)[:k]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(data), int(k), np.ascontiguousarray(init, np.int64), 1234 + len(name)


def call(data, k, niter, init_rows, seed, device=0):
    """fp_kmeans through the binding -> (return code, centroids f32 [k, dim], counts i64 [k])"""
    from fast_plaid_amd import _native as N
    data = np.ascontiguousarray(data, np.float16)
    init_rows = np.ascontiguousarray(init_rows, np.int64)
    cent = np.full((k, data.shape[1]), np.nan, np.float32)
    counts = np.full(k, -7, np.int64)
    vp = lambda a: a.ctypes.data  # noqa: E731
    rc = N.lib().fp_kmeans(device, vp(data), data.shape[0], data.shape[1], k, niter, vp(init_rows), seed, vp(cent), vp(counts))
    return rc, cent, counts


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from fast_plaid_amd import kmeans
    out = {}
    for name in sys.argv[2:]:
        data, k, init, seed = case(name)
        for it in NITERS:
            rc, cent, counts = call(data, k, it, init, seed)
            assert rc == 0, (name, it, rc)
            out[f"cent{it}_{name}"] = cent
            out[f"counts{it}_{name}"] = counts
            if it:
                t = kmeans.last_device_timings()
                out[f"chunks{it}_{name}"] = np.array([t["narrowed_chunks"], t["fallback_chunks"]])
    np.savez(sys.argv[1], **out)
    print("KMEANS_WORKER_OK")
