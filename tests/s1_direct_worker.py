"""GPU worker for tests/test_s1_direct_store.py: the streaming S1 kernel's direct write-out (FpS1Exact::direct, FP_TEST=s1_direct)
against the LDS-staged one.  The knob, FP_S1_STREAM, FP_S1_EXACT and FP_APPROX_IMPL are read once per process, so every variant
is one run of this file:  s1_direct_worker.py {trace|search} {a|b} OUT.npz

  trace   (run with FP_S1_EXACT=0) fp_search_trace of one query per shape: the centroid scores S as stored;
  search  fp_search of the batch in its default (lazy) form: checked here against fp_search_trace query by query, and
          written out with the batch's counters for the comparison between the two settings and with the oracle.

Shape group a runs with the default tiling (one tile per workgroup at these sizes): 96 centroids are less than one tile (rows
>= C are never written), 200 leave a tail tile of 72 rows.  Group b runs with FP_S1_STREAM=3: 1152 centroids are nine tiles at
three per workgroup, 1280 are ten whose last workgroup holds one, 200 are two tiles in ONE workgroup, the second partial.  Query
lengths 7 / 32 take the direct path (7: pad columns inside the 32-column group), 33 / 70 (Qp 64 / 128) the staged fallback;
batches of 1 / 3 / 5 / 9 leave B * Qp no multiple of the 128-column tile."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

# (n_centroids, dim, q_len, batch)
SHAPES = {
    "a": ((96, 128, 32, 1), (96, 64, 7, 3), (128, 128, 32, 5), (128, 256, 33, 3), (200, 128, 32, 9), (200, 64, 70, 5),
          (200, 256, 7, 9), (128, 64, 32, 9), (96, 256, 70, 1), (200, 128, 33, 1), (128, 256, 32, 1), (200, 64, 32, 3)),
    "b": ((1152, 128, 32, 5), (1152, 64, 7, 9), (1152, 256, 32, 3), (1280, 128, 32, 9), (1280, 256, 7, 5), (1280, 64, 33, 3),
          (1280, 128, 70, 1), (1152, 128, 33, 9), (200, 128, 32, 3), (1280, 64, 32, 1), (1152, 256, 7, 1)),
}
N_DOCS, DOC_LEN, N_FULL = 2000, 32, 256
TOP_K = N_FULL // 4
# (the lazy form needs the threshold probe, whose cut is the n_probe-th largest 128-centroid chunk maximum of a column: with one
# or two chunks in the table only n_probe = 1 keeps a batch from overflowing the probe's lists and being run again eagerly)
def n_probe(C):
    return 1 if C <= 256 else 4


def corpus(i, C, dim, Q, B):
    """index arrays and the query batch of shape number i (any centroid count: uniform random codes and residual bytes)"""
    import fast_plaid_amd as fp
    rng = np.random.default_rng(1000 + 17 * i + C)
    cent = rng.standard_normal((C, dim), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cent = cent.astype(np.float16)
    lens = np.full(N_DOCS, DOC_LEN, np.int64)
    codes = rng.integers(0, C, size=N_DOCS * DOC_LEN).astype(np.int64)
    res = rng.integers(0, 256, size=(N_DOCS * DOC_LEN, dim * 4 // 8), dtype=np.uint8)
    ivf, ivf_lengths = fp.synth.build_ivf(codes, lens, C)
    bw = fp.synth.bucket_weights(fp.synth.SynthSpec(n_docs=N_DOCS, doc_len=DOC_LEN, n_centroids=128, dim=dim))
    arr = dict(nbits=4, centroids=cent, bucket_weights=bw, ivf=ivf, ivf_lengths=ivf_lengths, doc_codes=codes, doc_residuals=res,
               doc_lengths=lens)
    toks = rng.integers(0, N_DOCS * DOC_LEN, size=(B, Q))
    v = cent[codes[toks]].astype(np.float32) + 0.3 * rng.standard_normal((B, Q, dim), dtype=np.float32) / np.sqrt(dim)
    q = v / np.linalg.norm(v, axis=2, keepdims=True)
    if i % 2 == 1:
        q[0] *= 7.5                       # an unnormalised query (scores beyond the excess table's clamp)
    if B >= 3 or i % 2 == 0:
        q[B - 1, max(Q // 2, 1):] = 0     # a query whose last rows are zero
    return arr, q.astype(np.float16)


def main():
    kind, group, out = sys.argv[1], sys.argv[2], sys.argv[3]
    import fast_plaid_amd as fp
    R = fp.fast_plaid_rust
    R.set_graph_replay(False)   # (a replayed graph reports no counters)
    res = {}
    for i, (C, dim, Q, B) in enumerate(SHAPES[group]):
        arr, q = corpus(i, C, dim, Q, B)
        params = R.SearchParameters(2000, N_FULL, TOP_K, n_probe(C))
        idx = R.construct_index(arr["nbits"], arr["centroids"], None, None, arr["bucket_weights"], arr["ivf"], arr["ivf_lengths"],
                                arr["doc_codes"], arr["doc_residuals"], arr["doc_lengths"], "cuda:0", False)
        if kind == "trace":
            res[f"S{i}"] = R.search_trace(idx, q[0], params)["S"].view(np.uint16)
            continue
        for rep in range(2):   # waited-for, then speculative
            pids, scores, counts = R.search_arrays(idx, q, params)
            lc = R.last_search_counts()
            res[f"lc{i}_{rep}"] = np.array([lc["candidates"], lc["approx_exact"], lc["repaired"], R.last_s1_counts()["lazy"]], np.int64)
            if os.environ.get("S1_DIRECT_VERBOSE"):
                print(i, (C, dim, Q, B), rep, res[f"lc{i}_{rep}"].tolist(), lc["s4_form"], lc["lazy_overflows"], flush=True)
            res[f"pids{i}_{rep}"], res[f"scores{i}_{rep}"], res[f"counts{i}_{rep}"] = pids.copy(), scores.copy(), counts.copy()
        for b in range(B):
            h = R.search_trace(idx, q[b], params)
            assert counts[b] == len(h["pids"]), (i, b, counts[b], len(h["pids"]))
            assert np.array_equal(pids[b, : counts[b]], h["pids"]), (i, b)
            assert np.array_equal(scores[b, : counts[b]], h["scores"]), (i, b)
    np.savez(out, **res)
    print("S1_DIRECT_OK")


if __name__ == "__main__":
    main()
