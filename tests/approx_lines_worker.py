"""GPU worker for tests/test_approx_lines_gpu.py: S4's exact kernel fed from the packed code lines (fp_kernels.hip k_approx_lines,
FP_TEST=ap_lines=1, the default) against the uoff / ucodes walk it replaces (ap_lines=0).  The knob, FP_APPROX_IMPL and
FP_S1_EXACT are read once per process, so every variant is one run of this file:  approx_lines_worker.py OUT.npz

Corpora: ~3000 documents whose numbers of DISTINCT codes are constructed -- KINDS below, the piece (6), quad (12 / 24) and line
(48) boundaries of the packed lines, 49 / 60 / 100 for the documents that keep the uoff / ucodes walk, a document without tokens
-- spread among documents of 1 .. 48 distinct codes, so that a wave of the kernel holds both branches.  Every query token sits
next to a code of one of the constructed documents, which makes them candidates.

Each shape runs with two parameter sets:
  wide    n_full 1024 (16 x 256 >= all documents): fp_search_trace's one call of the exact kernel is a wide launch too, so the trace's
          `approx` (the score of EVERY candidate) compares the two kernels document by document between the two settings;
  narrow  n_full 128, FP_TEST=l0_pilot=16: the pilot group (16 x 128 documents) is longer than the 2 x 6 x 32 lane groups the
          grid has per query, so lane groups take a second candidate (the prefetch path); the trace runs the one-quad kernel
          (candidates > 16 x 32), an independent reference for fp_search.
fp_search must equal fp_search_trace bit for bit (asserted here); everything is written out for the comparison between the two
settings and with the oracle."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

KINDS = (0, 1, 5, 6, 7, 12, 13, 24, 25, 47, 48, 49, 60, 100)   # distinct codes of the constructed documents
PER_KIND = 8
N_DOCS, DIM, N_PROBE, TOP_K = 3000, 64, 4, 20
# name -> (n_centroids, q_len, batch)
SHAPES = {
    "q7": (2048, 7, 5),                   # padded columns
    "q32": (4096, 32, 5),
    "q64": (8192, 64, 5),                 # two 32-column chunks: the decoded codes are used twice
    "b1": (2048, 32, 1),
    "ranges": ((1 << 17) + 16, 32, 5),    # two centroid ranges: interleaved 64- or 128-byte lines, the old kernel
}
PARAMS = {"wide": 1024, "narrow": 128}    # n_full_scores


def special_ids():
    """document ids of the constructed documents, by kind: spread over the whole id range"""
    ids = {}
    for j, k in enumerate(KINDS):
        ids[k] = [11 + 26 * (j + len(KINDS) * r) for r in range(PER_KIND)]
    assert max(max(v) for v in ids.values()) < N_DOCS
    return ids


def corpus(name):
    """index arrays and the query batch of a shape"""
    import fast_plaid_amd as fp
    C, Q, B = SHAPES[name]
    rng = np.random.default_rng(4242 + C + 7 * Q + B)
    cent = rng.standard_normal((C, DIM), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cent = cent.astype(np.float16)
    ndist = rng.integers(1, 49, size=N_DOCS)
    sp = special_ids()
    for k, ids in sp.items():
        ndist[ids] = k
    docs = []
    for d in range(N_DOCS):
        own = rng.choice(C, size=int(ndist[d]), replace=False)
        toks = np.concatenate([own, rng.choice(own, size=int(rng.integers(0, 9)))]) if ndist[d] else own
        docs.append(rng.permutation(toks).astype(np.int64))
    lens = np.array([len(t) for t in docs], np.int64)
    codes = np.concatenate(docs)
    res = rng.integers(0, 256, size=(len(codes), DIM * 4 // 8), dtype=np.uint8)
    ivf, ivf_lengths = fp.synth.build_ivf(codes, lens, C)
    bw = fp.synth.bucket_weights(fp.synth.SynthSpec(n_docs=N_DOCS, doc_len=32, n_centroids=128, dim=DIM))
    arr = dict(nbits=4, centroids=cent, bucket_weights=bw, ivf=ivf, ivf_lengths=ivf_lengths, doc_codes=codes, doc_residuals=res,
               doc_lengths=lens)
    # query token (b, t) sits next to a code of a constructed document; the kinds rotate so that a batch reaches all of them
    kinds = [k for k in KINDS if k]
    off = np.concatenate([[0], np.cumsum(lens)])
    pick = np.empty((B, Q), np.int64)
    for b in range(B):
        for t in range(Q):
            n = b * Q + t
            d = sp[kinds[n % len(kinds)]][(n // len(kinds)) % PER_KIND]
            pick[b, t] = codes[off[d] + int(rng.integers(0, lens[d]))]
    v = cent[pick].astype(np.float32) + 0.3 * rng.standard_normal((B, Q, DIM), dtype=np.float32) / np.sqrt(DIM)
    q = (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float16)
    return arr, q, ndist


def main():
    out = sys.argv[1]
    names = sys.argv[2:] or list(SHAPES)
    import fast_plaid_amd as fp
    from fast_plaid_amd import _native as N
    R = fp.fast_plaid_rust
    R.set_graph_replay(False)   # (a replayed graph launches nothing that the counters see)

    def line_launches():
        c = (ctypes.c_int64 * 7)()
        assert N.lib().fp_last_search_counts(ctypes.cast(c, ctypes.c_void_p), 7) == 7
        return int(c[6])

    res, ncmp = {}, 0
    for name in names:
        C, Q, B = SHAPES[name]
        arr, q, ndist = corpus(name)
        idx = R.construct_index(arr["nbits"], arr["centroids"], None, None, arr["bucket_weights"], arr["ivf"], arr["ivf_lengths"],
                                arr["doc_codes"], arr["doc_residuals"], arr["doc_lengths"], "cuda:0", False)
        for pname, n_full in PARAMS.items():
            params = R.SearchParameters(2000, n_full, TOP_K, N_PROBE)
            key = f"{name}_{pname}"
            for rep in range(2):   # waited-for, then speculative
                l0 = line_launches()
                pids, scores, counts = R.search_arrays(idx, q, params)
                l1 = line_launches()
            lc = R.last_search_counts()
            res[f"{key}_pids"], res[f"{key}_scores"], res[f"{key}_counts"] = pids.copy(), scores.copy(), counts.copy()
            res[f"{key}_form"] = np.array([{"exact": 0, "q8": 1, "l0": 2, "l0h": 3}.get(lc["s4_form"], -1), R.last_s1_counts()["lazy"],
                                           lc["candidates"], lc["approx_exact"], l1 - l0], np.int64)
            tl, wide_traces = 0, 0
            for b in range(B):
                t0 = line_launches()
                h = R.search_trace(idx, q[b], params)
                tl += line_launches() - t0
                wide_traces += int(len(h["cand"]) <= 16 * max(n_full // 4, 1))
                assert counts[b] == len(h["pids"]), (key, b, counts[b], len(h["pids"]))
                assert np.array_equal(pids[b, : counts[b]], h["pids"]), (key, b)
                assert np.array_equal(scores[b, : counts[b]], h["scores"]), (key, b)
                ncmp += 2
                res[f"{key}_cand{b}"], res[f"{key}_approx{b}"] = h["cand"], h["approx"]
                res[f"{key}_nd{b}"] = ndist[h["cand"]]   # distinct codes of every candidate
            res[f"{key}_trace"] = np.array([tl, wide_traces], np.int64)
            if os.environ.get("AP_LINES_VERBOSE"):
                print(key, res[f"{key}_form"].tolist(), res[f"{key}_trace"].tolist(), flush=True)
    res["ncmp"] = np.array([ncmp], np.int64)
    np.savez(out, **res)
    print("AP_LINES_OK", ncmp)


if __name__ == "__main__":
    main()
