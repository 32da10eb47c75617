"""GPU worker for tests/test_ivf_mark.py: S3's k_ivf_mark (the probed cells' IVF lists walked as aligned 16-byte vectors into a
per-query document bitmap) against numpy on a CONSTRUCTED corpus.  The knobs FP_TEST=ivf_tw / ivf_maxcells are read once per
process, so every setting is one run of this file:  ivf_mark_worker.py CASE   (the test sets FP_TEST; CASES below)

The reference is numpy, not another kernel: fp_search_trace returns the probed `cells` and the candidates `cand` of a query, and
the expected `cand` is np.unique over the concatenated IVF lists of exactly those cells, taken from the arrays the index was
built from (a cell at or beyond the list count contributes nothing), intersected with the subset where one is given.  On top of
that: check_trace against the C oracle on the same queries, fp_search on the batch against the traces query by query, and the
batch's candidate counter against the sum of the traces' candidate counts.

The corpus: codes are ASSIGNED so that the IVF holds (cell numbers: the constants below)
  the first list of the array (cell 0) and the last, ending on the array's last entry (cell C - 1);
  lists of 1, 2, 3, 4, 5 and 9 entries, starting at offsets 0, 1, 2 and 3 modulo 4 in the array (asserted in corpus());
  empty lists (cells 3, 12 .. 15);
  one list of 9 documents in 10 (more than 4096 entries at 5000 documents: several search levels, several wave-chunks);
  one list holding every document -- so that every document of any other probed list is in several probed lists;
  a list entirely below the first 512-document tile boundary and one entirely above the last.
Query rows are the centroids of exactly these cells, so that the probe selects them, and every case ASSERTS that the cells it
means to exercise are among the returned `cells` before it compares anything else."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

DIM, N_FULL, TOP_K = 64, 256, 64
FIRST, EMPTY, LONG, ALL, BELOW, ABOVE = 0, 3, 8, 9, 10, 11
SIZES = {0: 1, 1: 2, 2: 3, 4: 4, 5: 5, 6: 9, 7: 1}   # cell -> entries of the small lists
N_SPECIAL = 16                                        # cells 0 .. 15 are assigned by hand (3, 12 .. 15 stay empty)

# case -> (FP_TEST the test sets, n_docs, n_centroids, n_probe, queries as lists of cells ("Z": an all-zero query; -1: the last
# cell), query number with a subset or None, tiles the setting gives).  All queries of a case have the same length.
QA = [0, 1, 2, 3, 4, 5, 6, 7]
QB = [LONG, BELOW, ABOVE, -1, LONG, BELOW, ABOVE, -1]
QC = [ALL, EMPTY, 12, -1, FIRST, 5, ALL, ALL]
QD = [6, 7, BELOW, ABOVE, 1, 2, 4, -1]
Q10 = [0, 1, 2, 4, 5, 6, LONG, BELOW, ABOVE, -1]
Q10B = [ALL, EMPTY, 7, 12, 13, 14, 15, 0, 6, -1]
CASES = {
    "default": (dict(), 5000, 256, 2, [QA, QB, QC, "Z", QD], 1, 1),
    "tw16": (dict(ivf_tw=16), 5000, 256, 3, [QA, QB, QC], None, 12),
    "tw20": (dict(ivf_tw=20), 5000, 256, 1, [QB], None, 10),           # 192 words = 9.6 tiles: the last one overhangs W
    "tw64": (dict(ivf_tw=64), 2000, 1152, 4, [QD, QC, QB], None, 1),
    "maxcells3": (dict(ivf_maxcells=3), 5000, 256, 1, [Q10, Q10B, Q10, "Z", Q10B], None, 1),
    "maxcells3_tw16": (dict(ivf_maxcells=3, ivf_tw=16), 5000, 256, 1, [Q10, Q10B, "Z"], 0, 12),
}


def corpus(N, C, seed=7):
    """(index arrays, ivf offsets) of the constructed corpus"""
    import fast_plaid_amd as fp
    rng = np.random.default_rng(seed + N + C)
    cent = rng.standard_normal((C, DIM), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cent = cent.astype(np.float16)
    member = {c: np.sort(rng.choice(N, n, replace=False)) for c, n in SIZES.items()}
    member[FIRST] = np.array([7])
    member[LONG] = np.flatnonzero(np.arange(N) % 10 != 3)
    member[ALL] = np.arange(N)
    member[BELOW] = np.arange(5, 400, 3)
    member[ABOVE] = np.arange(N - 390, N, 2)
    member[C - 1] = np.sort(rng.choice(N, 3, replace=False))
    per_doc = [[] for _ in range(N)]
    for c, docs in member.items():
        for d in docs.tolist():
            per_doc[d].append(c)
    filler = rng.integers(N_SPECIAL, C - 1, size=(N, 3))
    for d in range(N):
        per_doc[d].extend(filler[d].tolist())
    lens = np.array([len(x) for x in per_doc], np.int64)
    codes = np.concatenate([np.asarray(x, np.int64) for x in per_doc])
    res = rng.integers(0, 256, size=(codes.shape[0], DIM * 4 // 8), dtype=np.uint8)
    ivf, ivf_lengths = fp.synth.build_ivf(codes, lens, C)
    off = np.concatenate([[0], np.cumsum(ivf_lengths.astype(np.int64))])
    # the construction holds what the docstring says
    for c, n in SIZES.items():
        assert ivf_lengths[c] == n, (c, ivf_lengths[c])
    assert {int(off[c]) % 4 for c in SIZES} == {0, 1, 2, 3}, [int(off[c]) for c in SIZES]
    assert off[FIRST] == 0 and ivf_lengths[FIRST] > 0 and off[C] == ivf.shape[0] and ivf_lengths[C - 1] == 3
    assert all(ivf_lengths[c] == 0 for c in (EMPTY, 12, 13, 14, 15))
    assert ivf_lengths[ALL] == N and (N < 5000 or ivf_lengths[LONG] > 4096)
    assert member[BELOW].max() < 512 and member[ABOVE].min() >= (N - 1) // 512 * 512
    bw = fp.synth.bucket_weights(fp.synth.SynthSpec(n_docs=N, doc_len=8, n_centroids=128, dim=DIM))
    arr = dict(nbits=4, centroids=cent, bucket_weights=bw, ivf=ivf, ivf_lengths=ivf_lengths, doc_codes=codes, doc_residuals=res,
               doc_lengths=lens)
    return arr, off


def queries(cent, cell_lists):
    C = cent.shape[0]
    Q = max(len(x) for x in cell_lists if x != "Z")
    q = np.zeros((len(cell_lists), Q, DIM), np.float16)
    for b, cl in enumerate(cell_lists):
        if cl != "Z":
            assert len(cl) == Q
            q[b] = cent[[c % C for c in cl]]
    return q


def expected_cand(cells, ivf, off, P, subset):
    lists = [ivf[off[c]: off[c + 1]] for c in cells.tolist() if 0 <= c < P]
    cand = np.unique(np.concatenate(lists)) if lists else np.zeros(0, np.int64)
    if subset is not None:
        cand = np.intersect1d(cand, np.asarray(subset, np.int64))
    return cand.astype(np.int64)


def run(name, arr, off, P, cell_lists, n_probe, sub_q, with_oracle):
    """one index, one batch: numpy reference per query, the oracle, fp_search against the traces, the candidate counter"""
    import fast_plaid_amd as fp
    import plaid_oracle as OC
    from parity import check_trace
    R = fp.fast_plaid_rust
    N, C = arr["doc_lengths"].shape[0], arr["centroids"].shape[0]
    q = queries(arr["centroids"], cell_lists)
    B, Q = q.shape[0], q.shape[1]
    params = R.SearchParameters(2000, N_FULL, TOP_K, n_probe)
    idx = R.construct_index(arr["nbits"], arr["centroids"], None, None, arr["bucket_weights"], arr["ivf"], arr["ivf_lengths"],
                            arr["doc_codes"], arr["doc_residuals"], arr["doc_lengths"], "cuda:0", False)
    orc = None
    if with_oracle:
        orc = OC.OracleIndex(nbits=arr["nbits"], centroids=arr["centroids"], bucket_weights=arr["bucket_weights"], ivf=arr["ivf"],
                             ivf_lengths=arr["ivf_lengths"], doc_codes=arr["doc_codes"], doc_residuals=arr["doc_residuals"],
                             doc_lengths=arr["doc_lengths"])
    subset = None if sub_q is None else np.concatenate([np.arange(0, N, 3), np.arange(N - 40, N)])
    subs = None if sub_q is None else [subset.tolist() if b == sub_q else list(range(N)) for b in range(B)]
    traces = []
    for b, cl in enumerate(cell_lists):
        sub = None if subs is None else subs[b]
        h = R.search_trace(idx, q[b], params, sub)
        if cl != "Z":   # the special cells were probed (a case whose lists were not selected must fail, not pass vacuously)
            want = {c % C for c in cl}
            if sub is not None:   # (a subset confines the probe to the centroids of its documents' codes)
                want = {c for c in want if c < P and np.isin(arr["ivf"][off[c]: off[c + 1]], sub).any()}
            assert want <= set(h["cells"].tolist()), (name, b, sorted(want - set(h["cells"].tolist())))
        exp = expected_cand(h["cells"], arr["ivf"], off, P, sub)
        print(name, "query", b, "cells", len(h["cells"]), "candidates", len(h["cand"]), "expected", len(exp), flush=True)
        assert np.array_equal(h["cand"], exp), (name, b, len(h["cand"]), len(exp), np.setxor1d(h["cand"], exp)[:16])
        if cl != "Z" and ALL in cl and sub is None:
            assert len(exp) == N
        if orc is not None:
            o = orc.search_trace(q[b], TOP_K, N_FULL, n_probe, sub)
            check_trace(h, o, Q, n_probe, N_FULL, TOP_K, strict_cells=cl != "Z")   # (a zero token probes all-tied centroids)
        traces.append(h)
    for rep in range(2):   # waited-for, then speculative
        pids, scores, counts = R.search_arrays(idx, q, params, subs)
        got = R.last_search_counts()["candidates"]
        want = sum(len(h["cand"]) for h in traces)
        print(name, "batch", rep, "candidates", got, "sum of traces", want, flush=True)
        assert got == want, (name, rep, got, want)
        for b, h in enumerate(traces):
            assert counts[b] == len(h["pids"]), (name, b, counts[b], len(h["pids"]))
            assert np.array_equal(pids[b, : counts[b]], h["pids"]), (name, b)
            assert np.array_equal(scores[b, : counts[b]], h["scores"]), (name, b)


def main():
    case = sys.argv[1]
    import fast_plaid_amd as fp
    fp.fast_plaid_rust.set_graph_replay(False)   # (a replayed graph reports no counters)
    opts, N, C, n_probe, cell_lists, sub_q, ntile = CASES[case]
    W = max(((N + 31) // 32 + 63) // 64 * 64, 64)
    if "ivf_tw" in opts:   # the setting gives the tiles the case is about
        assert -(-W // opts["ivf_tw"]) == ntile, (W, opts["ivf_tw"], ntile)
    arr, off = corpus(N, C)
    run(case, arr, off, C, cell_lists, n_probe, sub_q, True)
    if case in ("default", "tw16"):
        # an index with fewer lists than centroids: the probed cells at or beyond the list count contribute nothing.  (The
        # reference errs on such a cell and the oracle with it -- INTEGRATION.md, deviations -- so numpy is the only reference.)
        P = C - 8
        cut = dict(arr, ivf=arr["ivf"][: off[P]].copy(), ivf_lengths=arr["ivf_lengths"][:P].copy())
        run(case + "/short", cut, off, P, [[C - 1, C - 3, LONG, 5, 1, C - 8, P - 1, BELOW], QA], n_probe, None, False)
    print("IVF_MARK_OK")


if __name__ == "__main__":
    main()
