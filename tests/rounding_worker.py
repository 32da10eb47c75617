"""GPU worker for tests/test_rounding_boundaries_gpu.py: the constructed fp16 rounding-boundary fixtures of tests/golden/rounding
(make_rounding_fixtures.py there) on the device, against the C oracle bit for bit.  FP_S1_EXACT, FP_S1_STREAM, FP_S1_STATS,
FP_MAXSIM_REPAIR and FP_TEST are read once per process, so every variant is one run of this file:

    rounding_worker.py FAMILY [FAMILY ...]

Per family, every check runs even after another has failed; the last line printed is  ROUNDING_RESULT {json}  with, per family,
the failed checks (name -> message) and the S1 counters summed over the traced queries.  The checks:

  trace     fp_search_trace (the eager form: S certified and repaired inside S1) of every query: S, cells, candidates, approximate
            scores and the rerank list equal the oracle's bit for bit (parity.check_trace), for n_ivf_probe 1 and 4.  Strict cells,
            except in family A: its small integers make exact ties across the probe cut in every query, and there only a tie
            excuses other cells.  check_trace stops comparing where the cells (or, at an exact tie of the approximate score, the
            rerank lists) differ, so the traces that WERE compared to the end are counted: traces / cells_same / rerank_same
  search    fp_search of the batch returns what the traces return, bit for bit, and the oracle's ids; lazy_p1 / lazy_p4 report the
            form S1 ran in (fp_last_s1_counts: 1 lazy, 0 eager -- also when a lazy batch raised a flag and was run again eagerly)
  columns   fp_maxsim_columns over ALL documents: a column maximum that differs from the oracle's is flagged
  repair    with FP_MAXSIM_REPAIR=2 in the environment: every returned score equals the oracle's exact score bit for bit"""
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fast_plaid_amd as fp  # noqa: E402
import plaid_oracle as OC  # noqa: E402
from parity import check_final, check_trace, ulp_diff_f16  # noqa: E402

R = fp.fast_plaid_rust
ROUNDING_DIR = os.path.join(ROOT, "tests", "golden", "rounding")
INDEX_KEYS = ("centroids", "bucket_weights", "ivf", "ivf_lengths", "doc_codes", "doc_residuals", "doc_lengths")
# n_full_scores: the rerank list (a quarter of it) cuts inside the documents that hold the near-copies (300 documents at most)
N_FULL, PROBES = 64, (1, 4)
TOP_K = N_FULL // 4


def load(name):
    z = np.load(os.path.join(ROUNDING_DIR, name + ".npz"))
    a = {k: z[k] for k in z.files}
    hip = R.construct_index(int(a["nbits"]), a["centroids"], None, None, a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_codes"],
                            a["doc_residuals"], a["doc_lengths"], "cuda:0", False)
    orc = OC.OracleIndex(nbits=int(a["nbits"]), **{k: a[k] for k in INDEX_KEYS})
    return a, hip, orc


def run_family(name):
    a, hip, orc = load(name)
    q = a["queries"]
    B, Q = q.shape[0], q.shape[1]
    fails, s1 = {}, dict(flagged=0, changed=0, slow_path=0, unflagged_differences=0)
    cmp = dict(traces=0, cells_same=0, rerank_same=0)
    strict = name != "family_a"
    traces = {}

    def check(label, fn):
        try:
            fn()
        except Exception as e:   # noqa: BLE001  (reported to the test, with the first lines of the message)
            fails[label] = (str(e) or traceback.format_exc())[:600]

    for n_probe in PROBES:
        params = R.SearchParameters(2000, N_FULL, TOP_K, n_probe)
        for b in range(B):
            h = R.search_trace(hip, q[b], params)
            traces[(n_probe, b)] = h
            c = R.last_s1_counts()
            for k in s1:
                s1[k] += c[k]
            o = orc.search_trace(q[b], TOP_K, N_FULL, n_probe)

            def trace():
                d = check_trace(h, o, Q, n_probe, N_FULL, TOP_K, strict_cells=strict)
                cmp["cells_same"] += int(d.get("cells_same", False))
                cmp["rerank_same"] += int(d.get("rerank_same", False))
            cmp["traces"] += 1
            check(f"trace_p{n_probe}_q{b}", trace)

        def search():
            pids, scores, counts = R.search_arrays(hip, q, params)
            cmp[f"lazy_p{n_probe}"] = R.last_s1_counts()["lazy"]
            cmp[f"lazy_overflows_p{n_probe}"] = R.last_search_counts()["lazy_overflows"]
            ref = orc.search(q, TOP_K, N_FULL, n_probe)
            for b in range(B):
                h, n = traces[(n_probe, b)], int(counts[b])
                assert n == len(h["pids"]) == len(ref[b][0]), (b, n, len(h["pids"]), len(ref[b][0]))
                assert np.array_equal(pids[b, :n], h["pids"]) and np.array_equal(scores[b, :n].view(np.uint32), h["scores"].view(np.uint32)), \
                    f"query {b}: fp_search differs from fp_search_trace"
                check_final(pids[b, :n], scores[b, :n], ref[b][0], ref[b][1], TOP_K)
                if os.environ.get("FP_MAXSIM_REPAIR") == "2":
                    ex = orc.exact_scores(q[b], pids[b, :n])
                    bad = np.flatnonzero(scores[b, :n].view(np.uint32) != ex.view(np.uint32))
                    assert bad.size == 0, f"query {b}: repaired scores differ from the oracle's at {bad[:5].tolist()}: {scores[b, bad[:5]]} vs {ex[bad[:5]]}"
        check(f"search_p{n_probe}", search)

    def columns():
        pids = np.arange(a["doc_lengths"].shape[0], dtype=np.int64)
        n_flag = 0
        for b in range(B):
            got = R.maxsim_columns(hip, q[b], pids)
            want = orc.column_maxima(q[b], pids)
            flagged = ((got["flags"][:, np.arange(Q) // 32] >> (np.arange(Q) % 32).astype(np.uint32)) & 1).astype(bool)
            g = got["col_max"]
            gb, wb = g.view(np.uint16).copy(), want.view(np.uint16).copy()
            gb[gb == 0x8000], wb[wb == 0x8000] = 0, 0
            bad = (gb != wb) & ~flagged
            assert not bad.any(), f"query {b}: {int(bad.sum())} unflagged column maxima differ from the oracle's; first (doc, column) " \
                                  f"{np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} vs {want[bad][0]!r}"
            assert np.all(ulp_diff_f16(g[flagged], want[flagged]) <= 1)
            n_flag += int(flagged.sum())
        s1["columns_flagged"] = n_flag
    if name in ("family_a", "family_c"):
        check("columns", columns)
    return dict(fails=fails, s1=s1, compared=cmp)


def main():
    R.set_graph_replay(False)
    out = {name: run_family(name) for name in sys.argv[1:]}
    print("ROUNDING_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
