"""GPU worker for tests/test_assign_boundaries_gpu.py: the constructed assignment fixtures of tests/golden/assign
(make_assign_fixtures.py there; their CPU side is tests/test_assign_fixtures_cpu.py) on the device, bit for bit against the explicit
ascending-k chain model.  FP_TEST is read once per process, so every setting is one run of this file:

    assign_boundaries_worker.py CASE [CASE ...]        CASE = family:dim[:corpus], family in g, x, o (compress form), gl, ol2 (L2 form)

Every check of every case runs even after another has failed; the last line printed is  ASSIGN_BOUNDARIES_RESULT {json}  with, per
case, the failed checks (name -> message) and the counters read back.  The checks, the same in every setting:

  compress form   create.compress: codes == the model's; packed residual bytes == the model's h(x - c[code]) bucketised against the
                  fixture's cutoffs; last_compress_counts == (1, 1, 0) for a corpus of tokens with at most 8 candidates, (1, 1, 1)
                  with 9 or more, (1, 0, 0) under FP_TEST=assign_exact=1
  L2 form         fp_assign_l2 with the model's hn: labels == the model's.  fp_kmeans, niter = 1, on [table rows; tokens] with
                  init_rows = the table rows: counts and cent32 == kmeans_model.run's, narrowed_chunks == 1 (0 under
                  assign_exact=1), fallback_chunks == 1 exactly when a token has 9 or more candidates.
                  maintain.centroid_outliers: nearest == the model's labels, sqdist bits == update_policy_model's, the same chunk
                  counts"""
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "assign"))
import numpy as np  # noqa: E402

import kmeans_model as KM  # noqa: E402
import kmeans_worker as KW  # noqa: E402
import make_assign_fixtures as F  # noqa: E402
import update_policy_model as UM  # noqa: E402
from fptest_env import test_opt  # noqa: E402

EXACT = test_opt("assign_exact", "0") not in ("0", "")


def inputs(case):
    """-> (form, table fp16 [C, dim], tokens fp16 [T, dim], cutoffs fp16 [3] or None, tokens with 9 or more candidates?)"""
    family, dim, corpus = (case.split(":") + [None])[:3]
    dim = int(dim)
    if family in ("o", "ol2"):
        z = np.load(os.path.join(ROOT, "tests", "golden", "assign", f"o_d{dim}.npz"))
        pre = "c_" if family == "o" else "l2_"
        return ("compress" if family == "o" else "l2"), z[pre + "cent"], z[pre + "tok"], np.array([-0.05, 0.0, 0.05], np.float16), False
    fx = dict(g=F.family_g, gl=F.family_gl, x=F.family_x)[family](dim)
    return fx["form"], fx["cent"], fx["corpora"][corpus]["tok"], fx["cutoffs"], corpus == "ge9"


def run_case(case):
    from fast_plaid_amd import _native as N, create, kmeans, maintain
    from fast_plaid_amd.fast_plaid_rust import _ptr
    form, cent, tok, cutoffs, many = inputs(case)
    C, T = cent.shape[0], tok.shape[0]
    fails, info = {}, {}

    def check(label, fn):
        try:
            fn()
        except Exception as e:   # noqa: BLE001  (reported to the test, with the first lines of the message)
            fails[label] = (str(e) or traceback.format_exc())[:600]

    def differ(name, got, want):
        got = np.asarray(got)
        want = np.broadcast_to(np.asarray(want), got.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: {bad.size} of {np.asarray(want).size} differ; first rows {bad[:6].tolist()}: got " \
                              f"{np.asarray(got)[bad[:6]].tolist()}, want {np.asarray(want)[bad[:6]].tolist()}"

    if form == "compress":
        want = F.model_codes(tok, cent)
        codes, res = create.compress(cent, cutoffs, tok, F.NBITS, "cuda:0")
        n = create.last_compress_counts()
        info["counts"] = [n["chunks"], n["narrowed_chunks"], n["fallback_chunks"]]
        check("codes", lambda: differ("codes", codes, want))
        check("residuals", lambda: differ("residual rows", (res != F.model_residuals(tok, cent, want, cutoffs)).any(axis=1), False))

        def counts():
            assert info["counts"] == ([1, 0, 0] if EXACT else [1, 1, 1] if many else [1, 1, 0]), info["counts"]
        check("counts", counts)
        return dict(fails=fails, info=info)

    hn = F.model_hn(cent)
    want, _ = F.model_labels(tok, cent, hn)

    def assign_l2():
        labels = np.zeros(T, np.int64)
        N.check(N.lib().fp_assign_l2(0, _ptr(cent), _ptr(hn), C, cent.shape[1], _ptr(tok), T, _ptr(labels)))
        differ("fp_assign_l2 labels", labels, want)
    check("assign_l2", assign_l2)

    def kmeans_once():
        data = np.ascontiguousarray(np.concatenate([cent, tok]))
        init = np.arange(C, dtype=np.int64)
        ref = KM.run(data, C, 1, init, 77)
        assert np.array_equal(ref["cent16"][0], cent) and np.array_equal(ref["labels"][0][C:], want) and ref["reseeds"][0] == 0
        rc, c32, cnt = KW.call(data, C, 1, init, 77)
        assert rc == 0, N.last_error()
        t = kmeans.last_device_timings()
        info["kmeans_chunks"] = [t["narrowed_chunks"], t["fallback_chunks"]]
        differ("fp_kmeans counts", cnt, ref["counts"][1])
        differ("fp_kmeans cent32 rows", (c32.view(np.uint32) != ref["cent32"][1].view(np.uint32)).any(axis=1), False)
        assert info["kmeans_chunks"] == ([0, 0] if EXACT else [1, 1] if many else [1, 0]), info["kmeans_chunks"]
    check("kmeans", kmeans_once)

    def outliers():
        rows, sqdist, nearest = maintain.centroid_outliers(cent, tok, 0.5, "cuda:0")
        n = maintain.last_outlier_counts()
        info["outlier_counts"] = [n["chunks"], n["narrowed_chunks"], n["fallback_chunks"]]
        w_rows, w_sq, w_near = UM.outliers(cent, tok, UM.threshold_sq(0.5))
        assert np.array_equal(w_near, want)
        differ("nearest", nearest, want)
        differ("sqdist bits", sqdist.view(np.uint32), w_sq.view(np.uint32))
        differ("outlier rows", rows, w_rows)
        assert info["outlier_counts"] == ([1, 0, 0] if EXACT else [1, 1, 1] if many else [1, 1, 0]), info["outlier_counts"]
    check("outliers", outliers)
    return dict(fails=fails, info=info)


def main():
    out = {case: run_case(case) for case in sys.argv[1:]}
    print("ASSIGN_BOUNDARIES_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
