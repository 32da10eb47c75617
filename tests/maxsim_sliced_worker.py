"""GPU worker for tests/test_maxsim_sliced_gpu.py::test_sliced_repair_vs_oracle (FP_MAXSIM_REPAIR is read once per process).

The exact-order repair at a runtime dim (k_maxsim_repair_sl), on the shapes of the K-sliced MaxSim kernel:
  FP_MAXSIM_REPAIR=2  every flagged document is repaired: every returned score equals the oracle's exact score bit for bit;
  FP_MAXSIM_REPAIR=1  (the default) near-tied documents, and on these shapes every emitted document that has a flagged column: the
                      id lists are the oracle's (modulo its exact ties) and the returned scores equal the oracle's bit for bit too."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import fast_plaid_amd as fp  # noqa: E402
from repair_worker import mk, oracle  # noqa: E402

R = fp.fast_plaid_rust


def main():
    mode = int(os.environ.get("FP_MAXSIM_REPAIR", "1"))
    assert mode in (1, 2)
    from test_hip_parity import _same_order_modulo_ref_ties
    n_scores = n_lists = 0
    for (dim, nbits, n_docs, C, Q, seed) in ((40, 4, 4000, 256, 32, 1), (160, 2, 3000, 256, 32, 2), (320, 4, 2000, 256, 32, 3),
                                             (512, 8, 1500, 128, 32, 4), (1024, 4, 1000, 128, 32, 5), (40, 4, 4000, 256, 50, 1),
                                             (160, 2, 3000, 256, 50, 2), (320, 4, 2000, 256, 50, 3), (512, 8, 1500, 128, 50, 4),
                                             (1024, 4, 1000, 128, 50, 5)):
        spec = fp.synth.SynthSpec(n_docs=n_docs, doc_len=24, n_centroids=C, dim=dim, nbits=nbits, variable_len=True, seed=seed)
        arr = fp.synth.host_index_arrays(spec)
        idx, orc = mk(arr), oracle(arr)
        q = fp.synth.make_queries(spec, arr["centroids"], 3, Q)
        top_k, n_full, n_probe = 100, 512, 8
        pids, scores, counts = R.search_arrays(idx, q, R.SearchParameters(2000, n_full, top_k, n_probe))
        ref = orc.search(q, top_k, n_full, n_probe, nthreads=4)
        for b in range(q.shape[0]):
            n = int(counts[b])
            assert n == len(ref[b][0]), (dim, nbits, b, n, len(ref[b][0]))
            ex = orc.exact_scores(q[b], pids[b, :n])   # (both modes: the default one repairs every emitted flagged document here)
            bad = np.flatnonzero(scores[b, :n].view(np.uint32) != ex.view(np.uint32))
            assert bad.size == 0, (dim, nbits, Q, b, bad[:5], scores[b, bad[:5]], ex[bad[:5]])
            n_scores += n
            _same_order_modulo_ref_ties(pids[b, :n], ref[b][0], dict(zip(np.asarray(ref[b][0]).tolist(), np.asarray(ref[b][1]).tolist())))
            n_lists += 1
    print("SLICED_REPAIR_OK mode", mode, "scores", n_scores, "lists", n_lists)


if __name__ == "__main__":
    main()
