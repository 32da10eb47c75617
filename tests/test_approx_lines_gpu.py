"""S4's exact kernel fed from the packed code lines (fp_kernels.hip k_approx_lines: a candidate's codes from its aligned 128-byte
line at line <document id> instead of uoff -> ucodes) against the kernel it replaces in the wide launches: FP_TEST=ap_lines=1
(the default) against ap_lines=0 on small constructed corpora that go through the level-0 refine (FP_APPROX_IMPL=l0), shapes and
corpora in approx_lines_worker.py.  The knobs are read once per process, so every variant is a subprocess; the two settings of
one case run side by side.  Everything is compared bit for bit: fp_search with fp_search_trace (in the worker), the two
settings with each other (results, counters, and the trace's score of EVERY candidate), the id lists with the C oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import approx_lines_worker as W
import plaid_oracle as OC
from fptest_env import with_test_opts
from parity import check_final

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _oracle(name, n_full):
    """the oracle's result lists of a shape: computed once, shared by the cases, never modified"""
    if (name, n_full) not in _ORACLE:
        arr, q, _ = W.corpus(name)
        orc = OC.OracleIndex(nbits=arr["nbits"], centroids=arr["centroids"], bucket_weights=arr["bucket_weights"], ivf=arr["ivf"],
                             ivf_lengths=arr["ivf_lengths"], doc_codes=arr["doc_codes"], doc_residuals=arr["doc_residuals"],
                             doc_lengths=arr["doc_lengths"])
        _ORACLE[(name, n_full)] = orc.search(q, W.TOP_K, n_full, W.N_PROBE, nthreads=4)
    return _ORACLE[(name, n_full)]


def _run_pair(names, env, tmp_path):
    """the worker under ap_lines=0 and =1, side by side; returns the two result files"""
    env = with_test_opts(dict(env, FP_APPROX_IMPL="l0"), l0_pilot=16)
    procs = []
    for d in (0, 1):
        out = str(tmp_path / f"l{d}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "approx_lines_worker.py"), out] + list(names),
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=with_test_opts(env, ap_lines=d))))
    res = []
    for out, p in procs:
        txt = p.communicate(timeout=600)[0]
        assert p.returncode == 0 and "AP_LINES_OK" in txt, txt[-4000:]
        res.append(np.load(out))
    return res


def _compare(names, r0, r1, lazy):
    """both settings against each other and the oracle; returns the number of comparisons made"""
    n = int(r0["ncmp"][0]) + int(r1["ncmp"][0])   # fp_search == fp_search_trace, asserted in the workers
    assert int(r0["ncmp"][0]) > 0 and int(r1["ncmp"][0]) > 0
    for name in names:
        C, Q, B = W.SHAPES[name]
        single = C <= (1 << 17)   # one centroid range: the index carries 128-byte lines addressed by the document id
        seen = {k: 0 for k in W.KINDS if k}
        for pname, n_full in W.PARAMS.items():
            key = f"{name}_{pname}"
            for part in ("pids", "scores", "counts"):
                assert np.array_equal(r0[f"{key}_{part}"], r1[f"{key}_{part}"]), (key, part)
                n += 1
            f0, f1 = r0[f"{key}_form"], r1[f"{key}_form"]
            assert np.array_equal(f0[:4], f1[:4]), (key, f0, f1)    # form of S4, form of S1, candidates, exactly scored documents
            assert f1[0] == 2, (key, f1)                            # level 0 ran
            assert f1[1] == (1 if lazy else 0), (key, f1)           # S1's form (fp_last_s1_counts)
            # the kernel chosen: the line-fed one for the refine's two wide launches (per pass over the batch) and for a trace
            # whose candidates fit a wide launch -- never with ap_lines=0, never on a table of several ranges
            assert f0[4] == 0 and r0[f"{key}_trace"][0] == 0, (key, f0, r0[f"{key}_trace"])
            if single:
                assert f1[4] >= 2 and f1[4] % 2 == 0, (key, f1)
                assert r1[f"{key}_trace"][0] == r1[f"{key}_trace"][1], (key, r1[f"{key}_trace"])
            else:
                assert f1[4] == 0 and r1[f"{key}_trace"][0] == 0, (key, f1, r1[f"{key}_trace"])
            if pname == "wide":
                assert r1[f"{key}_trace"][1] == B, (key, r1[f"{key}_trace"])   # every trace scored its candidates in a wide launch
            ref = _oracle(name, n_full)
            for b in range(B):
                # the score of every candidate, document by document
                assert np.array_equal(r0[f"{key}_cand{b}"], r1[f"{key}_cand{b}"]), (key, b)
                a0, a1 = r0[f"{key}_approx{b}"], r1[f"{key}_approx{b}"]
                assert a0.shape == a1.shape and np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), (key, b, int((a0 != a1).sum()))
                n += 1
                if pname == "wide":
                    for k in seen:
                        seen[k] += int((r1[f"{key}_nd{b}"] == k).sum())
                for r in (r0, r1):
                    pids, scores, counts = r[f"{key}_pids"], r[f"{key}_scores"], r[f"{key}_counts"]
                    assert counts[b] == len(ref[b][0]), (key, b, counts[b], len(ref[b][0]))
                    check_final(pids[b, : counts[b]], scores[b, : counts[b]], ref[b][0], ref[b][1], W.TOP_K)
                    n += 1
        # every constructed number of distinct codes was among the candidates that the two kernels scored
        assert all(v > 0 for v in seen.values()), (name, seen)
    return n


@pytest.mark.parametrize("names", [("q7", "b1"), ("q32",), ("q64",), ("ranges",)], ids=lambda v: "+".join(v))
def test_lazy_form(names, tmp_path):
    """S1's lazy form (the default; asserted through fp_last_s1_counts): k_approx_lines<true>, with the negative-column flag."""
    env = dict(os.environ)
    env.pop("FP_S1_EXACT", None)
    r0, r1 = _run_pair(names, env, tmp_path)
    assert _compare(names, r0, r1, lazy=True) > 0


@pytest.mark.parametrize("names", [("q7", "b1"), ("q64",)], ids=lambda v: "+".join(v))
def test_eager_form(names, tmp_path):
    """FP_S1_EXACT=1: S holds the reference's values, k_approx_lines<false>."""
    r0, r1 = _run_pair(names, dict(os.environ, FP_S1_EXACT="1"), tmp_path)
    assert _compare(names, r0, r1, lazy=False) > 0
