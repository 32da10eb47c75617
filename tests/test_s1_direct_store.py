"""The streaming S1 kernel's direct write-out (S stored straight from the MFMA accumulators, the query columns relabelled on the
operand side; fp_kernels.hip k_centroid_scores_stream<.., true>) against the LDS-staged write-out it replaces for q_len <= 32:
FP_TEST=s1_direct=1 (the default) against s1_direct=0 on tiny corpora, shapes in s1_direct_worker.py.  The knob is read once per
process, so every variant is a subprocess; the two settings of one case run side by side."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plaid_oracle as OC
import s1_direct_worker as W
from fptest_env import with_test_opts
from parity import check_final

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _oracle(group):
    """the oracle's result lists for every shape of the group: computed once, shared by the cases, never modified"""
    if group not in _ORACLE:
        out = []
        for i, (C, dim, Q, B) in enumerate(W.SHAPES[group]):
            arr, q = W.corpus(i, C, dim, Q, B)
            orc = OC.OracleIndex(nbits=arr["nbits"], centroids=arr["centroids"], bucket_weights=arr["bucket_weights"], ivf=arr["ivf"],
                                 ivf_lengths=arr["ivf_lengths"], doc_codes=arr["doc_codes"], doc_residuals=arr["doc_residuals"],
                                 doc_lengths=arr["doc_lengths"])
            out.append(orc.search(q, W.TOP_K, W.N_FULL, W.n_probe(C), nthreads=4))
        _ORACLE[group] = out
    return _ORACLE[group]


def _run_pair(kind, group, env, tmp_path):
    """the worker under s1_direct=0 and =1, side by side; returns the two result files"""
    if group == "b":
        env = dict(env, FP_S1_STREAM="3")
    else:
        env.pop("FP_S1_STREAM", None)
    procs = []
    for d in (0, 1):
        out = str(tmp_path / f"d{d}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "s1_direct_worker.py"), kind, group, out],
                                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=with_test_opts(env, s1_direct=d))))
    res = []
    for out, p in procs:
        txt = p.communicate(timeout=600)[0]
        assert p.returncode == 0 and "S1_DIRECT_OK" in txt, txt[-4000:]
        res.append(np.load(out))
    return res


@pytest.mark.parametrize("group", ["a", "b"])
def test_plain_scores_bit_identical(group, tmp_path):
    """FP_S1_EXACT=0 (plain rounding, mode 0): fp_search_trace returns the same S, bit for bit, under both settings."""
    env = dict(os.environ, FP_S1_EXACT="0")
    r0, r1 = _run_pair("trace", group, env, tmp_path)
    for i, (C, dim, Q, B) in enumerate(W.SHAPES[group]):
        a, b = r0[f"S{i}"], r1[f"S{i}"]
        assert a.shape == b.shape == (C, Q), (i, a.shape, b.shape)
        assert np.array_equal(a, b), (i, C, dim, Q, int((a != b).sum()))
        assert a.any(), i


@pytest.mark.parametrize("impl", ["l0", ""])
@pytest.mark.parametrize("group", ["a", "b"])
def test_lazy_search_same_results_and_counts(group, impl, tmp_path):
    """fp_search in its default lazy form (under FP_APPROX_IMPL=l0: with the excess table from S1's epilogue): equal to
    fp_search_trace query by query (asserted in the worker), id lists equal to the oracle's, and the batch's counters --
    candidates, approx_exact, repaired, lazy == 1 -- the same under both settings (a changed excess byte or column maximum moves
    them)."""
    env = dict(os.environ)
    env.pop("FP_S1_EXACT", None)
    env.pop("FP_APPROX_IMPL", None)
    if impl:
        env["FP_APPROX_IMPL"] = impl
    r0, r1 = _run_pair("search", group, env, tmp_path)
    ref = _oracle(group)
    for i, (C, dim, Q, B) in enumerate(W.SHAPES[group]):
        for rep in range(2):
            for key in ("lc", "pids", "scores", "counts"):
                assert np.array_equal(r0[f"{key}{i}_{rep}"], r1[f"{key}{i}_{rep}"]), (key, i, rep, r0[f"{key}{i}_{rep}"], r1[f"{key}{i}_{rep}"])
            assert r1[f"lc{i}_{rep}"][3] == 1, (i, rep, r1[f"lc{i}_{rep}"])
            for r in (r0, r1):
                pids, scores, counts = r[f"pids{i}_{rep}"], r[f"scores{i}_{rep}"], r[f"counts{i}_{rep}"]
                for b in range(B):
                    assert counts[b] == len(ref[i][b][0]), (i, b, counts[b], len(ref[i][b][0]))
                    check_final(pids[b, : counts[b]], scores[b, : counts[b]], ref[i][b][0], ref[i][b][1], W.TOP_K)
