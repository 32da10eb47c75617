"""The K-sliced MFMA MaxSim kernel (k_maxsim_sl / k_maxsim_repair_sl in fp_maxsim.hip): the (dim, nbits) shapes without a
fixed-dim kernel, against the C oracle.  Shapes: dim 8 / 40 (absent units inside the first k-step), 136 (one unit past a slice
boundary), 320 (several slices), 1024 (one column chunk per launch); q_len 1 / 32 / 33 / 100 (one, two, four chunks)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import SCORE_TOL
from test_hip_parity import _hip_index, _load_golden, _oracle, _random_arrays, _same_order_modulo_ref_ties, fp, parity_ulp  # noqa: F401

pytestmark = pytest.mark.gpu

DRAWN = [(8, 4), (40, 1), (40, 8), (64, 8), (136, 2), (320, 4), (1024, 4), (1024, 1)]
QLENS = [1, 32, 33, 100]
FLAG_CAP = 0.25   # 4 x the largest derived window share, 2^-7 * dim / 128 = 6.25 % at dim 1024


@functools.lru_cache(maxsize=None)
def _drawn(dim, nbits):
    """48 documents over 64 centroids: lengths 0, 1, 16, 17 and random ones up to 40.  Centroids share a direction and the bucket
    weights are small, so that any two tokens have a cosine of about 0.85: every column maximum of a query made of noisy token
    copies lies in [0.5, 1), the binade the window share is derived for.  Returns (arrays, oracle, normalised tokens)."""
    from fast_plaid_amd import synth
    rng = np.random.default_rng(1000 * dim + nbits)
    lens = np.concatenate([[0, 1, 16, 17], rng.integers(1, 41, 44)]).astype(np.int64)
    arr = _random_arrays(rng, int(lens.sum()), 1, 64, dim, nbits, empty_frac=0.0)   # one token per document: re-cut below
    common = rng.standard_normal(dim, dtype=np.float32)
    cent = common / np.linalg.norm(common) + 0.3 * arr["centroids"].astype(np.float32)
    arr["centroids"] = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
    arr["bucket_weights"] = np.sort(rng.normal(0.0, 0.3 / np.sqrt(dim), 1 << nbits)).astype(np.float16)
    arr["doc_lengths"] = lens
    arr["ivf"], arr["ivf_lengths"] = synth.build_ivf(arr["doc_codes"], lens, 64)
    orc = _oracle(arr)
    tok = orc.decompress(arr["doc_codes"], arr["doc_residuals"]).astype(np.float32)
    return arr, orc, tok / np.linalg.norm(tok, axis=1, keepdims=True)


def _queries(tok, dim, B, Q, seed):
    rng = np.random.default_rng(seed)
    q = tok[rng.integers(0, tok.shape[0], (B, Q))] + 0.3 * rng.standard_normal((B, Q, dim), dtype=np.float32) / np.sqrt(dim)
    return (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float16)


def _cpu_flag_share(arr, orc, q, dim):
    """share of the (document, column) pairs whose fp32 maximum (numpy's sum order: an estimate of either side's) lies inside the
    kernel's window eps_rel * |q| around an fp16 rounding boundary of [0.5, 1)"""
    e = orc.decompress(arr["doc_codes"], arr["doc_residuals"]).astype(np.float32)
    n = np.sqrt((e * e).sum(axis=1)).astype(np.float16).astype(np.float32)
    S = (e / n[:, None]).astype(np.float16).astype(np.float32) @ q.astype(np.float32).T
    eps = 2.0 ** -19 * max(1.0, dim / 128) * np.linalg.norm(q.astype(np.float32), axis=1)
    ends = np.cumsum(arr["doc_lengths"])
    am = np.stack([S[b - l: b].max(axis=0) for b, l in zip(ends, arr["doc_lengths"]) if l])
    return float((2.0 ** -12 - np.abs(am - am.astype(np.float16).astype(np.float32)) <= eps).mean())


def _check_columns(R, hip, orc, arr, q, drawn_dim=0):
    lens = arr["doc_lengths"]
    Q = q.shape[0]
    pids = np.arange(len(lens), dtype=np.int64)
    wants = [np.full(Q, -10000.0, np.float16) if lens[pid] == 0 else orc.token_scores(q, pid).max(axis=1) for pid in pids.tolist()]
    if drawn_dim:   # the preconditions of the flag cap, on the CPU, before the GPU runs
        live = np.stack([w for w, l in zip(wants, lens) if l])
        assert np.all((live >= 0.5) & (live < 1.0)), f"column maxima outside [0.5, 1): {live.min()} .. {live.max()}"
        assert _cpu_flag_share(arr, orc, q, drawn_dim) <= FLAG_CAP
    got = R.maxsim_columns(hip, q, pids)
    nflag = 0
    for i, (pid, want) in enumerate(zip(pids.tolist(), wants)):
        flagged = np.array([(int(got["flags"][i, c // 32]) >> (c % 32)) & 1 for c in range(Q)], bool)
        g = got["col_max"][i]
        same = g.view(np.uint16) == want.view(np.uint16)
        assert np.all(same | flagged), f"doc {pid}: unflagged columns {np.nonzero(~same & ~flagged)[0].tolist()} differ from the reference"
        assert np.all(parity_ulp(g[flagged], want[flagged]) <= 1)
        ulps = np.spacing(np.abs(g[flagged]).astype(np.float16)).astype(np.float32) if flagged.any() else np.zeros(0, np.float32)
        assert abs(float(got["unc"][i]) - float(ulps.sum())) <= 1e-6 + 0.51 * float(ulps.sum()), (got["unc"][i], ulps.sum())
        if lens[pid] == 0:
            assert not flagged.any() and got["scores"][i] == np.float32(-10000.0 * Q)
        nflag += int(flagged.sum())
    print(f"flagged {nflag} of {Q * len(lens)} columns")
    assert nflag <= FLAG_CAP * Q * len(lens), f"{nflag} of {Q * len(lens)} columns flagged"


@pytest.mark.parametrize("dim,nbits", DRAWN, ids=[f"d{d}_nb{n}" for d, n in DRAWN])
@pytest.mark.parametrize("Q", QLENS)
def test_sliced_column_certification(fp, dim, nbits, Q):
    """fp_maxsim_columns on the sliced shapes: an unflagged column is the oracle's h(max_t sum_fp32 e^_t . q) bit for bit, a
    flagged one within one fp16 ulp, unc the sum of the flagged ulps, an empty document -10000 per column, at most 25 % flagged.
    (Before the sliced kernel these shapes returned col_max / flags as zeros.)"""
    arr, orc, tok = _drawn(dim, nbits)
    _check_columns(fp.fast_plaid_rust, _hip_index(fp, arr), orc, arr, _queries(tok, dim, 1, Q, Q)[0], dim)


def test_sliced_column_certification_golden_d40(fp):
    z, arr = _load_golden("d40_nb4")
    hip, orc = _hip_index(fp, arr), _oracle(arr)
    for b in range(min(2, z["queries"].shape[0])):
        _check_columns(fp.fast_plaid_rust, hip, orc, arr, z["queries"][b])


@pytest.mark.parametrize("dim,nbits", [(40, 1), (136, 2), (320, 4), (1024, 4)])
def test_sliced_search_parity(fp, dim, nbits):
    """fp_search on the drawn indexes: the C oracle's ids (modulo its exact ties), scores within 1e-3, and the batched call's
    result equal to fp_search_trace's."""
    R = fp.fast_plaid_rust
    arr, orc, tok = _drawn(dim, nbits)
    hip = _hip_index(fp, arr)
    q = _queries(tok, dim, 3, 33, dim)
    top_k, n_full, n_probe = 10, 128, 8
    params = R.SearchParameters(2000, n_full, top_k, n_probe)
    pids, scores, counts = R.search_arrays(hip, q, params)
    ref = orc.search(q, top_k, n_full, n_probe)
    for b in range(q.shape[0]):
        n = int(counts[b])
        rp, rs = ref[b]
        _same_order_modulo_ref_ties(pids[b, :n], rp, dict(zip(np.asarray(rp).tolist(), np.asarray(rs).tolist())))
        by_id = dict(zip(np.asarray(rp).tolist(), np.asarray(rs).tolist()))
        assert max(abs(by_id[int(p)] - float(s)) for p, s in zip(pids[b, :n], scores[b, :n])) <= SCORE_TOL
        tr = R.search_trace(hip, q[b], params)
        assert np.array_equal(pids[b, :n], tr["pids"]) and np.array_equal(scores[b, :n], tr["scores"])


@pytest.mark.parametrize("mode", ["2", "1"])
def test_sliced_repair_vs_oracle(fp, mode):
    """tests/maxsim_sliced_worker.py: with every flagged document repaired (FP_MAXSIM_REPAIR=2) every returned score is the
    oracle's bit for bit; with the default repair (near-tied documents, plus every emitted document that has a flagged column) the id
    lists are the oracle's, and so are the returned scores, bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FP_MAXSIM_REPAIR=mode)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "maxsim_sliced_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SLICED_REPAIR_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
