"""k_token_scores_tile / k_reconstruct_units (fp_token_scores.hip): token-score matrices and reconstruction at every dim and q_len
an index accepts, bit for bit against the C oracle.  dim 8 / 40 lie below one 64-dim slice, 72 / 136 one unit past a 64- / 128-dim
boundary, 320 has several slices, 1024 is the largest; document lengths 0 / 1 / 63 / 64 / 65 / 130 and q_len 1 / 64 / 65 / 100 sit
on the edges of the 64 x 64 tile.  Before these kernels (1024, 4) with q_len >= 36 was refused and dims above 512 were never run."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import SCORE_TOL
from test_hip_parity import _hip_index, _oracle, _random_arrays, fp  # noqa: F401

pytestmark = pytest.mark.gpu

TOK_SHAPES = [(8, 4), (40, 1), (72, 2), (136, 8), (320, 4), (1024, 4)]
REC_SHAPES = [(8, 4), (264, 2), (520, 4), (1024, 1), (1024, 8)]
QLENS = [1, 64, 65, 100]


@functools.lru_cache(maxsize=None)
def _drawn(dim, nbits):
    """12 documents over 64 centroids; the codes are random, so the stored order (sorted by code) is not the original one"""
    from fast_plaid_amd import synth
    rng = np.random.default_rng(2000 * dim + nbits)
    lens = np.concatenate([[0, 1, 63, 64, 65, 130], rng.integers(1, 41, 6)]).astype(np.int64)
    arr = _random_arrays(rng, int(lens.sum()), 1, 64, dim, nbits, empty_frac=0.0)   # one token per document: re-cut here
    arr["doc_lengths"] = lens
    arr["ivf"], arr["ivf_lengths"] = synth.build_ivf(arr["doc_codes"], lens, 64)
    return arr, _oracle(arr)


def _queries(dim, B, Q):
    q = np.random.default_rng(dim + Q).standard_normal((B, Q, dim), dtype=np.float32)
    return (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float16)


@pytest.mark.parametrize("dim,nbits", TOK_SHAPES, ids=[f"d{d}_nb{n}" for d, n in TOK_SHAPES])
@pytest.mark.parametrize("Q", QLENS)
def test_token_score_matrices_every_shape(fp, dim, nbits, Q):
    """every document as a hit of each of two queries: shape (Q, len) and the oracle's bits"""
    arr, orc = _drawn(dim, nbits)
    n = len(arr["doc_lengths"])
    q = _queries(dim, 2, Q)
    pids = np.tile(np.arange(n, dtype=np.int64), (2, 1))
    mats = fp.fast_plaid_rust.token_score_matrices(_hip_index(fp, arr), q, pids, np.full(2, n, np.int32))
    for b in range(2):
        assert len(mats[b]) == n
        for pid, m in enumerate(mats[b]):
            ref = orc.token_scores(q[b], pid)
            assert m.dtype == np.float16 and m.shape == ref.shape == (Q, int(arr["doc_lengths"][pid]))
            assert np.array_equal(m.view(np.uint16), ref.view(np.uint16)), f"query {b} doc {pid}: differs from the oracle"


@pytest.mark.parametrize("dim,nbits", REC_SHAPES, ids=[f"d{d}_nb{n}" for d, n in REC_SHAPES])
def test_reconstruction_every_shape(fp, dim, nbits):
    """all documents, original token order, fp32 rows equal to the oracle's fp16 rows widened; empty documents give empty arrays"""
    arr, orc = _drawn(dim, nbits)
    lens = arr["doc_lengths"]
    rows = fp.fast_plaid_rust.reconstruct_embeddings(_hip_index(fp, arr), list(range(len(lens))))
    assert [r.shape for r in rows] == [(int(l), dim) for l in lens] and all(r.dtype == np.float32 for r in rows)
    ref = orc.decompress(arr["doc_codes"], arr["doc_residuals"]).astype(np.float32)
    assert np.array_equal(np.concatenate(rows).view(np.uint32), ref.view(np.uint32))


def test_class_token_scores_dim_1024(fp):
    """FastPlaid.search_token_scores at dim 1024, q_len 64: search()'s (id, score) lists, the oracle's matrices, and the MaxSim of
    each matrix (fp32 sum of its fp16 row maxima) within SCORE_TOL of the returned score"""
    from fast_plaid_amd import search
    arr, orc = _drawn(1024, 4)
    q = _queries(1024, 2, 64)
    kw = dict(top_k=5, n_full_scores=64, n_ivf_probe=8, show_progress=False)
    with search.FastPlaid.from_arrays(arr, device="cuda:0") as fpi:
        plain = fpi.search(q, **kw)
        out = fpi.search_token_scores(q, **kw)
    assert [[(d, s) for d, s, _ in row] for row in out] == plain and all(len(row) > 0 for row in out)
    for b, row in enumerate(out):
        for d, s, m in row:
            assert np.array_equal(m.view(np.uint16), orc.token_scores(q[b], d).view(np.uint16))
            assert abs(np.float32(m.astype(np.float32).max(axis=1).sum(dtype=np.float32)) - s) <= SCORE_TOL


# ---- the constructed rounding fixtures (tests/golden/rounding): every token score on or next to an fp16 rounding boundary ----------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDING = ("family_a", "family_c")   # midpoints both ways, subnormals, zeros; self-matches


@functools.lru_cache(maxsize=None)
def _rounding(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "rounding", name + ".npz"))
    arr = {k: z[k] for k in z.files}
    arr["nbits"] = int(arr["nbits"])
    return arr


def _flat(mats):
    return np.concatenate([m.view(np.uint16).ravel() for row in mats for m in row])


def _rounding_device(fp, name):
    """token_score_matrices of every query against every document -> the bits, query by query, document by document"""
    arr = _rounding(name)
    q, n = arr["queries"], len(arr["doc_lengths"])
    pids = np.tile(np.arange(n, dtype=np.int64), (q.shape[0], 1))
    mats = fp.fast_plaid_rust.token_score_matrices(_hip_index(fp, arr), q, pids, np.full(q.shape[0], n, np.int32))
    assert all(m.shape == (q.shape[1], int(arr["doc_lengths"][d])) for row in mats for d, m in enumerate(row))
    return _flat(mats)


@functools.lru_cache(maxsize=None)
def _rounding_oracle(name):
    arr = _rounding(name)
    orc = _oracle(arr)
    return _flat([[orc.token_scores(q, d) for d in range(len(arr["doc_lengths"]))] for q in arr["queries"]])


@functools.lru_cache(maxsize=None)
def _family_a_integers():
    """family A's token scores from integer arithmetic (make_rounding_fixtures.family_a_counts derives the same integers): token =
    (centroid + weight) 2^-7, times 8 where a sparse row's token was normalised by 2^4 grid units; query row = integers 2^unit; every
    sum is exact in fp32 in any order, so the score is h() of the integer"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "rounding"))
    import make_rounding_fixtures as G
    arr = _rounding("family_a")
    cent, q, qu = arr["cent_int"].astype(np.int64), arr["q_int"].astype(np.int64), arr["q_log2_unit"]
    codes = arr["doc_codes"]
    w_int = np.rint(arr["bucket_weights"].astype(np.float64) * 2.0 ** -G.A_UNIT).astype(np.int64)
    tok = cent[codes] + w_int[G.unpack_residuals(arr["doc_residuals"])]
    tok_unit = np.where((codes >= 128) & (codes < 256), G.A_UNIT + 3, G.A_UNIT)
    on_grid = np.array_equal(G.decompress(arr["centroids"], arr["bucket_weights"], codes, G.unpack_residuals(arr["doc_residuals"])).astype(np.float64),
                             tok * 2.0 ** tok_unit[:, None])
    assert on_grid, "a token of family A left the grid"
    off = np.concatenate([[0], np.cumsum(arr["doc_lengths"])])
    out = []
    for b in range(q.shape[0]):
        assert (np.abs(q[b]) @ np.abs(tok.T)).max() < 1 << 24
        s = (q[b] @ tok.T).astype(np.float64) * 2.0 ** (qu[b][:, None] + tok_unit[None, :])      # [Q, T], exact
        out += [s[:, off[d]:off[d + 1]].astype(np.float16).view(np.uint16).ravel() for d in range(len(off) - 1)]
    return np.concatenate(out)


def _check_rounding(name, got):
    want = _rounding_oracle(name)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} of {want.size} token scores differ from the oracle's; first {bad[:5].tolist()}: " \
                          f"{got[bad[:5]].tolist()} vs {want[bad[:5]].tolist()}"
    if name == "family_a":
        ints = _family_a_integers()
        bad = np.flatnonzero(got != ints)
        assert bad.size == 0, f"family_a: {bad.size} token scores differ from h(integer score); first {bad[:5].tolist()}"


@pytest.mark.parametrize("name", ROUNDING)
def test_token_scores_on_the_rounding_fixtures(fp, name):
    """every query against every document of family A / C: the oracle's bits, and in family A h() of the integer scores"""
    _check_rounding(name, _rounding_device(fp, name))


def test_token_scores_on_the_rounding_fixtures_round1_kernel(tmp_path):
    """the same under FP_TEST=tok_tiled=0 (read once per process: this file run as a program)"""
    from fptest_env import with_test_opts
    out = str(tmp_path / "tok.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=with_test_opts(dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oracle")])), tok_tiled=0),
                       timeout=600)
    assert p.returncode == 0 and "TOKEN_SCORES_ROUNDING_OK" in p.stdout, p.stdout[-4000:]
    z = np.load(out)
    for name in ROUNDING:
        _check_rounding(name, z[name])


if __name__ == "__main__":
    import fast_plaid_amd
    np.savez(sys.argv[1], **{name_: _rounding_device(fast_plaid_amd, name_) for name_ in ROUNDING})
    print("TOKEN_SCORES_ROUNDING_OK")
