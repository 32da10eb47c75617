"""tests/golden/rounding/*.npz (constructed fp16 rounding-boundary inputs, see make_rounding_fixtures.py there) checked on the CPU
against integer arithmetic, the C oracle and the numpy restatement of the certification windows (tests/s1_window_model.py) -- no GPU
needed.  The fixtures keep their defining properties (so they cannot rot), and the window the library ships covers every pair
the search harvested.  tests/test_rounding_boundaries_gpu.py runs the same files on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDING_DIR = os.path.join(HERE, "golden", "rounding")
for p in (HERE, ROUNDING_DIR):
    if p not in sys.path:
        sys.path.insert(0, p)

import plaid_oracle as OC  # noqa: E402
import s1_window_model as M  # noqa: E402
import make_rounding_fixtures as G  # noqa: E402

INDEX_KEYS = ("centroids", "bucket_weights", "ivf", "ivf_lengths", "doc_codes", "doc_residuals", "doc_lengths")


def load(name):
    z = np.load(os.path.join(ROUNDING_DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def oracle(a):
    return OC.OracleIndex(nbits=int(a["nbits"]), **{k: a[k] for k in INDEX_KEYS})


@pytest.fixture(scope="module")
def fam_a():
    return load("family_a")


def _a_scores_int(a):
    """[C, B*Q] exact scores as integers and the power of two of their unit"""
    qf = a["q_int"].reshape(-1, a["q_int"].shape[2])
    return a["cent_int"].astype(np.int64) @ qf.astype(np.int64).T, a["cent_log2_unit"][:, None] + a["q_log2_unit"].reshape(1, -1)


def test_family_a_integer_dot_product_equals_the_fp32_chain(fam_a):
    a = fam_a
    S, unit = _a_scores_int(a)
    want = S.astype(np.float64) * 2.0 ** unit.astype(np.float64)
    q = a["queries"].reshape(-1, a["queries"].shape[2])
    got = M.chain32(a["centroids"][:, None, :], q[None, :, :])
    assert np.array_equal(got.astype(np.float64), want), "a chain rounded: the fixture is not on its grid"
    # ... and in another order (descending k): exact sums do not depend on it
    got = M.chain32(a["centroids"][:, None, ::-1], q[None, :, ::-1])
    assert np.array_equal(got.astype(np.float64), want)
    # the C oracle's S is h(exact)
    orc = oracle(a)
    for b in range(a["queries"].shape[0]):
        Sb = orc.search_trace(a["queries"][b], 10, 64, 1)["S"]
        Q = a["queries"].shape[1]
        assert np.array_equal(Sb.view(np.uint16), M.h_bits(want[:, b * Q:(b + 1) * Q]))


def test_family_a_tokens_stay_on_the_grid(fam_a):
    a = fam_a
    widx = G.unpack_residuals(a["doc_residuals"])
    assert np.array_equal(G.pack_residuals(widx), a["doc_residuals"])
    w_int = np.rint(a["bucket_weights"].astype(np.float64) * 2.0 ** -G.A_UNIT).astype(np.int64)
    tok = a["cent_int"].astype(np.int64)[a["doc_codes"]] + w_int[widx]
    ss = (tok * tok).sum(axis=1)
    assert np.all((ss == 4 ** 7) | (ss == 4 ** 4)), "a token's sum of squares is no power of 4"
    want = tok.astype(np.float64) * 2.0 ** G.A_UNIT / (np.sqrt(ss) * 2.0 ** G.A_UNIT)[:, None]
    got = oracle(a).decompress(a["doc_codes"], a["doc_residuals"])
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(G.decompress(a["centroids"], a["bucket_weights"], a["doc_codes"], widx).view(np.uint16), got.view(np.uint16))


def test_family_a_covers_the_advertised_categories(fam_a):
    a = fam_a
    s_counts, m_counts = G.family_a_counts(a)
    assert [s_counts[k] for k in G.CATS] == a["s_counts"].tolist() and [m_counts[k] for k in G.CATS] == a["m_counts"].tolist()
    for k in G.CATS:
        assert s_counts[k] >= 100 and m_counts[k] >= 100, (k, s_counts, m_counts)
    # a midpoint is where the two roundings of a one-step-off sum part: the oracle's column maxima are h(exact) there too
    orc = oracle(a)
    pids = np.arange(a["doc_lengths"].shape[0])
    tok = orc.decompress(a["doc_codes"], a["doc_residuals"])
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    for b in (0, 3):
        q = a["queries"][b]
        ex = np.stack([M.exact_dot_int(tok, q[j][None, :]) for j in range(q.shape[0])], axis=1)
        mx = np.stack([ex[off[d]:off[d + 1]].max(axis=0) for d in pids])
        assert np.array_equal(orc.column_maxima(q, pids).view(np.uint16), M.h_bits(M.fl32_of_int(mx)))


def _pairs(a, key):
    p = a[key]
    q = a["queries"].reshape(-1, a["queries"].shape[2])[p[:, 0]]
    c = a["centroids"][p[:, 1]]
    return q, c


def _flagged_any_shift(x, w, kappa, width=8):
    """per pair: flagged for EVERY x within +-width fp32 ulp / for ANY of them"""
    f = np.stack([M.s1_flagged(M.shift_ulps(x, s), w, kappa) for s in range(-width, width + 1)])
    return f.all(axis=0), f.any(axis=0)


@pytest.mark.parametrize("name,min_diff", [("family_b", 1), ("family_b_d64", 0)])
def test_family_b_pairs_keep_their_property(name, min_diff):
    """under the constants RECORDED in the fixture (those the search ran with): the harvested pairs are unflagged differences, the
    window-violating pairs violate the window"""
    a = load(name)
    dim = a["centroids"].shape[1]
    w0_log2, kappa_log2 = (float(v) for v in a["window_log2"])
    cnm = M.cent_norm_max(a["centroids"])
    assert cnm == np.float32(1.0)
    kappa = M.s1_kappa(dim, kappa_log2)
    assert a["pairs_diff"].shape[0] >= min_diff
    q, c = _pairs(a, "pairs_diff")
    if q.shape[0]:
        ch, x = M.chain32(c, q), M.fl32_of_int(M.exact_dot_int(c, q))
        assert np.all(M.h_bits(ch) != M.h_bits(x)), "a harvested pair no longer rounds differently"
        _, any_f = _flagged_any_shift(x, M.wcol(q, cnm, dim, w0_log2), kappa)
        assert not any_f.any(), "a harvested pair is flagged under the window it was harvested with"
        # what the C oracle stores for the pair is h(chain)
        orc = oracle(a)
        Q = a["queries"].shape[1]
        for (t, r), want in zip(a["pairs_diff"].tolist(), M.h_bits(ch).tolist()):
            S = orc.search_trace(a["queries"][t // Q], 10, 64, 1)["S"]
            assert int(S.view(np.uint16)[r, t % Q]) == want
    q, c = _pairs(a, "pairs_viol")
    assert q.shape[0] >= (100 if min_diff else 0)
    if q.shape[0]:
        ch, ex = M.chain32(c, q), M.exact_dot_int(c, q)
        x = M.fl32_of_int(ex)
        u = M.s1_u(x, M.wcol(q, cnm, dim, w0_log2), kappa).astype(np.float64)
        assert np.all(np.abs(ch.astype(np.float64) - ex.astype(np.float64) * 2.0 ** -48) > u)
        assert np.all(M.h_bits(ch) == M.h_bits(x))


@pytest.mark.parametrize("name", ["family_b", "family_b_d64"])
def test_family_b_tables_hold_same_sign_near_copies(name):
    """whatever the search harvested (nothing at dim 64), the fixture IS the same-sign family: at least 100 query tokens have a
    centroid in the table that is nearly a copy of them (cosine >= 0.95) with every one of the D products of one sign -- counted
    from the table itself, not from the recorded pair lists -- and the recorded lists name such pairs"""
    a = load(name)
    q = a["queries"].reshape(-1, a["queries"].shape[2]).astype(np.float64)
    c = a["centroids"].astype(np.float64)
    cos = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (c / np.linalg.norm(c, axis=1, keepdims=True)).T
    best = cos.argmax(axis=1)
    one_sign = np.all(q * c[best] > 0, axis=1)
    n = int(((cos.max(axis=1) >= 0.95) & one_sign).sum())
    assert n >= 100, f"{name}: only {n} query tokens have a same-sign near-copy centroid"
    pairs = np.concatenate([a["pairs_diff"], a["pairs_viol"], a["pairs_near"]])
    assert pairs.shape[0] >= 100 and np.all(cos[pairs[:, 0], pairs[:, 1]] >= 0.9)
    qn, cn = _pairs(a, "pairs_near")
    assert np.all(qn.astype(np.float64) * cn.astype(np.float64) > 0), "pairs_near: a product of the other sign"


@pytest.mark.parametrize("name", ["family_b", "family_b_d64"])
def test_shipped_window_flags_every_harvested_pair(name):
    """under the constants the library SHIPS (s1_window_model.S1_W0_LOG2 / S1_KAPPA_LOG2 = fp_engine.cpp's defaults): every
    harvested pair is flagged for every x within +-8 fp32 ulp of the exact sum, and the chain lies inside the window of every
    pair of the fixture, the window-violating ones of the old constants and the further near-copies included"""
    a = load(name)
    dim = a["centroids"].shape[1]
    cnm = M.cent_norm_max(a["centroids"])
    kappa = M.s1_kappa(dim)
    q, c = _pairs(a, "pairs_diff")
    if q.shape[0]:
        x = M.fl32_of_int(M.exact_dot_int(c, q))
        all_f, _ = _flagged_any_shift(x, M.wcol(q, cnm, dim), kappa)
        assert all_f.all(), f"{int((~all_f).sum())} of {q.shape[0]} harvested pairs escape the shipped window"
    for key in ("pairs_diff", "pairs_viol", "pairs_near"):
        q, c = _pairs(a, key)
        if q.shape[0]:
            ch, ex = M.chain32(c, q), M.exact_dot_int(c, q)
            x = M.fl32_of_int(ex)
            u = M.s1_u(x, M.wcol(q, cnm, dim), kappa).astype(np.float64)
            assert np.all(np.abs(ch.astype(np.float64) - x.astype(np.float64)) <= u), key


def test_family_c_queries_are_document_tokens_and_columns_keep_their_property():
    a = load("family_c")
    assert not a["bucket_weights"].any()
    orc = oracle(a)
    tok = orc.decompress(a["doc_codes"], a["doc_residuals"])
    dim = tok.shape[1]
    assert np.array_equal(a["queries"].reshape(-1, dim).view(np.uint16), tok[a["query_tokens"]].view(np.uint16))
    assert np.array_equal(G.decompress(a["centroids"], a["bucket_weights"], a["doc_codes"], G.unpack_residuals(a["doc_residuals"])).view(np.uint16),
                          tok.view(np.uint16))
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    pids = np.arange(a["doc_lengths"].shape[0])
    n = 0
    for b in range(a["queries"].shape[0]):
        q = a["queries"][b]
        mc, mx = G.c_column_maxima(tok, off, q)
        ref = orc.column_maxima(q, pids)
        assert np.array_equal(ref.view(np.uint16), M.h_bits(mc)), "the restated chain is not the oracle's"
        bad = (M.h_bits(mc) != M.h_bits(mx)) & ~M.maxsim_flagged(mx, M.maxsim_eps(q, dim, float(a["eps_log2"]))[None, :])
        got = sorted((b, int(j), int(d)) for d, j in zip(*np.nonzero(bad)))
        want = sorted(tuple(r) for r in a["cols_diff"].tolist() if r[0] == b)
        assert got == want
        n += len(got)
    assert n == a["cols_diff"].shape[0]
