"""The constructed assignment fixtures (tests/golden/assign/make_assign_fixtures.py) on the CPU: the committed files are what the
generator writes, every advertised category is there (counted from integer arithmetic), the gap that fixes each token's candidate
count holds, and the chain model's codes and labels equal the integer-arithmetic expectation, the ATen restatement and the numpy
k-means model.  tests/test_assign_boundaries_gpu.py runs the same fixtures on the device."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSIGN_DIR = os.path.join(ROOT, "tests", "golden", "assign")
sys.path.insert(0, ASSIGN_DIR)
import make_assign_fixtures as F  # noqa: E402

G_KINDS = {"le8": {"top2", "top3", "top8", "mid_tie_below", "mid_win_above", "mid_tie_above", "mid_lose_below", "neg3", "subnormal"},
           "ge9": {"top9", "top12", "zero", "equal"}}
GL_KINDS = {"le8": {"tie2", "tie3", "tie8", "step"}, "ge9": {"tie9"}, "rows": {"self"}}
X_KINDS = {"le8": {"inf_pair", "edge", "inf_single"}, "ge9": {"neg_inf_all"}}
GRID = [("g", d) for d in F.G_DIMS + F.G_EXTRA_DIMS] + [("gl", d) for d in F.GL_DIMS] + [("x", d) for d in F.X_DIMS]


@functools.lru_cache(maxsize=None)
def fixture(family, dim):
    return dict(g=F.family_g, gl=F.family_gl, x=F.family_x)[family](dim)


@functools.lru_cache(maxsize=None)
def order_twins(dim):
    z = np.load(os.path.join(ASSIGN_DIR, f"o_d{dim}.npz"))
    return {k: z[k] for k in z.files}


def test_the_generator_reproduces_the_committed_files():
    r = subprocess.run([sys.executable, os.path.join(ASSIGN_DIR, "make_assign_fixtures.py"), "--check"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f in os.listdir(ASSIGN_DIR):
        assert os.path.getsize(os.path.join(ASSIGN_DIR, f)) <= 300 * 1024, f


@pytest.mark.parametrize("family,dim", GRID)
def test_categories_gap_and_exact_range(family, dim):
    """every category has tokens, the last partial tile holds every group, every token's group is separated by the gap (so the
    candidate count is the group size), members of a compress group are spread over tiles and column halves"""
    fx = fixture(family, dim)
    kinds = dict(g=G_KINDS, gl=GL_KINDS, x=X_KINDS)[family]
    assert fx["cent"].shape[0] >= 256 and (family != "g" or fx["cent"].shape[0] > 3 * 128)
    for corpus, want in kinds.items():
        co = fx["corpora"][corpus]
        counts = F.check_groups(fx, corpus)            # asserts the exact range and the gap
        assert set(counts) == want, (corpus, counts)
        if corpus == "rows":
            continue
        T = co["tok"].shape[0]
        assert T % 128 != 0 and set(co["kind"][T - T % 128:]) == want, "a category is missing from the last partial tile"
        for t in np.flatnonzero((co["n_group"] >= 2) & (co["n_group"] <= F.MAXG) & (family != "x")):
            m = co["members"][t][:co["n_group"][t]]
            assert np.unique(m // 128).size >= min(m.size, 3) and np.unique(m % 128 < 64).size == 2 and np.unique(m % 64 < 32).size == 2
    if family == "g":      # the rounding the categories are named after, from the exact scores
        co, S, codes = fx["corpora"]["le8"], F.exact_scores(fx, "le8"), F.exact_codes(fx, "le8")
        with np.errstate(over="ignore"):
            H = S.astype(np.float16)
        for t in range(S.shape[0]):
            m = co["members"][t][:co["n_group"][t]]
            kind, s, h = str(co["kind"][t]), S[t, m], H[t, m]
            assert np.all(np.diff(s) > 0), "the exact scores of a group rise with the index"
            if kind.startswith(("top", "neg", "subnormal")) or kind.startswith("mid_tie"):
                assert np.unique(h).size == 1 and codes[t] == m[0]
            if kind == "mid_win_above":
                assert h[1] > h[0] and h[1].astype(np.float64) > s[1]
            if kind == "mid_lose_below":
                assert h[1] > h[0] and h[0].astype(np.float64) < s[0]
            if kind == "subnormal":
                assert np.abs(S[t]).max() < 2.0 ** -14
            if kind == "neg3":
                assert S[t].max() < 0
    if family == "x":
        S = F.exact_scores(fx, "ge9")
        assert S.max() <= -F.HALF_INF and np.all(F.exact_codes(fx, "ge9") == 0)
        co, S = fx["corpora"]["le8"], F.exact_scores(fx, "le8")
        codes = F.exact_codes(fx, "le8")
        for t in range(S.shape[0]):
            m = co["members"][t][:co["n_group"][t]]
            assert codes[t] == m[np.argmax(S[t, m] >= F.HALF_INF)], "the first +inf score wins"
        assert any(tuple(co["members"][t][:2]) == (5, 9) and tuple(S[t, [5, 9]]) == (70000.0, 100000.0) for t in range(S.shape[0]))


@pytest.mark.parametrize("family,dim", GRID)
def test_chain_model_equals_integer_arithmetic_and_the_restatements(family, dim):
    """codes / labels of the explicit ascending-k chain == the integer-arithmetic expectation == plaid_oracle_torch's
    compress_into_codes (compress form) resp. kmeans_model.assign (L2 form)"""
    fx = fixture(family, dim)
    for corpus, co in fx["corpora"].items():
        want = F.exact_codes(fx, corpus)
        if fx["form"] == "compress":
            import torch
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import plaid_oracle_torch as OT
            assert np.array_equal(F.model_codes(co["tok"], fx["cent"]), want)
            aten = OT.compress_into_codes(torch.from_numpy(co["tok"]), torch.from_numpy(fx["cent"])).numpy()
            assert np.array_equal(aten, want), f"ATen differs at {np.flatnonzero(aten != want)[:8].tolist()}"
        else:
            import kmeans_model as KM
            hn = F.model_hn(fx["cent"])
            assert np.array_equal(hn, KM.prepare(fx["cent"].astype(np.float32))[1])
            assert np.array_equal(F.model_labels(co["tok"], fx["cent"])[0], want)
            assert np.array_equal(KM.assign(co["tok"], fx["cent"], hn), want)


@pytest.mark.parametrize("dim", F.O_DIMS)
def test_order_twins_keep_their_property(dim):
    """the two orders of the same products round differently under chain32, the winner sits at the higher index in half of the
    triples, every other centroid is below the gap; the file records the search"""
    import kmeans_model as KM
    arr = order_twins(dim)
    n_c, n_l2 = F.check_o(arr, dim)
    print(f"dim {dim}: compress (chains, found, kept) = {arr['c_search'].tolist()}, L2 = {arr['l2_search'].tolist()}")
    assert n_c == arr["c_search"][2] and n_l2 == arr["l2_search"][2] and n_c > 0 and n_l2 > 0
    for form in ("c", "l2"):
        win, pair = arr[f"{form}_winner"], arr[f"{form}_pair"]
        hi = win == pair[:, 1]
        assert 0.3 < hi.mean() < 0.7
    assert np.array_equal(F.model_codes(arr["c_tok"], arr["c_cent"]), arr["c_winner"])
    hn = F.model_hn(arr["l2_cent"])
    assert np.array_equal(F.model_labels(arr["l2_tok"], arr["l2_cent"])[0], arr["l2_winner"])
    assert np.array_equal(KM.assign(arr["l2_tok"], arr["l2_cent"], hn), arr["l2_winner"])


@pytest.mark.parametrize("dim", F.O_DIMS)
def test_order_twins_under_the_aten_restatement(dim):
    """The existing tests treat ATen's half matmul and the header's chain as the same thing; on order twins that is a statement
    about ATen's summation order.  The header governs the device assertions; this test records whether ATen agrees."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import plaid_oracle_torch as OT
    arr = order_twins(dim)
    aten = OT.compress_into_codes(torch.from_numpy(arr["c_tok"]), torch.from_numpy(arr["c_cent"])).numpy()
    bad = np.flatnonzero(aten != arr["c_winner"])
    print(f"dim {dim}: ATen differs from the chain model on {bad.size} of {aten.size} order-twin tokens")
    assert bad.size == 0, bad[:8].tolist()
