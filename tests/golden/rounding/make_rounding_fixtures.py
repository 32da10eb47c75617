"""Generator of tests/golden/rounding/*.npz: index arrays and queries CONSTRUCTED to sit on or next to fp16 rounding boundaries,
the inputs the two certification windows (include/fastplaid.h, "CERTIFICATION WINDOWS") had never been shown.  Seeded, pure numpy,
reads nothing but tests/s1_window_model.py; rerunning it reproduces the committed files byte for byte (the archives are written
with fixed time stamps).  Run:  python tests/golden/rounding/make_rounding_fixtures.py [--check]

  family_a.npz      "exact grid".  Every entry is a small integer times a power of two (2^-7; a block of centroids and some query
                    rows on 2^-13) with sum |c_k q_k| below 2^24 grid units: every dot product is exact in fp32 in ANY summation
                    order and known from integer arithmetic.  Each token h(c + w) has a sum of squares that is a power of 4, so its
                    fp16 norm is a power of two and the normalised token stays on the grid.  Centroids come in RUNS c + i e_k
                    against query rows with q_k = +-1 grid unit, which makes the scores runs of consecutive integers: fp16
                    midpoints (ties to even, both directions), their neighbours one grid step away, fp16 subnormals, and -- from a
                    tile of sparse rows -- exact zeros.
  family_b.npz      "same-sign chains", dim 128.  Every entry is +-a or +-b for two fp16 amplitudes in [0.04, 0.125]; centroids are
                    copies of query tokens with 0..4 entries changed.  The products nearly all have the same sign, the chain's
                    roundings add up instead of cancelling.  pairs_diff: (query token, centroid) pairs found by the directed CPU
                    search below for which h(chain) != h(fl32(exact)) although no fp16 boundary lies within the window recorded in
                    the file of ANY x within +-8 fp32 ulp of the exact sum.  pairs_viol: pairs with |chain - x| > u and no fp16
                    difference.  pairs_near: further near-copies whose products all have one sign, those with the largest
                    |chain - x| / u of a random draw, so that EVERY query token has its near-copy centroid in the table whatever
                    the search found.
  family_b_d64.npz  the same family at dim 64 (the search found no difference and no window violation there -- the counts are
                    recorded; the table holds pairs_near only).
  family_c.npz      "MaxSim self-match": B's centroids, all bucket weights zero, short documents; the queries are rows of the
                    decompressed documents, so a query token equals a document token bit for bit.  cols_diff: (query, column,
                    document) triples whose reference column maximum differs from h(fl32(exact)) with no boundary within
                    2^-19 |q_col| (possibly none: the count is recorded)."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import s1_window_model as M  # noqa: E402

NBITS = 2
DIM = 128
Q_LEN = 32


# ------------------------------------------------------------------------------------------------------------------------------
# plumbing
def write_npz(path, arrays):
    """an .npz np.load reads, with fixed member time stamps (np.savez stamps the members with the wall clock)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(b, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())


def build_ivf(codes, lens, n_lists):
    """per centroid the ascending unique ids of the documents that hold it"""
    pid = np.repeat(np.arange(lens.shape[0], dtype=np.int64), lens)
    key = np.unique(codes.astype(np.int64) * np.int64(lens.shape[0]) + pid)
    cell = key // np.int64(lens.shape[0])
    return (key - cell * np.int64(lens.shape[0])).astype(np.int64), np.bincount(cell, minlength=n_lists).astype(np.int32)


def _rev_seg(v, nbits):
    r = np.zeros_like(v)
    for k in range(nbits):
        r |= ((v >> k) & 1) << (nbits - 1 - k)
    return r


def pack_residuals(widx, nbits=NBITS):
    """[T, dim] bucket indices -> [T, dim * nbits / 8] residual bytes as the index stores them: the first dimension of a byte in
    its top bits, every nbits-wide field bit-reversed (the reference's decompression undoes both)"""
    T, dim = widx.shape
    per = 8 // nbits
    v = widx.reshape(T, dim // per, per).astype(np.uint32)
    out = np.zeros((T, dim // per), np.uint32)
    for j in range(per):
        out |= _rev_seg(v[:, :, j], nbits) << ((per - 1 - j) * nbits)
    return out.astype(np.uint8)


def unpack_residuals(res, nbits=NBITS):
    T, pd = res.shape
    per = 8 // nbits
    out = np.zeros((T, pd, per), np.uint32)
    r = res.astype(np.uint32)
    for j in range(per):
        out[:, :, j] = _rev_seg((r >> ((per - 1 - j) * nbits)) & ((1 << nbits) - 1), nbits)
    return out.reshape(T, pd * per).astype(np.int64)


def decompress(cent, weights, codes, widx):
    """the reference's token reconstruction: e = h(w + c) per dimension, norm = h(sqrt(fp32 ascending sum of squares)),
    token = h(e / norm)"""
    e = (weights[widx].astype(np.float32) + cent[codes].astype(np.float32)).astype(np.float16)
    ss = np.zeros(e.shape[0], np.float32)
    for k in range(e.shape[1]):
        x = e[:, k].astype(np.float32)
        ss = (ss + (x * x).astype(np.float32)).astype(np.float32)
    n = np.sqrt(ss, dtype=np.float32).astype(np.float16).astype(np.float32)
    return (e.astype(np.float32) / n[:, None]).astype(np.float16)


def index_arrays(cent, weights, codes, res, lens):
    ivf, ivf_lengths = build_ivf(codes, lens, cent.shape[0])
    nb = int(np.log2(weights.shape[0]))
    return dict(nbits=np.int64(nb), centroids=cent.astype(np.float16), avg_residual=np.zeros(cent.shape[1], np.float16),
                bucket_cutoffs=np.zeros((1 << nb) - 1, np.float16), bucket_weights=weights.astype(np.float16), ivf=ivf,
                ivf_lengths=ivf_lengths, doc_codes=codes.astype(np.int64), doc_residuals=res.astype(np.uint8),
                doc_lengths=lens.astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------------------
# classification of exact scores (integers in grid units) against the fp16 grid
CATS = ("mid_even_down", "mid_even_up", "next_to_mid", "subnormal", "zero")


def classify(ints, log2_unit):
    """counts of exact values i * 2^log2_unit per category.  A value is a MIDPOINT when it lies exactly between two neighbouring fp16
    values (even_down: round-to-nearest-even takes the smaller magnitude); next_to_mid: one grid step away from a midpoint and not
    representable itself."""
    i = np.abs(np.asarray(ints, np.int64)).ravel()
    v = i.astype(np.float64) * 2.0 ** log2_unit
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    ulp_i = np.rint(2.0 ** (e - 10 - log2_unit))            # one fp16 step in grid units (>= 1 wherever rounding can happen)
    out = dict.fromkeys(CATS, 0)
    out["zero"] = int((i == 0).sum())
    out["subnormal"] = int(((i > 0) & (v < 2.0 ** -14)).sum())
    r = ulp_i >= 2
    u = np.where(r, ulp_i, 2).astype(np.int64)
    rem = i % u
    mid = r & (rem == u // 2)
    down = mid & ((i // u) % 2 == 0)
    out["mid_even_down"], out["mid_even_up"] = int(down.sum()), int((mid & ~down).sum())
    out["next_to_mid"] = int((r & (u >= 4) & ((rem == u // 2 - 1) | (rem == u // 2 + 1))).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# family A
A_UNIT = -7          # centroid / query / weight entries are integers * 2^-7 ...
A_TINY = -13         # ... except the tiny block and the tiny query rows: integers * 2^-13
A_TARGET = 4 ** 7    # sum of squares of a token's integers: norm = 2^7 grid units = 1.0


def _token_indices(rng, c_int, w_int, target, tries=4000):
    """bucket indices r [dim] with sum (c + w[r])^2 == target: random draws, then one coordinate moved to close the gap"""
    dim = c_int.shape[0]
    r = rng.integers(0, w_int.shape[0], (tries, dim))
    t = c_int[None, :] + w_int[r]
    gap = target - (t * t).sum(axis=1)
    hit = np.nonzero(gap == 0)[0]
    if hit.size:
        return r[hit[0]]
    for i in np.argsort(np.abs(gap), kind="stable")[:200]:
        # moving coordinate k to bucket j changes the sum by (c_k + w_j)^2 - t_k^2
        delta = (c_int[:, None] + w_int[None, :]) ** 2 - (t[i] ** 2)[:, None]
        k, j = np.nonzero(delta == gap[i])
        if k.size:
            out = r[i].copy()
            out[k[0]] = j[0]
            return out
    return None


def family_a(rng):
    dim = DIM
    w_int = np.array([-2, -1, 1, 2], np.int64)
    # tile 0: eight runs of sixteen centroids, base + i e_k.  Base rows of sum of squares a little under the target, so that tokens
    # base + w reach it.
    cent = np.zeros((384, dim), np.int64)
    run_k = np.zeros(8, np.int64)
    bases = np.zeros((8, dim), np.int64)
    for g in range(8):
        b = np.rint(rng.standard_normal(dim) * 11.2).astype(np.int64)
        bases[g], run_k[g] = b, g * 16 + 3
        for i in range(16):
            cent[g * 16 + i] = b
            cent[g * 16 + i, run_k[g]] += i
    # tile 1: sparse rows (one to three non-zero entries): zero scores against nearly every query row
    # (the first 96 only in the last 32 coordinates, off the runs' coordinates: the query rows that copy only the head of a base
    # score exactly zero against them as well)
    tail = np.setdiff1d(np.arange(96, dim), run_k)
    for r in range(128, 256):
        nz = rng.integers(1, 4)
        cent[r, rng.choice(tail if r < 224 else dim, nz, replace=False)] = rng.integers(1, 24, nz) * rng.choice([-1, 1], nz)
    # tile 2: 64 tiny rows (run base + i e_k on the 2^-13 grid; stored as integers of THAT grid), 64 ordinary rows
    tiny_base = rng.integers(-6, 7, dim)
    for i in range(64):
        cent[256 + i] = tiny_base
        cent[256 + i, 5] += i
    cent[320:] = np.rint(rng.standard_normal((64, dim)) * 11.2).astype(np.int64)
    scale = np.full(384, 2.0 ** A_UNIT)
    scale[256:320] = 2.0 ** A_TINY
    cent_f = (cent * scale[:, None]).astype(np.float16)
    weights = (w_int * 2.0 ** A_UNIT).astype(np.float16)

    # documents: codes among the run rows, the sparse rows and the ordinary rows (the tiny block is in the table only)
    usable = np.concatenate([np.arange(0, 256), np.arange(320, 384)])
    n_docs = 160
    lens = rng.integers(1, 7, n_docs).astype(np.int64)
    lens[:40] = 1
    codes, widx = [], []
    for _ in range(int(lens.sum())):
        while True:
            c = int(rng.choice(usable))
            target = A_TARGET if not 128 <= c < 256 else 4 ** 4     # sparse rows: tokens of small integers, norm 2^4 grid units
            r = _token_indices(rng, cent[c], w_int, target)
            if r is not None:
                break
        codes.append(c)
        widx.append(r)
    codes, widx = np.array(codes, np.int64), np.array(widx, np.int64)
    res = pack_residuals(widx)

    # queries [4, 32, dim] in integers; unit per row
    q = np.zeros((4, Q_LEN, dim), np.int64)
    q_unit = np.full((4, Q_LEN), A_UNIT)
    for b in range(4):
        for t in range(Q_LEN):
            kind = (t + b) % 8
            g = (t // 2 + 3 * b) % 8
            if kind in (0, 1, 2):            # near-copy of a run's base; part of it, to reach the lower binades
                keep = dim if kind == 0 else (dim // 2 if kind == 1 else dim // 4)
                q[b, t, :keep] = bases[g, :keep]
                q[b, t, :keep] += (rng.integers(-1, 2, dim) * (rng.random(dim) < 0.2))[:keep]
                q[b, t, run_k[g]] = 1 if t % 4 < 2 else -3
            elif kind == 3:                  # a token of the corpus (the approximate and the exact stage see a self-match)
                i = int(rng.integers(0, codes.shape[0]))
                q[b, t] = cent[codes[i]] + w_int[widx[i]]
            elif kind == 4:                  # tiny row: subnormal scores against the tiny block, +-1 on its run coordinate
                q[b, t] = rng.integers(-3, 4, dim) * (rng.random(dim) < 0.5)
                q[b, t, 5] = 1 if t % 2 else -1
                q_unit[b, t] = A_TINY
            elif kind == 5:                  # one or two non-zero entries: exact zeros against most rows
                nz = 1 + t % 2
                q[b, t, rng.choice(dim, nz, replace=False)] = rng.integers(1, 16, nz)
            elif kind == 6:                  # tiny and sparse: subnormal column maxima
                q[b, t, rng.choice(dim, 2, replace=False)] = rng.choice([-1, 1], 2)
                q_unit[b, t] = A_TINY
            else:                            # ordinary dense row
                q[b, t] = np.rint(rng.standard_normal(dim) * 11.2).astype(np.int64)
    q[3, Q_LEN - 6:] = 0                     # a padded query: zero rows
    q_f = (q * 2.0 ** q_unit[:, :, None]).astype(np.float16)
    assert np.array_equal(q_f.astype(np.float64), q * 2.0 ** q_unit[:, :, None]) and np.array_equal(cent_f.astype(np.float64), cent * scale[:, None])

    arr = index_arrays(cent_f, weights, codes, res, lens)
    arr["queries"] = q_f
    # integer images for the CPU test: value = int * 2^log2_unit
    arr["cent_int"], arr["cent_log2_unit"] = cent.astype(np.int16), np.log2(scale).astype(np.int64)
    arr["q_int"], arr["q_log2_unit"] = q.astype(np.int16), q_unit.astype(np.int64)
    s_counts, m_counts = family_a_counts(arr)
    arr["s_counts"], arr["m_counts"] = (np.array([c[k] for k in CATS], np.int64) for c in (s_counts, m_counts))   # in the order of CATS
    return arr


def family_a_counts(arr):
    """category counts of the centroid scores and of the per-document column maxima, from integer arithmetic"""
    cent, cu, q, qu = arr["cent_int"].astype(np.int64), arr["cent_log2_unit"], arr["q_int"].astype(np.int64), arr["q_log2_unit"]
    qf = q.reshape(-1, q.shape[2])
    nzrow = (qf != 0).any(axis=1)
    S = cent @ qf.T                                            # [C, B*Q] int64, exact
    assert (np.abs(cent) @ np.abs(qf.T)).max() < 1 << 24, "a partial sum could leave fp32's exact range"
    s_counts = dict.fromkeys(CATS, 0)
    for u_c in np.unique(cu):
        for u_q in np.unique(qu):
            sel = S[np.ix_(cu == u_c, (qu.ravel() == u_q) & nzrow)]
            for k, v in classify(sel, int(u_c + u_q)).items():
                s_counts[k] += v
    # tokens in integers of 2^-7 (sparse-row tokens are normalised by 2^4 grid units -> scaled by 8: value = int * 2^-7 * 2^3)
    codes, widx = arr["doc_codes"], unpack_residuals(arr["doc_residuals"])
    w_int = np.rint(arr["bucket_weights"].astype(np.float64) * 2.0 ** -A_UNIT).astype(np.int64)
    tok = cent[codes] + w_int[widx]
    tok_unit = np.where((codes >= 128) & (codes < 256), A_UNIT + 3, A_UNIT)      # after the division by the norm (2^7 resp. 2^4 grid units)
    off = np.concatenate([[0], np.cumsum(arr["doc_lengths"])])
    T = tok @ qf.T                                             # [tokens, B*Q]
    m_counts = dict.fromkeys(CATS, 0)
    for u_q in np.unique(qu):
        cols = np.nonzero(qu.ravel() == u_q)[0]
        # column maxima in the common unit 2^(A_UNIT + u_q): sparse-row tokens count 8 units
        Tc = T[:, cols] * np.where(tok_unit == A_UNIT, 1, 8)[:, None]
        mx = np.stack([Tc[off[d]:off[d + 1]].max(axis=0) for d in range(len(off) - 1)])
        for k, v in classify(mx, int(A_UNIT + u_q)).items():
            m_counts[k] += v
    return s_counts, m_counts


# ------------------------------------------------------------------------------------------------------------------------------
# family B
B_AMP_LO, B_AMP_HI = 0.04, 0.125
B_SEARCH_SPECS = 64_000_000    # the budget: (a, b, product counts) combinations whose exact sum is computed (integer arithmetic, cheap) ...
B_SEARCH_CHUNK = 2_000_000     # ... in chunks of this many
B_SEARCH_ORDERS = 24           # random orders of the entries tried per combination that passes the filter
B_SEARCH_CHAINS = 4_000_000    # at most this many chains are evaluated
B_MAX_DIFF = 48                # harvested pairs kept
B_N_VIOL = 208                 # window-violating pairs kept
B_N_NEAR = 240                 # further near-copies (all products of one sign, largest |chain - x| / u first) to fill the table with
# the window S1 shipped with when the fixture was made (w0, kappa as powers of two): what the pairs were harvested against.  Fixed
# here -- NOT s1_window_model's shipped constants, which follow the library -- so that the files stay what they are.
B_HARVEST_W0_LOG2, B_HARVEST_KAPPA_LOG2 = -21.5, -20.0
C_HARVEST_EPS_LOG2 = -19.0


def _amp_grid():
    bits = np.arange(0x2000, 0x3000, dtype=np.uint16)           # fp16 values in [2^-7, 2^-3)
    v = bits.view(np.float16)
    return v[(v >= np.float16(B_AMP_LO)) & (v <= np.float16(B_AMP_HI))]


def _build_pair(rng, dim, a, b, na, k_ab_a, k_ab_b, k_neg_a, k_neg_b):
    """query token: na entries of amplitude a, the others b, random signs and order.  Centroid: a copy, except that k_ab_a of the a
    entries hold b and k_ab_b of the b entries hold a (product a b), and k_neg_a / k_neg_b entries hold the other sign (product
    -a^2 / -b^2)."""
    amp = np.where(np.arange(dim) < na, a, b).astype(np.float16)
    sg = rng.choice([-1.0, 1.0], dim).astype(np.float16)
    camp, csg = amp.copy(), sg.copy()
    camp[:k_ab_a] = b
    csg[k_ab_a:k_ab_a + k_neg_a] *= -1
    camp[na:na + k_ab_b] = a
    csg[na + k_ab_b:na + k_ab_b + k_neg_b] *= -1
    perm = rng.permutation(dim)
    return (amp * sg)[perm].astype(np.float16), (camp * csg)[perm].astype(np.float16)


def _unflagged_all_shifts(x, w, kappa, width=8):
    ok = np.ones(np.shape(x), bool)
    for s in range(-width, width + 1):
        ok &= ~M.s1_flagged(M.shift_ulps(x, s), w, kappa)
    return ok


def search_b(rng, dim, w0_log2, kappa_log2):
    """directed search.  The exact sum of a pair depends only on the amplitudes and on how many products are a^2, b^2, a b and
    negative; the chain's rounding errors depend on the ORDER too.  So: draw combinations, keep those whose exact sum lies
    between one and two windows (plus 8 fp32 ulp) away from an fp16 boundary -- integer arithmetic only --, and run the chain for
    a number of random orders of those."""
    grid = _amp_grid()
    kappa = M.s1_kappa(dim, kappa_log2)
    found, viol, near, chains = [], [], [], 0
    for chunk in range(B_SEARCH_SPECS // B_SEARCH_CHUNK):
        if chains >= B_SEARCH_CHAINS or len(found) >= B_MAX_DIFF:
            break
        f, v, nr, n_ch = _search_b_chunk(rng, dim, w0_log2, kappa, grid, B_MAX_DIFF - len(found), chunk == 0)
        found += f
        viol += v
        near += nr
        chains += n_ch
    return found[:B_MAX_DIFF], viol, near, chains


def _search_b_chunk(rng, dim, w0_log2, kappa, grid, want, with_viol):
    n = B_SEARCH_CHUNK
    a, b = grid[rng.integers(0, grid.size, n)], grid[rng.integers(0, grid.size, n)]
    na = rng.integers(4, dim - 3, n)                                     # (at least four entries of either amplitude: room for the changes)
    k = rng.integers(0, 3, (n, 4)) * (rng.random((n, 4)) < 0.25)          # k_ab_a, k_ab_b, k_neg_a, k_neg_b: 0 .. 2 each, mostly 0
    k[k.sum(axis=1) > 4] = 0
    nb = dim - na
    A, Bv = (a.astype(np.float64) * 2.0 ** 24).astype(np.int64), (b.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    ex = (na - k[:, 0] - 2 * k[:, 2]) * A * A + (nb - k[:, 1] - 2 * k[:, 3]) * Bv * Bv + (k[:, 0] + k[:, 1]) * A * Bv   # units of 2^-48
    qq = (na * A * A + nb * Bv * Bv).astype(np.float64) * 2.0 ** -48
    cc = ((na - k[:, 0] + k[:, 1]) * A * A + (nb - k[:, 1] + k[:, 0]) * Bv * Bv).astype(np.float64) * 2.0 ** -48
    x = M.fl32_of_int(ex)
    w = (np.float32(np.exp2(np.float32(w0_log2))) * M.dim_scale(dim) * np.sqrt(qq)).astype(np.float32)   # (the filter's estimate; pairs are verified with wcol)
    u = M.s1_u(x, w, kappa).astype(np.float64)
    d = M.boundary_distance(ex.astype(np.float64) * 2.0 ** -48)
    band = (cc <= 1.0) & (a != b) & (d > u + 9 * np.spacing(np.abs(x)).astype(np.float64)) & (d < 2.0 * u)
    cand = np.nonzero(band)[0]
    found, chains = [], 0
    for start in range(0, cand.size, 4096):
        if len(found) >= want:
            break
        idx = cand[start:start + 4096]
        for o in range(B_SEARCH_ORDERS):
            if idx.size == 0:
                break
            pr = [_build_pair(rng, dim, a[i], b[i], int(na[i]), *(int(v) for v in k[i])) for i in idx]
            qp, cp = np.array([p[0] for p in pr]), np.array([p[1] for p in pr])
            assert np.array_equal(M.exact_dot_int(cp, qp), ex[idx])
            ch = M.chain32(cp, qp)
            chains += idx.size
            hit = (M.h_bits(ch) != M.h_bits(x[idx])) & _unflagged_all_shifts(x[idx], M.wcol(qp, 1.0, dim, w0_log2), kappa)
            for j in np.nonzero(hit)[0]:
                found.append((qp[j].copy(), cp[j].copy()))
            idx = idx[~hit]                                      # one order per combination
    if not with_viol:
        return found, [], [], chains
    # window violations without an fp16 difference: plain random combinations
    sel = np.nonzero((cc <= 1.0) & (a != b))[0][:24 * B_N_VIOL]
    pr = [_build_pair(rng, dim, a[i], b[i], int(na[i]), *(int(v) for v in k[i])) for i in sel]
    qp, cp = np.array([p[0] for p in pr]), np.array([p[1] for p in pr])
    ch = M.chain32(cp, qp)
    uu = M.s1_u(x[sel], M.wcol(qp, 1.0, dim, w0_log2), kappa).astype(np.float64)
    v = (np.abs(ch.astype(np.float64) - ex[sel].astype(np.float64) * 2.0 ** -48) > 1.02 * uu) & (M.h_bits(ch) == M.h_bits(x[sel]))
    viol = [(qp[j].copy(), cp[j].copy()) for j in np.nonzero(v)[0][:B_N_VIOL]]
    # ... and, whatever the search finds, the near-copies of the same draw whose chain comes closest to the window's edge, among
    # those whose products ALL have one sign: the table holds same-sign chains also where nothing violates the window (dim 64)
    ratio = np.abs(ch.astype(np.float64) - ex[sel].astype(np.float64) * 2.0 ** -48) / uu
    ratio[v | (k[sel, 2] + k[sel, 3] > 0)] = -1.0
    order = np.argsort(-ratio, kind="stable")[:B_N_NEAR]
    near = [(qp[j].copy(), cp[j].copy()) for j in order if ratio[j] >= 0]
    return found, viol, near, chains


def family_b(rng, dim, n_cent):
    found, viol, near, chains = search_b(rng, dim, B_HARVEST_W0_LOG2, B_HARVEST_KAPPA_LOG2)
    n_q = 8 * Q_LEN
    pairs = (found + viol + near)[:n_q]                 # every query token is one member of a near-copy pair
    n_diff = min(len(found), n_q)
    n_viol = min(len(viol), n_q - n_diff)
    grid = _amp_grid()
    # query tokens: the pairs' first members, then palette rows
    qtok, cent = [p[0] for p in pairs], [p[1] for p in pairs]

    def palette():
        while True:
            q, _ = _build_pair(rng, dim, grid[rng.integers(0, grid.size)], grid[rng.integers(0, grid.size)], int(rng.integers(0, dim + 1)), 0, 0, 0, 0)
            if (q.astype(np.float64) ** 2).sum() <= 1.0:
                return q
    while len(qtok) < n_q:
        qtok.append(palette())
    while len(cent) < n_cent:
        cent.append(palette())
    qtok, cent = np.array(qtok), np.array(cent)
    # spread the near-copies over the table's tiles and the query tokens over the queries
    prow, pq = rng.permutation(n_cent), rng.permutation(n_q)
    cent_t, q_t = np.zeros_like(cent), np.zeros_like(qtok)
    cent_t[prow], q_t[pq] = cent, qtok
    pair_idx = np.stack([pq[:len(pairs)], prow[:len(pairs)]], axis=1).astype(np.int64)      # (flat query token, centroid row)
    assert M.cent_norm_max(cent_t) == np.float32(1.0)
    # documents: up to eight tokens, every near-copy centroid in at least one of them; ordinary weights, random residual bytes
    n_docs = 300
    lens = rng.integers(1, 9, n_docs).astype(np.int64)
    T = int(lens.sum())
    codes = rng.integers(0, n_cent, T)
    slots = rng.permutation(T)[:len(pairs)]
    codes[slots] = pair_idx[:, 1]
    res = rng.integers(0, 256, (T, dim * NBITS // 8)).astype(np.uint8)
    weights = np.array([-0.0575, -0.0159, 0.0159, 0.0575], np.float32).astype(np.float16)
    arr = index_arrays(cent_t, weights, codes, res, lens)
    arr["queries"] = q_t.reshape(8, Q_LEN, dim)
    arr["pairs_diff"], arr["pairs_viol"], arr["pairs_near"] = pair_idx[:n_diff], pair_idx[n_diff:n_diff + n_viol], pair_idx[n_diff + n_viol:]
    arr["window_log2"] = np.array([B_HARVEST_W0_LOG2, B_HARVEST_KAPPA_LOG2], np.float64)    # the constants the pairs were harvested under
    arr["search_chains"] = np.int64(chains)
    return arr


# ------------------------------------------------------------------------------------------------------------------------------
# family C
def c_column_maxima(tok, off, q):
    """per (document, query column): fp32 maximum of the chains and of the fp32-rounded exact sums"""
    n_docs = len(off) - 1
    ch = np.stack([M.chain32(tok, q[j][None, :]) for j in range(q.shape[0])], axis=1)                       # [T, Q]
    ex = np.stack([M.fl32_of_int(M.exact_dot_int(tok, q[j][None, :])) for j in range(q.shape[0])], axis=1)
    mc = np.stack([ch[off[d]:off[d + 1]].max(axis=0) for d in range(n_docs)])
    mx = np.stack([ex[off[d]:off[d + 1]].max(axis=0) for d in range(n_docs)])
    return mc, mx


def family_c(rng, b_arr):
    cent = b_arr["centroids"]
    dim = cent.shape[1]
    weights = np.zeros(1 << NBITS, np.float16)
    n_docs = 300
    lens = rng.integers(1, 6, n_docs).astype(np.int64)
    T = int(lens.sum())
    codes = rng.integers(0, cent.shape[0], T)
    near = np.concatenate([b_arr["pairs_diff"][:, 1], b_arr["pairs_viol"][:, 1], b_arr["pairs_near"][:, 1]])
    codes[rng.permutation(T)[:near.size]] = near
    widx = np.zeros((T, dim), np.int64)
    res = pack_residuals(widx)
    tok = decompress(cent, weights, codes, widx)
    off = np.concatenate([[0], np.cumsum(lens)])
    # candidate query rows: every token against the documents; keep the rows with most unflagged differences, fill with the rest
    eps_all = M.maxsim_eps(tok, dim, C_HARVEST_EPS_LOG2)
    score = np.zeros(T, np.int64)
    for s in range(0, T, 64):
        mc, mx = c_column_maxima(tok, off, tok[s:s + 64])
        bad = (M.h_bits(mc) != M.h_bits(mx)) & ~M.maxsim_flagged(mx, eps_all[None, s:s + 64])
        score[s:s + 64] = bad.sum(axis=0)
    order = np.argsort(-score, kind="stable")
    n_q = 8 * Q_LEN
    pick = order[:n_q]
    pick = pick[rng.permutation(n_q)]
    q = tok[pick].reshape(8, Q_LEN, dim)
    diff = []
    for b in range(8):
        mc, mx = c_column_maxima(tok, off, q[b])
        bad = (M.h_bits(mc) != M.h_bits(mx)) & ~M.maxsim_flagged(mx, M.maxsim_eps(q[b], dim, C_HARVEST_EPS_LOG2)[None, :])
        for d, j in zip(*np.nonzero(bad)):
            diff.append((b, j, d))
    arr = index_arrays(cent, weights, codes, res, lens)
    arr["queries"] = q
    arr["query_tokens"] = pick.astype(np.int64)        # the corpus tokens the query rows were taken from
    arr["cols_diff"] = np.array(diff, np.int64).reshape(-1, 3)
    arr["eps_log2"] = np.float64(C_HARVEST_EPS_LOG2)
    return arr


# ------------------------------------------------------------------------------------------------------------------------------
def generate():
    out = {}
    out["family_a"] = family_a(np.random.default_rng(20260101))
    out["family_b"] = family_b(np.random.default_rng(20260102), 128, 512)
    out["family_b_d64"] = family_b(np.random.default_rng(20260103), 64, 256)
    out["family_c"] = family_c(np.random.default_rng(20260104), out["family_b"])
    return out


def main():
    check = "--check" in sys.argv
    out = generate()
    s_counts, m_counts = family_a_counts(out["family_a"])
    print("family_a  centroid scores :", s_counts)
    print("family_a  column maxima   :", m_counts)
    for k in CATS:
        assert s_counts[k] > 0, f"family A: no centroid score in category {k}"
        assert m_counts[k] > 0, f"family A: no column maximum in category {k}"
    for name in ("family_b", "family_b_d64"):
        a = out[name]
        print(f"{name}: {a['pairs_diff'].shape[0]} unflagged differences, {a['pairs_viol'].shape[0]} window violations without a "
              f"difference, {a['pairs_near'].shape[0]} further near-copies, {int(a['search_chains'])} chains evaluated")
    print(f"family_c: {out['family_c']['cols_diff'].shape[0]} unflagged column differences")
    for name, arr in out.items():
        path = os.path.join(HERE, name + ".npz")
        if check:
            tmp = io.BytesIO()
            write_npz(tmp, arr)
            with open(path, "rb") as f:
                assert f.read() == tmp.getvalue(), f"{name}.npz differs from what the generator writes"
        else:
            write_npz(path, arr)
        print(name, "ok" if check else "written")


if __name__ == "__main__":
    main()
