"""Constructed inputs for the nearest-centroid assignment (fp_compress, fp_assign_l2, fp_kmeans, fp_centroid_outliers): near-ties,
fp16 rounding edges and fp16 overflow, the inputs drawn corpora never hold.  Seeded, pure numpy, reads nothing but
tests/s1_window_model.py.  Families G, GL and X are cheap and are produced by these functions at test time; family O needs a
search and is committed (o_d128.npz, o_d136.npz; rerunning reproduces the files byte for byte, fixed time stamps).
Run:  python tests/golden/assign/make_assign_fixtures.py [--check]

Expected codes and labels come from MODEL below: one ascending-k fp32 chain per (token, centroid), h() of it (compress form) or
fl32(chain - hn) (L2 form), first maximal index -- include/fastplaid.h's statement, no library matmul.

  G   "exact grid", compress form.  Entries are small integers times 2^-7 with sum |x_k c_k| < 2^24 grid units: every dot product
      is exact in fp32 in any order and known from integer arithmetic.  A token's GROUP is a run of centroids base + i e_k against
      x_k = +-1: consecutive integer scores at the top of its score list, every other centroid below a gap (GAP below).  Groups:
      top-n scores that round to ONE fp16 value (n = 2, 3, 8 | 9, 12; the largest exact score at the highest index, members spread
      over 128-centroid tiles, both 64-column halves and both 32-column halves of a wave), the top score on an fp16 midpoint with a
      neighbour one grid step away (ties-to-even towards and away from the neighbour), all scores negative, all scores subnormal
      (a token on the 2^-13 grid), an all-zero token, a token whose scores are all equal.  Corpus "le8" holds the tokens with at
      most 8 candidates, "ge9" those with 9 or more: fp_compress_last_counts is (1, 1, 0) resp. (1, 1, 1).
  GL  the same grid in the L2 form (score = dot - hn, both exact): exact fp32 ties between centroids of different dot and different
      hn, and pairs one grid step apart that an fp16 rounding would merge.
  X   integer grid, scores beyond fp16's range: two +inf scores (70000 at the lower, 100000 at the higher index), the edge pair
      65519 -> 65504 / 65520 -> +inf, a single +inf at a high index, and tokens whose scores are ALL <= -65520 (code 0).
  O   "order twins": same-sign chains of two fp16 amplitudes in [0.04, 0.125]; centroid c' is c with entries exchanged between
      positions where the token holds the same value -- the same multiset of exact products, the same exact sum, another order.
      Compress triples: h(chain(x, c)) != h(chain(x, c')).  L2 triples: fl32(chain - hn) differs.  The file records the number of
      chains the search evaluated and the number of triples it found.

GAP: every centroid outside a token's group scores at least 4 W below the group's reference value, W an upper bound of the window
the narrowing can use -- compress: 2^-8 max(|m|, 2^-14) + 4 D 2^-23 l1(x) max|c|; L2: 4 (D 2^-23 l1(x) max|c| + 2^-22 (l1(x) max|c| +
max hn)) -- and every member lies within one fp16 step (L2: exactly on) the reference value.  The candidate count of a token is
then its group size by construction, whatever window (between one fp16 step and W) the code under test uses."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import s1_window_model as M  # noqa: E402

NBITS = 2
G_DIMS = (8, 72, 128, 136, 264, 1024)
G_EXTRA_DIMS = (64,)        # the other dim with a fixed-dim MFMA kernel (FP_TEST=assign_sliced=1 sends 64 and 128 through the sliced one)
GL_DIMS = (72, 128, 256)
X_DIMS = (128, 136)
O_DIMS = (128, 136)
HALF_INF = 65520            # h(x) = +inf from here on
MAXG = 12                   # the largest constructed group that is listed member by member


# ------------------------------------------------------------------------------------------------------------------------------
# MODEL: the header's arithmetic
def chain_scores(x16, c16):
    """[T, C] fp32: ascending-k chain of every (token, centroid) pair; a product of two fp16 values is exact in fp32"""
    x, c = np.asarray(x16, np.float16).astype(np.float32), np.asarray(c16, np.float16).astype(np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc += x[:, k, None] * c[None, :, k]
    return acc


def model_codes(x16, c16):
    """codes[t] = argmax_c h(chain), first maximal index"""
    with np.errstate(over="ignore"):
        return np.argmax(chain_scores(x16, c16).astype(np.float16), axis=1).astype(np.int64)


def model_hn(c16):
    """hn[c] = 0.5f * ascending-d fp32 chain of c[d]^2"""
    c = np.asarray(c16, np.float16).astype(np.float32)
    acc = np.zeros(c.shape[0], np.float32)
    for k in range(c.shape[1]):
        acc = acc + c[:, k] * c[:, k]
    return (np.float32(0.5) * acc).astype(np.float32)


def model_labels(x16, c16, hn=None):
    """labels[t] = argmax_c fl32(chain - hn[c]), first maximal index -> (labels, scores [T, C])"""
    s = chain_scores(x16, c16) - (model_hn(c16) if hn is None else hn)[None, :]
    return np.argmax(s, axis=1).astype(np.int64), s


def model_residuals(x16, c16, codes, cutoffs16, nbits=NBITS):
    """r = h(x - c[code]); bucket = #{i : cutoffs[i] < r}; every bucket as nbits bits LSB first, the stream packed big-endian"""
    r = (np.asarray(x16, np.float16).astype(np.float32) - np.asarray(c16, np.float16)[codes].astype(np.float32)).astype(np.float16)
    bucket = (np.asarray(cutoffs16, np.float16).astype(np.float32)[None, None, :] < r.astype(np.float32)[:, :, None]).sum(axis=2)
    per = 8 // nbits
    v = bucket.reshape(r.shape[0], r.shape[1] // per, per).astype(np.uint32)
    out = np.zeros(v.shape[:2], np.uint32)
    for j in range(per):
        f = np.zeros_like(out)
        for kbit in range(nbits):
            f |= ((v[:, :, j] >> kbit) & 1) << (nbits - 1 - kbit)
        out |= f << ((per - 1 - j) * nbits)
    return out.astype(np.uint8)


def window_bound(form, dim, l1, cmax, m_abs=0.0, hnmax=0.0):
    """W of the module docstring, in float64"""
    if form == "l2":
        return 4.0 * (dim * 2.0 ** -23 * l1 * cmax + 2.0 ** -22 * (l1 * cmax + hnmax))
    return 2.0 ** -8 * np.maximum(m_abs, 2.0 ** -14) + 4.0 * dim * 2.0 ** -23 * l1 * cmax


def write_npz(path, arrays):
    """an .npz np.load reads, with fixed member time stamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(b, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())


# ------------------------------------------------------------------------------------------------------------------------------
# exact-grid builder (G, GL, X)
def _h16_of_int(i, log2_unit):
    """fp16 rounding of i * 2^log2_unit straight from the integer (one rounding, double -> half)"""
    with np.errstate(over="ignore"):
        return (np.asarray(i, np.int64).astype(np.float64) * 2.0 ** log2_unit).astype(np.float16)


def _solve(rng, x, free, k, target, b0):
    """integer centroid b: b0 moved by single steps on the free coordinates until x . b is within a small remainder of `target`,
    the remainder on coordinate k (x_k = +-1).  x . b == target exactly."""
    b = b0.copy()
    b[k] = 0
    diff = int(target) - int(x @ b)
    for _ in range(100000):
        ok = free[(x[free] != 0) & (np.abs(x[free]) <= abs(diff))]
        if abs(diff) <= 24 or ok.size == 0:
            break
        d = int(ok[rng.integers(ok.size)])
        s = 1 if diff > 0 else -1
        b[d] += s * (1 if x[d] > 0 else -1)
        diff -= s * abs(int(x[d]))
    b[k] = int(x[k]) * diff
    assert int(x @ b) == int(target) and abs(diff) <= 400, (diff, target)
    return b


def _spread(rng, n, taken, C):
    """n free centroid indices, ascending: at least min(n, 3) different 128-centroid tiles, both halves of a tile (c % 128 < 64 and
    >= 64) and both halves of a wave's 64 columns (c % 64 < 32 and >= 32) wherever n >= 2"""
    pool = np.setdiff1d(np.arange(C), np.fromiter(taken, np.int64, len(taken)))
    for _ in range(10000):
        idx = np.sort(rng.choice(pool, n, replace=False))
        if n == 1 or (np.unique(idx // 128).size >= min(n, 3) and np.unique(idx % 128 < 64).size == 2 and np.unique(idx % 64 < 32).size == 2):
            return idx
    raise AssertionError("no placement")


def _draw_x(rng, dim, free, norm2, k, toks):
    """integer token: normal entries on the free coordinates with a sum of squares near norm2, x_k = +-1; at a cosine below 0.5 to
    every earlier token (a small dim has few nearly orthogonal directions: another group's centroids must stay below the gap)"""
    while True:
        x = np.zeros(dim, np.int64)
        x[free] = np.rint(rng.standard_normal(free.size) * np.sqrt(norm2 / free.size)).astype(np.int64)
        if 0.8 * norm2 <= int(x @ x) <= 1.2 * norm2 and all(x @ t["x"] < 0.5 * np.sqrt(float(x @ x) * float(t["x"] @ t["x"]) + 1) for t in toks):
            break
    x[k] = 1 if rng.random() < 0.5 else -1
    return x


def _grid_table(rng, dim, C, norm2, free):
    """filler table: normal rows of a quarter of the tokens' sum of squares on the free coordinates"""
    cent = np.zeros((C, dim), np.int64)
    cent[:, free] = np.rint(rng.standard_normal((C, free.size)) * np.sqrt(norm2 / 4 / free.size)).astype(np.int64)
    return cent


def _finish(name, form, dim, cent_unit, cent, toks, rng, T):
    """common tail: corpora (every group's token repeated over rows, all groups once more in the last partial tile), fp16 arrays,
    group lists, integer scores, categories"""
    scale = 2.0 ** cent_unit[:, None]
    out = dict(name=name, form=form, dim=dim, cent_unit=cent_unit, cent_int=cent, cent=(cent * scale).astype(np.float16), corpora={})
    assert np.array_equal(out["cent"].astype(np.float64), cent * scale)
    for corpus in ("le8", "ge9"):
        grp = [t for t in toks if t["corpus"] == corpus]
        if not grp:
            continue
        n = T[corpus]
        assert n % 128 != 0 and len(grp) <= n % 128, (corpus, len(grp), n)
        order = np.concatenate([rng.permutation(len(grp)) for _ in range(n // len(grp) + 2)])[:n]
        order[n - len(grp):] = rng.permutation(len(grp))          # every group in the last partial tile
        x_int = np.stack([grp[g]["x"] for g in order])
        x_unit = np.array([grp[g]["x_unit"] for g in order], np.int64)
        tok = (x_int * 2.0 ** x_unit[:, None]).astype(np.float16)
        assert np.array_equal(tok.astype(np.float64), x_int * 2.0 ** x_unit[:, None])
        members = np.full((n, MAXG), -1, np.int64)
        for r, g in enumerate(order):
            m = grp[g]["members"]
            if m is not None:
                members[r, :len(m)] = m
        out["corpora"][corpus] = dict(tok=tok, x_int=x_int, x_unit=x_unit, kind=np.array([grp[g]["kind"] for g in order]),
                                      members=members, n_group=np.array([grp[g]["n"] for g in order], np.int64))
    out["cutoffs"] = (np.array([-2, 0, 2]) * 2.0 ** int(cent_unit.max())).astype(np.float16)
    return out


def family_g(dim, seed=None):
    """-> fixture dict (see _finish): table [400, dim], corpus le8 of 293 tokens, corpus ge9 of 163"""
    rng = np.random.default_rng(20261100 + dim if seed is None else seed)
    C, unit, A = 400, -7, 64
    k, z, y = 0, dim - 1, dim - 2
    free = np.arange(1, dim - 2)
    norm2 = 24000                                   # scores of a group near 24000 * 2^-14 = 1.46: one fp16 step = 16 grid units
    # coordinate z holds A in every row (a token with x_z != 0 moves ALL its scores), coordinate y small negative values (the
    # subnormal token's scores against the ordinary rows)
    cent = _grid_table(rng, dim, C, norm2, free)
    cent[:, z] = A
    cent[:, y] = -rng.integers(12, 41, C)
    cent_unit = np.full(C, unit)
    taken, toks = set(), []

    def group(kind, corpus, targets, x_z=0):
        """a token and its run: centroid i scores targets[0] + i exactly (consecutive targets), ascending with the index"""
        x = _draw_x(rng, dim, free, norm2, k, toks)
        x[z] = x_z
        v = targets(int(x @ x) - x_z * x_z + x_z * A)
        n = len(v)
        idx = _spread(rng, n, taken, C)
        taken.update(idx.tolist())
        b0 = x.copy()
        b0[z], b0[y] = A, cent[idx[0], y]
        base = _solve(rng, x, free, k, v[0], b0)
        for i, c in enumerate(idx):
            cent[c] = base
            cent[c, y] = -int(rng.integers(12, 41))
            cent[c, k] += int(x[k]) * (v[i] - v[0])
        toks.append(dict(kind=kind, corpus=corpus, x=x, x_unit=unit, members=idx, n=n))

    def top(n):      # n consecutive integers that all round to v (v / 16 even: v - 8 .. v + 8 do)
        return lambda s: [32 * (s // 32) - n // 2 + i for i in range(n)]

    def mid(parity, side):   # the midpoint M = v + 8 (side = +1) or v - 8 (side = -1) and its neighbour towards v, v / 16 of the given parity
        def f(s):
            v = 32 * (s // 32) + 16 * parity
            return [v + 7, v + 8] if side > 0 else [v - 8, v - 7]
        return f

    for rep in range(2):
        for n in (2, 3, 8):
            group(f"top{n}", "le8", top(n))
        for n in (9, 12):
            group(f"top{n}", "ge9", top(n))
        group("neg3", "le8", lambda s: [32 * (s // 32) - 1 + i for i in range(3)], x_z=-688)      # s = |x|^2 - 44032: about -20000
    group("mid_tie_below", "le8", mid(0, +1))       # M = v + 8 rounds DOWN to v and ties with v + 7 at the lower index
    group("mid_win_above", "le8", mid(1, +1))       # M = v + 8 rounds UP to v + 16 and beats v + 7
    group("mid_tie_above", "le8", mid(0, -1))       # M = v - 8 (lower index) rounds UP to v and ties with v - 7
    group("mid_lose_below", "le8", mid(1, -1))      # M = v - 8 rounds DOWN to v - 16 and loses to v - 7 at the higher index
    # all scores subnormal: x = 2^-13 e_y against a tiny block of four rows on the 2^-13 grid (z: A as everywhere, y: 199 .. 202):
    # scores 199 .. 202 units of 2^-26, one fp16 subnormal step = 4 units, all four round to 50 steps (202 = 50.5 ties to even);
    # the ordinary rows score c_y 2^-20 < 0
    idx = _spread(rng, 4, taken, C)
    taken.update(idx.tolist())
    cent[idx], cent_unit[idx] = 0, -13
    cent[idx, z], cent[idx, y] = A << 6, [199, 200, 201, 202]
    x = np.zeros(dim, np.int64)
    x[y] = 1
    toks.append(dict(kind="subnormal", corpus="le8", x=x, x_unit=-13, members=idx, n=4))
    x = np.zeros(dim, np.int64)
    toks.append(dict(kind="zero", corpus="ge9", x=x, x_unit=unit, members=None, n=C))
    x = np.zeros(dim, np.int64)
    x[z] = 3
    toks.append(dict(kind="equal", corpus="ge9", x=x, x_unit=unit, members=None, n=C))
    return _finish(f"g_d{dim}", "compress", dim, cent_unit, cent, toks, rng, dict(le8=293, ge9=163))


def family_x(dim, seed=None):
    """fp16 overflow: integer entries (unit 2^0), table [300, dim]"""
    rng = np.random.default_rng(20261300 + dim if seed is None else seed)
    C, unit, A = 300, 0, 128
    k, z = 0, dim - 1
    free = np.arange(1, dim - 1)
    norm2 = 66000
    cent = _grid_table(rng, dim, C, norm2, free)
    cent[:, z] = A
    taken, toks = set(), []

    def group(kind, targets, idx=None):
        idx = _spread(rng, len(targets), taken, C) if idx is None else np.asarray(idx)
        taken.update(idx.tolist())
        x = _draw_x(rng, dim, free, norm2, k, toks)
        b0 = x.copy()
        b0[z] = A
        for c, v in zip(idx, targets):
            cent[c] = _solve(rng, x, free, k, v, b0)
        toks.append(dict(kind=kind, corpus="le8", x=x, x_unit=unit, members=idx, n=len(targets)))

    taken.update([C - 3, 257])
    group("inf_pair", [70000, 100000], idx=[5, 9])
    group("inf_pair", [70000, 100000])
    group("inf_pair", [HALF_INF, 65536])
    group("edge", [65519, HALF_INF])                 # 65504 at the lower index, +inf at the higher
    group("edge", [65519, HALF_INF])
    group("inf_single", [80000], idx=[C - 3])
    group("inf_single", [HALF_INF], idx=[257])
    for _ in range(3):                               # every score <= -65520: x_z * A = -140800 under cross scores below 75000
        x = _draw_x(rng, dim, free, norm2, k, toks)
        x[z] = -1100
        toks.append(dict(kind="neg_inf_all", corpus="ge9", x=x, x_unit=unit, members=None, n=C))
    return _finish(f"x_d{dim}", "compress", dim, np.full(C, unit), cent, toks, rng, dict(le8=135, ge9=131))


def family_gl(dim, seed=None):
    """exact grid, L2 form: members are x + delta, score = (|x|^2 - |delta|^2) / 2"""
    rng = np.random.default_rng(20261200 + dim if seed is None else seed)
    C, unit = 300, -7
    free = np.arange(dim)
    norm2 = 24000
    cent = _grid_table(rng, dim, C, norm2, free)
    taken, toks = set(), []
    # |delta| = a: siblings of a group lie a^2 units of 2^-15 apart as tokens of their own, outside the gap of 4 W
    l1 = dim * 0.8 * np.sqrt(norm2 / dim) * 2.0 ** unit
    cmax = 5.0 * np.sqrt(norm2 / dim) * 2.0 ** unit
    a = int(np.ceil(np.sqrt(1.5 * 4 * window_bound("l2", dim, l1, cmax, hnmax=norm2 * 2.0 ** (2 * unit - 1)) * 2.0 ** 15))) + 2

    def group(kind, corpus, n, step=False):
        idx = _spread(rng, n, taken, C)
        taken.update(idx.tolist())
        while True:
            x = np.rint(rng.standard_normal(dim) * np.sqrt(norm2 / dim)).astype(np.int64)
            pos = rng.permutation(dim)
            pos = pos[np.unique(x[pos], return_index=True)[1]]      # coordinates that hold different values: different dots and hn
            if pos.size < n + 1:
                continue
            s = int(x @ x) - a * a
            if not step or _h16_of_int(s, 2 * unit - 1) == _h16_of_int(s - 1, 2 * unit - 1):
                break
        pos = rng.permutation(pos)
        for i, c in enumerate(idx):
            cent[c] = x
            cent[c, pos[i]] += a if rng.random() < 0.5 else -a
        if step:          # the lower index one grid step FARTHER: an fp16 rounding merges the two and takes it
            cent[idx[0], pos[n]] += 1
        toks.append(dict(kind=kind, corpus=corpus, x=x, x_unit=unit, members=idx, n=n))

    for rep in range(3):
        group("tie2", "le8", 2)
        group("tie3", "le8", 3)
        group("step", "le8", 2, step=True)
    group("tie8", "le8", 8)
    for rep in range(2):
        group("tie9", "ge9", 9)
    fx = _finish(f"gl_d{dim}", "l2", dim, np.full(C, unit), cent, toks, rng, dict(le8=165, ge9=133))
    # fp_kmeans is handed the table's rows as data rows: every row as a token of its own, nearest to itself
    members = np.full((C, MAXG), -1, np.int64)
    members[:, 0] = np.arange(C)
    fx["corpora"]["rows"] = dict(tok=fx["cent"], x_int=cent, x_unit=np.full(C, unit), kind=np.array(["self"] * C), members=members,
                                 n_group=np.ones(C, np.int64))
    return fx


# ------------------------------------------------------------------------------------------------------------------------------
# integer-arithmetic view of a fixture (CPU test, category counts)
def exact_scores(fx, corpus):
    """[T, C] float64, exact: the integer dot products scaled by their units (compress), 2 dot - |c|^2 scaled by its unit over 2
    (L2: dot - hn).  Asserts that every partial sum stays inside fp32's exact range."""
    c, cu, co = fx["cent_int"], fx["cent_unit"], fx["corpora"][corpus]
    x = co["x_int"]
    assert (np.abs(x) @ np.abs(c.T)).max() < 1 << 24, "outside fp32's exact range"
    S = x @ c.T
    if fx["form"] == "l2":
        assert (c * c).sum(axis=1).max() < 1 << 24
        S = 2 * S - (c * c).sum(axis=1)[None, :]
        assert np.abs(S).max() < 1 << 24
        return S.astype(np.float64) * 2.0 ** (2 * int(cu[0]) - 1)
    return S.astype(np.float64) * 2.0 ** (co["x_unit"][:, None] + cu[None, :])


def check_groups(fx, corpus):
    """the module docstring's GAP condition for every token of a corpus -> {kind: tokens}.  Integers and float64 only: nothing here
    depends on the code under test."""
    co, dim = fx["corpora"][corpus], fx["dim"]
    C = fx["cent_int"].shape[0]
    S = exact_scores(fx, corpus)
    cmax = float(np.abs(fx["cent"].astype(np.float64)).max())
    hnmax = float(0.5 * (fx["cent"].astype(np.float64) ** 2).sum(axis=1).max())
    counts = {}
    for t in range(S.shape[0]):
        l1 = np.abs(co["x_int"][t]).sum() * 2.0 ** co["x_unit"][t]
        s = S[t]
        m = s.max()
        mem = co["members"][t][co["members"][t] >= 0] if co["n_group"][t] <= MAXG else np.arange(C)
        inside = np.zeros(C, bool)
        inside[mem] = True
        if fx["form"] == "l2":            # members: within one grid step of the maximum (an exact tie is always a candidate)
            W, ref, step = window_bound("l2", dim, l1, cmax, hnmax=hnmax), m, 2.0 ** (2 * int(fx["cent_unit"][0]) - 1)
        else:
            ref = float(HALF_INF) if m >= HALF_INF else (-np.inf if m <= -HALF_INF else m)
            W = window_bound("compress", dim, l1, cmax, m_abs=abs(m))
            step = (32.0 if abs(ref) >= 65504 else float(np.spacing(np.float16(abs(ref))))) if np.isfinite(ref) else 0.0
        assert inside.sum() == co["n_group"][t], (fx["name"], corpus, t)
        assert np.all(s[inside] >= ref - step), (fx["name"], corpus, t, co["kind"][t], "a member outside one fp16 step")
        assert np.all(s[~inside] < ref - 4 * W), (fx["name"], corpus, t, co["kind"][t], "a centroid inside the gap")
        assert corpus == "rows" or (co["n_group"][t] <= 8) == (corpus == "le8")
        counts[str(co["kind"][t])] = counts.get(str(co["kind"][t]), 0) + 1
    return counts


def exact_codes(fx, corpus):
    """the expected codes / labels from the exact scores: first maximal h16(score) (compress), first maximal score (L2)"""
    S = exact_scores(fx, corpus)
    if fx["form"] == "l2":
        return np.argmax(S, axis=1).astype(np.int64)
    with np.errstate(over="ignore"):
        return np.argmax(S.astype(np.float16), axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# family O
O_AMP_LO, O_AMP_HI, O_AMP_GAP = 0.04, 0.125, 0.03
O_CHUNK, O_MAX_CHAINS = 50_000, 6_000_000      # draws per round (two chains each), the budget
O_TRIPLES, O_C, O_T = 48, 272, 150


def _o_draw(rng, dim, n):
    bits = np.arange(0x2000, 0x3000, dtype=np.uint16).view(np.float16)
    grid = bits[(bits >= np.float16(O_AMP_LO)) & (bits <= np.float16(O_AMP_HI))]
    a, b = grid[rng.integers(0, grid.size, n)], grid[rng.integers(0, grid.size, n)]
    ok = np.abs(a.astype(np.float64) - b.astype(np.float64)) >= O_AMP_GAP
    a, b = a[ok], b[ok]
    n = a.size
    sg = rng.choice([-1.0, 1.0], (n, dim)).astype(np.float16)
    x = (np.where(rng.random((n, dim)) < 0.5, a[:, None], b[:, None]) * sg).astype(np.float16)
    c = (np.where(rng.random((n, dim)) < 0.5, a[:, None], b[:, None]) * sg).astype(np.float16)      # every product positive
    # the twin: c's entries shuffled inside every class of positions where x holds the same value
    cls = x.view(np.uint16).astype(np.float64)
    src = np.argsort(cls + rng.random((n, dim)) * 0.5, axis=1, kind="stable")
    dst = np.argsort(cls, axis=1, kind="stable")
    c2 = np.empty_like(c)
    np.put_along_axis(c2, dst, np.take_along_axis(c, src, axis=1), axis=1)
    return x, c, c2


def search_o(rng, dim, l2):
    """-> (triples [(x, winner, loser)], chains evaluated, triples found).  Compress: the fp16 roundings of the two chains differ;
    L2: fl32(chain - hn) differs (the exact values are equal in both forms: the same products, the same squares)."""
    found, chains, n_found = [], 0, 0
    while chains < O_MAX_CHAINS and len(found) < O_TRIPLES:
        x, c, c2 = _o_draw(rng, dim, O_CHUNK)
        s1, s2 = M.chain32(c, x), M.chain32(c2, x)
        chains += 2 * x.shape[0]
        if l2:
            s1, s2 = s1 - model_hn(c), s2 - model_hn(c2)
            hit = s1 != s2
        else:
            hit = M.h_bits(s1) != M.h_bits(s2)
        n_found += int(hit.sum())
        for j in np.nonzero(hit)[0][:O_TRIPLES - len(found)]:
            found.append((x[j], c[j], c2[j]) if s1[j] > s2[j] else (x[j], c2[j], c[j]))
    return found, chains, n_found


def family_o_part(rng, dim, l2):
    found, chains, n_found = search_o(rng, dim, l2)
    x0, _, _ = _o_draw(rng, dim, 4 * O_C)
    cent = x0[:O_C].copy()                                   # fillers: sign patterns of their own, cross scores near zero
    slots = rng.permutation(O_C)[:2 * len(found)].reshape(-1, 2)
    slots.sort(axis=1)
    win = np.zeros(len(found), np.int64)
    for i, (x, w, l) in enumerate(found):
        lo, hi = slots[i]
        win[i] = hi if i % 2 == 0 else lo                    # the chain's winner at the higher index in half of the triples
        cent[win[i]], cent[lo + hi - win[i]] = w, l
    order = np.concatenate([rng.permutation(len(found)) for _ in range(O_T // max(len(found), 1) + 1)])[:O_T] if found else np.zeros(0, np.int64)
    tok = np.stack([found[i][0] for i in order]) if found else np.zeros((0, dim), np.float16)
    return dict(cent=cent, tok=tok, winner=win[order], pair=slots[order], search=np.array([chains, n_found, len(found)], np.int64))


def family_o(dim):
    rng = np.random.default_rng(20261400 + dim)
    out = {}
    for form, l2 in (("c", False), ("l2", True)):
        for k, v in family_o_part(rng, dim, l2).items():
            out[f"{form}_{k}"] = v
    return out


def check_o(arr, dim):
    """the triples keep their property under the chain, every other centroid lies below the gap -> (compress triples, L2 triples)"""
    for form in ("c", "l2"):
        cent, tok, win, pair = (arr[f"{form}_{k}"] for k in ("cent", "tok", "winner", "pair"))
        if tok.shape[0] == 0:
            continue
        lose = pair.sum(axis=1) - win
        r = np.arange(tok.shape[0])
        s = chain_scores(tok, cent)
        l1 = np.abs(tok.astype(np.float64)).sum(axis=1)
        cmax = float(np.abs(cent.astype(np.float64)).max())
        ex = tok.astype(np.float64) @ cent.astype(np.float64).T
        if form == "l2":
            hn = model_hn(cent)
            hnx = 0.5 * (cent.astype(np.float64) ** 2).sum(axis=1)
            s, ex = s - hn[None, :], ex - hnx[None, :]
            assert np.all(s[r, win] > s[r, lose]), "an L2 twin lost its fp32 difference"
            W = window_bound("l2", dim, l1, cmax, hnmax=float(hnx.max()))
        else:
            assert np.all(M.h_bits(s[r, win]).view(np.float16) > M.h_bits(s[r, lose]).view(np.float16)), "a twin lost its fp16 difference"
            W = window_bound("compress", dim, l1, cmax, m_abs=np.abs(ex[r, win]))
        assert np.array_equal(M.exact_dot_int(cent[win], tok), M.exact_dot_int(cent[lose], tok)), "twins with different exact sums"
        rest = ex.copy()
        rest[r, win] = rest[r, lose] = -np.inf
        assert np.all(rest.max(axis=1) < ex[r, win] - 4 * W), "a third centroid inside the gap"
        if form == "l2":     # fp_kmeans is handed the table's rows as data rows: each nearest to itself, everything else below the gap
            c64 = cent.astype(np.float64)
            rows = c64 @ c64.T - hnx[None, :]
            own = np.diag(rows).copy()
            np.fill_diagonal(rows, -np.inf)
            Wr = window_bound("l2", dim, np.abs(c64).sum(axis=1), cmax, hnmax=float(hnx.max()))
            assert np.all(rows.max(axis=1) < own - 4 * Wr), "a table row with a second candidate"
    return int(np.unique(arr["c_winner"]).size), int(np.unique(arr["l2_winner"]).size)


# ------------------------------------------------------------------------------------------------------------------------------
def main():
    check = "--check" in sys.argv
    for name, dims, fam in (("G", G_DIMS + G_EXTRA_DIMS, family_g), ("GL", GL_DIMS, family_gl), ("X", X_DIMS, family_x)):
        for dim in dims:
            fx = fam(dim)
            print(f"{name} dim {dim}:", {co: check_groups(fx, co) for co in fx["corpora"]})
    import time
    for dim in O_DIMS:
        t0 = time.time()
        arr = family_o(dim)
        print(f"O dim {dim}: {time.time() - t0:.0f} s")
        n_c, n_l2 = check_o(arr, dim)
        print(f"O dim {dim}: compress {arr['c_search'].tolist()} (chains, found, kept), L2 {arr['l2_search'].tolist()}; distinct winners {n_c} / {n_l2}")
        path = os.path.join(HERE, f"o_d{dim}.npz")
        if check:
            tmp = io.BytesIO()
            write_npz(tmp, arr)
            with open(path, "rb") as f:
                assert f.read() == tmp.getvalue(), f"o_d{dim}.npz differs from what the generator writes"
        else:
            write_npz(path, arr)
        print(f"o_d{dim}", "ok" if check else "written")


if __name__ == "__main__":
    main()
