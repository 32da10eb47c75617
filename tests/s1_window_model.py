"""numpy restatement of the two certification windows (include/fastplaid.h, "CERTIFICATION WINDOWS"), line by line in the
device's arithmetic -- no GPU needed.  Used by tests/golden/rounding/make_rounding_fixtures.py (the search for inputs the windows
do not cover) and by tests/test_rounding_fixtures_cpu.py.

  chain32        the reference's centroid score / token score before its fp16 rounding: acc = fma(c_k, q_k, acc), k ascending, in
                 fp32 (oracle/plaid_oracle.c search_one, S1; the product of two fp16 values is exact in fp32, so the fused and
                 the unfused chain are the same numbers)
  exact_dot      the same sum without any rounding, as an integer multiple of 2^-48
  wcol           S1's absolute window term of a query row, w0 * dim_scale * cent_norm_max * |q_n|_2 as k_pack_queries computes it
                 (fp_kernels.hip) from the host's factor (fp_engine.cpp run_front, max_row_norm_f16)
  s1_flagged     s1_certify's rule (fp_kernels.hip): u = fma(|x|, kappa, w); flagged when h(x + u) and h(x - u) differ in their bits
  maxsim_flagged the MaxSim column rule (fp_maxsim.hip, k_maxsim5 / k_maxsim6 epilogue): the fp32 column maximum lies within
                 eps_rel * |q_col|_2 of an fp16 rounding boundary

The constants are the library's defaults and live HERE for the tests: S1's in fp_engine.cpp run_front (s1_w0_log2, s1_kappa_log2,
dim_scale), MaxSim's in fp_maxsim.hip (eps_env, the same dim scale).  A change of a default there is a change here."""
import numpy as np

S1_W0_LOG2 = -21.5       # fp_engine.cpp: fp_test_opt("s1_w0_log2", -21.5)
S1_KAPPA_LOG2 = float(np.log2(72.0) - 24.0)   # fp_engine.cpp: fp_test_opt("s1_kappa_log2", log2(72) - 24); kappa = (D / 2 + D / 16) 2^-24 at D = 128:
#   the reference's chain rounds D - 1 partial sums, each by at most half an ulp <= 2^-24 |partial sum|; products of one sign and of
#   comparable size make the partial sums grow linearly to |x|, their sum is ~|x| D / 2; the MFMA's D / 16 accumulator roundings
#   and its undocumented rounding inside a block get |x| D / 16.  (Until the constructed fixtures of tests/golden/rounding: 2^-20,
#   an empirical margin.)
MAXSIM_EPS_LOG2 = -19.0  # fp_maxsim.hip: eps_env = 2^-19


def dim_scale(dim):
    """both windows were measured at dim 128 and grow with the number of terms above it"""
    return np.float32(dim / 128.0) if dim > 128 else np.float32(1.0)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def h_bits(x):
    """fp16 bits of the round-to-nearest-even conversion of fp32 values"""
    return f32(x).astype(np.float16).view(np.uint16)


def chain32(c, q):
    """[n] fp32: ascending chain over the last axis of two [n, D] (or broadcastable) fp16 arrays"""
    c, q = np.broadcast_arrays(np.asarray(c, np.float16), np.asarray(q, np.float16))
    acc = np.zeros(c.shape[:-1], np.float32)
    for k in range(c.shape[-1]):
        acc = (acc + c[..., k].astype(np.float32) * q[..., k].astype(np.float32)).astype(np.float32)   # product exact, one rounding
    return acc


def _int24(a):
    """fp16 values as integers in units of 2^-24 (exact for every finite fp16 value; entries up to 4 so that products of two and
    sums of 256 of them stay inside int64)"""
    a = np.asarray(a, np.float16).astype(np.float64)
    assert np.all(np.abs(a) <= 4.0), "exact_dot: entries beyond 4 are outside the range this helper was written for"
    i = a * 2.0 ** 24
    assert np.all(i == np.rint(i))
    return i.astype(np.int64)


def exact_dot_int(c, q):
    """[n] int64: sum_k c_k q_k in units of 2^-48, no rounding anywhere"""
    c, q = np.broadcast_arrays(_int24(c), _int24(q))
    assert c.shape[-1] <= 256
    return (c * q).sum(axis=-1, dtype=np.int64)


def fl32_of_int(i, log2_unit=-48):
    """fp32 rounding (nearest even) of i * 2^log2_unit.  The conversion goes through a sum of two doubles that is exact, so the
    only rounding is the final one to fp32."""
    i = np.asarray(i, np.int64)
    hi = (i >> 20 << 20)
    lo = i - hi                                # |lo| < 2^20, hi a multiple of 2^20 of at most 43 significant bits: both exact
    d = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.all(np.abs(i) < (1 << 52)), "fl32_of_int: beyond the exact range of a double"
    return (d * 2.0 ** log2_unit).astype(np.float32)


def shift_ulps(x, n):
    """x moved by n fp32 steps (n of either sign), away from or towards zero as the sign says"""
    x = f32(x).copy()
    for _ in range(abs(int(n))):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


def row_norm32(q):
    """|q_n|_2 as k_pack_queries / the MaxSim prologue compute it: ss = fma(x, x, ss) ascending in fp32, then sqrtf"""
    q = np.asarray(q, np.float16)
    ss = np.zeros(q.shape[:-1], np.float32)
    for k in range(q.shape[-1]):
        x = q[..., k].astype(np.float64)
        ss = (ss.astype(np.float64) + x * x).astype(np.float32)   # x*x and the sum are exact in double: one rounding, as the fma
    return np.sqrt(ss, dtype=np.float32)


def cent_norm_max(centroids):
    """max_row_norm_f16: the largest centroid norm, at least 1, from double sums"""
    c = np.asarray(centroids, np.float16).astype(np.float64)
    return np.float32(max(1.0, float(np.sqrt((c * c).sum(axis=1)).max())))


def wcol(q, cnm, dim, w0_log2=S1_W0_LOG2):
    w0 = np.float32(np.exp2(np.float32(w0_log2)))
    host = np.float32(np.float32(w0 * dim_scale(dim)) * np.float32(cnm))   # s1x_w0 * dim_scale * cent_norm_max, left to right in fp32
    return (host * row_norm32(q)).astype(np.float32)


def s1_kappa(dim, kappa_log2=S1_KAPPA_LOG2):
    return np.float32(np.float32(np.exp2(np.float32(kappa_log2))) * dim_scale(dim))


def s1_u(x, w, kappa):
    """the window's half-width: one fma in the kernel"""
    return (np.abs(f32(x)).astype(np.float64) * np.float64(kappa) + f32(w).astype(np.float64)).astype(np.float32)


def s1_flagged(x, w, kappa):
    x = f32(x)
    u = s1_u(x, w, kappa)
    return h_bits(x + u) != h_bits(x - u)


def maxsim_eps(q, dim, eps_log2=MAXSIM_EPS_LOG2):
    return (np.float32(np.float32(2.0 ** eps_log2) * dim_scale(dim)) * row_norm32(q)).astype(np.float32)


def maxsim_flagged(am, eps):
    am = f32(am)
    hm = am.astype(np.float16).astype(np.float32)
    ef = (am.view(np.uint32) >> 23) & 0xFF
    ef = np.maximum(ef, 113)                                    # fp16 subnormal range: fixed spacing 2^-24
    halfulp = ((ef - 11).astype(np.uint32) << 23).view(np.float32)
    dist = (halfulp - np.abs(am - hm)).astype(np.float32)
    return ~(dist > f32(eps))


def boundary_distance(x):
    """float64 distance of x to the nearest fp16 rounding boundary (the midpoint of two neighbouring fp16 values), for |x| below
    the fp16 maximum -- the search's coarse filter; the properties themselves are checked with s1_flagged / maxsim_flagged"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    ulp = 2.0 ** (e - 10)
    r = x / ulp - np.floor(x / ulp)
    d_in = np.abs(r - 0.5) * ulp
    # (the boundaries inside x's binade, 2^e + (i + 1/2) ulp, are covered by r; the one below the binade's first value lies a
    # quarter of this binade's step under 2^e, because the binade below has half the step)
    d_lo = np.where(e > -14, x - (2.0 ** e - ulp / 4), np.inf)
    return np.minimum(d_in, d_lo)
