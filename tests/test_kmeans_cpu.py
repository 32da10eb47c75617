"""CPU tests (no GPU) of the native k-means trainer's surface and of the numpy model the GPU tests compare it with
(tests/kmeans_model.py): fp_kmeans is declared, exported and bound; it has no CPU path; the model's int64 fixed-point sums are the
exact sums; the refusal bound is the header's."""
import ctypes
import os
import re

import numpy as np
import pytest

import kmeans_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fastplaid.h")).read()


def test_fp_kmeans_is_declared_exported_and_bound():
    from fast_plaid_amd import _native, kmeans
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+fp_kmeans\s*\(([^)]*)\)", code)
    assert m, "fp_kmeans is not declared in include/fastplaid.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("int ") and "uint64_t" in args[7], args
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "fp_kmeans")
    res, argtypes = _native.SYMBOLS["fp_kmeans"]
    assert res is ctypes.c_int and len(argtypes) == 10 and argtypes[7] is ctypes.c_uint64
    assert callable(kmeans.lloyd_device)
    assert not re.search(r"k-means[^.]*stay on the host", re.sub(r"\s*\n \*\s*", " ", _header()))


def test_fp_kmeans_has_no_cpu_path():
    """without a device the trainer fails with an error; it does not fall back to the host loop"""
    from fast_plaid_amd import _native, kmeans
    if _native.lib().fp_device_count() > 0:
        pytest.skip("a GPU is visible")
    rng = np.random.default_rng(0)
    data = rng.standard_normal((64, 16)).astype(np.float16)
    with pytest.raises(ValueError, match="no HIP device"):
        kmeans.lloyd_device(data, 4, 2, np.random.default_rng(1), seed=3)
    with pytest.raises(ValueError, match="no HIP device"):
        kmeans.compute_kmeans([data[:30], data[30:]], 16, kmeans_niters=1, native=True)


def test_model_sums_are_exact():
    """every finite fp16 value is an integer multiple of 2^-24, so the int64 sums equal Python's big-integer sums of the values as
    fractions -- in any order -- on unit-scale data, on values up to 300 and on subnormals"""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    parts = [rng.standard_normal(400), rng.uniform(-300, 300, 400), rng.uniform(-6e-5, 6e-5, 300),
             np.array([65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 0.0, -0.0, 300.0, 2.0 ** -14])]
    x = np.concatenate(parts).astype(np.float16).reshape(-1, 4)
    sub = np.abs(x.astype(np.float32))
    assert ((sub > 0) & (sub < 2.0 ** -14)).sum() > 50 and sub.max() == 65504.0      # subnormals and the largest value are in
    fx = M.fixed(x)
    for v, f in zip(x.ravel().tolist(), fx.ravel().tolist()):
        assert Fraction(v) * 2 ** 24 == f                                            # the conversion is exact, value by value
    labels = rng.integers(0, 5, x.shape[0])
    S, cnt = M.sums(x, labels, 5)
    perm = rng.permutation(x.shape[0])
    S2, cnt2 = M.sums(x[perm], labels[perm], 5)
    assert np.array_equal(S, S2) and np.array_equal(cnt, cnt2)                        # order-free
    for c in range(5):
        rows = x[labels == c]
        assert cnt[c] == rows.shape[0]
        for d in range(4):
            big = sum((Fraction(v) for v in rows[:, d].tolist()), Fraction(0)) * 2 ** 24
            assert big.denominator == 1 and int(big) == int(S[c, d]), (c, d)


def test_refusal_bound_is_the_headers():
    """the header promises a refusal at n * max|x| * 2^24 >= 2^62; below it no int64 sum can overflow"""
    assert "n * max|x| * 2^24 >= 2^62" in re.sub(r"\s*\n \*\s*", " ", _header())
    for mx in (np.float16(1.0), np.float16(300.0), np.float16(65504.0), np.float16(2.0 ** -24), np.float16(0.5)):
        v = int(M.fixed(mx))
        edge = -(-2 ** 62 // v)                       # the smallest refused n
        assert M.refused(edge, mx) and not M.refused(edge - 1, mx)
        assert M.refused(edge, -mx)
        assert (edge - 1) * v < 2 ** 62 < 2 ** 63 - 1    # every partial sum of an accepted call fits int64 with a bit to spare
    assert not M.refused(2 ** 31, np.float16(0.0))
    assert M.refused(2 ** 23, np.float16(65504.0)) and not M.refused(2 ** 22, np.float16(65504.0)) and not M.refused(2 ** 23, np.float16(300.0))
