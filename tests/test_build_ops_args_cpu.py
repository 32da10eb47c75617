"""CPU tests (no GPU) of the four stand-alone index-build operators' argument refusals (fp_compress, fp_assign_l2, fp_kmeans,
fp_centroid_outliers): every refusal that happens before the device is touched, by return code and by the exact fp_last_error()
text; the *_last_* queries answer 0 after a refused call; a refused fp_centroid_outliers leaves *out_count at 0.  The library loads
without a GPU, and no case here starts one."""
import ctypes

import numpy as np
import pytest

FP_EINVAL, FP_EHIP, FP_EUNSUPPORTED = -1, -3, -4
NO_DEVICE = "no HIP device available (this library has no CPU path)"
DIMS = "dim must be in [1, 256] or a multiple of 8 up to 1024"


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _h(*shape):
    return np.zeros(shape, np.float16)


def _compress(L, centroids, C, dim, nbits, T=4):
    cut = np.zeros(255, np.float16)
    emb, codes, res = _h(T, max(dim, 1)), np.zeros(T, np.int64), np.zeros((T, max(dim, 1)), np.uint8)
    return L.fp_compress(0, _p(centroids), C, dim, nbits, _p(cut), _p(emb), T, _p(codes), _p(res))


def _assign(L, half_sqnorm, dim, C=2, T=4):
    labels = np.zeros(T, np.int64)
    return L.fp_assign_l2(0, _p(_h(C, dim)), _p(half_sqnorm), C, dim, _p(_h(T, dim)), T, _p(labels))


def _kmeans(L, n, dim, k, niter, init_rows):
    out = np.zeros((k, max(dim, 1)), np.float32)
    return L.fp_kmeans(0, _p(_h(n, max(dim, 1))), n, dim, k, niter, _p(np.asarray(init_rows, np.int64)), 1, _p(out), None)


def _outliers(L, dim, threshold_sq, out_count, C=2, T=4):
    rows = np.zeros(T, np.int64)
    return L.fp_centroid_outliers(0, _p(_h(C, dim)), C, dim, _p(_h(T, dim)), T, threshold_sq, _p(rows), _p(out_count), None, None)


def _new_count():
    return np.full(1, 7, np.int64)


# (id, call, return code, fp_last_error()); every expectation is read off the operators' validation code
CASES = [
    ("compress-null-centroids", lambda L: _compress(L, None, 2, 8, 4), FP_EINVAL, "bad argument"),
    ("compress-nbits-3", lambda L: _compress(L, _h(2, 8), 2, 8, 3), FP_EINVAL, "nbits must divide 8 (1, 2, 4 or 8)"),
    ("compress-dim-257", lambda L: _compress(L, _h(2, 257), 2, 257, 8), FP_EUNSUPPORTED,
     "fp_compress: " + DIMS + ", with dim * nbits a multiple of 8"),
    ("compress-dim-1032", lambda L: _compress(L, _h(2, 1032), 2, 1032, 4), FP_EUNSUPPORTED,
     "fp_compress: " + DIMS + ", with dim * nbits a multiple of 8"),
    ("compress-dim-3-nbits-2", lambda L: _compress(L, _h(2, 3), 2, 3, 2), FP_EUNSUPPORTED,
     "fp_compress: " + DIMS + ", with dim * nbits a multiple of 8"),
    ("compress-too-many-centroids", lambda L: _compress(L, _h(1), 2**31 - 1, 8, 4), FP_EUNSUPPORTED, "too many centroids"),
    ("assign-null-half-sqnorm", lambda L: _assign(L, None, 8), FP_EINVAL, "bad argument"),
    ("assign-dim-260", lambda L: _assign(L, np.zeros(2, np.float32), 260), FP_EUNSUPPORTED, "fp_assign_l2: " + DIMS),
    ("kmeans-niter-negative", lambda L: _kmeans(L, 8, 8, 2, -1, [0, 1]), FP_EINVAL, "bad argument"),
    ("kmeans-fewer-points-than-centroids", lambda L: _kmeans(L, 3, 8, 4, 2, [0, 1, 2, 0]), FP_EINVAL,
     "fp_kmeans: fewer training points (3) than centroids (4)"),
    ("kmeans-init-row-outside", lambda L: _kmeans(L, 8, 8, 3, 2, [0, 8, 1]), FP_EINVAL, "fp_kmeans: init_rows[1] outside [0, n)"),
    ("kmeans-dim-0", lambda L: _kmeans(L, 8, 0, 2, 2, [0, 1]), FP_EUNSUPPORTED, "fp_kmeans: " + DIMS),
    ("outliers-null-out-count", lambda L: _outliers(L, 8, 1.0, None), FP_EINVAL, "bad argument"),
    ("outliers-threshold-nan", lambda L: _outliers(L, 8, float("nan"), _new_count()), FP_EINVAL,
     "fp_centroid_outliers: threshold_sq must be a number >= 0"),
    ("outliers-threshold-negative", lambda L: _outliers(L, 8, -0.5, _new_count()), FP_EINVAL,
     "fp_centroid_outliers: threshold_sq must be a number >= 0"),
    ("outliers-dim-258", lambda L: _outliers(L, 258, 1.0, _new_count()), FP_EUNSUPPORTED, "fp_centroid_outliers: " + DIMS),
]


def _last_flags(L):
    cp, km, co = np.zeros(7, np.int64), np.zeros(7, np.float32), np.zeros(7, np.int64)
    return (L.fp_compress_last_counts(_p(cp), 7), L.fp_kmeans_last_timings(_p(km), 7), L.fp_centroid_outliers_last_counts(_p(co), 7))


@pytest.fixture(scope="module")
def L():
    """the library, with one refused call of each operator that keeps figures behind it: whatever an earlier test of this process
    left in the thread's *_last_* figures is gone (fp_assign_l2 keeps none and resets none)"""
    from fast_plaid_amd import _native
    lib = _native.lib()
    assert _compress(lib, None, 2, 8, 4) == FP_EINVAL
    assert _kmeans(lib, 8, 8, 2, -1, [0, 1]) == FP_EINVAL
    assert _outliers(lib, 8, -1.0, _new_count()) == FP_EINVAL
    return lib


@pytest.mark.parametrize("call,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal_before_the_device(L, call, code, message):
    from fast_plaid_amd import _native
    assert call(L) == code
    assert _native.last_error() == message
    assert _last_flags(L) == (0, 0, 0)


@pytest.mark.parametrize("dim,threshold_sq", [(8, float("nan")), (8, -0.5), (258, 1.0)], ids=["nan", "negative", "dim-258"])
def test_refused_outliers_call_zeroes_out_count(L, dim, threshold_sq):
    count = _new_count()
    assert _outliers(L, dim, threshold_sq, count) < 0
    assert count[0] == 0


def test_valid_calls_without_a_device_fail_with_the_no_device_message(L):
    """only where no device is visible: an otherwise valid call of each operator stops at the device count"""
    from fast_plaid_amd import _native
    if L.fp_device_count() == 0:
        count = _new_count()
        for call in (lambda: _compress(L, _h(2, 8), 2, 8, 4), lambda: _assign(L, np.zeros(2, np.float32), 8),
                     lambda: _kmeans(L, 8, 8, 2, 2, [0, 1]), lambda: _outliers(L, 8, 1.0, count)):
            assert call() == FP_EHIP
            assert _native.last_error() == NO_DEVICE
            assert _last_flags(L) == (0, 0, 0)
        assert count[0] == 0
