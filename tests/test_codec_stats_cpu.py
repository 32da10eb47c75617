"""CPU tests (no GPU) of fp_residual_stats and what sits on it: the symbol is declared, exported and bound; its argument refusals
happen before the device is touched; create._kth_from_hist reads every order statistic of an fp16 array from its histogram; the
public signatures carry native_codec keyword-only and off by default."""
import ctypes
import inspect

import numpy as np
import pytest

FP_EINVAL, FP_EUNSUPPORTED = -1, -4
DIMS = "fp_residual_stats: dim must be in [1, 256] or a multiple of 8 up to 1024"


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _stats(L, dim, T=4, hist=True):
    w = max(dim, 1)
    h = np.zeros(65536, np.int64) if hist else None
    return L.fp_residual_stats(0, _p(np.zeros((2, w), np.float16)), 2, dim, _p(np.zeros((4, w), np.float16)), T, None, _p(h),
                               _p(np.zeros(w, np.int64)), None)


def test_symbol_exported_and_bound():
    """(that the header declares it is test_host_cpu's comparison of the header with _native.SYMBOLS and the library)"""
    from fast_plaid_amd import _native
    assert "fp_residual_stats" in _native.SYMBOLS
    assert _native.lib().fp_residual_stats.argtypes == _native.SYMBOLS["fp_residual_stats"][1]


@pytest.mark.parametrize("kw,code,message", [
    (dict(dim=0), FP_EUNSUPPORTED, DIMS), (dict(dim=260), FP_EUNSUPPORTED, DIMS), (dict(dim=1032), FP_EUNSUPPORTED, DIMS),
    (dict(dim=8, hist=False), FP_EINVAL, "bad argument"), (dict(dim=8, T=-1), FP_EINVAL, "bad argument"),
], ids=["dim-0", "dim-260", "dim-1032", "null-histogram", "negative-n-tokens"])
def test_refusal_before_the_device(kw, code, message):
    from fast_plaid_amd import _native
    assert _stats(_native.lib(), **kw) == code
    assert _native.last_error() == message


def test_kth_from_hist_equals_sort():
    from fast_plaid_amd import create
    rng = np.random.default_rng(5)
    bits = np.concatenate([
        rng.integers(0, 0x7C00, 2500).astype(np.uint16) | (rng.integers(0, 2, 2500).astype(np.uint16) << 15),   # any finite value
        rng.integers(0, 0x0400, 600).astype(np.uint16) | (rng.integers(0, 2, 600).astype(np.uint16) << 15),     # subnormals and zeros
        np.repeat(np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF], np.uint16), 100),  # duplicates, both zeros, extremes
    ])
    vals = np.sort(bits.view(np.float16))
    hist = np.bincount(bits, minlength=65536).astype(np.int64)
    got = np.array([create._kth_from_hist(hist, k) for k in range(vals.shape[0])], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, vals.astype(np.float32))
    assert not np.signbit(got[vals == 0]).any()   # a zero is reported as +0.0


def test_native_codec_is_keyword_only_and_off():
    from fast_plaid_amd import create, maintain
    from fast_plaid_amd.search import FastPlaid
    for fn in (FastPlaid.create, FastPlaid.update):
        par = inspect.signature(fn).parameters["native_codec"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    for fn in (create.build_index_arrays, create.create_index, maintain.update_index):
        assert inspect.signature(fn).parameters["native_codec"].default is False
    assert inspect.signature(create.train_codec).parameters["native"].default is False
