"""fp_residual_stats (k_residual_tile, k_hist16) against a plain numpy restatement, bit for bit; its refusals that need the device;
train_codec(native=True) and create_index(native_codec=True) against the host path."""
import filecmp
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data(dim, n, C):
    """unit-norm fp16 centroids and tokens (centroid + noise).  The centroids' last dim is +0.0.  With n >= 4: tokens 0 and 3 equal
    a centroid (zero residuals), token 1 has -0.0 in the last dim (residual -0.0), token 2 is centroid 0 with dim 1 one fp16 step
    above a value near 0.01 (a subnormal residual, 2^-17)."""
    rng = np.random.default_rng(1000 * dim + C)
    cent = rng.standard_normal((C, dim)).astype(np.float32)
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
    cent[:, dim - 1] = 0.0
    cent[0, 1] = 0.01
    x = cent[rng.integers(0, C, n)].astype(np.float32) + 0.3 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    if n >= 4:
        x[0], x[3], x[2] = cent[1], cent[0], cent[0]
        x[1, dim - 1] = -0.0
        x[2, 1] = np.nextafter(cent[0, 1], np.float16(1))
    return cent, x


# one token; a tile and one; a short tile and slice; a 16-byte unit past a slice; scalar loads and a masked unit; the MFMA narrowing;
# 16 slices; two chunks
@pytest.mark.parametrize("dim,n,C", [(8, 1, 4), (8, 65, 4), (64, 63, 16), (72, 64, 16), (100, 65, 16), (128, 200, 300), (1024, 65, 256),
                                     (8, 2**20 + 65, 4)])
def test_residual_stats_bit_for_bit(dim, n, C):
    from fast_plaid_amd import create
    cent, x = data(dim, n, C)
    got = create.residual_stats(cent, x, "cuda:0")
    codes, _ = create.compress(cent, np.zeros(3, np.float16), x, 2, "cuda:0")
    assert np.array_equal(got["codes"], codes)
    r = x - cent[codes]   # fp16 - fp16: one fp32 subtraction rounded once
    assert r.dtype == np.float16
    if n >= 4:
        assert np.signbit(r[1, dim - 1]) and r[1, dim - 1] == 0 and r[2, 1] == np.float16(2.0 ** -17) and not r[0].any()
    assert np.array_equal(got["hist"], np.bincount(r.view(np.uint16).ravel(), minlength=65536))
    assert np.array_equal(got["abs_sum"], (np.abs(r).astype(np.float64) * 2.0 ** 24).astype(np.int64).sum(axis=0))
    r32, acc = r.astype(np.float32), np.zeros(n, np.float32)
    for d in range(dim):
        acc = acc + r32[:, d] * r32[:, d]
    assert np.array_equal(got["norms"].view(np.uint32), np.sqrt(acc).view(np.uint32))


@pytest.mark.parametrize("x0,c0,message", [(60000.0, -60000.0, "fp_residual_stats: a residual overflows fp16"),
                                           (np.inf, 1.0, "fp_residual_stats: the embeddings hold a value that is not finite")])
def test_refusals_on_the_device(x0, c0, message):
    from fast_plaid_amd import _native
    cent, x = np.full((1, 8), 1.0, np.float16), np.full((5, 8), 1.0, np.float16)
    cent[0, 3], x[4, 3] = c0, x0
    hist, abs_sum = np.zeros(65536, np.int64), np.zeros(8, np.int64)
    rc = _native.lib().fp_residual_stats(0, cent.ctypes.data, 1, 8, x.ctypes.data, 5, None, hist.ctypes.data, abs_sum.ctypes.data, None)
    assert rc == -1 and _native.last_error() == message   # FP_EINVAL


@pytest.mark.parametrize("nbits", [2, 4])
def test_native_codec_against_the_host_path(nbits, tmp_path):
    from fast_plaid_amd import create
    dim = 128
    cent, x = data(dim, 3000, 300)
    cut, wts, avg, thr = create.train_codec(x, cent, nbits, "cuda:0", with_threshold=True)
    ncut, nwts, navg, nthr = create.train_codec(x, cent, nbits, "cuda:0", with_threshold=True, native=True)
    assert np.array_equal(ncut, cut) and np.array_equal(nwts, wts)
    np.testing.assert_allclose(navg, avg, rtol=2e-3)
    np.testing.assert_allclose(nthr, thr, rtol=(2 * dim + 4) * 2.0 ** -24)   # fp32 sums of dim terms >= 0, a square root, a lerp
    docs = [x[i: i + 30] for i in range(0, 3000, 30)]
    for name, native in (("host", False), ("native", True)):
        create.create_index(str(tmp_path / name), docs, cent, nbits=nbits, device="cuda:0", heldout=x, native_codec=native)
    files = sorted(f for f in os.listdir(tmp_path / "host") if f.endswith((".codes.npy", ".residuals.npy")) or f.startswith("ivf"))
    assert len(files) >= 4
    assert filecmp.cmpfiles(tmp_path / "host", tmp_path / "native", files, shallow=False) == (files, [], [])
