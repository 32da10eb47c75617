"""fp_centroid_outliers at the dims above 256 an index accepts, against its numpy restatement (tests/update_policy_model.py): rows,
squared distances (as uint32 words) and nearest centroids equal bit for bit, with the chains through LDS (k_out_prepare_sl,
k_outlier_dist_sl) and, under FP_TEST=out_staged=0, with one thread per row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import outliers_worker as W
import update_policy_model as M
from fptest_env import with_test_opts

pytestmark = pytest.mark.gpu

SHAPES = {264: (300, 1000),   # (C, T): the narrowing, a ragged last tile, a short last slice (8 of 64 dims)
          520: (20, 515),     # the all-chain assignment; two tiles plus three tokens
          1024: (256, 700)}   # all eight K-slices


@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_bit_identical_to_the_model(dim, staged):
    if not staged:   # the switch is read inside the library: the staged case of this dim again, in a process of its own
        p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", f"{__file__}::test_bit_identical_to_the_model[{dim}-1]"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=with_test_opts(dict(os.environ), out_staged=0))
        assert p.returncode == 0 and "1 passed" in p.stdout, p.stdout[-4000:]
        return
    from fast_plaid_amd import _native
    C, T = SHAPES[dim]
    rng = np.random.default_rng(8000 + dim)
    cent = rng.standard_normal((C, dim), dtype=np.float32)
    cent = np.ascontiguousarray((cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16))
    noise = rng.standard_normal((T, dim), dtype=np.float32)
    noise *= rng.uniform(0.05, 0.9, (T, 1)).astype(np.float32) / np.linalg.norm(noise, axis=1, keepdims=True)
    x = np.ascontiguousarray((cent[rng.integers(0, C, T)].astype(np.float32) + noise).astype(np.float16))
    same = rng.random(T) < 0.1
    x[same] = cent[rng.integers(0, C, int(same.sum()))]          # bit-for-bit copies of a centroid
    sq, near, _ = M.distances(cent, x)
    row = int(np.argsort(sq, kind="stable")[T // 2])
    thr = sq[row]                                                # an exact tie in the strict compare, about half the rows above it
    want_rows = np.flatnonzero(sq > thr).astype(np.int64)
    assert row not in want_rows and 0.3 * T <= want_rows.shape[0] <= 0.7 * T and (sq[same] <= 1e-3).all() and same.sum() >= 20
    assert all(((want_rows >= t0) & (want_rows < t0 + 256)).any() for t0 in range(0, T, 256))   # every tile flags some
    rc, rows, sqdist, nearest = W.call(cent, x, thr)
    assert rc == 0, (dim, _native.last_error())
    assert np.array_equal(nearest, near) and np.array_equal(sqdist.view(np.uint32), sq.view(np.uint32))
    assert rows.dtype == np.int64 and np.array_equal(rows, want_rows)
    c = W.last_counts()    # the labels came from the K-sliced narrowing itself: no chunk was redone by the all-chain kernel
    assert (c["chunks"], c["narrowed_chunks"], c["fallback_chunks"]) == (1, 1 if C >= 256 else 0, 0), c
