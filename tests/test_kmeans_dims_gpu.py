"""fp_kmeans at the dims above 256 an index accepts (multiples of 8 up to 1024), against its numpy restatement
(tests/kmeans_model.py): centroids equal as uint32 words and counts equal after 0, 1 and 3 iterations (k_km_sum_units, a finalise row
of up to 1024 floats, the K-sliced L2 assignment over several K-slices); then create, search and the outlier operator at dim 320."""
import numpy as np
import pytest

import kmeans_model as M
import kmeans_worker as W
import update_policy_model as U

pytestmark = pytest.mark.gpu

NITERS = (0, 1, 3)
SHAPES = {264: (1500, 300, 1.0),     # (n, k, scale).  33 units: half a stride; three K-slices in the narrowing, ragged tiles on both axes
          520: (700, 16, 1.0),       # 65 units: one live lane in the second stride; k < 256 takes the all-chain assignment
          768: (1100, 256, 300.0),   # large fixed-point terms
          1024: (1300, 257, 1.0)}    # all 128 units, eight K-slices


def _case(dim):
    """-> (data, k, init_rows, seed, model run): two heavy blobs with ONE initial centroid each (lists shared by several
    waves), k - 3 blobs of a few points with one each (many cluster changes in a slice), init_rows[1] == init_rows[0] (an empty twin)"""
    n, k, scale = SHAPES[dim]
    rng = np.random.default_rng(7000 + dim)
    ntiny = k - 3
    tiny = max(2, min(6, (n // 3) // ntiny))
    nbig = n - ntiny * tiny
    blob = np.concatenate([np.zeros(nbig - nbig // 3, np.int64), np.ones(nbig // 3, np.int64), 2 + np.repeat(np.arange(ntiny), tiny)])
    centers = rng.standard_normal((2 + ntiny, dim), dtype=np.float32) / np.float32(np.sqrt(dim))
    data = ((centers[blob] + np.float32(0.1 / np.sqrt(dim)) * rng.standard_normal((n, dim), dtype=np.float32)) * np.float32(scale))
    order = rng.permutation(n)
    data, blob = np.ascontiguousarray(data[order].astype(np.float16)), blob[order]
    first = np.array([np.flatnonzero(blob == b)[0] for b in range(2 + ntiny)], np.int64)   # one row of every blob
    init = np.concatenate([first[:1], first[:1], first[1:]])
    return data, k, init, 99 + dim, M.run(data, k, max(NITERS), init, 99 + dim)


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_bit_identical_to_the_model(dim):
    from fast_plaid_amd import _native, kmeans
    data, k, init, seed, ref = _case(dim)
    cnt = ref["counts"][1]    # not vacuous, on the model alone: a list of over two slices, a run of very short lists, a reseeded twin
    small = (cnt > 0) & (cnt < 8)
    assert cnt.max() > 256 and (small[:-3] & small[1:-2] & small[2:-1] & small[3:]).any(), (dim, cnt.max())
    assert ref["reseeds"][0] >= 1 and cnt[0] > 0 and cnt[1] == 0, (dim, ref["reseeds"])
    assert SHAPES[dim][2] == 1 or np.abs(data.astype(np.float32)).max() > 30
    for it in NITERS:
        rc, cent, counts = W.call(data, k, it, init, seed)
        assert rc == 0, (dim, it, _native.last_error())
        assert np.array_equal(counts, ref["counts"][it]), (dim, it)
        assert np.array_equal(cent.view(np.uint32), ref["cent32"][it].view(np.uint32)), (dim, it)
    # the last call's labels came from the K-sliced narrowing itself (the repeated init row: two tied candidates, ASSIGN_CAP is 8)
    t = kmeans.last_device_timings()
    assert (t["narrowed_chunks"], t["fallback_chunks"]) == ((max(NITERS), 0) if k >= 256 else (0, 0)), t


def test_create_search_and_outliers_at_dim_320(tmp_path):
    """the directory's centroids are compute_kmeans(native=True)'s, two documents' own tokens find them, the outlier rows are the model's"""
    from fast_plaid_amd import kmeans, maintain, search
    from fast_plaid_amd.search import index_io
    dim, rng = 320, np.random.default_rng(320)
    base = rng.standard_normal((40, dim), dtype=np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)

    def rows(n):
        d = base[rng.integers(0, 40, n)] + 0.2 * rng.standard_normal((n, dim), dtype=np.float32) / np.sqrt(dim)
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float16)

    docs = [rows(int(rng.integers(5, 25))) for _ in range(150)]
    q = np.stack([np.pad(docs[i][:12], ((0, 12 - min(12, docs[i].shape[0])), (0, 0))) for i in (3, 77)])
    path = str(tmp_path / "native320")
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.create(docs, kmeans_niters=4, nbits=4, seed=1, use_triton_kmeans=True)
        out = fpi.search(q, top_k=3, show_progress=False)
        assert [row[0][0] for row in out] == [3, 77]
    cent = np.ascontiguousarray(np.asarray(index_io.load_index_arrays(path)["centroids"]))
    want = kmeans.compute_kmeans(docs, dim, kmeans_niters=4, seed=1, native=True)
    assert want.dtype == np.float16 and want.shape[1] == dim and np.array_equal(cent.view(np.uint16), want.view(np.uint16))
    fresh = np.concatenate([rows(250), (rows(50).astype(np.float32) * -1).astype(np.float16)])   # a sixth of them far from every centroid
    got_rows, sqdist, nearest = maintain.centroid_outliers(cent, fresh, 0.5)
    want_rows, want_sq, want_near = U.outliers(cent, fresh, U.threshold_sq(0.5))
    assert 0 < want_rows.shape[0] < fresh.shape[0] and np.array_equal(got_rows, want_rows) and np.array_equal(nearest, want_near)
    assert np.array_equal(sqdist.view(np.uint32), want_sq.view(np.uint32))
