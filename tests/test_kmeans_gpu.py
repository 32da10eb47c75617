"""fp_kmeans, the device-resident k-means trainer, against its numpy restatement (tests/kmeans_model.py): centroids and cluster
sizes equal bit for bit after 0, 1 and 4 iterations on every path -- the MFMA narrowing with ragged tiles, the exact kernel,
exact ties and empty clusters, an overflowing candidate list, a chunk boundary, unnormalised data -- then the error codes,
determinism, blob recovery and FastPlaid.create(use_triton_kmeans=True) end to end.  Inputs: tests/kmeans_worker.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_model as M
import kmeans_worker as W
from fptest_env import with_test_opts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL = {}


def _model(name):
    """the model's run of a case over max(NITERS) iterations: computed once, shared by the tests, never modified"""
    if name not in _MODEL:
        data, k, init, seed = W.case(name)
        _MODEL[name] = M.run(data, k, max(W.NITERS), init, seed)
    return _MODEL[name]


def _same(name, it, cent, counts):
    ref = _model(name)
    want_c, want_n = ref["cent32"][it], ref["counts"][it]
    print(f"{name} niter={it}: centroid words that differ {int((cent.view(np.uint32) != want_c.view(np.uint32)).sum())} of {cent.size}, "
          f"counts that differ {int((counts != want_n).sum())}, reseeds in the model {ref['reseeds'][:it]}")
    assert np.array_equal(counts, want_n), (name, it)
    assert np.array_equal(cent.view(np.uint32), want_c.view(np.uint32)), (name, it)


def _parity_inputs():
    """the blobs and the 150-document corpus of test_hip_parity.test_kmeans_assignment_and_create_without_centroids: its generator's
    draws replayed in its order -> (centers f32 [8, 64], pts f16 [4000, 64], docs)"""
    rng = np.random.default_rng(11)
    dim = 64
    rng.standard_normal((37, dim))
    rng.standard_normal((5000, dim))
    centers = rng.standard_normal((8, dim)).astype(np.float32) * 4
    pts = (centers[rng.integers(0, 8, 4000)] + 0.1 * rng.standard_normal((4000, dim), dtype=np.float32)).astype(np.float16)
    dim = 128
    base = rng.standard_normal((40, dim), dtype=np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    docs = []
    for _ in range(150):
        n = int(rng.integers(5, 25))
        d = base[rng.integers(0, 40, n)] + 0.2 * rng.standard_normal((n, dim), dtype=np.float32) / np.sqrt(dim)
        docs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float16))
    return centers, pts, docs


@pytest.fixture(scope="module")
def fp():
    import fast_plaid_amd
    from fast_plaid_amd import _native
    assert _native.lib().fp_device_count() >= 1, "no MI355X visible"
    return fast_plaid_amd


@pytest.mark.parametrize("name", ["mfma128", "mfma64", "exact48", "exact128", "ties", "cap", "big"])
def test_bit_identical_to_the_model(fp, name):
    from fast_plaid_amd import kmeans
    data, k, init, seed = W.case(name)
    for it in W.NITERS:
        rc, cent, counts = W.call(data, k, it, init, seed)
        assert rc == 0, (name, it, fp._native.last_error())
        _same(name, it, cent, counts)
    t = kmeans.last_device_timings()      # of the last call: one chunk per iteration
    print(name, t)
    if name.startswith("exact"):
        assert t["narrowed_chunks"] == 0
    else:
        assert t["narrowed_chunks"] == max(W.NITERS)
        assert (t["fallback_chunks"] >= 1) if name == "cap" else (t["fallback_chunks"] == 0 or name == "ties")
    ref = _model(name)
    if name == "ties":   # not vacuous: the twins were empty and the hash reseeded them
        assert ref["reseeds"][0] >= 2 and ref["counts"][1][1] == 0 and ref["counts"][1][3] == 0 and ref["counts"][1][5] == 0
        assert ref["counts"][1][0] > 0 and ref["counts"][1][2] >= 2 and ref["counts"][1][4] >= 2
    if name == "cap":    # the 20 identical centroids: everything they attract goes to the first
        assert ref["counts"][1][0] >= 20 and not ref["counts"][1][1:20].any()
    if name == "big":
        assert np.abs(data.astype(np.float32)).max() > 290


@pytest.mark.parametrize("name", ["mfma128", "exact48"])
def test_labels_are_assign_l2s(fp, name):
    """the labels of an iteration are what fp_assign_l2 returns for the same cent16 (and hn): the model's against the device's"""
    from fast_plaid_amd import _native as N, kmeans
    data, k, init, seed = W.case(name)
    ref = _model(name)
    for it in (0, 1):
        cent16, hn = ref["cent16"][it], ref["hn"][it]
        lab = np.zeros(data.shape[0], np.int64)
        N.check(N.lib().fp_assign_l2(0, cent16.ctypes.data, hn.ctypes.data, k, data.shape[1], data.ctypes.data, data.shape[0], lab.ctypes.data))
        assert np.array_equal(lab, ref["labels"][it]), (name, it, int((lab != ref["labels"][it]).sum()))
        lab2 = kmeans.assign_l2(cent16, data)
        print(f"{name} it={it}: labels that differ from kmeans.assign_l2: {int((lab2 != ref['labels'][it]).sum())}")
        assert np.array_equal(lab2, ref["labels"][it]), (name, it)


def test_chunk_boundary(fp, tmp_path):
    """FP_TEST=kmeans_chunk=1000 with n = 2500: three assignment chunks, the last one short; the second case overflows its
    candidate lists, so the chunks' fallback flags are read back too"""
    out = str(tmp_path / "chunk.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kmeans_worker.py"), out, "chunk", "chunkcap"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=with_test_opts(dict(os.environ), kmeans_chunk=1000), timeout=600)
    assert p.returncode == 0 and "KMEANS_WORKER_OK" in p.stdout, p.stdout[-4000:]
    z = np.load(out)
    for name in ("chunk", "chunkcap"):
        for it in W.NITERS:
            _same(name, it, z[f"cent{it}_{name}"], z[f"counts{it}_{name}"])
            if it:   # three chunks per iteration took the narrowing; the identical centroids sent some on to the exact kernel
                assert z[f"chunks{it}_{name}"][0] == 3 * it and (z[f"chunks{it}_{name}"][1] >= 1) == (name == "chunkcap"), z[f"chunks{it}_{name}"]


def test_domain_errors(fp):
    data, k, init, seed = W.case("exact48")
    bad = data.copy()
    bad[1234, 17] = np.inf
    assert W.call(bad, k, 1, init, seed)[0] == -1 and "finite" in fp._native.last_error()           # FP_EINVAL
    bad[1234, 17] = np.nan
    assert W.call(bad, k, 1, init, seed)[0] == -1
    assert W.call(data[:30], k, 1, np.arange(k) % 30, seed)[0] == -1                                    # k > n
    for v in (-1, data.shape[0]):
        oob = init.copy()
        oob[5] = v
        assert W.call(data, k, 1, oob, seed)[0] == -1 and "init_rows" in fp._native.last_error()
    assert W.call(np.zeros((100, 300), np.float16), 4, 1, np.arange(4), seed)[0] == -4                 # FP_EUNSUPPORTED: dim
    rc, cent, counts = W.call(data, k, 1, init, seed)                                                   # and the handle still works
    assert rc == 0
    _same("exact48", 1, cent, counts)


def test_deterministic_and_recovers_blobs(fp):
    from fast_plaid_amd import kmeans
    data, k, init, seed = W.case("ties")
    a, b = W.call(data, k, 4, init, seed), W.call(data, k, 4, init, seed)
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    # the blob check of test_kmeans_assignment_and_create_without_centroids, restated for lloyd_device
    dim = 64
    centers, pts, _ = _parity_inputs()
    got = kmeans.lloyd_device(pts, 8, 10, np.random.default_rng(0), seed=0, max_points_per_centroid=None)
    assert got.dtype == np.float32 and got.shape == (8, dim)
    dist = np.linalg.norm(got[:, None, :] - centers[None, :, :], axis=-1)
    assert (dist.min(axis=0) < 0.5).sum() >= 6       # random-point init may merge a pair of blobs; most are recovered
    t = kmeans.last_device_timings()
    assert t["iterations"] == 10 and all(t[s] >= 0 for s in ("upload", "assign", "index", "sum", "finalise"))


def test_create_with_the_native_trainer(fp, tmp_path):
    """FastPlaid.create(docs, use_triton_kmeans=True) on the corpus of test_kmeans_assignment_and_create_without_centroids builds a
    searchable directory; compute_kmeans(native=True) returns unit-norm fp16 rows; use_triton_kmeans=None keeps the host path value
    for value (kmeans.lloyd called directly under compute_kmeans's protocol)."""
    from fast_plaid_amd import kmeans, search
    from fast_plaid_amd.search import index_io
    dim = 128
    _, _, docs = _parity_inputs()
    q = np.stack([np.pad(docs[i][:12], ((0, 12 - min(12, docs[i].shape[0])), (0, 0))) for i in (3, 77)])
    path = str(tmp_path / "native")
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.create(docs, kmeans_niters=4, nbits=4, seed=1, use_triton_kmeans=True)
        out = fpi.search(q, top_k=3, show_progress=False)
        assert [row[0][0] for row in out] == [3, 77]
    cent = kmeans.compute_kmeans(docs, dim, kmeans_niters=4, seed=1, native=True)
    assert cent.dtype == np.float16 and cent.ndim == 2 and cent.shape[1] == dim
    assert np.allclose(np.linalg.norm(cent.astype(np.float32), axis=1), 1.0, atol=2e-3)
    assert np.array_equal(np.asarray(index_io.load_index_arrays(path)["centroids"]).view(np.uint16), cent.view(np.uint16))
    # the default path: compute_kmeans's protocol around kmeans.lloyd, as before
    g = np.random.default_rng(1)
    picked = g.permutation(150)[: min(1 + int(16 * math.sqrt(120 * 150)), 150)]
    samples = np.concatenate([docs[i] for i in picked]).astype(np.float16)
    k = min(int(2 ** math.floor(math.log2(16 * math.sqrt(samples.shape[0] / 150 * 150)))), samples.shape[0])
    want = kmeans.lloyd(samples, k, 4, g, "cuda:0", 256)
    want = (want / np.maximum(np.linalg.norm(want, axis=1, keepdims=True), 1e-12)).astype(np.float16)
    assert np.array_equal(kmeans.compute_kmeans(docs, dim, kmeans_niters=4, seed=1).view(np.uint16), want.view(np.uint16))
    path2 = str(tmp_path / "host")
    with search.FastPlaid(index=path2, device="cuda:0") as fpi:
        fpi.create(docs, kmeans_niters=4, nbits=4, seed=1, use_triton_kmeans=None)
    assert np.array_equal(np.asarray(index_io.load_index_arrays(path2)["centroids"]).view(np.uint16), want.view(np.uint16))
