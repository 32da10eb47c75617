"""The nearest-centroid assignment at every accepted dim (k_assign_mfma_sl, the sliced k_assign_exact) behind fp_compress,
fp_assign_l2 and fp_kmeans, against the ATen restatement and the numpy k-means model, bit for bit.  Run as a program (FP_TEST is
read inside the library: a setting is one process), `test_assign_sliced_gpu.py OUT.npz` compresses the TWO_KERNELS cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (dim, nbits, C): one 8-dim unit; an odd unit count; dim 96; one unit past a 64-, 128- and 256-dim boundary; two large dims; a
# small table (the sliced exact kernel directly); 12 copies of one centroid (narrowing, overflow, then the sliced exact kernel)
CASES = [(8, 8, 300), (40, 4, 300), (96, 4, 300), (72, 2, 300), (136, 4, 257), (264, 2, 300), (768, 4, 1030), (1024, 1, 300),
         (520, 4, 77), (384, 4, 4096)]
TWO_KERNELS = [(128, 4, 300), (64, 2, 300)]   # dims with a fixed-dim MFMA kernel: FP_TEST=assign_sliced=1 sends them through the sliced one


def corpus(dim, nbits, C, n_docs=60):
    """unit-norm centroids with exact duplicates at rows 3, 7 and C - 1, tokens = centroid + noise, 20 % of them on the duplicated
    centroid; C == 4096: 12 copies of one centroid with 10 % of the tokens -> (docs, cent) as fp16 torch tensors.
    The (1, 1, 0) counts asserted below are conditions on these draws, checked on the CPU when the seeds were fixed (an fp32 matmul
    for the MFMA scores, k_assign_thr's window widened by 1e-6): at most 4 centroids inside the window of any token of CASES and
    TWO_KERNELS, 13 in the 12-copy case; k_assign_thr_l2's window holds at most 2 in every iteration of the k-means cases."""
    import torch
    g = torch.Generator().manual_seed(7000 + dim + C)
    cent = torch.nn.functional.normalize(torch.randn(C, dim, generator=g), dim=-1).to(torch.float16)
    cent[7] = cent[3]
    cent[C - 1] = cent[3]
    if C == 4096:
        cent[100:112] = cent[50]
    docs = []
    for _ in range(n_docs):
        n = int(torch.randint(1, 50, (1,), generator=g))
        pick = torch.randint(0, C, (n,), generator=g)
        pick[torch.rand(n, generator=g) < 0.2] = 3
        if C == 4096:
            pick[torch.rand(n, generator=g) < 0.1] = 50
        d = cent[pick].float() + 0.25 * torch.randn(n, dim, generator=g) / dim ** 0.5
        docs.append(torch.nn.functional.normalize(d, dim=-1).to(torch.float16))
    assert sum(d.shape[0] for d in docs) % 128 != 0
    return docs, cent


def built(docs, cent, nbits):
    """create.build_index_arrays of a corpus and the counts of its last fp_compress (the whole corpus, one chunk)"""
    from fast_plaid_amd import create as CR
    got = CR.build_index_arrays([d.numpy() for d in docs], cent.numpy(), nbits, "cuda:0")
    n = CR.last_compress_counts()
    return got, (n["chunks"], n["narrowed_chunks"], n["fallback_chunks"])


@pytest.mark.parametrize("dim,nbits,C", CASES)
def test_compress_matches_the_aten_restatement(dim, nbits, C):
    import plaid_oracle_torch as OT
    docs, cent = corpus(dim, nbits, C)
    ref = OT.build_index_arrays(docs, cent, nbits, cast_cutoffs=False)
    T = int(ref["doc_lengths"].sum())
    got, counts = built(docs, cent, nbits)
    assert np.array_equal(got["doc_codes"], ref["doc_codes"].numpy()[:T]), "nearest-centroid codes differ"
    assert np.array_equal(got["doc_residuals"], ref["doc_residuals"].numpy()[:T]), "packed residual bytes differ"
    for k in ("bucket_cutoffs", "bucket_weights"):
        assert np.array_equal(got[k].view(np.uint16), ref[k].numpy().view(np.uint16)), k
    assert np.array_equal(got["ivf"], ref["ivf"].numpy()) and np.array_equal(got["ivf_lengths"], ref["ivf_lengths"].numpy())
    assert counts == ((1, 0, 0) if C < 256 else (1, 1, 1) if C == 4096 else (1, 1, 0))


@pytest.mark.parametrize("dim,C", [(264, 70), (1024, 300)])
def test_assign_l2_matches_the_model(dim, C):
    import kmeans_model as M
    from fast_plaid_amd import kmeans
    rng = np.random.default_rng(dim + C)
    cent = (rng.standard_normal((C, dim)) / np.sqrt(dim)).astype(np.float16)
    cent[5] = cent[2]                                   # an exact tie: the lower index wins
    data = (cent[rng.integers(0, C, 333)].astype(np.float32) + 0.5 * rng.standard_normal((333, dim)) / np.sqrt(dim)).astype(np.float16)
    hn = (0.5 * (cent.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)   # kmeans.assign_l2's own
    want = M.assign(data, cent, hn)
    got = kmeans.assign_l2(cent, data)
    assert np.array_equal(got, want)
    assert not (want == 5).any() and (want == 2).any()


@pytest.mark.parametrize("dim,k", [(96, 300), (256, 300)])
def test_kmeans_narrows_at_other_dims(dim, k):
    import kmeans_model as M
    import kmeans_worker as W
    from fast_plaid_amd import _native as N, kmeans
    rng = np.random.default_rng(dim)
    data = W._unit(rng, 1501, dim)
    init = np.ascontiguousarray(rng.permutation(1501)[:k], np.int64)
    ref = M.run(data, k, 4, init, 99)
    for it in (0, 1, 4):
        rc, cent, counts = W.call(data, k, it, init, 99)
        assert rc == 0, N.last_error()
        assert np.array_equal(counts, ref["counts"][it])
        assert np.array_equal(cent.view(np.uint32), ref["cent32"][it].view(np.uint32))
    t = kmeans.last_device_timings()
    assert t["narrowed_chunks"] == 4 and t["fallback_chunks"] == 0, t


def test_the_two_mfma_kernels_agree(tmp_path):
    from fptest_env import with_test_opts
    out = str(tmp_path / "sliced.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=with_test_opts(dict(os.environ), assign_sliced=1), timeout=600)
    assert p.returncode == 0 and "ASSIGN_SLICED_OK" in p.stdout, p.stdout[-4000:]
    z = np.load(out)
    for dim, nbits, C in TWO_KERNELS:
        got, counts = built(*corpus(dim, nbits, C), nbits)
        assert counts == (1, 1, 0) and tuple(z[f"counts{dim}"]) == (1, 1, 0)
        assert got["doc_codes"].tobytes() == z[f"codes{dim}"].tobytes() and got["doc_residuals"].tobytes() == z[f"res{dim}"].tobytes()


def test_create_search_update_at_dim_384(tmp_path):
    from fast_plaid_amd import search
    rng = np.random.default_rng(5)
    dim, C = 384, 300
    cent = rng.standard_normal((C, dim), dtype=np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    docs = []
    for _ in range(205):
        n = int(rng.integers(4, 30))
        d = cent[rng.integers(0, C, n)] + 0.3 * rng.standard_normal((n, dim), dtype=np.float32) / np.sqrt(dim)
        docs.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float16))
    query = lambda ids: np.stack([np.pad(docs[i][:16], ((0, 16 - min(16, docs[i].shape[0])), (0, 0))) for i in ids])  # noqa: E731
    path = str(tmp_path / "idx")
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.create(docs[:200], centroids=cent, nbits=4)
        assert os.path.exists(os.path.join(path, "metadata.json"))
    with search.FastPlaid(index=path, device="cuda:0") as again:    # a fresh object loads the directory from disk
        out = again.search(query((5, 50, 150)), top_k=3, n_ivf_probe=8, show_progress=False)
        assert [row[0][0] for row in out] == [5, 50, 150]
        again.update(docs[200:])
        out = again.search(query((50, 200, 204)), top_k=3, n_ivf_probe=8, show_progress=False)
        assert [row[0][0] for row in out] == [50, 200, 204]


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    res = {}
    for dim_, nbits_, C_ in TWO_KERNELS:
        got_, counts_ = built(*corpus(dim_, nbits_, C_), nbits_)
        res[f"codes{dim_}"], res[f"res{dim_}"], res[f"counts{dim_}"] = got_["doc_codes"], got_["doc_residuals"], np.array(counts_)
    np.savez(sys.argv[1], **res)
    print("ASSIGN_SLICED_OK")
