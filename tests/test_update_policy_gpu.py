"""FastPlaid.update(buffer_size=...) end to end on a dim-128 corpus of 300 short documents: an index that receives documents from
another distribution gains exactly the centroids the model's outlier set asks for and stays searchable and oracle-consistent; the
policy's directory equals the one the existing pieces give when called by hand; no drift adds no centroid; the default update is
unchanged; a small index that kept its embeddings is rebuilt."""
import json
import os
import shutil

import numpy as np
import pytest

import update_policy_model as M

pytestmark = pytest.mark.gpu

DIM, N_A, N_DOCS = 128, 40, 300
BUFFER, SCRATCH = 8, 6


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _docs(rng, base, n, noise=0.2):
    out = []
    for _ in range(n):
        ln = int(rng.integers(5, 13))
        d = base[rng.integers(0, base.shape[0], ln)] + noise * rng.standard_normal((ln, DIM), dtype=np.float32) / np.sqrt(DIM)
        out.append(_unit(d).astype(np.float16))
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """clusters A with an index created on them (once; the tests work on copies), clusters B far from every A centroid"""
    from fast_plaid_amd import _native, search
    assert _native.lib().fp_device_count() >= 1, "no MI355X visible"
    rng = np.random.default_rng(77)
    base_a = _unit(rng.standard_normal((N_A, DIM), dtype=np.float32))
    base_b = _unit(rng.standard_normal((10, DIM), dtype=np.float32))
    docs_a = _docs(rng, base_a, N_DOCS)
    path = str(tmp_path_factory.mktemp("policy") / "a")
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.create(docs_a, centroids=base_a.astype(np.float16), nbits=4, seed=3)
    return dict(path=path, base_a=base_a, base_b=base_b, docs_a=docs_a, docs_b=_docs(rng, base_b, 12),
                docs_tight=_docs(rng, base_a, 9, noise=0.05), root=os.path.dirname(path))


def _copy(world, name):
    dst = os.path.join(world["root"], name)
    shutil.copytree(world["path"], dst)
    return dst


def _files(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


def _same_dir(a, b):
    fa, fb = _files(a), _files(b)
    assert sorted(fa) == sorted(fb), sorted(set(fa) ^ set(fb))
    diff = [f for f in fa if fa[f] != fb[f]]
    assert not diff, diff


def _model_outliers(path, docs):
    """the model's outlier rows of `docs` against the directory as it stands"""
    cent = np.load(os.path.join(path, "centroids.npy")).astype(np.float16)
    thr = float(np.load(os.path.join(path, "cluster_threshold.npy")).item())
    flat = np.concatenate(docs)
    return flat, M.outliers(cent, flat, M.threshold_sq(thr))[0]


def _check_against_oracle(fpi, path, queries, top_k=5):
    from class_fuzz_worker import oracle_of
    from parity import check_final
    arr, orc = oracle_of(path)
    out = fpi.search(queries, top_k=top_k, n_full_scores=64, n_ivf_probe=4, show_progress=False)
    L = max(q.shape[0] for q in queries)
    for b, row in enumerate(out):
        q3 = np.pad(queries[b], ((0, L - queries[b].shape[0]), (0, 0)))[None]
        ref = orc.search(q3, top_k, 64, 4)[0]
        check_final(np.array([p for p, _ in row], np.int64), np.array([s for _, s in row], np.float32), ref[0], ref[1], top_k)
    return arr, out


def test_drift_grows_the_centroids_and_composes(world):
    from fast_plaid_amd import kmeans, maintain, search
    path = _copy(world, "drift")
    b = world["docs_b"]
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.update(b[:5], buffer_size=BUFFER, start_from_scratch=SCRATCH)        # 5 < 8: appended and remembered
        assert [d.shape[0] for d in maintain.load_list_arrays(os.path.join(path, "buffer.npy"))] == [d.shape[0] for d in b[:5]]
        assert np.load(os.path.join(path, "centroids.npy")).shape[0] == N_A
        assert json.load(open(os.path.join(path, "metadata.json")))["num_documents"] == N_DOCS + 5
        by_hand = os.path.join(world["root"], "by_hand")
        shutil.copytree(path, by_hand)
        flat, rows = _model_outliers(path, b[:9])
        assert rows.shape[0] == flat.shape[0] > 40                                # clusters B: every token is far from every A centroid
        k_new = M.appended(rows.shape[0])
        assert k_new == 4
        fpi.update(b[5:9], buffer_size=BUFFER, start_from_scratch=SCRATCH)       # 9 >= 8: expand, insert the nine again
        assert maintain.last_outlier_counts()["chunks"] == 1
        meta = json.load(open(os.path.join(path, "metadata.json")))
        cent = np.load(os.path.join(path, "centroids.npy"))
        assert cent.shape[0] == N_A + k_new == meta["num_partitions"] == np.load(os.path.join(path, "ivf_lengths.npy")).shape[0]
        assert meta["num_documents"] == N_DOCS + 9 and not os.path.exists(os.path.join(path, "buffer.npy"))
        queries = [b[2], b[7], world["docs_a"][11]]
        arr, out = _check_against_oracle(fpi, path, queries)
        assert [row[0][0] for row in out] == [N_DOCS + 2, N_DOCS + 7, 11]
        assert arr["centroids"].shape[0] == N_A + k_new
        codes_b = arr["doc_codes"][int(arr["doc_lengths"][:N_DOCS].sum()):]
        assert (codes_b >= N_A).all()                                             # the B tokens are quantised against the NEW centroids
    # composition: the same directory from the existing pieces called by hand
    buf = maintain.load_list_arrays(os.path.join(by_hand, "buffer.npy"))
    maintain.delete_from_index(by_hand, list(range(N_DOCS, N_DOCS + 5)))
    docs = buf + [np.asarray(d) for d in b[5:9]]
    flat, rows = _model_outliers(by_hand, docs)
    new = kmeans.compute_kmeans(flat[rows].reshape(rows.shape[0], 1, DIM), DIM, "cuda:0", 4, 256, 42, None,
                                num_partitions=M.k_update(rows.shape[0]), native=False)
    old = np.load(os.path.join(by_hand, "centroids.npy"))
    np.save(os.path.join(by_hand, "centroids.npy"), np.concatenate([old, new.astype(np.float32)]))
    lens = np.load(os.path.join(by_hand, "ivf_lengths.npy"))
    np.save(os.path.join(by_hand, "ivf_lengths.npy"), np.concatenate([lens, np.zeros(new.shape[0], lens.dtype)]))
    meta = json.load(open(os.path.join(by_hand, "metadata.json")))
    meta["num_partitions"] = N_A + new.shape[0]
    json.dump(meta, open(os.path.join(by_hand, "metadata.json"), "w"), indent=4)
    os.remove(os.path.join(by_hand, "buffer.npy"))
    maintain.update_index(by_hand, docs, "cuda:0", update_threshold=True)
    _same_dir(path, by_hand)


def test_native_trainer_is_selected(world):
    """use_triton_kmeans=True trains the new centroids with fp_kmeans, as in create"""
    from fast_plaid_amd import kmeans, search
    path = _copy(world, "native")
    b = world["docs_b"]
    flat, rows = _model_outliers(path, b[:8])
    want = kmeans.compute_kmeans(flat[rows].reshape(rows.shape[0], 1, DIM), DIM, "cuda:0", 4, 256, 42, None,
                                 num_partitions=M.k_update(rows.shape[0]), native=True)
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.update(b[:8], buffer_size=BUFFER, start_from_scratch=SCRATCH, use_triton_kmeans=True)
        _check_against_oracle(fpi, path, [b[0], b[5]])
    cent = np.load(os.path.join(path, "centroids.npy"))
    assert np.array_equal(cent[N_A:], want.astype(np.float32))


def test_no_drift_adds_no_centroid(world):
    from fast_plaid_amd import search
    path = _copy(world, "nodrift")
    # from clusters A, tighter than the corpus: the threshold is the corpus's own 0.75 quantile of residual norms, so a quarter of
    # equally noisy tokens would count as outliers by construction
    docs = world["docs_tight"][:8]
    flat, rows = _model_outliers(path, docs)
    assert rows.shape[0] == 0
    before = open(os.path.join(path, "centroids.npy"), "rb").read()
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.update(docs, buffer_size=BUFFER, start_from_scratch=SCRATCH)
        arr, out = _check_against_oracle(fpi, path, [docs[3], world["docs_a"][5]])
        assert [row[0][0] for row in out] == [N_DOCS + 3, 5]
    assert open(os.path.join(path, "centroids.npy"), "rb").read() == before
    meta = json.load(open(os.path.join(path, "metadata.json")))
    assert meta["num_partitions"] == json.load(open(os.path.join(world["path"], "metadata.json")))["num_partitions"]
    assert meta["num_documents"] == N_DOCS + 8 and not os.path.exists(os.path.join(path, "buffer.npy"))


def test_default_update_is_unchanged(world):
    from fast_plaid_amd import maintain, search
    a, b = _copy(world, "default_a"), _copy(world, "default_b")
    docs = world["docs_b"][:3] + world["docs_tight"][:3]
    for flag in (False, True):
        with search.FastPlaid(index=a, device="cuda:0") as fpi:
            fpi.update(docs, update_threshold_centroids=flag)
        maintain.update_index(b, docs, "cuda:0", update_threshold=flag)
        _same_dir(a, b)
    assert not os.path.exists(os.path.join(a, "buffer.npy")) and np.load(os.path.join(a, "centroids.npy")).shape[0] == N_A
    # create / delete without the new arguments write and touch nothing new
    with search.FastPlaid(index=a, device="cuda:0") as fpi:
        fpi.delete([1, N_DOCS])
    maintain.delete_from_index(b, [1, N_DOCS])
    _same_dir(a, b)
    assert not os.path.exists(os.path.join(world["path"], "embeddings.npy"))


def test_rebuild_from_scratch(world):
    from fast_plaid_amd import maintain, search
    from fast_plaid_amd.search import index_io
    path = os.path.join(world["root"], "scratch")
    docs = world["docs_a"][:4] + world["docs_b"][:5]
    emb = os.path.join(path, "embeddings.npy")
    with search.FastPlaid(index=path, device="cuda:0") as fpi:
        fpi.create(docs[:4], seed=1, start_from_scratch=SCRATCH)
        assert [d.shape[0] for d in maintain.load_list_arrays(emb)] == [d.shape[0] for d in docs[:4]]
        fpi.update(docs[4:6], buffer_size=BUFFER, start_from_scratch=SCRATCH)    # 4 <= 6 and the embeddings were kept: rebuilt with all six
        kept = maintain.load_list_arrays(emb)
        assert len(kept) == 6 and all(np.array_equal(k, d) for k, d in zip(kept, docs[:6]))
        assert index_io.load_index_arrays(path)["doc_lengths"].tolist() == [d.shape[0] for d in docs[:6]]
        fpi.update(docs[6:9], buffer_size=BUFFER, start_from_scratch=SCRATCH)    # 6 <= 6: rebuilt with nine, past the limit
        assert not os.path.exists(emb) and not os.path.exists(os.path.join(path, "buffer.npy"))
        arr, out = _check_against_oracle(fpi, path, [docs[1], docs[5], docs[8]], top_k=3)
        assert arr["doc_lengths"].tolist() == [d.shape[0] for d in docs] and [row[0][0] for row in out] == [1, 5, 8]
        fpi.delete([0])                                                           # nothing kept any more: the plain delete
        assert json.load(open(os.path.join(path, "metadata.json")))["num_documents"] == 8
    # delete on a directory that keeps its embeddings filters them too
    path2 = os.path.join(world["root"], "scratch2")
    with search.FastPlaid(index=path2, device="cuda:0") as fpi:
        fpi.create(docs[:5], seed=1, start_from_scratch=SCRATCH)
        fpi.delete([1, 3])
    kept = maintain.load_list_arrays(os.path.join(path2, "embeddings.npy"))
    assert len(kept) == 3 and all(np.array_equal(k, docs[i]) for k, i in zip(kept, (0, 2, 4)))
