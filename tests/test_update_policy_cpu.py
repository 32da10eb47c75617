"""The update policy's control flow without a device: maintain.process_update / update_centroids driven with the recording stand-ins
of tests/update_policy_scenarios.py, held (a) to the REFERENCE's own run of the same scenarios
(tests/golden/pyboundary/process_update.npz, written by make_process_update_golden.py from python/fast_plaid/search/update.py) --
the same calls in the same order with the same arguments, the same files afterwards -- and (b) to expectations read off the cited
lines; then delete()'s bookkeeping on buffer.npy / embeddings.npy and the public signature."""
import inspect
import json
import os

import numpy as np
import pytest

import update_policy_model as M
import update_policy_scenarios as S
from fast_plaid_amd import maintain

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyboundary", "process_update.npz")
_RUNS = {}


def _run(name, root):
    """our mirror on one scenario -> (trace, arrays, directory snapshot, directory snapshot before); run once, shared, never modified"""
    if name not in _RUNS:
        sc = S.SCENARIOS[name]
        path, updates = S.prepare(name, str(root), maintain.save_list_arrays)
        before = S.snapshot(path, maintain.load_list_arrays)
        rec = S.Recorder(path, np.asarray, maintain.save_list_arrays)
        for docs in updates:
            maintain.process_update(index_path=path, devices=["cpu"], indices_dict={"cpu": object()}, documents_embeddings=docs, metadata=None,
                                    start_from_scratch=sc["start_from_scratch"], buffer_size=sc["buffer_size"], create_fn=rec.create,
                                    delete_fn=rec.delete, compute_kmeans_fn=rec.compute_kmeans, format_embeddings_fn=list, update_fn=rec.update,
                                    reload_fn=rec.reload, outliers_fn=rec.outliers, **S.POLICY)
        _RUNS[name] = (rec.trace, rec.arrays, S.snapshot(path, maintain.load_list_arrays), before, updates)
    return _RUNS[name]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("policy")


@pytest.mark.parametrize("name", list(S.SCENARIOS))
def test_same_calls_and_files_as_the_reference(root, name):
    trace, arrays, snap, _, _ = _run(name, root)
    got = S.flatten(trace, arrays, snap)
    z = np.load(GOLDEN)
    want = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    assert want, name
    assert json.loads(str(got["trace"])) == json.loads(str(want["trace"])), name
    assert sorted(got) == sorted(want), (name, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (name, k)


def _fns(trace):
    return [c["fn"] for c in trace]


def test_no_directory_creates(root):
    for name in ("no_dir", "no_metadata"):   # update.py:271-290
        trace, arrays, snap, _, updates = _run(name, root)
        assert _fns(trace) == ["create", "reload"]
        assert trace[0]["start_from_scratch"] == 10 and trace[0]["metadata"] is None and "compress_only" not in trace[0]
        assert np.array_equal(arrays["call0"], np.concatenate(updates[0]))


def test_rebuild_from_the_kept_embeddings(root):
    trace, arrays, snap, before, updates = _run("scratch_kept", root)   # :313-349
    assert _fns(trace) == ["create", "reload"] and trace[0]["compress_only"] is False and trace[0]["metadata"] is None
    assert arrays["call0_lens"].tolist() == [3] * 5 + [4, 2, 5]                                # the kept documents first, then the new ones
    assert np.array_equal(arrays["call0"], np.concatenate([before["embeddings"]] + updates[0]))
    assert "embeddings.npy" in snap["files"] and snap["embeddings_lens"].shape[0] == 8        # 8 <= 10: still kept
    trace, arrays, snap, _, _ = _run("scratch_crossing", root)
    assert _fns(trace) == ["create", "reload"] and arrays["call0_lens"].shape[0] == 12
    assert "embeddings.npy" not in snap["files"]                                               # 12 > 10: :339-342 removes it
    assert _run("scratch_compress_only", root)[0][0]["compress_only"] is True
    # at most start_from_scratch documents but nothing kept: the buffering path (:314-316 needs the file)
    trace, arrays, snap, _, updates = _run("scratch_no_file", root)
    assert _fns(trace) == ["update", "reload"] and trace[0]["update_threshold_centroids"] is False
    assert snap["buffer_lens"].tolist() == [4, 2, 5]


def test_buffer_grows_below_buffer_size(root):
    trace, arrays, snap, before, updates = _run("buffer_twice", root)   # :431-452
    assert _fns(trace) == ["update", "reload", "update", "reload"]
    assert [c["update_threshold_centroids"] for c in trace if c["fn"] == "update"] == [False, False]
    assert arrays["call0_lens"].tolist() == [4, 2, 5] and arrays["call2_lens"].tolist() == [3, 2]   # each call inserts only its own documents
    assert snap["buffer_lens"].tolist() == [4, 2, 5, 3, 2] and np.array_equal(snap["buffer"], np.concatenate(updates[0] + updates[1]))
    assert snap["buffer_dtype"] == "float16"
    assert snap["centroids"].tobytes() == before["centroids"].tobytes() and "compute_kmeans" not in _fns(trace)   # far tokens, but no expansion yet


def test_buffer_reached(root):
    trace, arrays, snap, before, updates = _run("reached_with_buffer", root)   # :379-429
    assert _fns(trace) == ["delete", "compute_kmeans", "reload", "update", "reload"]
    assert trace[0]["subset"] == [45, 46, 47, 48, 49] and trace[0]["_delete_metadata"] is False and trace[0]["_delete_buffer"] is False
    n_out = 4 + 1 + 5 + 2                                                       # the far tokens of the buffer and of the update
    km = trace[1]
    assert km["num_partitions"] == 4 and km["dim"] == S.DIM and km["use_triton_kmeans"] is False and km["seed"] == 42 and km["device"] == "cpu"
    assert arrays["call1"].shape == (n_out, S.DIM)
    flat = np.concatenate([before["buffer"]] + updates[0])
    assert np.array_equal(arrays["call1"], flat[np.flatnonzero(np.linalg.norm(flat.astype(np.float32), axis=1) > 2)])   # in row order
    assert trace[3]["update_threshold_centroids"] is True and arrays["call3_lens"].tolist() == [3, 4, 2, 1, 6, 5, 3, 2, 1]
    assert "buffer.npy" not in snap["files"]
    k_new = M.appended(n_out)
    assert k_new == 4 and snap["centroids"].shape == (S.N_CENT + k_new, S.DIM) and snap["centroids_dtype"] == "float32"   # :177-181
    assert np.array_equal(snap["centroids"][: S.N_CENT], before["centroids"].astype(np.float32))
    assert np.array_equal(snap["centroids"][S.N_CENT:], arrays["call1"][:k_new].astype(np.float32))
    assert snap["ivf_lengths"].tolist() == list(range(1, S.N_CENT + 1)) + [0] * k_new and snap["ivf_lengths_dtype"] == "int32"
    meta = json.loads(str(snap["metadata_json"]))
    assert meta["num_partitions"] == S.N_CENT + k_new and meta["num_documents"] == 50 - 5 + 9
    # without a buffer file nothing is deleted
    trace, arrays, snap, _, _ = _run("reached_at_once", root)
    assert _fns(trace) == ["compute_kmeans", "reload", "update", "reload"] and trace[2]["update_threshold_centroids"] is True


def test_no_outliers_leaves_the_centroid_files(root):
    trace, arrays, snap, before, _ = _run("reached_no_outliers", root)   # :155-158
    assert _fns(trace) == ["delete", "reload", "update", "reload"] and trace[2]["update_threshold_centroids"] is True
    for k in ("centroids", "centroids_dtype", "ivf_lengths"):
        assert snap[k].tobytes() == before[k].tobytes(), k
    assert json.loads(str(snap["metadata_json"]))["num_partitions"] == S.N_CENT and "buffer.npy" not in snap["files"]


def test_compress_only_has_no_lists_to_extend(root):
    trace, arrays, snap, before, _ = _run("reached_compress_only", root)   # :183-188
    assert "compute_kmeans" in _fns(trace) and "ivf_lengths.npy" not in snap["files"]
    assert snap["centroids"].shape[0] == S.N_CENT + M.appended(5 * 3 + 3 * 4)
    assert json.loads(str(snap["metadata_json"]))["compress_only"] is True


@pytest.mark.parametrize("n_out, k", [(1, 4), (256, 4), (257, 8), (1025, 20)])
def test_k_update(root, n_out, k):
    trace, arrays, snap, _, _ = _run(f"k_update_{n_out}", root)   # :161-162
    assert M.k_update(n_out) == k and trace[0]["fn"] == "compute_kmeans" and trace[0]["num_partitions"] == k
    assert arrays["call0"].shape[0] == n_out and snap["centroids"].shape[0] == S.N_CENT + min(k, n_out)


def _kept_dir(path, n_docs, n_kept, n_buf):
    rng = np.random.default_rng(9)
    kept = [S.near_doc(rng, 2 + i) for i in range(n_kept)]
    buf = [S.near_doc(rng, 20 + i) for i in range(n_buf)]
    S.make_dir(path, n_docs, kept=kept or None, buffer=buf or None, save_list=maintain.save_list_arrays)
    return kept, buf


def _after_delete(path, n_docs, subset):
    """filter_kept_embeddings as FastPlaid.delete calls it: after the native delete has lowered num_documents"""
    meta = json.load(open(os.path.join(path, "metadata.json")))
    meta["num_documents"] = n_docs - len(subset)
    json.dump(meta, open(os.path.join(path, "metadata.json"), "w"))
    maintain.filter_kept_embeddings(path, subset)
    return sorted(os.listdir(path))


def test_delete_bookkeeping(tmp_path):
    # fast_plaid.py:1093-1116: embeddings.npy is indexed like the index
    p = str(tmp_path / "kept")
    kept, _ = _kept_dir(p, 6, 6, 0)
    _after_delete(p, 6, [1, 4, 17])
    rest = maintain.load_list_arrays(os.path.join(p, "embeddings.npy"))
    assert [r.shape[0] for r in rest] == [2, 4, 5, 7] and all(np.array_equal(r, kept[i]) for r, i in zip(rest, (0, 2, 3, 5)))
    assert "embeddings.npy" not in _after_delete(p, 4, [0, 1, 2, 3])                      # nothing left: the file goes
    # :1118-1143: the buffer holds the LAST documents, counted from num_documents as read after the delete
    p = str(tmp_path / "buf")
    _, buf = _kept_dir(p, 20, 0, 4)
    _after_delete(p, 20, [3, 15])                 # 18 documents left, buffer = ids 14..17: id 15 is its entry 1
    rest = maintain.load_list_arrays(os.path.join(p, "buffer.npy"))
    assert [r.shape[0] for r in rest] == [20, 22, 23] and np.array_equal(rest[1], buf[2])
    before = open(os.path.join(p, "buffer.npy"), "rb").read()
    _after_delete(p, 18, [0, 1])                  # outside the buffer: untouched
    assert open(os.path.join(p, "buffer.npy"), "rb").read() == before
    # the policy's own delete of the buffered documents (the last len(buffer) ids) leaves buffer.npy to process_update
    p = str(tmp_path / "own")
    _kept_dir(p, 20, 0, 4)
    assert "buffer.npy" in _after_delete(p, 20, [16, 17, 18, 19])
    assert len(maintain.load_list_arrays(os.path.join(p, "buffer.npy"))) == 4
    # neither file: nothing changes
    p = str(tmp_path / "plain")
    _kept_dir(p, 20, 0, 0)
    files = sorted(os.listdir(p))
    assert _after_delete(p, 20, [2, 3]) == files


def test_public_surface(tmp_path):
    from fast_plaid_amd.search import FastPlaid
    sig = inspect.signature(FastPlaid.update).parameters
    assert sig["buffer_size"].default is None and sig["buffer_size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["start_from_scratch"].default == 999 and sig["use_triton_kmeans"].default is False and sig["seed"].default == 42
    assert list(sig)[:5] == ["self", "documents_embeddings", "metadata", "batch_size", "update_threshold_centroids"]
    assert inspect.signature(FastPlaid.create).parameters["start_from_scratch"].default is None
    d = inspect.signature(FastPlaid.delete).parameters
    assert d["_delete_metadata"].default is True and d["_delete_buffer"].default is True
    fp = FastPlaid(index=str(tmp_path / "nothing"), device="cuda:0")
    with pytest.raises(ValueError, match="update_threshold_centroids"):
        fp.update([np.zeros((3, 16), np.float16)], buffer_size=8, update_threshold_centroids=True)
    with pytest.raises(NotImplementedError):
        fp.update([np.zeros((3, 16), np.float16)], metadata=[{}], buffer_size=8)
    with pytest.raises(FileNotFoundError):   # the default path as before: no index, nothing to append to
        fp.update([np.zeros((3, 16), np.float16)])
