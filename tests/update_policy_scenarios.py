"""Scenarios of the update policy (python/fast_plaid/search/update.py:206-452 process_update, :65-203 update_centroids) and the
recording stand-ins that drive them -- shared by tests/test_update_policy_cpu.py, which runs OUR mirror (maintain.process_update),
and by tests/golden/pyboundary/make_process_update_golden.py, which runs the REFERENCE's module on the same inputs and stores what
it did.  Nothing here touches a device: every collaborator is a stand-in that records its call and applies the one side effect
the control flow depends on (the document count in metadata.json, embeddings.npy on create).

A run's record: `trace`, the calls in order, each {"fn", scalar arguments, "arrays": the name its embeddings go by}, the embeddings
themselves as arrays, and the directory afterwards (file list, metadata.json text, centroids / ivf_lengths / buffer / embeddings)."""
import json
import os

import numpy as np

DIM = 16
N_CENT = 8
THRESHOLD = 0.5


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def centroids():
    return _unit(np.random.default_rng(5).standard_normal((N_CENT, DIM))).astype(np.float16)


def near_doc(rng, n):
    """n tokens within 0.1 of a centroid: squared distance below 0.02, far under THRESHOLD^2 = 0.25"""
    c = centroids().astype(np.float32)
    return (c[rng.integers(0, N_CENT, n)] + 0.1 * _unit(rng.standard_normal((n, DIM)))).astype(np.float16)


def far_doc(rng, n):
    """n tokens of norm 3: at least (3 - 1)^2 = 4 from every unit centroid"""
    return (3.0 * _unit(rng.standard_normal((n, DIM)))).astype(np.float16)


def make_dir(path, n_docs, compress_only=False, kept=None, buffer=None, save_list=None):
    os.makedirs(path, exist_ok=True)
    meta = {"num_chunks": 1, "nbits": 4, "num_partitions": N_CENT, "num_embeddings": 10 * n_docs, "num_documents": n_docs, "avg_doclen": 10.0}
    if compress_only:
        meta["compress_only"] = True
    with open(os.path.join(path, "metadata.json"), "w") as f:
        json.dump(meta, f, indent=2)
    np.save(os.path.join(path, "centroids.npy"), centroids())
    np.save(os.path.join(path, "cluster_threshold.npy"), np.asarray(THRESHOLD, np.float32).reshape(()))
    if not compress_only:
        np.save(os.path.join(path, "ivf_lengths.npy"), np.arange(1, N_CENT + 1, dtype=np.int32))
    if kept is not None:
        save_list(os.path.join(path, "embeddings.npy"), kept)
    if buffer is not None:
        save_list(os.path.join(path, "buffer.npy"), buffer)


def _docs(seed, spec):
    """spec: list of ("near" | "far", n_tokens) per document, or ("mixed", n_near, n_far) -> one document"""
    rng = np.random.default_rng(seed)
    out = []
    for s in spec:
        if s[0] == "mixed":
            out.append(np.concatenate([near_doc(rng, s[1]), far_doc(rng, s[2])]))
        else:
            out.append((near_doc if s[0] == "near" else far_doc)(rng, s[1]))
    return out


def _k(n_out):
    return dict(dir=dict(n_docs=50), updates=[[("mixed", 3, n_out)]], start_from_scratch=10, buffer_size=1)


# name -> dir: make_dir's arguments (None: no directory; "empty": a directory without metadata.json), kept / buffer: document
# specs of embeddings.npy / buffer.npy, updates: the document specs of successive process_update calls
SCENARIOS = {
    "no_dir": dict(dir=None, updates=[[("near", 4), ("near", 6)]], start_from_scratch=10, buffer_size=8),
    "no_metadata": dict(dir="empty", updates=[[("near", 4)]], start_from_scratch=10, buffer_size=8),
    "scratch_kept": dict(dir=dict(n_docs=5), kept=[("near", 3)] * 5, updates=[[("near", 4), ("far", 2), ("near", 5)]], start_from_scratch=10,
                         buffer_size=8),
    "scratch_no_file": dict(dir=dict(n_docs=5), updates=[[("near", 4), ("far", 2), ("near", 5)]], start_from_scratch=10, buffer_size=8),
    "scratch_crossing": dict(dir=dict(n_docs=8), kept=[("near", 3)] * 8, updates=[[("near", 4)] * 4], start_from_scratch=10, buffer_size=8),
    "scratch_compress_only": dict(dir=dict(n_docs=5, compress_only=True), kept=[("near", 3)] * 5, updates=[[("near", 4)]],
                                  start_from_scratch=10, buffer_size=8),
    "buffer_twice": dict(dir=dict(n_docs=50), updates=[[("near", 4), ("far", 2), ("near", 5)], [("far", 3), ("near", 2)]],
                         start_from_scratch=10, buffer_size=8),
    "reached_with_buffer": dict(dir=dict(n_docs=50), buffer=[("near", 3), ("far", 4), ("near", 2), ("far", 1), ("near", 6)],
                                updates=[[("far", 5), ("near", 3), ("far", 2), ("near", 1)]], start_from_scratch=10, buffer_size=8),
    "reached_at_once": dict(dir=dict(n_docs=50), updates=[[("far", 3)] * 4 + [("near", 3)] * 4], start_from_scratch=10, buffer_size=8),
    "reached_no_outliers": dict(dir=dict(n_docs=50), buffer=[("near", 3)] * 5, updates=[[("near", 4)] * 3], start_from_scratch=10,
                                buffer_size=8),
    "reached_compress_only": dict(dir=dict(n_docs=50, compress_only=True), buffer=[("far", 3)] * 5, updates=[[("far", 4)] * 3],
                                  start_from_scratch=10, buffer_size=8),
    "k_update_1": _k(1), "k_update_256": _k(256), "k_update_257": _k(257), "k_update_1025": _k(1025),
}
POLICY = dict(batch_size=25_000, kmeans_niters=4, max_points_per_centroid=256, n_samples_kmeans=None, seed=42, use_triton_kmeans=False)


def prepare(name, root, save_list):
    """-> (index_path, [documents of every update])"""
    sc = SCENARIOS[name]
    path = os.path.join(root, name)
    if sc["dir"] == "empty":
        os.makedirs(path)
    elif sc["dir"] is not None:
        make_dir(path, save_list=save_list, kept=_docs(101, sc["kept"]) if "kept" in sc else None,
                 buffer=_docs(202, sc["buffer"]) if "buffer" in sc else None, **sc["dir"])
    return path, [_docs(303 + i, spec) for i, spec in enumerate(sc["updates"])]


def brute_min_l2sq(cent, x):
    """exact float32 nearest squared distance, what the reference's CPU branch asks usearch for (update.py:127-141)"""
    c = np.asarray(cent, np.float32)
    x = np.asarray(x, np.float32)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=-1, dtype=np.float32).min(axis=1)


class Recorder:
    """the stand-ins; `to_np` turns whatever the driver hands over (numpy arrays, torch tensors) into numpy"""

    def __init__(self, index_path, to_np, save_list):
        self.path, self.to_np, self.save_list = index_path, to_np, save_list
        self.trace, self.arrays = [], {}

    def _keep(self, docs):
        name = f"call{len(self.trace)}"
        docs = [self.to_np(d) for d in docs]
        self.arrays[name + "_lens"] = np.array([d.shape[0] for d in docs], np.int64)
        self.arrays[name] = np.concatenate([d.reshape(-1, d.shape[-1]) for d in docs]) if docs else np.zeros((0, DIM), np.float16)
        return name

    def _meta(self, fn):
        p = os.path.join(self.path, "metadata.json")
        with open(p) as f:
            meta = json.load(f)
        fn(meta)
        with open(p, "w") as f:
            json.dump(meta, f, indent=2)

    def create(self, documents_embeddings, **kw):
        docs = [self.to_np(d) for d in documents_embeddings]
        self.trace.append(dict(fn="create", arrays=self._keep(docs), **kw))
        os.makedirs(self.path, exist_ok=True)
        meta = {"num_chunks": 1, "nbits": 4, "num_partitions": N_CENT, "num_documents": len(docs)}
        if kw.get("compress_only"):
            meta["compress_only"] = True
        with open(os.path.join(self.path, "metadata.json"), "w") as f:
            json.dump(meta, f, indent=2)
        if len(docs) <= kw["start_from_scratch"]:   # fast_plaid.py:575-582
            self.save_list(os.path.join(self.path, "embeddings.npy"), docs)

    def delete(self, subset, **kw):
        self.trace.append(dict(fn="delete", subset=[int(i) for i in subset], **kw))
        self._meta(lambda m: m.update(num_documents=m["num_documents"] - len(subset)))

    def update(self, embeddings, device, batch_size, update_threshold_centroids, **ignored):
        self.trace.append(dict(fn="update", arrays=self._keep(embeddings), device=device, batch_size=batch_size,
                               update_threshold_centroids=update_threshold_centroids))
        self._meta(lambda m: m.update(num_documents=m["num_documents"] + len(embeddings)))

    def compute_kmeans(self, documents_embeddings, **kw):
        rows = self.to_np(documents_embeddings)
        rows = rows.reshape(-1, rows.shape[-1])
        self.trace.append(dict(fn="compute_kmeans", arrays=self._keep([rows]), **kw))
        return rows[: min(kw["num_partitions"], rows.shape[0])].astype(np.float32)   # "centroids": the first K outlier rows

    def reload(self):
        self.trace.append(dict(fn="reload"))

    def outliers(self, cent, flat, threshold, device):
        d = brute_min_l2sq(cent, flat)
        return np.flatnonzero(d > threshold ** 2).astype(np.int64), d, None


def snapshot(index_path, load_list):
    """the directory as arrays: file list, metadata.json text, the files update_centroids and the buffering write"""
    out = {"files": np.array(sorted(os.listdir(index_path)) if os.path.isdir(index_path) else [], dtype="U64")}
    p = os.path.join(index_path, "metadata.json")
    if os.path.exists(p):
        out["metadata_json"] = np.array(open(p).read())
    for f in ("centroids.npy", "ivf_lengths.npy", "cluster_threshold.npy"):
        if os.path.exists(os.path.join(index_path, f)):
            a = np.load(os.path.join(index_path, f))
            out[f[:-4]] = a
            out[f[:-4] + "_dtype"] = np.array(str(a.dtype))
    for f in ("buffer.npy", "embeddings.npy"):
        if os.path.exists(os.path.join(index_path, f)):
            docs = [np.asarray(d) for d in load_list(os.path.join(index_path, f))]
            out[f[:-4] + "_lens"] = np.array([d.shape[0] for d in docs], np.int64)
            out[f[:-4]] = np.concatenate(docs) if docs else np.zeros((0, DIM), np.float16)
            out[f[:-4] + "_dtype"] = np.array(str(docs[0].dtype) if docs else "")
    return out


def flatten(record_trace, arrays, snap):
    """one scenario's record as a flat {key: array} (what the golden file stores per scenario)"""
    out = {"trace": np.array(json.dumps(record_trace, sort_keys=True))}
    out.update({"arr_" + k: v for k, v in arrays.items()})
    out.update({"dir_" + k: v for k, v in snap.items()})
    return out
