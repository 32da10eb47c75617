"""Generates tests/golden/pyboundary/process_update.npz  (run in the build container only; reads /root/reference).

What is pinned: the control flow of the REFERENCE's update policy -- `process_update` and `update_centroids` of
python/fast_plaid/search/update.py -- executed here on the seeded dim-16 scenarios of tests/update_policy_scenarios.py.  update.py
is imported from /root/reference by file path inside a throw-away package; what it imports is satisfied by placeholders: the native
`fast_plaid_rust` (a recording `update`), `usearch.index.Index` (an exact float32 brute-force nearest-distance stand-in), the sqlite
filtering, and the loader functions (recording reloads; an own object-array writer for the buffer).  create / delete /
compute_kmeans are the scenarios' recording stand-ins, the same objects the test hands to our mirror.  The run uses device "cpu",
the branch that needs no GPU; the stand-in for usearch answers what the device branch computes, the nearest squared distance.
Only OUTPUTS are stored -- the call sequence, the arguments, the resulting files; nothing of the reference's source is copied."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # tests/
import update_policy_scenarios as S  # noqa: E402

REF = "/root/reference/python/fast_plaid/search/update.py"
CUR = {}   # the running scenario's Recorder


def save_list(path, tensors):
    data = np.empty(len(tensors), dtype=object)
    for i, t in enumerate(tensors):
        data[i] = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    with open(path, "wb") as f:
        np.save(f, data, allow_pickle=True)


def load_list(path):
    return list(np.load(path, allow_pickle=True))


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class BruteIndex:
    def __init__(self, ndim, metric):
        assert metric == "l2sq"

    def add(self, keys, vectors):
        self.c = np.asarray(vectors, np.float32)

    def search(self, batch, k):
        assert k == 1
        return types.SimpleNamespace(distances=S.brute_min_l2sq(self.c, batch).reshape(-1, 1))


def reference_module():
    def placeholder(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def reload_index(index_path, devices, indices, low_memory):
        CUR["rec"].reload()
        return {d: object() for d in devices}

    def load_cpu(index_path):
        CUR["rec"].reload()
        return {}

    pkg = placeholder("fast_plaid")
    pkg.__path__ = []
    pkg.fast_plaid_rust = placeholder("fast_plaid.fast_plaid_rust", update=lambda **kw: CUR["rec"].update(**kw))
    placeholder("usearch").__path__ = []
    placeholder("usearch.index", Index=BruteIndex)
    placeholder("fast_plaid.filtering", update=None)
    sp = placeholder("fast_plaid.search")
    sp.__path__ = []
    placeholder("fast_plaid.search.load", _construct_index_from_tensors=lambda data, device, low_memory: object(),
                _load_index_tensors_cpu=load_cpu, _reload_index=reload_index, save_list_tensors_on_disk=save_list)
    spec = importlib.util.spec_from_file_location("fast_plaid.search.update", REF)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "fast_plaid.search"
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_module()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, sc in S.SCENARIOS.items():
            path, updates = S.prepare(name, tmp, save_list)
            rec = CUR["rec"] = S.Recorder(path, to_np, save_list)
            for docs in updates:
                ref.process_update(
                    index_path=path, devices=["cpu"], torch_path="", low_memory=True, indices_dict={"cpu": object()},
                    documents_embeddings=[torch.from_numpy(d) for d in docs], metadata=None, start_from_scratch=sc["start_from_scratch"],
                    buffer_size=sc["buffer_size"], create_fn=rec.create, delete_fn=rec.delete,
                    compute_kmeans_fn=lambda **kw: torch.from_numpy(rec.compute_kmeans(**kw)),
                    format_embeddings_fn=list, **S.POLICY)
            for k, v in S.flatten(rec.trace, rec.arrays, S.snapshot(path, load_list)).items():
                out[f"{name}/{k}"] = v
            print(name, [c["fn"] for c in rec.trace])
    np.savez_compressed(os.path.join(HERE, "process_update.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
