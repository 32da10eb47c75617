"""Index maintenance, the native part of the reference:

  update   rust/lib.rs:292-320 -> rust/index/update.rs:30-473   append documents with the EXISTING codec
  delete   rust/lib.rs:322-340 -> rust/index/delete.rs:26-145   drop documents, renumber, rebuild the IVF

Both are file operations on the index directory around one device step (fp_compress for the new documents).

The buffering / re-clustering policy the reference wraps around them in Python (python/fast_plaid/search/update.py) is mirrored
below: `process_update` (:206-452) and `update_centroids` (:65-203), with the collaborators passed in as the reference passes them.
Its outlier step is `centroid_outliers`, the device operator fp_centroid_outliers (the reference's device branch :143-150; its
CPU branch asks the external `usearch` package for the same nearest distance).  FastPlaid.update runs the policy when it is given
a `buffer_size`; without one it appends directly.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from . import _native
from . import create as _create
from . import synth
from .fast_plaid_rust import _device_id, _np, _ptr

_APPEND_TO_LAST_BELOW = 2000      # update.rs:77: a last chunk with fewer documents is extended instead of starting a new one
_PROC_CHUNK = 25_000              # update.rs:28 DEFAULT_PROC_CHUNK_SIZE


def _read_json(p):
    with open(p) as f:
        return json.load(f)


def _write_json(p, obj, pretty=False):
    with open(p, "w") as f:
        json.dump(obj, f, indent=2 if pretty else None)


def _rebuild_ivf(index_path: str, n_chunks: int, n_partitions: int):
    """per-centroid ascending unique document ids over every chunk (create.rs:528-559 / optimize_ivf :55-132;
    update.rs merges the new ids into the old lists, which yields the same lists)."""
    codes, lens = [], []
    for i in range(n_chunks):
        cp = os.path.join(index_path, f"{i}.codes.npy")
        if os.path.exists(cp):
            codes.append(np.load(cp).astype(np.int64))
            lens.extend(_read_json(os.path.join(index_path, f"doclens.{i}.json")))
    codes = np.concatenate(codes) if codes else np.zeros(0, np.int64)
    lens = np.asarray(lens, np.int64)
    ivf, ivf_lengths = synth.build_ivf(codes, lens, n_partitions)
    np.save(os.path.join(index_path, "ivf.npy"), ivf.astype(np.int64))
    np.save(os.path.join(index_path, "ivf_lengths.npy"), ivf_lengths.astype(np.int32))
    return int(codes.shape[0]), int(lens.shape[0])


def update_index(index_path: str, documents_embeddings, device: str = "cuda:0", update_threshold: bool = False) -> None:
    """update.rs:30-473."""
    meta_path = os.path.join(index_path, "metadata.json")
    meta = _read_json(meta_path)
    n_chunks = int(meta["num_chunks"])
    nbits = int(meta["nbits"])
    n_partitions = int(meta["num_partitions"])
    old_total = int(meta.get("num_embeddings", 0))
    old_docs = int(meta.get("num_documents", 0))
    old_avg = float(meta.get("avg_doclen", 0.0))
    compress_only = bool(meta.get("compress_only", False))
    cent = np.load(os.path.join(index_path, "centroids.npy")).astype(np.float16)
    cut = np.load(os.path.join(index_path, "bucket_cutoffs.npy")).astype(np.float16)
    docs = [_np(d, np.float16) for d in documents_embeddings]
    if not docs:
        return
    start, append_to_last, emb_off = n_chunks, False, old_total
    if n_chunks > 0:
        lm_path = os.path.join(index_path, f"{n_chunks - 1}.metadata.json")
        if os.path.exists(lm_path):
            lm = _read_json(lm_path)
            if int(lm.get("num_documents", 1 << 60)) < _APPEND_TO_LAST_BELOW:
                start, append_to_last = n_chunks - 1, True
                emb_off = int(lm["embedding_offset"]) if "embedding_offset" in lm else old_total - int(lm.get("num_embeddings", 0))
    chunk = min(_PROC_CHUNK, 1 + len(docs))
    n_new_chunks = -(-len(docs) // chunk)
    norms = []
    for i in range(n_new_chunks):
        part = docs[i * chunk: (i + 1) * chunk]
        emb = np.concatenate(part)
        codes, packed = _create.compress(cent, cut, emb, nbits, device)
        lens = [int(d.shape[0]) for d in part]
        if update_threshold:
            res = (emb - cent[codes]).astype(np.float32)
            norms.append(np.sqrt((res * res).sum(axis=1, dtype=np.float32)))
        g = start + i
        if i == 0 and append_to_last and os.path.exists(os.path.join(index_path, f"{g}.codes.npy")):
            codes = np.concatenate([np.load(os.path.join(index_path, f"{g}.codes.npy")).astype(np.int64), codes])
            packed = np.concatenate([np.load(os.path.join(index_path, f"{g}.residuals.npy")).astype(np.uint8), packed])
            lens = list(_read_json(os.path.join(index_path, f"doclens.{g}.json"))) + lens
        np.save(os.path.join(index_path, f"{g}.codes.npy"), codes.astype(np.int64))
        np.save(os.path.join(index_path, f"{g}.residuals.npy"), packed.astype(np.uint8))
        _write_json(os.path.join(index_path, f"doclens.{g}.json"), lens)
        _write_json(os.path.join(index_path, f"{g}.metadata.json"),
                    {"num_documents": len(lens), "num_embeddings": int(codes.shape[0]), "embedding_offset": emb_off}, pretty=True)
        emb_off += int(codes.shape[0])
    if update_threshold and norms:   # update.rs:283-310: 0.75 quantile of the new residual norms, count-weighted with the old value
        new = np.sort(np.concatenate(norms))
        new_thr = float(_create._quantile(new, 0.75))
        tp = os.path.join(index_path, "cluster_threshold.npy")
        if os.path.exists(tp):
            old_thr = float(np.load(tp))
            new_thr = (old_thr * old_total + new_thr * new.shape[0]) / (old_total + new.shape[0])
        np.save(tp, np.asarray(new_thr, np.float64))   # update.rs:303: Tensor::from(f64) -> a 0-dim Double
    total_chunks = start + n_new_chunks
    if not compress_only:   # update.rs:325-444 merges the new ids into the old lists; rebuilding from every chunk yields the same lists
        _rebuild_ivf(index_path, total_chunks, n_partitions)
    new_tokens = int(sum(d.shape[0] for d in docs))
    N = old_docs + len(docs)                      # update.rs:447-471 (avg_doclen from the OLD average, as the reference computes it)
    _write_json(meta_path, {"num_chunks": total_chunks, "nbits": nbits, "num_partitions": n_partitions, "num_embeddings": old_total + new_tokens,
                            "num_documents": N, "avg_doclen": ((old_avg * old_docs + new_tokens) / N) if N else 0.0,
                            "compress_only": compress_only}, pretty=True)


def delete_from_index(index_path: str, subset) -> None:
    """delete.rs:26-145: documents are addressed by position; the survivors are renumbered consecutively."""
    meta_path = os.path.join(index_path, "metadata.json")
    meta = _read_json(meta_path)
    n_chunks, nbits, n_partitions = int(meta["num_chunks"]), int(meta["nbits"]), int(meta["num_partitions"])
    drop = set(int(x) for x in subset)
    doc0 = 0
    for i in range(n_chunks):
        dl_path = os.path.join(index_path, f"doclens.{i}.json")
        lens = list(_read_json(dl_path))
        keep_doc = np.array([(doc0 + j) not in drop for j in range(len(lens))], bool)
        if not keep_doc.all():
            keep_tok = np.repeat(keep_doc, np.asarray(lens, np.int64))
            codes = np.load(os.path.join(index_path, f"{i}.codes.npy"))[keep_tok]
            res = np.load(os.path.join(index_path, f"{i}.residuals.npy"))[keep_tok]
            new_lens = [ln for ln, k in zip(lens, keep_doc) if k]
            np.save(os.path.join(index_path, f"{i}.codes.npy"), codes)
            np.save(os.path.join(index_path, f"{i}.residuals.npy"), res)
            _write_json(dl_path, new_lens)
            cm_path = os.path.join(index_path, f"{i}.metadata.json")
            cm = _read_json(cm_path) if os.path.exists(cm_path) else {}
            cm["num_documents"] = len(new_lens)
            cm["num_embeddings"] = int(codes.shape[0])
            _write_json(cm_path, cm, pretty=True)
        doc0 += len(lens)
    # delete.rs:105-143 never looks at compress_only: the lists are rebuilt from the chunks' codes and the metadata is written WITHOUT
    # the key -- deleting from a compress_only index leaves a searchable one.  Followed to the letter (until round 6 this kept the
    # flag and wrote no lists; tests/maintain_fuzz_worker.py compares the directories file by file).
    T, N = _rebuild_ivf(index_path, n_chunks, n_partitions)
    _write_json(meta_path, {"num_chunks": n_chunks, "nbits": nbits, "num_partitions": n_partitions, "num_embeddings": T,
                            "avg_doclen": (T / N) if N else 0.0, "num_documents": N}, pretty=True)


# ---- the update policy (python/fast_plaid/search/update.py) ---------------------------------------------------------------------
def centroid_outliers(centroids, embeddings, threshold: float, device: str = "cuda:0", rows_only: bool = False):
    """update.py:143-150 on the device (fp_centroid_outliers; include/fastplaid.h states the arithmetic): the rows of `embeddings`
    whose squared distance to the nearest centroid exceeds threshold^2.  -> (rows int64 ascending, sqdist float32 [T],
    nearest int64 [T]); rows_only: the two per-token arrays stay on the device and come back as None (what the policy needs)."""
    cent = _np(centroids, np.float16)
    emb = _np(embeddings, np.float16)
    if cent.ndim != 2 or emb.ndim != 2 or cent.shape[1] != emb.shape[1]:
        raise ValueError("centroids and embeddings must be [n, dim] with the same dim")
    T = int(emb.shape[0])
    rows = np.zeros(T, np.int64)
    sqdist = None if rows_only else np.zeros(T, np.float32)
    nearest = None if rows_only else np.zeros(T, np.int64)
    count = np.zeros(1, np.int64)
    _native.check(_native.lib().fp_centroid_outliers(_device_id(device), _ptr(cent), cent.shape[0], cent.shape[1], _ptr(emb), T,
                                         float(np.float32(float(threshold) ** 2)), _ptr(rows), _ptr(count), _ptr(sqdist), _ptr(nearest)))
    return rows[: int(count[0])].copy(), sqdist, nearest


def last_outlier_counts() -> dict:
    """Of this thread's last fp_centroid_outliers call: chunks processed / through the MFMA narrowing / sent on to the exact
    kernel, and the device microseconds of its four phases ({} when that call failed)."""
    import ctypes
    out = (ctypes.c_int64 * 7)()
    if _native.lib().fp_centroid_outliers_last_counts(out, 7) <= 0:
        return {}
    return dict(chunks=out[0], narrowed_chunks=out[1], fallback_chunks=out[2], upload_us=out[3], assign_us=out[4], outlier_us=out[5],
                download_us=out[6])


def save_list_arrays(path: str, arrays) -> None:
    """load.py:430-444 save_list_tensors_on_disk: a 1-D object array of the per-document arrays, pickled."""
    data = np.empty(len(arrays), dtype=object)
    for i, a in enumerate(arrays):
        data[i] = np.asarray(a)
    with open(path, "wb") as f:   # (np.save would append ".npy" to a name without it; the names here carry it)
        np.save(f, data, allow_pickle=True)


def load_list_arrays(path: str) -> list:
    return list(np.load(path, allow_pickle=True))


def update_centroids(index_path: str, new_embeddings, cluster_threshold: float, device: str, kmeans_niters: int,
                     max_points_per_centroid: int, seed: int, compute_kmeans_fn, n_samples_kmeans: int | None = None,
                     use_triton_kmeans: bool | None = None, outliers_fn=None) -> int:
    """update.py:65-203: cluster the embeddings farther than `cluster_threshold` from every centroid and append the new centroids.
    Returns how many were appended (the reference returns nothing)."""
    centroids_path = os.path.join(index_path, "centroids.npy")
    if not os.path.exists(centroids_path):   # :103-105
        return 0
    existing = np.load(centroids_path)       # :107
    if isinstance(new_embeddings, (list, tuple)):   # :110-116
        flat = np.concatenate([np.asarray(e) for e in new_embeddings])
    else:
        flat = np.asarray(new_embeddings)
    if flat.ndim == 3:
        flat = flat[0]
    if outliers_fn is None:
        rows, _, _ = centroid_outliers(existing, flat, cluster_threshold, device, rows_only=True)   # :121-150
    else:
        rows, _, _ = outliers_fn(existing, flat, cluster_threshold, device)
    outliers = flat[np.asarray(rows, np.int64)]                            # :152
    n_out = int(outliers.shape[0])
    if n_out == 0:                                                         # :155-158
        return 0
    k_update = max(1, math.ceil(n_out / max_points_per_centroid) * 4)      # :161-162
    # :164-174.  The reference hands compute_kmeans the [n_out, dim] tensor, whose "documents" are its rows: one-row documents here,
    # which gives the document sample of fast_plaid.py:109-122 over the rows and K = min(k_update, rows)
    new = compute_kmeans_fn(documents_embeddings=outliers.reshape(n_out, 1, outliers.shape[1]), dim=int(outliers.shape[1]), device=device,
                            kmeans_niters=kmeans_niters, max_points_per_centroid=max_points_per_centroid, seed=seed,
                            n_samples_kmeans=n_samples_kmeans, use_triton_kmeans=use_triton_kmeans, num_partitions=k_update)
    new = np.asarray(new).astype(np.float32)                               # :177
    k_new = int(new.shape[0])
    final = np.concatenate([existing, new], axis=0)                        # :179 (an fp16 table becomes fp32: numpy's promotion, as there)
    np.save(centroids_path, final)                                         # :181
    ivf_path = os.path.join(index_path, "ivf_lengths.npy")                 # :183-188 (absent for compress_only)
    if os.path.exists(ivf_path):
        ivf_lengths = np.load(ivf_path)
        np.save(ivf_path, np.concatenate([ivf_lengths, np.zeros(k_new, dtype=ivf_lengths.dtype)]))
    meta_path = os.path.join(index_path, "metadata.json")                  # :190-198
    if os.path.exists(meta_path):
        meta = _read_json(meta_path)
        meta["num_partitions"] = int(final.shape[0])
        with open(meta_path, "w") as f:
            json.dump(meta, f, indent=4)
    return k_new


def process_update(index_path: str, devices, indices_dict, documents_embeddings, metadata, batch_size: int, kmeans_niters: int,
                   max_points_per_centroid: int, n_samples_kmeans: int | None, seed: int, start_from_scratch: int, buffer_size: int,
                   use_triton_kmeans: bool | None, create_fn, delete_fn, compute_kmeans_fn, format_embeddings_fn, update_fn, reload_fn,
                   outliers_fn=None) -> None:
    """update.py:206-452 with its control flow.  update_fn stands where the reference calls fast_plaid_rust.update, reload_fn where
    it calls _reload_index / partial_reload; indices_dict is the live device -> index mapping.  Not mirrored: the metadata.db
    bookkeeping (:301-311; metadata filtering is outside this package)."""
    meta_path = os.path.join(index_path, "metadata.json")
    if not os.path.exists(index_path) or not os.path.exists(meta_path):   # :271-290
        create_fn(documents_embeddings=documents_embeddings, kmeans_niters=kmeans_niters, max_points_per_centroid=max_points_per_centroid,
                  n_samples_kmeans=n_samples_kmeans, batch_size=batch_size, seed=seed, use_triton_kmeans=use_triton_kmeans,
                  metadata=metadata, start_from_scratch=start_from_scratch)
        reload_fn()
        return
    documents_embeddings = list(format_embeddings_fn(documents_embeddings))   # :292
    meta = _read_json(meta_path)                                               # :294-297
    num_documents_in_index = meta.get("num_documents", start_from_scratch + 1)
    compress_only = meta.get("compress_only", False)
    emb_path = os.path.join(index_path, "embeddings.npy")
    if num_documents_in_index <= start_from_scratch and os.path.exists(emb_path):   # :313-349 rebuild from the kept embeddings
        documents_embeddings = load_list_arrays(emb_path) + documents_embeddings
        create_fn(documents_embeddings=documents_embeddings, kmeans_niters=kmeans_niters, max_points_per_centroid=max_points_per_centroid,
                  n_samples_kmeans=n_samples_kmeans, batch_size=batch_size, seed=seed, use_triton_kmeans=use_triton_kmeans,
                  metadata=None, start_from_scratch=start_from_scratch, compress_only=compress_only)
        if len(documents_embeddings) > start_from_scratch and os.path.exists(emb_path):
            os.remove(emb_path)
        reload_fn()
        return
    if devices[0] not in indices_dict or indices_dict[devices[0]] is None:   # :351-363
        reload_fn()
        if indices_dict.get(devices[0]) is None:
            raise RuntimeError("Index not loaded for update.")
    cluster_threshold = float(np.load(os.path.join(index_path, "cluster_threshold.npy")).item())   # :365-366
    buffer_path = os.path.join(index_path, "buffer.npy")
    existing_buffer = load_list_arrays(buffer_path) if os.path.exists(buffer_path) else []         # :368-375
    total_new_docs = len(documents_embeddings) + len(existing_buffer)                              # :377
    if total_new_docs >= buffer_size:   # :379-429 buffer reached: expand the centroids, then insert everything that was buffered
        if len(existing_buffer) > 0:    # the buffered documents are the last ones of the index
            start_del_idx = num_documents_in_index - len(existing_buffer)
            documents_embeddings = existing_buffer + documents_embeddings
            delete_fn(subset=list(range(start_del_idx, num_documents_in_index)), _delete_metadata=False, _delete_buffer=False)
        update_centroids(index_path=index_path, new_embeddings=documents_embeddings, cluster_threshold=cluster_threshold, device=devices[0],
                         kmeans_niters=kmeans_niters, max_points_per_centroid=max_points_per_centroid, n_samples_kmeans=n_samples_kmeans,
                         seed=seed, compute_kmeans_fn=compute_kmeans_fn, use_triton_kmeans=use_triton_kmeans, outliers_fn=outliers_fn)
        reload_fn()
        if os.path.exists(buffer_path):
            os.remove(buffer_path)
        update_fn(index_path=index_path, device=devices[0], embeddings=documents_embeddings, batch_size=batch_size,
                  update_threshold_centroids=True)
        reload_fn()
        return
    # :431-452 buffer not reached: remember the documents and append them with the codec as it is
    save_list_arrays(buffer_path, existing_buffer + documents_embeddings)
    update_fn(index_path=index_path, device=devices[0], embeddings=documents_embeddings, batch_size=batch_size,
              update_threshold_centroids=False)
    reload_fn()


def filter_kept_embeddings(index_path: str, subset) -> None:
    """fast_plaid.py:1075-1143, after the native delete: drop the deleted documents from embeddings.npy and buffer.npy too.  As
    there, num_documents is read AFTER the delete, and `_delete_buffer` is accepted by delete() but never consulted."""
    meta_path = os.path.join(index_path, "metadata.json")
    num_documents = _read_json(meta_path).get("num_documents", 0) if os.path.exists(meta_path) else 0
    buffer_path = os.path.join(index_path, "buffer.npy")
    num_buffer_docs = len(np.load(buffer_path, allow_pickle=True)) if os.path.exists(buffer_path) else 0
    buffer_start_idx = num_documents - num_buffer_docs          # :1090-1091: the buffered documents are the most recent ones
    emb_path = os.path.join(index_path, "embeddings.npy")
    if os.path.exists(emb_path):                                # :1093-1116
        emb = np.load(emb_path, allow_pickle=True)
        gone = {int(i) for i in subset if i < len(emb)}
        if gone:
            rest = [emb[i] for i in range(len(emb)) if i not in gone]
            if rest:
                save_list_arrays(emb_path, rest)
            else:
                os.remove(emb_path)
    if os.path.exists(buffer_path) and num_buffer_docs > 0:     # :1118-1143
        gone = {int(i) - buffer_start_idx for i in subset if buffer_start_idx <= i < num_documents}
        if gone:
            buf = np.load(buffer_path, allow_pickle=True)
            rest = [buf[i] for i in range(num_buffer_docs) if i not in gone]
            if rest:
                save_list_arrays(buffer_path, rest)
            else:
                os.remove(buffer_path)
