"""GPU worker for tests/test_index_lifetime_gpu.py: the life of an fp_index (fp_index.cpp) through the C ABI, in one process:
    index_lifetime_worker.py OUT.json

refusals  fp_index_create refuses, after device work has begun, a document code equal to C, an IVF entry equal to N, a negative
          document length and a negative IVF length: FP_EINVAL, the message, *out null.  Then the same process builds a valid
          index, and fp_search of 2 queries on it equals fp_search_trace bit for bit.
layouts   one index per branch of the layout code (CONFIGS): fp_index_export and fp_index_read_doc of every document return the
          input arrays (a document without tokens included); IVF lists handed over shuffled and with repeats come back from
          fp_index_read_ivf ascending and unique, and export's ivf_lengths agree; 20 create / destroy rounds of the same index.
figures   fp_index_device_bytes and fp_index_num_code_lines of every index, written out for the test's table.

Indexes hold ~300 documents of 0 .. 40 tokens, drawn with a fixed seed.  Each group's verdict ("ok" or the failed assertion) goes
into OUT.json; the exit status is 0 when all are ok."""
import ctypes as C
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

FP_OK, FP_EINVAL = 0, -1
N_DOCS, MAX_LEN, ROUNDS = 300, 40, 20
# name -> (dim, nbits, n_centroids): the branches of finish_layout
CONFIGS = {
    "native128": (128, 4, 256),            # residual rows in the MaxSim kernel's unit order, per-token reciprocals
    "padded96": (96, 4, 256),              # S1 reads a zero-padded view of the centroid table
    "sliced40": (40, 2, 256),              # padded view, K-sliced MaxSim
    "lines8": (8, 8, (1 << 17) + 256),     # two centroid ranges: packed code lines (fp_index_num_code_lines > 0)
    "empty": (64, 2, 64),                  # no document at all
}
SYNTH = dict(n_docs=N_DOCS, doc_len=MAX_LEN, n_centroids=256, variable_len=True, seed=11)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def arrays(name):
    """host arrays of a configuration: `ivf` / `ivf_lengths` are the ascending unique lists, `ivf_in` / `ivf_lengths_in` the same
    lists shuffled and with repeats (what the index is built from)"""
    import fast_plaid_amd as fp
    dim, nbits, Cn = CONFIGS[name]
    rng = np.random.default_rng(1900 + dim + nbits)
    n = 0 if name == "empty" else N_DOCS
    lens = rng.integers(0, MAX_LEN + 1, size=n).astype(np.int64)
    if n:
        lens[[5, n - 1]] = 0          # documents without tokens, the last one among them
        lens[17] = MAX_LEN
    T = int(lens.sum())
    codes = rng.integers(0, Cn, size=T).astype(np.int64)
    res = rng.integers(0, 256, size=(T, dim * nbits // 8), dtype=np.uint8)
    cent = rng.standard_normal((Cn, dim), dtype=np.float32)
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
    bw = np.linspace(-0.1, 0.1, 1 << nbits).astype(np.float16)
    ivf, ivfl = fp.synth.build_ivf(codes, lens, Cn) if n else (np.zeros(0, np.int64), np.zeros(Cn, np.int32))
    off = np.concatenate([[0], np.cumsum(ivfl.astype(np.int64))])
    messy = []
    for c in np.flatnonzero(ivfl):
        lst = ivf[off[c]: off[c + 1]]
        messy.append(rng.permutation(np.concatenate([lst, lst[: int(rng.integers(0, 3))]])))
    ivfl_in = ivfl.copy()
    ivfl_in[np.flatnonzero(ivfl)] = [len(m) for m in messy]
    ivf_in = np.concatenate(messy).astype(np.int64) if messy else np.zeros(1, np.int64)   # (never a null pointer: null = compress_only)
    return dict(nbits=nbits, dim=dim, centroids=cent, bucket_weights=bw, doc_codes=codes, doc_residuals=res, doc_lengths=lens,
                ivf=ivf, ivf_lengths=ivfl, ivf_in=ivf_in, ivf_lengths_in=ivfl_in)


def create(L, a, **repl):
    """fp_index_create from the arrays (`repl` replaces some) -> (return code, handle or None)"""
    from fast_plaid_amd import _native as N
    a = dict(a, **repl)
    keep = [np.ascontiguousarray(a[k]) for k in ("centroids", "bucket_weights", "ivf_in", "ivf_lengths_in", "doc_codes", "doc_residuals",
                                                 "doc_lengths")]
    cent, bw, ivf, ivfl, codes, res, lens = keep
    # (an index without documents hands over valid pointers too: one spare entry behind each empty array)
    spare = np.zeros(8, np.int64)
    d = N.FpIndexDesc(a["nbits"], a["dim"], cent.shape[0], _ptr(cent), None, None, _ptr(bw), _ptr(ivf), _ptr(ivfl), ivfl.shape[0],
                      _ptr(codes if codes.size else spare), _ptr(res if res.size else spare), _ptr(lens if lens.size else spare),
                      lens.shape[0], 0)
    h = C.c_void_p(0xDEAD0)
    rc = L.fp_index_create(C.byref(d), 0, C.byref(h))
    return rc, h.value


def figures(L, h):
    return [int(L.fp_index_device_bytes(h)), int(L.fp_index_num_code_lines(h))]


def check_read_back(L, h, a, cells):
    """export, read_doc of every document and read_ivf of `cells` against the arrays"""
    lens, codes, res = a["doc_lengths"], a["doc_codes"], a["doc_residuals"]
    n, T, Cn, pr = lens.shape[0], int(lens.sum()), a["ivf_lengths"].shape[0], res.shape[1]
    assert (L.fp_index_num_docs(h), L.fp_index_num_tokens(h), L.fp_index_num_centroids(h)) == (n, T, Cn)
    assert (L.fp_index_dim(h), L.fp_index_nbits(h)) == (a["dim"], a["nbits"])
    tot = int(L.fp_index_ivf_total(h))
    assert tot == a["ivf"].shape[0], (tot, a["ivf"].shape[0])
    x_codes, x_res, x_lens = np.full(T + 1, -7, np.int64), np.full((T + 1, pr), 0xA5, np.uint8), np.full(n + 1, -7, np.int64)
    x_ivf, x_ivfl = np.full(tot + 1, -7, np.int64), np.full(Cn + 1, -7, np.int32)
    assert L.fp_index_export(h, _ptr(x_codes), _ptr(x_res), _ptr(x_lens), _ptr(x_ivf), _ptr(x_ivfl)) == FP_OK
    assert np.array_equal(x_lens[:n], lens) and x_lens[n] == -7
    assert np.array_equal(x_codes[:T], codes) and x_codes[T] == -7
    assert np.array_equal(x_res[:T], res) and np.all(x_res[T] == 0xA5)
    assert np.array_equal(x_ivf[:tot], a["ivf"]) and x_ivf[tot] == -7
    assert np.array_equal(x_ivfl[:Cn], a["ivf_lengths"]) and x_ivfl[Cn] == -7
    off = np.concatenate([[0], np.cumsum(lens)])
    d_codes, d_res = np.zeros(MAX_LEN, np.int64), np.zeros((MAX_LEN, pr), np.uint8)
    for d in range(n):
        got = L.fp_index_read_doc(h, d, _ptr(d_codes), _ptr(d_res), MAX_LEN)
        assert got == lens[d], (d, got)
        assert np.array_equal(d_codes[:got], codes[off[d]: off[d + 1]]), d
        assert np.array_equal(d_res[:got], res[off[d]: off[d + 1]]), d
    ioff = np.concatenate([[0], np.cumsum(a["ivf_lengths"].astype(np.int64))])
    pids = np.zeros(max(n, 1), np.int64)
    for c in cells:
        got = L.fp_index_read_ivf(h, int(c), _ptr(pids), pids.shape[0])
        want = a["ivf"][ioff[c]: ioff[c + 1]]
        assert got == want.shape[0], (c, got)
        assert np.array_equal(pids[:got], want) and np.all(np.diff(want) > 0), c


def group_refusals(L, out):
    from fast_plaid_amd import _native as N
    import fast_plaid_amd as fp
    R = fp.fast_plaid_rust
    a = arrays("native128")
    n, Cn = a["doc_lengths"].shape[0], a["centroids"].shape[0]

    def spoilt(key, at, value):
        v = a[key].copy()
        v[at] = value
        return {key: v}

    cases = [
        (spoilt("doc_codes", 123, Cn), f"doc_codes (centroid ids): 1 entries outside [0, {Cn})"),
        (spoilt("ivf_in", 77, n), f"ivf (document ids): 1 entries outside [0, {n})"),
        (spoilt("doc_lengths", 200, -1), "negative document length"),
        (spoilt("ivf_lengths_in", int(np.flatnonzero(a["ivf_lengths_in"])[3]), -2), "negative ivf length"),
    ]
    for repl, message in cases:
        rc, h = create(L, a, **repl)
        assert rc == FP_EINVAL, (message, rc, N.last_error())
        assert N.last_error() == message, (message, N.last_error())
        assert h is None, message
    # the same process goes on: a valid index, and fp_search == fp_search_trace bit for bit
    idx = R.construct_index(a["nbits"], a["centroids"], None, None, a["bucket_weights"], a["ivf_in"], a["ivf_lengths_in"], a["doc_codes"],
                            a["doc_residuals"], a["doc_lengths"], "cuda:0")
    rng = np.random.default_rng(5)
    v = a["centroids"][rng.integers(0, Cn, size=(2, 16))].astype(np.float32) + 0.3 * rng.standard_normal((2, 16, 128), dtype=np.float32) / np.sqrt(128)
    q = (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float16)
    params = R.SearchParameters(2000, 64, 10, 4)
    pids, scores, counts = R.search_arrays(idx, q, params)
    for b in range(2):
        t = R.search_trace(idx, q[b], params)
        assert counts[b] == len(t["pids"]) > 0, (b, counts[b])
        assert np.array_equal(pids[b, : counts[b]], t["pids"]), b
        assert np.array_equal(scores[b, : counts[b]].view(np.uint32), t["scores"].view(np.uint32)), b
    idx.close()
    out["searched"] = int(counts.sum())


def group_layouts(L, out):
    from fast_plaid_amd import _native as N
    import fast_plaid_amd as fp
    fig = {}
    for name in CONFIGS:
        a = arrays(name)
        rc, h = create(L, a)
        assert rc == FP_OK and h, (name, N.last_error())
        fig[name] = figures(L, h)
        Cn = a["ivf_lengths"].shape[0]
        # (the table of 2^17 + 256 lists: the ends, the range boundary and a stride of the lists in between)
        cells = range(Cn) if Cn <= 1024 else sorted({0, 1, (1 << 17) - 1, 1 << 17, Cn - 1, *range(3, Cn, 1009)})
        check_read_back(L, h, a, cells)
        L.fp_index_destroy(h)
        for r in range(ROUNDS):
            rc, h = create(L, a)
            assert rc == FP_OK and h, (name, r, N.last_error())
            assert figures(L, h) == fig[name], (name, r)
            L.fp_index_destroy(h)
    assert fig["lines8"][1] > 0, fig
    # the synthetic corpus: the device generates what synth.host_index_arrays computes on the host, its IVF lists included
    spec = fp.synth.SynthSpec(**SYNTH)
    a = fp.synth.host_index_arrays(spec)
    a["dim"] = spec.dim
    for r in range(ROUNDS + 1):
        idx = fp.fast_plaid_rust.construct_synthetic_index(spec, "cuda:0")
        if r == 0:
            fig["synthetic"] = figures(L, idx._h)
            check_read_back(L, idx._h, a, range(spec.n_centroids))
        assert figures(L, idx._h) == fig["synthetic"], r
        idx.close()
    out["figures"] = fig


def main():
    from fast_plaid_amd import _native as N
    L = N.lib()
    out = {}
    for name, group in (("refusals", group_refusals), ("layouts", group_layouts)):
        try:
            group(L, out)
            out[name] = "ok"
        except Exception:   # noqa: BLE001 -- the verdict travels to the test; nothing more runs on the device after a failure
            out[name] = traceback.format_exc()
            break
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
    ok = out.get("refusals") == "ok" and out.get("layouts") == "ok"
    print("INDEX_LIFETIME_OK" if ok else "INDEX_LIFETIME_FAILED", json.dumps(out.get("figures")))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
