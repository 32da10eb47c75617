#!/usr/bin/env python3
"""fp_token_scores and fp_reconstruct_embeddings: the tile / unit kernels (fp_token_scores.hip, the default path) against the
kernels they replaced (FP_TEST=tok_tiled=0).

For every (dim, nbits, q_len) in SHAPES: a synthetic index of --docs documents x 128 tokens, one search of 16 queries for the top
1000 documents each, then
  tok_ms   host clock around the COMPUTING fp_token_scores call for all hits (upload of queries and hit arrays, kernel, download
           of the matrices; the sizing call is made once before and is not timed),
  rec_ms   host clock around fp_reconstruct_embeddings for the documents of the first query's hits,
one warm-up call and --steps timed calls each.  Each path runs in a child process of its own (FP_TEST is read once per process);
the children alternate (new, old, new, old, ...), --repeats pairs in one session.  The old path is the baseline; shapes it cannot
serve (LDS: (q_len + 1) * dim * 4 B above 150 KB; dim above 512 for the reconstruction) are run on the new path alone.  The
verdict per shared shape: the new median does not lie above the old median by more than the old series' own spread (max - min).
sha1 = digest of the matrices / rows of the last call: both paths must print the same one.  The report goes to --out and stdout."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 4, 32), (768, 4, 32), (1024, 4, 64)]
DOC_LEN, BATCH, TOP_K, N_FULL, N_PROBE = 128, 16, 1000, 4096, 32


def child(a):
    import numpy as np
    import fast_plaid_amd as fp
    from fast_plaid_amd import _native as N
    R = fp.fast_plaid_rust
    old = "tok_tiled=0" in os.environ.get("FP_TEST", "")
    for dim, nbits, Q in SHAPES:
        tok_ok = not old or (Q + 1) * dim * 4 <= 150 * 1024
        rec_ok = not old or dim <= 512
        if not (tok_ok or rec_ok):
            continue
        spec = fp.synth.SynthSpec(n_docs=a.docs, doc_len=DOC_LEN, n_centroids=fp.synth.default_num_centroids(a.docs * DOC_LEN), dim=dim,
                                  nbits=nbits, seed=42)
        cent, bw = fp.synth.centroids(spec), fp.synth.bucket_weights(spec)
        index = R.construct_synthetic_index(spec, "cuda:0", centroids=cent, bucket_weights=bw)
        q = np.ascontiguousarray(fp.synth.make_queries(spec, cent, BATCH, Q, seed=1000), np.float16)
        pids, _, counts = R.search_arrays(index, q, R.SearchParameters(2000, N_FULL, TOP_K, N_PROBE))
        pids, counts = np.ascontiguousarray(pids, np.int64), np.ascontiguousarray(counts, np.int32)
        hits = int(counts.sum())
        row = dict(dim=dim, nbits=nbits, q_len=Q, hits=hits, out_mb=0.0, tok_ms=[], rec_ms=[], tok_sha1="", rec_sha1="")
        if tok_ok:
            offs = np.zeros(hits + 1, np.int64)
            call = lambda out, cap: N.check(N.lib().fp_token_scores(index._h, R._ptr(q), BATCH, Q, dim, R._ptr(pids), R._ptr(counts),
                                                                    pids.shape[1], R._ptr(offs), out, cap))
            call(None, 0)   # sizing
            out = np.zeros(int(offs[-1]), np.float16)
            row["out_mb"] = out.nbytes / 1e6
            for i in range(1 + a.steps):
                t0 = time.perf_counter()
                call(R._ptr(out), out.shape[0])   # returns after the download: a synchronise
                if i:
                    row["tok_ms"].append((time.perf_counter() - t0) * 1e3)
            row["tok_sha1"] = hashlib.sha1(out.tobytes()).hexdigest()[:12]
            del out
        if rec_ok:
            docs = np.ascontiguousarray(pids[0, : counts[0]], np.int64)
            lens = np.zeros(max(len(docs), 1), np.int64)
            rows = np.zeros((len(docs) * DOC_LEN, dim), np.float32)
            for i in range(1 + a.steps):
                t0 = time.perf_counter()
                N.check(N.lib().fp_reconstruct_embeddings(index._h, R._ptr(docs), len(docs), R._ptr(rows), rows.shape[0], R._ptr(lens)))
                if i:
                    row["rec_ms"].append((time.perf_counter() - t0) * 1e3)
            row["rec_sha1"] = hashlib.sha1(rows.tobytes()).hexdigest()[:12]
            del rows
        print(json.dumps(row), flush=True)
        del index


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=8000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_token_scores.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"new": {}, "old": {}}
    for rep in range(a.repeats):
        for mode in ("new", "old"):
            env = dict(os.environ)
            if mode == "old":
                env["FP_TEST"] = ",".join(x for x in (env.get("FP_TEST", ""), "tok_tiled=0") if x)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--docs", str(a.docs), "--steps", str(a.steps)], env=env,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{mode} child failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    res[mode].setdefault((d["dim"], d["nbits"], d["q_len"]), []).append(d)
    out = [f"fp_token_scores / fp_reconstruct_embeddings, new (default) against old (FP_TEST=tok_tiled=0): {a.docs} documents x {DOC_LEN} tokens, "
           f"{BATCH} queries x top {TOP_K}; {a.repeats} alternating child processes per path, {a.steps} timed calls each after one warm-up.",
           "Every timed call, ms, one bracket per process in run order; med = median of the per-process medians, spread = their max - min.", ""]
    ok = True
    for shp in SHAPES:
        n = res["new"].get(shp, [])
        o = res["old"].get(shp, [])
        out.append(f"dim {shp[0]} nbits {shp[1]} q_len {shp[2]}: {n[0]['hits']} hits, matrices {n[0]['out_mb']:.1f} MB")
        for key, name in (("tok_ms", "token scores "), ("rec_ms", "reconstruction")):
            ser = {m: [statistics.median(x[key]) for x in rows if x[key]] for m, rows in (("new", n), ("old", o))}
            sha = {m: sorted({x[key[:3] + "_sha1"] for x in rows if x[key]}) for m, rows in (("new", n), ("old", o))}
            for m, rows in (("new", n), ("old", o)):
                s = ser[m]
                calls = " ".join("[" + " ".join(f"{v:.2f}" for v in x[key]) + "]" for x in rows if x[key])
                out.append(f"  {name} {m}: " + ("not served" if not s else f"{calls}   med {statistics.median(s):.2f}  spread {max(s) - min(s):.2f}  "
                                                                              f"sha1 {' '.join(sha[m])}"))
            if ser["new"] and ser["old"]:
                mn, mo, sp = statistics.median(ser["new"]), statistics.median(ser["old"]), max(ser["old"]) - min(ser["old"])
                good = mn <= mo + sp and sha["new"] == sha["old"]
                ok = ok and good
                out.append(f"  {name} verdict: new {mn:.2f} ms against old {mo:.2f} ms (+ spread {sp:.2f}), ratio {mo / mn:.2f}x, outputs "
                           f"{'equal' if sha['new'] == sha['old'] else 'DIFFER'}: {'met' if good else 'NOT met'}")
        out.append("")
    out.append("acceptance (new median not above old median + old spread at every shared shape, same outputs): " + ("met" if ok else "NOT met"))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
