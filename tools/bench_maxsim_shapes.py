#!/usr/bin/env python3
"""The exact stage (S6 + S7) on the shapes of the K-sliced MFMA kernel, against the generic exact-chain kernel it replaced.

For every (dim, nbits) in SHAPES: a synthetic index (--docs documents x 64 tokens), batches of 16 queries x 32 tokens,
n_full_scores 4096 (1024 exact-scored documents per query).  Two figures per shape and kernel:
  stage_ms   HIP-event time of "S6+S7 maxsim" (+ "S7 order repair" reported next to it) from fp_last_search_timings, graph replay off;
  call_ms    host clock around whole fp_search calls (they end in the download of the results), graph replay on.
Each kernel runs in a child process of its own (FP_TEST is read once per process): the new path as is, the parent's kernel under
FP_TEST=ms_sliced=0.  The children alternate, --repeats times each, in one session; a difference counts when the slower repeat of
one side is faster than the faster repeat of the other.  Bytes per step (DESIGN section 4's accounting): centroid row + residual
row + 4 B code per exact-scored token.  The report goes to --out (and stdout)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(40, 4), (160, 4), (320, 4), (512, 4), (1024, 4), (64, 8), (256, 8)]
DOC_LEN, BATCH, QLEN, N_FULL, TOP_K, N_PROBE = 64, 16, 32, 4096, 100, 8


def child(a):
    import fast_plaid_amd as fp
    R = fp.fast_plaid_rust
    for dim, nbits in SHAPES:
        spec = fp.synth.SynthSpec(n_docs=a.docs, doc_len=DOC_LEN, n_centroids=fp.synth.default_num_centroids(a.docs * DOC_LEN), dim=dim,
                                  nbits=nbits, seed=42)
        cent, bw = fp.synth.centroids(spec), fp.synth.bucket_weights(spec)
        index = R.construct_synthetic_index(spec, "cuda:0", centroids=cent, bucket_weights=bw)
        params = R.SearchParameters(2000, N_FULL, TOP_K, N_PROBE)
        batches = [fp.synth.make_queries(spec, cent, BATCH, QLEN, seed=1000 + i) for i in range(a.warmup + a.steps)]
        for i in range(a.warmup):
            R.search_arrays(index, batches[i], params)
        t0 = time.perf_counter()
        for i in range(a.steps):
            R.search_arrays(index, batches[a.warmup + i], params)   # returns host arrays: the call ends in a synchronise
        call_ms = (time.perf_counter() - t0) / a.steps * 1e3
        was = R.set_graph_replay(False)
        R.search_arrays(index, batches[0], params)
        stage = repair = 0.0
        cand = 0
        for i in range(a.steps):
            R.search_arrays(index, batches[a.warmup + i], params)
            t = R.last_search_timings()
            stage += t["S6+S7 maxsim"]
            repair += t.get("S7 order repair", 0.0)
            cand += R.last_search_counts()["candidates"]
        R.set_graph_replay(was)
        print(json.dumps(dict(dim=dim, nbits=nbits, call_ms=call_ms, stage_ms=stage / a.steps, repair_ms=repair / a.steps,
                              candidates_per_query=cand / a.steps / BATCH)), flush=True)
        del index


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_maxsim_sliced.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"sliced": {}, "generic": {}}
    for rep in range(a.repeats):
        for mode in ("sliced", "generic"):
            env = dict(os.environ)
            if mode == "generic":
                env["FP_TEST"] = ",".join(x for x in (env.get("FP_TEST", ""), "ms_sliced=0") if x)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--docs", str(a.docs), "--steps", str(a.steps), "--warmup",
                                str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{mode} child failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    res[mode].setdefault((d["dim"], d["nbits"]), []).append(d)
    R = N_FULL // 4
    out = [f"S6+S7 on the shapes of k_maxsim_sl against k_maxsim_generic (FP_TEST=ms_sliced=0): {a.docs} documents x {DOC_LEN} tokens, batch "
           f"{BATCH} x {QLEN}, n_full_scores {N_FULL}, top_k {TOP_K}; {a.repeats} alternating child processes per kernel, {a.steps} steps each.",
           "ms are medians over the repeats [min .. max]; bytes = (2 dim + dim nbits / 8 + 4) B x exact-scored tokens per step.", ""]
    ok = True
    for shp in SHAPES:
        s, g = res["sliced"][shp], res["generic"][shp]
        med = lambda rows, k: statistics.median(x[k] for x in rows)
        rng = lambda rows, k: f"[{min(x[k] for x in rows):.3f} .. {max(x[k] for x in rows):.3f}]"
        nbytes = (2 * shp[0] + shp[0] * shp[1] // 8 + 4) * BATCH * min(R, int(s[0]["candidates_per_query"])) * DOC_LEN
        faster = max(x["stage_ms"] for x in s) < min(x["stage_ms"] for x in g)
        ok = ok and faster
        out.append(f"dim {shp[0]:4d} nbits {shp[1]}: stage sliced {med(s, 'stage_ms'):.3f} {rng(s, 'stage_ms')} ms, generic {med(g, 'stage_ms'):.3f} "
                   f"{rng(g, 'stage_ms')} ms, ratio {med(g, 'stage_ms') / med(s, 'stage_ms'):.1f}x{'' if faster else '  (NOT beyond the spread)'}; "
                   f"{nbytes / med(s, 'stage_ms') / 1e9:.2f} TB/s; repair sliced {med(s, 'repair_ms'):.3f} ms, generic {med(g, 'repair_ms'):.3f} ms; "
                   f"call sliced {med(s, 'call_ms'):.3f} {rng(s, 'call_ms')} ms, generic {med(g, 'call_ms'):.3f} {rng(g, 'call_ms')} ms, "
                   f"ratio {med(g, 'call_ms') / med(s, 'call_ms'):.2f}x; candidates per query {s[0]['candidates_per_query']:.0f}")
    out.append("")
    out.append("acceptance (sliced stage faster than generic at every shape by more than the spread): " + ("met" if ok else "NOT met"))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
