#!/bin/bash
# S4 refine, k_approx fed from the packed code lines (FP_TEST=ap_lines, fp_kernels.hip k_approx_lines): the measurements behind
# profiles/r13_approx_lines.txt.  PARENT = a library built from the parent commit (default tools/libs/libfastplaid_parent.so).
#   approx_lines_ab.sh prof     rocprofv3 kernel summary of the plain bench command: this tree, then the parent's library
#   approx_lines_ab.sh step     ten bench runs alternating ap_lines=0 / default on this tree's library, five of the parent's
#                               library, --dump-outputs of both forms compared byte for byte
#   approx_lines_ab.sh small    one A/B pair each at --batch 1 and --batch 8
# Every GPU step runs under its own time limit; the script stops at the first step that fails.
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R" || exit 1
OUT="${OUT:-$R/bench_out/approx_lines}"   # (bench_out/ is ignored by git)
PARENT="${PARENT:-$R/tools/libs/libfastplaid_parent.so}"
mkdir -p "$OUT"

line() {   # one bench run -> "<tag> ms_per_step p50"
  local tag="$1"; shift
  timeout -k 10 300 python bench.py --gpus 1 --steps 60 --warmup 10 "$@" 2> "$OUT/last.err" | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$tag', round(d['ms_per_step'], 4), 'p50', round(d.get('p50_ms', 0), 4))"
}

prof() {   # kernel summary of the plain bench command -> the k_approx / k_l0_scan lines
  local tag="$1"
  rm -rf "$OUT/prof_$tag"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$tag" -o run -- python "$R/bench.py" --gpus 1 --steps 20 --warmup 5 > "$OUT/prof_$tag.log" 2>&1 || return 1
  python - "$OUT/prof_$tag" "$tag" <<'PY'
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/run_kernel_stats.csv", recursive=True)[0]
tot = 0.0
rows = list(csv.DictReader(open(f)))
for r in rows:
    tot += float(r["TotalDurationNs"])
for r in rows:
    if "k_approx" in r["Name"] or "k_l0_scan" in r["Name"]:
        print(sys.argv[2], r["Name"].split("(")[0].replace("void ", ""), "calls", r["Calls"], "avg_us %.1f" % (float(r["AverageNs"]) / 1e3),
              "min_us %.1f" % (float(r["MinNs"]) / 1e3), "max_us %.1f" % (float(r["MaxNs"]) / 1e3), "share %.2f %%" % (100 * float(r["TotalDurationNs"]) / tot))
PY
  rm -rf "$OUT/prof_$tag"   # (the traces are large; the summary lines above are the record)
}

case "$1" in
  prof)
    prof tree && FP_LIB_PATH="$PARENT" prof parent ;;
  step)
    for i in 1 2 3 4 5; do
      FP_TEST=ap_lines=0 line "ap_lines=0" --dump-outputs "$OUT/dump0" || exit 1
      line "ap_lines=1" --dump-outputs "$OUT/dump1" || exit 1
    done
    for i in 1 2 3 4 5; do
      FP_LIB_PATH="$PARENT" line "parent" --dump-outputs "$OUT/dumpp" || exit 1
    done
    for f in pids scores counts; do
      cmp "$OUT/dump0/$f.npy" "$OUT/dump1/$f.npy" && cmp "$OUT/dumpp/$f.npy" "$OUT/dump1/$f.npy" && echo "dump $f: byte-identical (ap_lines=0, ap_lines=1, parent)" || exit 1
    done ;;
  small)
    for b in 1 8; do
      FP_TEST=ap_lines=0 line "batch=$b ap_lines=0" --batch $b || exit 1
      line "batch=$b ap_lines=1" --batch $b || exit 1
    done ;;
  *) echo "usage: $0 prof|step|small"; exit 2 ;;
esac
