#!/bin/bash
# bench line, then the SAME command under rocprofv3 --kernel-trace --stats on the SAME box; from that trace: the kernel-stats CSV and the
# three roofline fractions recomputed from kernel timestamps (tools/trace_roofline.py). Summaries go to gpurun_out/<tag>/ (copy to profiles/).
# usage: bash tools/bench_profile.sh <tag> [bench args...]
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TAG=$1; shift
OUT=$GRAFT_REPO_ROOT/gpurun_out/$TAG
mkdir -p "$OUT"
cd "$GRAFT_REPO_ROOT"
echo "== bench $*"
timeout -k 10 500 python3 bench.py --full "$@" > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo "bench failed"; tail -20 "$OUT/bench.err"; exit 1; }
python3 - <<PY
import json
d = json.load(open("$OUT/bench.json")); r = d["roofline"]
print("value", round(d["value"], 2), "ms/step", round(d["ms_per_step"], 1), "| frac(wall)", round(r["frac"], 4), "frac_union", round(r["frac_union"], 4), "frac_launch", round(r["frac_launch"], 4),
      "avg_us", round(r["avg_launch_us"], 1), "| excl TF", round(r.get("exclusive_achieved") or 0, 1))
print("hbm", json.dumps(r.get("hbm_kernels")))
print("cpu", json.dumps(d.get("cpu_baseline")))
PY
cd /tmp && export TMPDIR=/tmp
echo "== rocprofv3 --kernel-trace --stats (same command without the cpu baseline, the extra full-N sweep and the full fine-tune child process)"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats" -- python3 "$ROOT/bench.py" --full "$@" --no-cpu-baseline --no-full-n --no-full-ft > "$OUT/traced_bench.json" 2> "$OUT/stats.err"
echo "rc=$?"
python3 "$GRAFT_REPO_ROOT/tools/trace_roofline.py" "$OUT/stats" "$OUT/traced_bench.json" | tee "$OUT/roofline_from_trace.json"
python3 - <<PY
import csv, glob, shutil
f = glob.glob("$OUT/stats/**/*kernel_stats.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
tot = sum(float(x["TotalDurationNs"]) for x in rows)
for x in rows[:16]:
    print(f'{x["Name"][:70]:70s} calls {x["Calls"]:>7s} avg_us {float(x["AverageNs"])/1e3:9.1f} pct {100*float(x["TotalDurationNs"])/tot:5.1f}')
shutil.copy(f, "$OUT/kernel_stats.csv")
PY
python3 "$GRAFT_REPO_ROOT/tools/trace_exposed.py" "$OUT/stats" "$OUT/traced_bench.json" > "$OUT/exposed.txt" 2>&1; head -30 "$OUT/exposed.txt"
rm -rf "$OUT/stats"   # the raw kernel trace stays on the box: gpurun merges at most 64 MiB back
