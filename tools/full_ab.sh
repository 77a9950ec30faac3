#!/bin/bash
# full fine-tune bench (BASELINE config 3 on one GPU), interleaved arms of environment settings: bash tools/full_ab.sh <tag> <rounds> <steps> "VAR=a" "VAR=b VAR2=c" ...
cd $GRAFT_REPO_ROOT
TAG=$1; ROUNDS=$2; STEPS=$3; shift 3
mkdir -p gpurun_out/$TAG
: > gpurun_out/$TAG/summary.txt
for round in $(seq 1 $ROUNDS); do
  i=0
  for arm in "$@"; do
    i=$((i+1))
    f=gpurun_out/$TAG/arm$i.r$round
    env $arm timeout -k 10 400 python3 bench.py --train-mode full --k 8 --steps $STEPS --warmup 0 --full --no-cpu-baseline > $f.json 2> $f.err || { echo "arm '$arm' failed"; tail -5 $f.err; exit 1; }
    python3 - <<PY | tee -a gpurun_out/$TAG/summary.txt
import json
d = json.load(open("$f.json")); r = d["roofline"]; a = r.get("hbm_kernels", {}).get("adamw", {})
print("round $round [$arm]: %.2f QA/s  wall %.1f s  frac(wall) %.4f  union %.4f  pp avg %.1f us  adamw alone %.1f ms (%.0f GB/s)" % (d["value"], r["wall_ms"] / 1e3, r["frac"], r["frac_union"], r["avg_launch_us"], a.get("avg_launch_us", 0) / 1e3, a.get("achieved_GBps", 0)))
PY
  done
done
