#!/bin/bash
# interleaved A/B rounds of environment settings on the default bench (whole sweep, short): bash tools/ab.sh <tag> <rounds> "VAR=a" "VAR=b [VAR2=c]" ... [-- bench args]
# every arm runs in its own process; rounds are interleaved (arm 1, arm 2, ..., arm 1, ...) so box drift hits all arms alike
# an arm may carry its own bench arguments after " :: " ("TST_X=1 :: --stack 5 --tile-policy 3"); use X=0 as a no-op environment
cd $GRAFT_REPO_ROOT
TAG=$1; ROUNDS=$2; shift 2
ARMS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do ARMS+=("$1"); shift; done
[ "${1:-}" == "--" ] && shift
mkdir -p gpurun_out/$TAG
: > gpurun_out/$TAG/summary.txt
for round in $(seq 1 $ROUNDS); do
  i=0
  for arm in "${ARMS[@]}"; do
    i=$((i+1))
    f=gpurun_out/$TAG/arm$i.r$round
    aenv="${arm%% :: *}"; aargs=""; [ "$aenv" != "$arm" ] && aargs="${arm#* :: }"
    env $aenv timeout -k 10 300 python3 bench.py --steps 10 --warmup 2 --full --no-cpu-baseline --no-full-n --no-full-ft "$@" $aargs > $f.json 2> $f.err || { echo "arm '$arm' failed"; tail -5 $f.err; exit 1; }
    python3 - <<PY | tee -a gpurun_out/$TAG/summary.txt
import json
d = json.load(open("$f.json")); r = d["roofline"]
print("round $round [$arm]: %.2f QA/s  frac(wall) %.4f  union %.4f  launch %.4f  pp avg %.1f us  contraction launches/step %.0f" % (d["value"], r["frac"], r["frac_union"], r["frac_launch"], r["avg_launch_us"], r["all_contraction_launches"] / d["steps"]))
PY
  done
done
