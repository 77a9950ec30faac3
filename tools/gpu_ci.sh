#!/bin/bash
# GPU-box check run: per-kernel parity, engine parity, smoke. A step that times out, is killed, aborts (134) or dies of a
# segmentation fault (139) ends the run (no further GPU step on the card after a hang or a crash); ordinary test failures do not.
set -u
mkdir -p gpurun_out
rm -f gpurun_out/kernel_report.txt gpurun_out/engine_report.txt gpurun_out/strict_report.txt
run() {
  local name=$1; shift
  echo "=== $name: $*" | tee -a gpurun_out/ci.log
  timeout -k 10 "$TMO" "$@" > "gpurun_out/$name.log" 2>&1
  local rc=$?
  echo "=== $name rc=$rc" | tee -a gpurun_out/ci.log
  tail -n 25 "gpurun_out/$name.log"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "step $name hung/killed: stopping" | tee -a gpurun_out/ci.log; exit $rc; fi
  if [ $rc -eq 134 ] || [ $rc -eq 139 ]; then echo "step $name aborted/crashed: stopping (its rc line above is in the log)"; exit $rc; fi
  return 0
}
: > gpurun_out/ci.log
TMO=${TMO:-420}
run kernels python -m pytest tests/test_kernels_gpu.py tests/test_kernels_gpt2_gpu.py tests/test_attention_long_gpu.py tests/test_head_norm_gpu.py tests/test_decode_kernels_gpu.py tests/test_sample_kernels_gpu.py tests/test_candidate_kernels_gpu.py tests/test_optim_kernels_gpu.py -q -m gpu -p no:cacheprovider
run engine python -m pytest tests/test_engine_gpu.py tests/test_stacked_gpu.py tests/test_full_finetune_gpu.py tests/test_ddp_gpu.py tests/test_io_gpu.py tests/test_edge_cases_gpu.py tests/test_diagnostic_gpu.py tests/test_torch_coexist_gpu.py tests/test_agreement_gpu.py tests/test_zero_gpu.py tests/test_long_sequences_gpu.py tests/test_generate_gpu.py tests/test_tensor_names_gpu.py tests/test_heldout_gpu.py tests/test_create_gpu.py -q -m gpu -p no:cacheprovider
run sample python -m pytest tests/test_sample_gpu.py -q -m gpu -p no:cacheprovider
run candidates python -m pytest tests/test_candidates_gpu.py -q -m gpu -p no:cacheprovider
run qwen3 python -m pytest tests/test_qwen3_gpu.py -q -m gpu -p no:cacheprovider
run attribution python -m pytest tests/test_attribution_gpu.py -q -m gpu -p no:cacheprovider
run ig python -m pytest tests/test_ig_gpu.py -q -m gpu -p no:cacheprovider
run strict python -m pytest tests/test_strict_gpu.py -q -m gpu -p no:cacheprovider
run smoke python -c "import __graft_entry__ as g; g.smoke()"
run fullsize python -m pytest tests/test_fullsize_gpu.py -q -m gpu -p no:cacheprovider
for extra in "$@"; do run "$(echo "$extra" | tr -c 'a-zA-Z0-9' '_' | cut -c1-40)" bash -c "$extra"; done
exit 0
