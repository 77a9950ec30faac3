#!/usr/bin/env python3
"""bench.py -- QA-pairs/sec of the k-fold TsT-LLM hot path on N MI355X (BASELINE.json metric).

Metric as SURVEY.md §8(d) defines it:  QA/s = N / wall(sweep),  sweep = all k folds x (E epochs of fine-tuning on N(k-1)/k + held-out
scoring of N/k), also reported as QA-passes/s = N((k-1)E + 1) / wall.

Workload (N=1 default = BASELINE.json configs[1]): k=5 TsT on VSI-Bench-shaped synthetic text-only QA, Llama-3-8B shape (random-init
bf16 base, frozen) + LoRA r=16 on all seven linears, micro-batch 16, AdamW + clip 1.0, linear LR decay, E=1.

DEFAULT MODE (--mode sweep): one WHOLE k-fold sweep, run by the product's own fold loop (tst.diagnose.diagnose: per-fold adapter
reset, one shuffled epoch with its ragged last micro-batch, then the held-out scoring tail, then the gather of s(x)), on a benchmark
set of N = 16 * k * steps QA pairs. A STEP is one "fold quantum" of that sweep for every fold: 4 optimizer micro-steps (64 training
passes) + 1 scoring micro-batch (16 QA) per fold -- in a k=5, E=1 sweep every QA pair is trained on 4 times and scored once, so `steps`
quanta per fold ARE the sweep over N = 80 * steps pairs. --steps 64 (the default) is the full N = 5120 set of BASELINE.md; the driver's
--steps 20 is the same sweep over N = 1600.  value = N / wall.  --warmup W runs an untimed sweep over 80 * W pairs first (code
objects loaded, clocks settled), on the same contexts.
--mode quantum is round 1's steady-state loop (4 train micro-steps then 1 scoring micro-batch, repeated; no fold resets, no tail).

Resident folds: a GPU hosts its folds at once: 288 GB HBM hold one copy of the frozen weights + one adapter / optimizer set per fold
(tst_fork); the folds are STACKED up to --stack per context (include/tst_hip.h "stacked folds": lockstep steps on concatenated
micro-batches, every frozen projection one contraction over all stacked folds' tokens), contexts have their own HIP streams.

Multi-GPU (driver: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...): k is FIXED by --k (5: BASELINE config 2
on more GPUs; 8: config 3's one-fold-per-GPU placement, with --train-mode full its full fine-tune). Fold f runs on rank f mod N
(tst.kfold.folds_for_rank), no data-path collective; every rank runs its folds' part of the same sweep, the wall time is the MAX over
ranks, value = N / wall: total work is fixed, "scaling": "strong", bounded by k / ceil(k / N) (k=5: 5 GPUs busy at N=8). The only
exchange is the control-plane barrier / max-reduce of the timing (torch.distributed gloo, CPU tensors).

A plain run sets up, warms up, times the sweep and prints the JSON line (metric, value, unit, ms_per_step = timed wall / steps, ...; `roofline`
null). --dump-outputs DIR also writes what the timed sweep handed its caller (per QA pair, in id order: s(x), predicted option, correct,
fold; per fold: first / last loss, min / max gradient norm; quantum mode: the last step's scores and context 0's loss / gradient norm) as
DIR/<name>.npy in float64. Everything else runs only with --full: the HIP-event brackets and the clock sampler in the timed region, the
untimed extra steps, the N = 5120 sweep (config.full_n), the config 3 child (config.full_ft) and the CPU legs (cpu_baseline).

With --full the JSON line also carries
  roofline     : the dominant kernel (the projection contraction gemm_pp_kernel, 256x256 ping-pong tile): algorithmic FLOPs
                 2*M*N*(K+K2) of its launches in the timed region / the time it occupied the GPU there, measured with HIP events on the
                 launch streams; `frac` = FLOPs / WALL of the timed region (the conservative headline, checkable on the driver's clock),
                 `frac_union` (union of the launch intervals) and `frac_launch` (per-launch event brackets = what rocprofv3 --stats
                 reports); all three are recomputed from a kernel trace of the same command by tools/bench_profile.sh
                 (profiles/r03_*); `traffic` from the committed PMC summary of this configuration; `hbm_kernels`: achieved GB/s of the HBM-bound kernels (AdamW, SwiGLU, RMSNorm) from their own event
                 brackets in an extra, untimed step
  cpu_baseline : the step restated in torch CPU ops (oracle/llama_aten.py: the ATen kernels the HF path dispatches to) and the numpy oracle
                 (oracle/llama_np.py), both fp32 on the host cores, timed on a bounded slice of the same workload (`legs`; `value` = the ATen leg).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "test-set-training_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LLAMA3_8B = dict(vocab_size=128256, hidden_size=4096, num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128, intermediate_size=14336,
                 rope_theta=500000.0, rms_norm_eps=1e-5)
TINY = dict(vocab_size=1024, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128, intermediate_size=512,
            rope_theta=500000.0, rms_norm_eps=1e-5)
QWEN25_7B = dict(vocab_size=152064, hidden_size=3584, num_layers=28, num_heads=28, num_kv_heads=4, head_dim=128, intermediate_size=18944,
                 rope_theta=1000000.0, rms_norm_eps=1e-6, qkv_bias=True)   # BASELINE.json config 4's base
GPT2_SMALL = dict(arch="gpt2", vocab_size=50257, hidden_size=768, num_layers=12, num_heads=12, num_kv_heads=12, head_dim=64, intermediate_size=3072,
                  max_position=1024, layer_norm_eps=1e-5)                  # BASELINE.json config 1's base
MODELS = {"llama3-8b": ("Llama-3-8B", LLAMA3_8B), "qwen2.5-7b": ("Qwen2.5-7B", QWEN25_7B), "gpt2-small": ("GPT-2-small", GPT2_SMALL), "tiny": ("tiny", TINY)}
MFMA_PEAK_TFLOPS = 2500.0  # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
F32_MFMA_PEAK_TFLOPS = 157.3   # v_mfma_f32_16x16x4_f32 (fp32 in / acc: the strict mode's contractions), same guide "Peak FP32 (matrix)"
TRAIN_BS, SCORE_BS, TRAIN_PER_STEP = 16, 16, 4
REFERENCE_HF = {"value": 2.78, "unit": "QA-train-passes/s", "kind": "reference", "cores": 8,
                "hardware": "authoring container, 8 CPU threads, no GPU (not the GPU box's host)",
                "sample": "HF Trainer.train(use_cpu=True), transformers 5.15.0 / torch 2.10.0, adamw_torch_fused, fp32: random-init GPT-2-small "
                          "(124,439,808 params), N=64 synthetic QA, S=128, micro-batch 8, 1 epoch = 23.0 s",
                "source": "BASELINE.md section 2 (measured once while surveying; the reference Python cannot run on the GPU box)"}
DOMINANT_VARIANT, DOMINANT_KERNEL = 0, "gemm_nt_kernel<128,128,2,2>"  # re-set in main() from the tile policy


def matmul_params(cfg):
    d, F, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    dq, dkv = cfg["num_heads"] * cfg["head_dim"], cfg["num_kv_heads"] * cfg["head_dim"]
    return cfg["num_layers"] * (d * (dq + 2 * dkv) + dq * d + 3 * d * F), V * d


def pmc_traffic(model, policy, folds, stack=1):
    """roofline.traffic: HBM bytes per launch of the dominant kernel from the PMC counters. Counters cannot be read from
    inside the timed run (a --pmc pass serialises every dispatch), so the figure comes from the committed summary of
    `tools/pmc_bench.sh bench` = two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; FETCH doubled for gfx950, KiB -> B)
    over this same command at --steps 1, and only for the configuration that summary was taken on."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r??_pmc_bench_f{folds}_s{stack}_summary.json")))   # the newest round's summary wins
    name = os.path.basename(cands[-1]) if cands else None
    path = os.path.join(ROOT, "profiles", name or "-")
    if model != "llama3-8b" or name is None or not os.path.exists(path):
        return {"traffic": None}
    rows = [row for row in json.load(open(path)) if row["kernel"].startswith("gemm_pp_kernel")]   # (instantiations of the tile are separate rows)
    n = sum(r["launches"] for r in rows)
    if n:
        return {"traffic": sum(r["hbm_bytes_per_launch"] * r["launches"] for r in rows) / n, "traffic_unit": "bytes per launch (fetch x2-corrected + write)",
                "traffic_source": "profiles/" + name + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes over this configuration: "
                                  "tools/pmc_bench.sh bench)"}
    return {"traffic": None}


def pmc_mfma_busy(model, folds, stack=1):
    """roofline.mfma_busy: share of the dominant kernel's SIMD-cycles in which the MFMA pipe was busy, from the committed summary of
    `tools/pmc_mfma.sh` (one rocprofv3 --pmc pass with SQ_VALU_MFMA_BUSY_CYCLES, SQ_BUSY_CYCLES, GRBM_GUI_ACTIVE over this command at --steps 1; a PMC pass
    serialises the dispatches, so the figure is per launch ALONE on the GPU, like `traffic`). Only for the configuration the summary was taken on."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r??_pmc_mfma_f{folds}_s{stack}_summary.json")))   # the newest round's summary
    path = cands[-1] if cands else ""
    if model != "llama3-8b" or not path:
        return {"mfma_busy": None}
    rows = [r for r in json.load(open(path)) if r["kernel"].startswith("gemm_pp_kernel")]
    n = sum(r["launches"] for r in rows)
    if not n:
        return {"mfma_busy": None}
    w = lambda k: sum(r[k] * r["launches"] for r in rows) / n
    return {"mfma_busy": w("mfma_busy"), "mfma_busy_clock_mhz": (w("clock_mhz") if all(r.get("clock_mhz") for r in rows) else None),
            "mfma_busy_source": "profiles/" + os.path.basename(path) + " (SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8) per launch, dispatches serialised by the profiler)"}


def usable_cpus():
    """CPUs this process may actually run on: the affinity mask cut by the cgroup's CPU quota (a GPU box hands a one-GPU job a share of its host cores;
    a thread pool sized to the host's logical CPU count then oversubscribes that share many times over)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: None if t.split()[0] == "max" else int(t.split()[0]) / int(t.split()[1])),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: None if int(t) <= 0 else int(t) / int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()))):
        try:
            q = parse(open(path).read())
            if q:
                n = min(n, max(1, int(q)))
            break
        except Exception:  # noqa: BLE001
            continue
    return max(1, n)


def cpu_baseline(cfg, samples, lora_r, lora_alpha, model_key="llama3-8b", only=None):
    """The path on the GPU box's host cores, on a bounded slice: 1- and 2-layer slices of the same shape, one train micro-batch (16 QA) + one
    scoring batch (16 QA); per-layer and head costs are extrapolated linearly to L layers. Two legs:
      aten  -- oracle/llama_aten.py: the step restated in torch CPU ops (F.linear, SDPA, F.silu, F.cross_entropy, autograd), i.e. the ATen kernels
               the reference HF / PyTorch path dispatches to, on right-padded batches as HF runs them: the credible stand-in for "the reference
               CPU path on the same box's cores" (the reference Python itself cannot travel to the GPU box). `value` is this leg when torch imports.
      numpy -- oracle/llama_np.py: the hand-written fp32 port (BLAS matmuls, Python loops elsewhere), the checker of the GPU tests."""
    from oracle.llama_np import LlamaOracle, hf_weight_names, weight_shape
    from tst import data as D

    rng = np.random.default_rng(0)
    block = (0.02 * rng.standard_normal(1 << 20)).astype(np.float32)

    def cheap(shape):
        n = int(np.prod(shape))
        return np.resize(block, n).reshape(shape) if len(shape) > 1 else np.ones(shape, np.float32)

    mods = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp", "up_proj": "mlp",
            "down_proj": "mlp"}
    L = cfg["num_layers"]

    def leg(make, label, extra, reps=1, warm=False):
        t = {}
        for nl in (1, 2):
            c = dict(cfg, num_layers=nl)
            w = {name: cheap(weight_shape(c, name)) for name in hf_weight_names(c)}
            lora = {}
            for l in range(nl):
                for m, sub in mods.items():
                    dout, din = weight_shape(c, f"model.layers.{l}.{sub}.{m}.weight")
                    lora[f"layers.{l}.{m}.lora_A"] = cheap((lora_r, din))
                    lora[f"layers.{l}.{m}.lora_B"] = cheap((dout, lora_r))
            orc = make(c, w, lora)
            tr, sc = D.collate(samples[:TRAIN_BS]), D.collate(samples[TRAIN_BS:TRAIN_BS + SCORE_BS])
            if warm and nl == 1:   # one UNTIMED call first: thread pool start-up, allocator growth, first-touch of the weights
                orc.loss_and_grads(*tr)
            best = [float("inf"), float("inf")]
            for rep in range(reps):   # best of `reps`: the first call of a torch process also pays its thread pool and allocator warm-up
                t0 = time.perf_counter()
                orc.loss_and_grads(*tr)
                t1 = time.perf_counter()
                orc.score_rows(*sc, D.OPTION_IDS)
                t2 = time.perf_counter()
                best = [min(best[0], t1 - t0), min(best[1], t2 - t1)]
            t[nl] = tuple(best)
            del orc, w, lora
        train = t[1][0] + (L - 1) * (t[2][0] - t[1][0])
        score = t[1][1] + (L - 1) * (t[2][1] - t[1][1])
        step_s = TRAIN_PER_STEP * train + score
        return dict(value=SCORE_BS / step_s, unit="QA-pairs/s", cores=n_use, host_logical_cpus=os.cpu_count(), kind="port", engine=label,
                    sample=f"{extra}, 1- and 2-layer slices of the {L}-layer shape on one 16-QA train micro-batch + one 16-QA scoring batch; "
                           f"per-layer cost extrapolated x{L} (train step {train:.1f} s, scoring batch {score:.1f} s)", **{})

    n_use = usable_cpus()   # threads of both legs = the CPUs this job may run on (affinity mask and cgroup quota), not the host's logical CPU count
    if only == "aten":   # (the child process of the parent's call below)
        import torch
        from oracle.llama_aten import LlamaAten
        default_threads = torch.get_num_threads()
        torch.set_num_threads(n_use)
        out = leg(lambda c, w, lora: LlamaAten(c, w, lora, lora_r, lora_alpha), "aten",
                  f"torch {torch.__version__} CPU ops (oracle/llama_aten.py: F.linear / SDPA / silu / cross_entropy + autograd, fp32, right-padded "
                  f"batches as HF runs them), torch.set_num_threads({n_use}) = the CPUs usable by this job (torch's default here: {default_threads}; host logical CPUs: "
                  f"{os.cpu_count()}), one untimed call first, then best of 2 calls", reps=2, warm=True)
        out["kind"], out["threads"], out["torch_default_threads"] = "aten", n_use, default_threads
        return out
    try:   # the BLAS pool of the numpy leg at the same size
        from threadpoolctl import threadpool_limits
        blas_limit = threadpool_limits(limits=n_use)
    except Exception:  # noqa: BLE001
        blas_limit = None
    numpy_leg = leg(lambda c, w, lora: LlamaOracle(c, w, lora, lora_r, lora_alpha, bf16=False), "numpy",
                    f"numpy fp32 oracle (oracle/llama_np.py), BLAS threads {'limited to ' + str(n_use) if blas_limit else 'at the library default'}", warm=True)
    numpy_leg["threads"] = n_use if blas_limit else None
    if blas_limit is not None:
        blas_limit.restore_original_limits()
    # the ATen leg runs in a CHILD process: torch is imported there, never into the process that holds the HIP library and the measurement
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-leg", "aten", "--model", model_key, "--lora-r", str(lora_r),
                            "--lora-alpha", str(lora_alpha)], capture_output=True, text=True, timeout=600)
        aten_leg = json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:   # torch not importable on this host, or the child failed: the numpy port stands alone
        numpy_leg["aten_unavailable"] = repr(e)[:300]
        return numpy_leg
    out = dict(aten_leg, kind="port")   # (the contract's vocabulary: a restatement timed on the host cores is a "port"; which one: "engine")
    out["legs"] = {"aten": aten_leg, "numpy": numpy_leg}
    return out


def full_ft_leg(steps):
    """BASELINE config 3 measured inside the driver's run: `bench.py --train-mode full --k 8 --steps <steps>` in a child process (its own 160 GB context; the parent has
    released its contexts), reduced to the fields a reader needs. Never raises: the headline line must not be lost over this leg."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--train-mode", "full", "--k", "8", "--steps", str(steps), "--warmup", "0", "--full", "--no-cpu-baseline", "--no-full-n", "--no-full-ft"]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"child rc={r.returncode}: {r.stderr[-400:]}"}
        d = json.loads(line[-1])
        roof = d.get("roofline") or {}
        adam = (roof.get("hbm_kernels") or {}).get("adamw") or {}
        return {"workload": d["config"]["workload"], "k": 8, "n_qa": d["config"].get("n_qa"), "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
                "frac": roof.get("frac"), "frac_union": roof.get("frac_union"), "wall_s": roof.get("wall_ms", 0.0) / 1e3, "adamw_GBps_alone": adam.get("achieved_GBps"),
                "last_loss": d["config"].get("last_loss"), "child_wall_s": time.perf_counter() - t0,
                "note": "BASELINE config 3 on ONE GPU (the 8-GPU form puts one fold on each GPU): run in a child process behind the headline sweep, not part of `value`"}
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one float64 DIR/<name>.npy per array. Should the arrays pass DUMP_MAX_BYTES (a sweep of some 26 000 steps), the longest ones are
    cut to a fixed, seeded sample of their rows (the same rows for all of them), so that two builds still compare row for row."""
    arrays = {name: np.asarray(a, np.float64).ravel() for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        n = max(len(a) for a in arrays.values())
        keep = np.sort(np.random.default_rng(0).choice(n, int(n * DUMP_MAX_BYTES / total), replace=False))
        arrays = {name: (a[keep] if len(a) == n else a) for name, a in arrays.items()}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def sweep_layout(k, rank, world, train_mode="lora", stack=3, layout="folds"):
    """which folds of the k-fold sweep this rank runs and how they sit on its GPU: (fold ids, resident folds F, folds stacked per
    context S, contexts). k is a property of the workload (BASELINE.json: 5 or 8), never of the GPU count.
    layout "folds": fold f -> rank f mod world (tst.kfold.folds_for_rank), ranks beyond k idle; a full fine-tune owns its
    weights, so its folds run one at a time. layout "dp-stacked" (LoRA): EVERY rank hosts all k folds in the one-GPU layout and the
    ranks share each fold's batches (tst.diagnose.diagnose_dp_stacked)."""
    from tst import kfold
    mine = list(range(k)) if layout == "dp-stacked" else kfold.folds_for_rank(k, rank, world)
    F = 1 if train_mode == "full" else max(1, len(mine))
    S = max(1, min(stack, F)) if train_mode == "lora" else 1
    return mine, F, S, (F + S - 1) // S


def union_ms_of(intervals):
    """total time covered by a set of [start, end] intervals (ms)"""
    tot, cs, ce = 0.0, None, None
    for s_, e_ in sorted(intervals):
        if ce is None or s_ > ce:
            if ce is not None:
                tot += ce - cs
            cs, ce = s_, e_
        else:
            ce = max(ce, e_)
    if ce is not None:
        tot += ce - cs
    return tot


def roofline_of(ctxs, dom, policy, args, F, SK, wall_s):
    """dominant-kernel roofline object from the HIP-event brackets logged since profile_enable (all contexts of this rank).
    Three views of the same FLOPs:
      frac        = FLOPs / WALL time of the timed region: what the GPU delivered on the driver's own clock -- the headline, conservative
      frac_union  = FLOPs / union of the launch intervals over all streams (the time at least one such kernel was on the GPU)
      frac_launch = FLOPs / sum of the per-launch brackets (= rocprofv3 --stats' average duration x launches; with several streams a
                    bracket also holds the wait for CUs the other stream's tiles occupy)
    tools/bench_profile.sh recomputes all three from a rocprofv3 --kernel-trace of the same command (profiles/r03_*)."""
    iv = [c.profile_intervals(ctxs[0], variant=dom, unsplit_only=False) for c in ctxs]
    st_all, en_all = np.concatenate([x[0] for x in iv]), np.concatenate([x[1] for x in iv])
    union = union_ms_of(zip(st_all.tolist(), en_all.tolist()))
    t_ref = float(st_all.min()) if len(st_all) else 0.0
    t_end = float(en_all.max()) if len(en_all) else 0.0

    def busy_bins(st, en, nb=20):
        """fraction of each 1/nb of [t_ref, t_end] in which this stream has a dominant-kernel launch in flight (launches of one stream do not overlap)"""
        if not len(st) or t_end <= t_ref:
            return None
        w = (t_end - t_ref) / nb
        out = np.zeros(nb)
        for a, b in zip(st.tolist(), en.tolist()):
            i0, i1 = int((a - t_ref) / w), min(nb - 1, int((b - t_ref) / w))
            for i in range(max(0, i0), i1 + 1):
                out[i] += max(0.0, min(b, t_ref + (i + 1) * w) - max(a, t_ref + i * w))
        return [round(float(v / w), 3) for v in out]

    per_stream = [{"busy_by_twentieth": busy_bins(x[0], x[1]), "union_ms": union_ms_of(zip(x[0].tolist(), x[1].tolist())), "first_start_ms": float(x[0].min()) - t_ref if len(x[0]) else None,
                   "last_end_ms": float(x[1].max()) - t_ref if len(x[1]) else None, "launches": int(len(x[0]))} for x in iv]
    ms_t = flop_t = launches_t = ms_all = launches_all = 0
    for c in ctxs:
        a1, a2, a3 = c.profile_read(variant=dom, unsplit_only=False, reset=False)
        b1, b2, b3 = c.profile_read(variant=-1, unsplit_only=False, reset=True)
        ms_t, flop_t, launches_t, ms_all, launches_all = ms_t + a1, flop_t + a2, launches_t + a3, ms_all + b1, launches_all + b3
        c.profile_enable(0)
    ach_w = (flop_t / wall_s / 1e12) if wall_s > 0 else None
    ach_u = (flop_t / (union * 1e-3) / 1e12) if union > 0 else None
    ach_l = (flop_t / (ms_t * 1e-3) / 1e12) if ms_t > 0 else None
    peak = F32_MFMA_PEAK_TFLOPS if getattr(args, "precision", "bf16") == "strict" else MFMA_PEAK_TFLOPS
    fr = lambda a: a / peak if a else None
    return {"bound": "mfma", "achieved": ach_w, "peak": peak, "unit": "TFLOP/s", "frac": fr(ach_w),
            "frac_definition": "dominant-kernel algorithmic FLOPs of the timed region / wall time of the timed region / peak",
            "achieved_union": ach_u, "frac_union": fr(ach_u), "achieved_launch": ach_l, "frac_launch": fr(ach_l),
            **pmc_traffic(args.model, policy, F, SK),
            "kernel": DOMINANT_KERNEL + " (split-K launches include their slab reduce)", "launches": launches_t,
            "avg_launch_us": (1e3 * ms_t / launches_t) if launches_t else None, "flop_per_launch": (flop_t / launches_t) if launches_t else None,
            "flop_total": flop_t, "wall_ms": 1e3 * wall_s, "gpu_occupied_ms": union, "sum_of_launch_ms": ms_t, "streams": len(ctxs), "concurrent_folds": F,
            "per_stream": per_stream, "streams_overlap_ms": sum(x["union_ms"] for x in per_stream) - union if len(per_stream) == 2 else None,
            "measured": "HIP events on each context's launch stream over the timed region; union = union of the launch intervals",
            "all_contraction_launches": launches_all, "all_contractions_sum_of_launch_ms": ms_all}


def hbm_kernel_rates(ctx, one_step):
    """achieved HBM GB/s of the bandwidth-bound kernel classes (north_star: "achieved-HBM-GB/s counters against gfx950 peak"): one extra,
    untimed step of context 0 alone with every launch of those classes bracketed by HIP events; algorithmic bytes / bracket time."""
    ctx.sync()
    ctx.profile_enable(3)
    one_step()
    ctx.sync()
    out = {}
    for name, vid in (("adamw", 101), ("swiglu_fwd_bwd", 102), ("rmsnorm_fwd_bwd", 103)):
        ms, work, n = ctx.profile_read(variant=vid, unsplit_only=False, reset=False)
        if n:
            out[name] = {"achieved_GBps": work / (ms * 1e-3) / 1e9 if ms > 0 else None, "launches": n, "avg_launch_us": 1e3 * ms / n,
                         "algorithmic_MB_per_launch": work / n / 1e6, "peak_GBps": 8000.0, "achievable_GBps": 6290.0}
    ms, work, n = ctx.profile_read(variant=104, unsplit_only=False, reset=False)
    if n:
        out["attention_fwd"] = {"achieved_TFLOPs": work / (ms * 1e-3) / 1e12 if ms > 0 else None, "launches": n, "avg_launch_us": 1e3 * ms / n}
    ctx.profile_read(variant=-1, reset=True)
    ctx.profile_enable(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64, help="fold quanta per fold; sweep mode: N = 16 * k * steps QA pairs (64 = the full 5120-pair set at k=5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="sweep", choices=["sweep", "quantum"], help="sweep: a whole k-fold sweep through tst.diagnose, value = N / wall "
                    "(the metric as defined); quantum: round 1's steady-state loop of fold quanta")
    ap.add_argument("--model", default="llama3-8b", choices=sorted(MODELS), help="llama3-8b is the configuration the metric is quoted on; the others are "
                    "the bases of BASELINE.json configs 4 and 1")
    ap.add_argument("--eval-bs", type=int, default=16, help="QA pairs per fold in one held-out scoring pass (sweep mode). A throughput knob only: a sample's score does not depend on "
                    "what it is batched with (packed varlen, row-wise ops); HF's per_device_eval_batch_size plays the same role")
    ap.add_argument("--k", type=int, default=5, help="folds of the sweep: FIXED, also with --gpus > 1 (5: configs[1]; 8: config 3's one fold per GPU)")
    ap.add_argument("--folds-per-gpu", type=int, default=0, help="quantum mode: resident folds per GPU (default 5); sweep mode: this rank's folds are all resident")
    ap.add_argument("--stack", type=int, default=3, help="folds STACKED per context (include/tst_hip.h: one lockstep step over the folds' concatenated "
                    "micro-batches); the resident folds are spread over ceil(folds / stack) contexts (HIP streams)")
    ap.add_argument("--tile-policy", type=int, default=-1, help="0: 128x128 contraction tiles, 1: 256x256 ping-pong tiles, 3: the same with split-K; default 1 with several streams, else 3")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: roofline (HIP events, held clock, extra untimed steps), "
                    "config.full_n, config.full_ft, cpu_baseline; the --no-* options below switch single parts of it off")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-clock", action="store_true", help="do not sample the held shader clock during the timed sweep (roofline.clock_mhz_mean)")
    ap.add_argument("--no-full-n", action="store_true", help="do not run the extra N = 5120 sweep behind a shorter timed sweep (config.full_n)")
    ap.add_argument("--no-full-ft", action="store_true", help="do not run the short BASELINE config 3 leg (Llama-3-8B FULL fine-tune, k = 8, N = 640) in a child process behind the "
                                                             "headline sweep (config.full_ft)")
    ap.add_argument("--full-ft-steps", type=int, default=5, help="fold quanta per fold of the config.full_ft leg (5: N = 640)")
    ap.add_argument("--cpu-baseline-leg", default=None, choices=["aten"], help="internal: run ONE leg of cpu_baseline in this (child) process, print its JSON, exit (no GPU, no HIP library)")
    ap.add_argument("--lora-r", type=int, default=16)
    ap.add_argument("--lora-alpha", type=float, default=32.0)
    ap.add_argument("--no-events", action="store_true", help="do not bracket launches with HIP events (PMC passes: rocprofv3 --pmc serialises every dispatch; the run is then only a workload, its JSON line carries no roofline)")
    ap.add_argument("--layout", default="auto", choices=["auto", "folds", "dp-stacked"], help="how a k-fold sweep is spread over --gpus N ranks. folds (= auto): fold f on rank "
                    "f mod N, no collective (bounded by k / ceil(k / N)), the one-GPU training recipe. dp-stacked (LoRA, explicit only): every rank hosts ALL k folds in the "
                    "one-GPU layout, the ranks take disjoint micro-batches of every fold (HF DDP semantics: effective batch 16 x N, 1 / N of the optimizer steps) and "
                    "all-reduce the stacked LoRA gradient once per context and step over RCCL; held-out scoring is sharded by rank without a collective; falls back to "
                    "folds, and says so, when the RCCL groups cannot be formed; reported under its own metric label")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "strict"], help="strict = the fp32 parity mode (every tensor fp32, fp32 MFMA: the arithmetic 's(x) "
                    "within 1e-3 of the reference' is asserted in); one fold per context (no stacking), ~16x slower contractions: a record, not the headline")
    ap.add_argument("--train-mode", default="lora", choices=["lora", "full"], help="full = BASELINE.json config 3 (every weight trainable, one fold resident per GPU); "
                    "the default line stays the LoRA configuration the metric is quoted on")
    args = ap.parse_args()
    if args.cpu_baseline_leg:   # child of cpu_baseline(): the same first 32 synthetic QA pairs, one leg, one JSON line
        from tst import data as D
        cfg = dict(MODELS[args.model][1])
        print(json.dumps(cpu_baseline(cfg, D.synth_vsi(2 * TRAIN_BS, cfg["vocab_size"]), args.lora_r, args.lora_alpha, args.model, only=args.cpu_baseline_leg)))
        return
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    events = args.full and not args.no_events   # HIP-event brackets over the timed region: the roofline object (--full only)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # dp-stacked on 2+ ranks: the preflight children (tst/ddp.py) are spawned HERE, before this process has loaded the HIP library or made any HIP call;
    # they rendezvous through a file of their own and are collected further down, once this process's control plane is up
    preflight = None
    if args.layout == "dp-stacked" and world > 1 and "RANK" in os.environ and os.environ.get("TST_BENCH_SHARE_GPU") != "1" and args.train_mode == "lora" and args.mode == "sweep":
        from tst import ddp as _ddp
        preflight = _ddp.preflight_start(rank, world, local_rank)
    from tst import data as D
    from tst import lib, kfold
    lib.load()
    n_dev = lib.device_count()
    dist = torch = None
    if "RANK" in os.environ:  # launched by torch.distributed.run (also with --nproc-per-node 1): gloo control plane on CPU tensors only
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # gloo announces its connections on the process's stdout (C++ side): keep stdout for the one JSON line
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
            dist.barrier()   # first collective: the pairwise connections (and their messages) happen here
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    from tst.trainer import TrainArgs, collate_stacked, linear_lr, place_folds
    from tst import diagnose as DG
    from tst import score as S

    model_name, cfg = MODELS[args.model]
    targs = TrainArgs(num_train_epochs=1)
    EVAL_BS = SCORE_BS
    if args.mode == "sweep":
        EVAL_BS = targs.per_device_eval_batch_size = max(1, args.eval_bs)
    rehearsal = os.environ.get("TST_BENCH_SHARE_GPU") == "1" and world > 1   # launch-path rehearsal on a one-GPU box: ranks share device 0
    if rehearsal and n_dev > 0:
        local_rank = local_rank % n_dev
    if n_dev <= local_rank:
        raise SystemExit(f"bench.py needs GPU {local_rank}: libtst_hip has no CPU fallback")
    k = args.k
    if args.precision == "strict":
        args.stack = 1   # stacked folds are a bf16-path feature
    layout = args.layout
    if layout == "auto":
        # auto = the collective-free fold layout north_star names, whatever N is: fold f on GPU f mod N, the per-device batch of 16 and the optimizer-step count
        # of the one-GPU line. dp-stacked changes the training recipe (global batch 16 x N, 1 / N of the steps per fold) and its 2+-rank RCCL exchange has
        # never run on hardware: it is an explicit choice (--layout dp-stacked), reported under its own metric label.
        layout = "folds"
    if layout == "dp-stacked" and (args.train_mode != "lora" or args.mode != "sweep"):
        raise SystemExit("--layout dp-stacked is the LoRA sweep layout")
    layout_note = None
    if preflight is not None and dist is not None:
        # PREFLIGHT in throw-away child processes (tst/ddp.py), started at the top of main(): the 2+-rank RCCL exchange has never run on hardware in this
        # build and ncclCommInitRank blocks without a bound -- a hang there must not take the bench down. Every rank's child forms one communicator over
        # all ranks and runs two tiny stacked data-parallel steps; children that hang are killed at 150 s; any failure -> the fold layout.
        ok, msg = _ddp.preflight_finish(preflight)
        flag = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if float(flag.item()) < 1.0:
            layout = "folds"
            layout_note = f"dp-stacked preflight failed ({msg if not ok else 'on another rank'}) -> fold layout"
    if args.mode == "sweep":
        mine, F, SK, NC = sweep_layout(k, rank, world, args.train_mode, args.stack, layout)   # k is never changed by the GPU count
    else:
        F = 1 if args.train_mode == "full" else max(1, args.folds_per_gpu or 5)
        mine = [(rank * F + i) % k for i in range(F)]
        SK = max(1, min(args.stack, F)) if args.train_mode == "lora" else 1
        NC = (F + SK - 1) // SK   # contexts (streams) on this GPU
    global DOMINANT_VARIANT, DOMINANT_KERNEL
    policy = lib.set_tile_policy(args.tile_policy if args.tile_policy >= 0 else (1 if NC > 1 else 3))
    if policy:
        kind = int(os.environ.get("TST_BIG_KIND", "5"))
        DOMINANT_VARIANT, DOMINANT_KERNEL = (5, "gemm_pp_kernel (256x256x64 ping-pong tile)") if kind == 5 else (4, "gemm_big_kernel (256x256x64 tile)")
    if args.precision == "strict":
        DOMINANT_VARIANT, DOMINANT_KERNEL = 30, "gemm_f32_kernel<NT> (64x64x32 tile, v_mfma_f32_16x16x4_f32)"
    dom = DOMINANT_VARIANT
    def barrier():
        if dist is not None:
            dist.barrier()

    def max_over_ranks(x):
        if dist is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def min_over_ranks(x):
        return -max_over_ranks(-x)

    def make_contexts():
        root = lib.Context(cfg, device=local_rank, max_tokens=max(TRAIN_BS, EVAL_BS) * 128 * SK, max_seqs=max(TRAIN_BS, EVAL_BS) * SK,
                           max_labelled=4 * max(TRAIN_BS, EVAL_BS) * SK, max_position=128, lora_r=targs.lora_r, lora_alpha=targs.lora_alpha,
                           lora_targets=targs.lora_targets, weight_decay=targs.weight_decay, max_grad_norm=targs.max_grad_norm, train_mode=args.train_mode,
                           n_stack=SK, precision=args.precision)
        root.init_random(seed=0, std=0.02)
        return [root] + [root.fork() for _ in range(NC - 1)]

    ctxs = make_contexts() if mine else []
    if layout == "dp-stacked":   # (also at world 1, where the group is a 1-rank communicator: the same code path end to end)
        # context j of every rank joins RCCL communicator j. The 2+-rank exchange has never run on hardware (one-GPU boxes only): if any rank
        # cannot form its groups or finish one tiny step within 120 s, ALL ranks fall back to the fold layout and the line says so.
        from tst import ddp
        os.environ.setdefault("TST_DP_TIMEOUT_S", "120")
        ok = 1.0
        try:
            ddp.init_stacked_groups(ctxs, rank, world) if dist is not None else [c.dp_init(c.dp_unique_id(), 1, 0) for c in ctxs]
            probe = D.synth_vsi(2 * SK, cfg["vocab_size"], seed=11)
            for c in ctxs:
                parts = [(sl, probe[2 * sl:2 * sl + 2]) for sl in range(SK)]
                ids, labels, cu, seq_slot = collate_stacked(parts)
                c.train_step_stacked_dp_async(ids, labels, cu, seq_slot, [0.0] * SK, [world * D.count_labelled(b) for _, b in parts])
            for c in ctxs:
                c.fetch_metrics_stacked()
                c.sync()
        except Exception as e:  # noqa: BLE001  (TstError, RCCL failure, timeout)
            ok = 0.0
            layout_note = f"dp-stacked self-test failed on rank {rank}: {e!r}"
        if min_over_ranks(ok) < 1.0:
            for c in reversed(ctxs):
                c.close()
            layout = "folds"
            layout_note = (layout_note or "dp-stacked self-test failed on another rank") + " -> fell back to the fold layout"
            mine, F, SK, NC = sweep_layout(k, rank, world, args.train_mode, args.stack, layout)
            policy = lib.set_tile_policy(args.tile_policy if args.tile_policy >= 0 else (1 if NC > 1 else 3))
            ctxs = make_contexts() if mine else []

    def sync_all():
        for c in ctxs:
            c.sync()

    def sum_over_ranks(x):
        if dist is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.SUM)
        return float(tt.item())

    def gather_on_rank0(items):
        """every rank's list, concatenated on rank 0 (None elsewhere)"""
        if dist is None:
            return list(items)
        parts = [None] * world if rank == 0 else None
        dist.gather_object(list(items), parts, dst=0)
        return [x for p in parts for x in p] if rank == 0 else None

    extra = {}
    if args.mode == "sweep":
        # ------------------------------------------------------------------ the metric as defined: one whole k-fold sweep
        per_step = TRAIN_BS * k          # QA pairs one fold quantum of every fold accounts for
        n_timed, n_warm = per_step * args.steps, per_step * args.warmup
        vocab = cfg["vocab_size"]
        samples = D.synth_vsi(n_timed, vocab)                              # numpy default_rng(20251121): BASELINE.md section 3
        warm = D.synth_vsi(max(n_warm, 2 * k), vocab, seed=7) if args.warmup > 0 else []
        group = ctxs if len(ctxs) > 1 or SK > 1 else (ctxs[0] if ctxs else None)

        def sweep(smp):
            if not mine:
                return [], []
            if layout == "dp-stacked":
                return DG.diagnose_dp_stacked(ctxs, smp, k, targs, rank=rank, world=world, out_dir=None, resume=False)
            return DG.diagnose(group, smp, k, targs, rank=rank, world=world, out_dir=None, resume=False)

        if warm:
            sweep(warm)
        sync_all()
        barrier()
        for c in ctxs:
            c.profile_enable(1 if events else 0)
        # the shader clock the chip HOLDS under this load, sampled every 50 ms by a one-wave probe on a stream of its own (tst_clock_probe): the 2.5 PFLOP/s
        # peak assumes 2.4 GHz, and `frac_at_held_clock` restates `frac` against the clock actually held (rank 0's GPU)
        clock = lib.ClockSampler(local_rank).start() if (ctxs and args.full and not args.no_clock) else None
        t0 = time.perf_counter()
        records, stats = sweep(samples)          # per fold: adapter reset, one shuffled epoch (ragged last micro-batch), held-out scoring tail
        sync_all()
        elapsed_local = time.perf_counter() - t0
        clock_mhz = clock.stop() if clock else []
        barrier()
        elapsed = max_over_ranks(elapsed_local)
        n_scored = int(sum_over_ranks(len(records)))
        if n_scored != n_timed:
            raise SystemExit(f"sweep scored {n_scored} of {n_timed} QA pairs")
        # a fold that silently did not train must not produce a number: every step's loss and gradient norm finite, the gradient norm never zero (the
        # outputs themselves are at chance by construction -- random base, 80 steps at lr 5e-5 -- and could not show it)
        sick = [st for st in stats if st.get("steps", 0) and (not st["loss_finite"] or not (st["grad_norm_min"] > 0.0))]
        if sick:
            raise SystemExit(f"fold(s) {[st['fold'] for st in sick]} did not train: loss / gradient norm non-finite or a zero gradient norm ({sick[0]})")
        if args.dump_outputs:
            recs, sts = gather_on_rank0(records), gather_on_rank0(stats)
            if rank == 0:
                recs.sort(key=lambda r: r["id"])
                sts = sorted({st["fold"]: st for st in sts}.values(), key=lambda st: st["fold"])   # (dp-stacked: every rank reports every fold)
                dump_outputs(args.dump_outputs, {**{key: [r[key] for r in recs] for key in ("s", "pred", "correct", "fold")},
                                                 **{"fold_" + key: [np.nan if st.get(key) is None else st[key] for st in sts]
                                                    for key in ("first_loss", "last_loss", "grad_norm_min", "grad_norm_max")}})
        units = n_timed
        acc = float(np.mean([r["correct"] for r in records])) if records else None
        mean_s = float(np.mean([r["s"] for r in records])) if records else None
        passes = n_timed * ((k - 1) * targs.num_train_epochs + 1)
        last_loss = stats[-1]["last_loss"] if stats else None
        workload = (f"k={k} TsT SWEEP over N={n_timed} synthetic VSI-Bench-shaped text-only QA pairs (per fold: adapter reset, 1 epoch of "
                    f"{(k - 1) * n_timed // k // TRAIN_BS} LoRA micro-steps of 16 QA, held-out scoring of {n_timed // k} QA; = {args.steps} fold quanta per fold), "
                    if args.train_mode == "lora" else
                    f"k={k} TsT SWEEP over N={n_timed} synthetic VSI-Bench-shaped text-only QA pairs, FULL fine-tune (fp32 master + AdamW over all parameters), ")
        extra = {"n_qa": n_timed, "qa_passes_per_s": passes / elapsed, "heldout_acc": acc, "mean_s": mean_s, "last_loss": last_loss,
                 "rank0_wall_s": elapsed_local, "layout": layout}
        if layout == "dp-stacked":
            extra.update({"folds_by_rank": [list(range(k))] * world, "effective_train_batch": TRAIN_BS * world,
                          "optimizer_steps_per_fold": -(-((k - 1) * n_timed // k) // (TRAIN_BS * world)),
                          "scaling_bound": "linear in n_gpus (every GPU keeps the one-GPU layout; one all-reduce of the stacked LoRA gradient per context and step)",
                          "hardware_status": "2+-rank RCCL exchange unverified before this run (one-GPU boxes only); a self-test guards it and falls back to layout=folds"})
        else:
            extra.update({"folds_by_rank": [kfold.folds_for_rank(k, r, world) for r in range(world)],
                          "scaling_bound": f"k / ceil(k / n_gpus) = {k / -(-k // world):.2f}x over one GPU"})
        if args.layout == "auto" and args.train_mode == "lora":
            # both facts of the choice, in the line: what auto runs and what the alternative would change
            extra["layout_choice"] = {"auto": "folds",
                                      "folds": f"fold f on GPU f mod N, no data-path collective, the one-GPU recipe (batch {TRAIN_BS}, same optimizer steps); bounded by "
                                               f"k / ceil(k / N) = {k / -(-k // world):.2f}x at N = {world}",
                                      "dp-stacked": f"--layout dp-stacked: every GPU hosts all {k} folds and the ranks share each fold's batches over RCCL -- near-linear in N by "
                                                    f"construction, but a DIFFERENT training recipe (global batch {TRAIN_BS} x N, 1 / N of the optimizer steps per fold) whose "
                                                    f"2+-rank exchange has not run on hardware; reported under its own metric label"}
        if layout_note:
            extra["layout_note"] = layout_note
        train_parts = None
    else:
        # ------------------------------------------------------------------ round 1's steady-state loop of fold quanta
        n_samples = 512 if args.model == "tiny" else 5120
        samples = D.synth_vsi(n_samples, cfg["vocab_size"])
        assign = kfold.kfold_assign(len(samples), k, True, 42)
        need_train = (args.steps + args.warmup) * TRAIN_PER_STEP * TRAIN_BS
        need_held = (args.steps + args.warmup) * SCORE_BS
        where = place_folds(F, ctxs)
        on_ctx = [[(sl, i) for i, (jj, sl) in enumerate(where) if jj == j] for j in range(NC)]
        train, held = [], []
        for i, (j, sl) in enumerate(where):
            tr, he = kfold.fold_indices(assign, mine[i])
            train.append([samples[tr[q % len(tr)]] for q in range(need_train)])
            held.append([samples[he[q % len(he)]] for q in range(need_held)])
            ctxs[j].select_slot(sl)
            ctxs[j].reset_trainable(seed=mine[i])
        for c in ctxs:
            c.select_slot(0)
        total_opt_steps = (len(samples) - len(samples) // k) // TRAIN_BS
        pending = [None] * len(ctxs)

        def fetch_scores():
            out = []
            for j, c in enumerate(ctxs):
                if pending[j] is not None:
                    logp, corr, optl, rseq = c.score_rows_fetch()
                    out.append(S.bias_scores(pending[j], logp, corr, optl, rseq))
                    pending[j] = None
            return out

        def train_micro(j, i, m, lr):
            parts = [(sl, train[f][(i * TRAIN_PER_STEP + m) * TRAIN_BS:(i * TRAIN_PER_STEP + m + 1) * TRAIN_BS]) for sl, f in on_ctx[j]]
            if SK == 1:
                ids, labels, cu = D.collate(parts[0][1])
                ctxs[j].train_step_async(ids, labels, cu, lr)
            else:
                ids, labels, cu, seq_slot = collate_stacked(parts)
                ctxs[j].train_step_stacked_async(ids, labels, cu, seq_slot, [lr] * SK)

        def score_micro(j, i):
            parts = [(sl, held[f][i * SCORE_BS:(i + 1) * SCORE_BS]) for sl, f in on_ctx[j]]
            ids, labels, cu, seq_slot = collate_stacked(parts)
            ctxs[j].score_rows_async(ids, labels, cu, D.OPTION_IDS, seq_slot if SK > 1 else None)
            return [x for _, b in parts for x in b]

        def run_step(i):
            for m in range(TRAIN_PER_STEP):
                for j in range(NC):
                    train_micro(j, i, m, linear_lr(i * TRAIN_PER_STEP + m, total_opt_steps, targs.learning_rate))
            out = fetch_scores()
            for j in range(NC):
                pending[j] = score_micro(j, i)
            return out

        for i in range(args.warmup):
            run_step(i)
        fetch_scores()
        sync_all()
        barrier()
        for c in ctxs:
            c.profile_enable(1 if events else 0)
        t0 = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            run_step(i)
        res = fetch_scores()
        sync_all()
        elapsed = max_over_ranks(time.perf_counter() - t0)
        barrier()
        units = world * F * SCORE_BS * args.steps
        loss, gnorm = ctxs[0].fetch_metrics()
        if args.dump_outputs:
            scored = gather_on_rank0(res)   # the last step's held-out scores, context by context, rank by rank
            if rank == 0:
                dump_outputs(args.dump_outputs, {"s": np.concatenate([r[0] for r in scored]), "pred": np.concatenate([r[1] for r in scored]),
                                                 "correct": np.concatenate([r[2] for r in scored]), "loss": [loss], "grad_norm": [gnorm]})
        extra = {"qa_passes_per_s": world * F * (TRAIN_PER_STEP * TRAIN_BS + SCORE_BS) * args.steps / elapsed, "last_loss": loss, "last_grad_norm": gnorm,
                 "heldout_acc_last_batch": float(np.mean(np.concatenate([r[2] for r in res]))), "folds_on_rank0": mine}
        workload = f"k={k} TsT fold quantum loop ({TRAIN_PER_STEP}x16 QA LoRA train steps + 16 QA held-out scoring per fold and step; steady state, no fold resets), "

    roof = roofline_of(ctxs, dom, policy, args, F, SK, elapsed) if (ctxs and events) else None   # wall = MAX over ranks: conservative
    if roof is not None and args.mode == "sweep" and clock_mhz:
        cm = np.array(clock_mhz, np.float64)
        roof.update({"clock_mhz_mean": float(cm.mean()), "clock_mhz_min": float(cm.min()), "clock_mhz_max": float(cm.max()), "clock_samples": int(len(cm)),
                     "clock_source": "tst_clock_probe every 50 ms over the timed region: d(s_memtime) / d(s_memrealtime) x 100 MHz from one probe wave",
                     "frac_at_held_clock": (roof["frac"] * 2400.0 / float(cm.mean())) if roof.get("frac") else None,
                     "frac_at_held_clock_definition": "frac x 2400 MHz / clock_mhz_mean: the same FLOPs against the MFMA peak at the clock the chip held"})
    if roof is not None:
        roof.update(pmc_mfma_busy(args.model, F, SK))

    full_n = None
    if rank == 0 and events:   # --full from here on (a --no-events profiler pass runs none of it)
        # one extra untimed step of context 0 alone: HBM-bound kernel classes, and the dominant kernel with the GPU to itself
        def one_step():
            smp = samples[:TRAIN_BS * SK]
            parts = [(sl, smp[sl * TRAIN_BS:(sl + 1) * TRAIN_BS]) for sl in range(SK)]
            if SK == 1:
                ids, labels, cu = D.collate(parts[0][1])
                ctxs[0].train_step_async(ids, labels, cu, 0.0)
            else:
                ids, labels, cu, seq_slot = collate_stacked(parts)
                ctxs[0].train_step_stacked_async(ids, labels, cu, seq_slot, [0.0] * SK)
        sync_all()
        hbm = hbm_kernel_rates(ctxs[0], one_step)
        ctxs[0].profile_enable(1)
        one_step()
        ctxs[0].sync()
        ms, flop, launches = ctxs[0].profile_read(variant=dom, unsplit_only=False, reset=True)
        ctxs[0].profile_enable(0)
        roof["exclusive_achieved"] = (flop / (ms * 1e-3) / 1e12) if ms > 0 else None
        roof["exclusive_avg_launch_us"] = (1e3 * ms / launches) if launches else None
        # the two extra single-context steps above come AFTER the timed region: a kernel trace of this command holds the timed launches
        # right before them (tools/trace_roofline.py cuts the trace there)
        roof["launches_after_timed_region"] = 2 * launches
        roof["hbm_kernels"] = hbm
        # The metric is quoted on the FULL N = 5120 set; the driver's command (--steps 20) times N = 1600. So that the driver's own
        # run also carries the quoted configuration, the full sweep runs once more here, in the same process and on the same contexts, after everything
        # the headline `value` is computed from (--no-full-n skips it; the default --steps 64 IS the full set). One GPU, LoRA sweep only.
        n_full = TRAIN_BS * k * 64
        if args.mode == "sweep" and world == 1 and args.train_mode == "lora" and not args.no_full_n and n_timed < n_full and args.model != "tiny":
            smp_full = D.synth_vsi(n_full, vocab)
            for c in ctxs:
                c.profile_enable(1)
            t0 = time.perf_counter()
            rec_full, _ = sweep(smp_full)
            sync_all()
            wall_full = time.perf_counter() - t0
            n_l = 0
            for c in ctxs:
                n_l += c.profile_read(variant=dom, unsplit_only=False, reset=True)[2]
                c.profile_enable(0)
            if len(rec_full) != n_full:
                raise SystemExit(f"full-N sweep scored {len(rec_full)} of {n_full} QA pairs")
            full_n = {"n_qa": n_full, "value": n_full / wall_full, "unit": "QA-pairs/s", "wall_s": wall_full, "steps_equivalent": 64,
                      "heldout_acc": float(np.mean([r["correct"] for r in rec_full])),
                      "note": "the same sweep over the full N = 5120 set, run once after the timed region in the same process (not part of `value`)"}
            roof["launches_after_timed_region"] += int(n_l)
    if rank == 0:
        out = {
            "metric": "QA-pairs/sec, full k-fold TsT on VSI-Bench text-only" + (f" [dp-stacked recipe: global batch {TRAIN_BS * world}]" if layout == "dp-stacked" and world > 1 else ""),
            "value": units / elapsed,
            "unit": "QA-pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000.0 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong" if args.mode == "sweep" else "weak", "vs_baseline": None,
            "dtype": "f32" if args.precision == "strict" else "bf16", "data": "synthetic",
            "config": {"workload": workload + f"{model_name} shape, "
                                   + (f"LoRA r={targs.lora_r} all-linear" if args.train_mode == "lora" else "every weight trainable")
                                   + (", fp32 STRICT parity mode" if args.precision == "strict" else ", bf16") + ", packed varlen, E=1",
                       "mode": args.mode, "k": k, "micro_batch": TRAIN_BS, "eval_batch": EVAL_BS, "folds_per_gpu": F, "stack": SK, "contexts_per_gpu": NC,
                       "parallelism": (f"dp-stacked: all {k} folds resident on every one of the {world} GPU(s) ({NC} HIP stream(s) x up to {SK} folds stacked per lockstep step); "
                                       f"the ranks take disjoint 16-QA micro-batches of every fold (global batch {TRAIN_BS * world}), one RCCL all-reduce of the stacked LoRA "
                                       f"gradient per context and step; held-out scoring sharded by rank, no collective" if layout == "dp-stacked" else
                                       f"fold-parallel: fold f on GPU f mod {world}; on a GPU its {F} folds are resident (shared frozen weights; {NC} HIP stream(s) x up to "
                                       f"{SK} folds stacked per lockstep step); no data-path collective"), **extra},
            "roofline": roof,
        }
        if args.no_events:
            out["note"] = "--no-events run (profiler workload): no roofline object"
        # BASELINE config 3 on this GPU (Llama-3-8B FULL fine-tune, k = 8; one fold resident at a time, ~160 GB): the LoRA contexts are closed first, then a CHILD
        # process runs `bench.py --train-mode full --k 8 --steps 5` (N = 640) and its line is folded in here, so that the driver's own run carries the number
        if (events and world == 1 and args.mode == "sweep" and args.train_mode == "lora" and args.model == "llama3-8b" and args.precision == "bf16" and not args.no_full_ft
                and not rehearsal):
            for c in reversed(ctxs):
                c.close()
            ctxs = []
            out["config"]["full_ft"] = full_ft_leg(args.full_ft_steps)
        if os.environ.get("TST_WHATIF", "0") not in ("", "0"):
            out["diagnostic"] = f"TST_WHATIF={os.environ['TST_WHATIF']}: a kernel class was NOT run (timing-only ablation, engine.hip whatif()); the value is not a measurement of the product"
        if full_n:
            out["config"]["full_n"] = full_n
        if layout == "dp-stacked":   # a different recipe from the one-GPU / BASELINE line at per-device batch 16: said at the top level, never compared with a baseline
            out["effective_train_batch"] = extra.get("effective_train_batch")
            out["optimizer_steps_per_fold"] = extra.get("optimizer_steps_per_fold")
            out["vs_baseline"] = None
        if rehearsal:
            out["rehearsal"] = f"{world} ranks shared ONE GPU (TST_BENCH_SHARE_GPU=1): exercises the launch path only, the value is not a measurement"
        if events and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(cfg, samples, targs.lora_r, targs.lora_alpha, args.model)
            except Exception as e:  # the baseline is a reported side figure; never lose the GPU line over it
                out["cpu_baseline"] = {"value": None, "unit": "QA-pairs/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e!r}"}
            # the reference stack itself (HF Trainer) cannot travel to the GPU box; its figure was measured in the authoring container
            # and is quoted with its hardware -- another model size, another unit: context only
            out["cpu_baseline"]["reference_hf"] = REFERENCE_HF
        print(json.dumps(out))
    for c in reversed(ctxs):
        c.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
