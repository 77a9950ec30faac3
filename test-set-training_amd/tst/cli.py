"""`python -m tst.cli diagnose|prune|rf|export ...` -- the TsT command line (upstream has no CLI to match yet,
SURVEY §7 hard part 2: the surface is defined and frozen here, names mirror HF TrainingArguments).

Launch one process per GPU for multi-GPU runs (python -m torch.distributed.run --nproc-per-node N -m tst.cli diagnose ...).
--layout folds (default): ranks split the folds (fold f -> rank f % world), no collective is used: shards are files under --out.
--layout dp-stacked (LoRA): every rank hosts ALL folds (stacked contexts) and the ranks share every fold's batches (global batch = world x
per-device batch, one RCCL all-reduce of the stacked LoRA gradient per context and step); scoring is sharded by rank, rank 0 writes the shards.
--dp N: groups of N ranks share one fold at a time (BASELINE.json config 4; --dp-mode shard | replicate).
"""
import argparse
import json
import os
import sys

import numpy as np

MODEL_SHAPES = {
    "llama3-8b": dict(vocab_size=128256, hidden_size=4096, num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128, intermediate_size=14336,
                      rope_theta=500000.0, rms_norm_eps=1e-5),
    # BASELINE.json config 3's base (q/k/v bias; modeling_qwen2.py:189-191)
    "qwen2.5-7b": dict(vocab_size=152064, hidden_size=3584, num_layers=28, num_heads=28, num_kv_heads=4, head_dim=128, intermediate_size=18944,
                       rope_theta=1000000.0, rms_norm_eps=1e-6, qkv_bias=True),
    # Qwen3 (dense): no q/k/v bias, RMSNorm over head_dim on every q and k head (modeling_qwen3.py:237-238, 252-253); head_dim is 128 at every size,
    # so num_heads * head_dim != hidden_size at the small ones
    "qwen3-8b": dict(vocab_size=151936, hidden_size=4096, num_layers=36, num_heads=32, num_kv_heads=8, head_dim=128, intermediate_size=12288,
                     rope_theta=1000000.0, rms_norm_eps=1e-6, qk_norm=True),
    "qwen3-0.6b": dict(vocab_size=151936, hidden_size=1024, num_layers=28, num_heads=16, num_kv_heads=8, head_dim=128, intermediate_size=3072,
                       rope_theta=1000000.0, rms_norm_eps=1e-6, qk_norm=True),
    # BASELINE.json config 1's base (configuration_gpt2.py:83-103)
    "gpt2-small": dict(arch="gpt2", vocab_size=50257, hidden_size=768, num_layers=12, num_heads=12, num_kv_heads=12, head_dim=64,
                       intermediate_size=3072, max_position=1024, layer_norm_eps=1e-5),
    "tiny-gpt2": dict(arch="gpt2", vocab_size=1001, hidden_size=128, num_layers=2, num_heads=2, num_kv_heads=2, head_dim=64, intermediate_size=512,
                      max_position=128, layer_norm_eps=1e-5),
    "tiny": dict(vocab_size=1024, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128, intermediate_size=512,
                 rope_theta=500000.0, rms_norm_eps=1e-5),
}


def build_parser():
    ap = argparse.ArgumentParser(prog="tst")
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("diagnose", "prune"):
        p = sub.add_parser(name)
        p.add_argument("--model", default="tiny", choices=sorted(MODEL_SHAPES))
        p.add_argument("--weights-seed", type=int, default=0, help="random-init base weights (no pretrained assets offline)")
        p.add_argument("--model-dir", default=None, help="local HuggingFace checkpoint directory (config.json + model.safetensors[.index.json]; "
                       "Llama / Qwen2 / Qwen3 / GPT-2): shapes and weights come from it instead of --model / --weights-seed (tst/io.py)")
        p.add_argument("--data", default="synthetic-vsi", help="synthetic-vsi, or with --data-file the name recorded in the outputs")
        p.add_argument("--data-file", default=None, help="QA JSONL {id, question, options (optional), answer}: the benchmark's text-only records; "
                       "needs --tokenizer (tst/io.py: load_qa_jsonl)")
        p.add_argument("--tokenizer", default=None, help="tokenizer.json (tokenizers format); default <model-dir>/tokenizer.json")
        p.add_argument("--max-len", type=int, default=128, help="longest sequence: prompts are cut from the left, the answer always survives")
        p.add_argument("--n-samples", type=int, default=512)
        p.add_argument("--k", type=int, default=5)
        p.add_argument("--out", required=True)
        p.add_argument("--learning-rate", type=float, default=5e-5)
        p.add_argument("--num-train-epochs", type=int, default=3)
        p.add_argument("--per-device-train-batch-size", type=int, default=16)
        p.add_argument("--weight-decay", type=float, default=0.0)
        p.add_argument("--max-grad-norm", type=float, default=1.0)
        p.add_argument("--warmup-steps", type=int, default=0)
        p.add_argument("--seed", type=int, default=42)
        p.add_argument("--lora-r", type=int, default=16)
        p.add_argument("--lora-alpha", type=float, default=32.0)
        p.add_argument("--train-mode", default="lora", choices=["lora", "full"], help="full = every weight trainable (BASELINE.json config 3)")
        p.add_argument("--config", default=None, help="YAML file whose keys are the option names above with underscores, as in HF TrainingArguments "
                       "(learning_rate, num_train_epochs, per_device_train_batch_size, weight_decay, max_grad_norm, warmup_steps, seed, "
                       "lora_r, lora_alpha, k, model, train_mode, ...); command-line flags given explicitly win")
        p.add_argument("--logging-steps", type=int, default=50, help="every N optimizer steps one {fold, step, loss, grad_norm, lr} line goes to <out>/train_log.jsonl")
        p.add_argument("--folds-per-gpu", type=int, default=0, help="folds resident on one GPU at once (LoRA only: forked contexts share the frozen "
                       "base); 0 = 3 when this rank has that many folds to run, else what it has")
        p.add_argument("--stack", type=int, default=0, help="folds stacked per context (LoRA only; include/tst_hip.h 'stacked folds': the folds of a "
                       "context train in lockstep on their concatenated micro-batches, the frozen projections see one long contraction); "
                       "0 = up to 3 per context")
        p.add_argument("--gradient-accumulation-steps", type=int, default=1, help="micro-batches per optimizer update, normalised by ONE num_items_in_batch "
                       "(HF TrainingArguments.gradient_accumulation_steps; trainer.py:1740-1758, 2141-2175)")
        p.add_argument("--layout", default="folds", choices=["folds", "dp-stacked"], help="multi-GPU placement of a LoRA sweep: folds = fold f on rank f mod world, "
                       "no collective; dp-stacked = every rank hosts all k folds in stacked contexts and the ranks take disjoint micro-batches of every fold "
                       "(effective batch = world x per-device batch; one all-reduce per context and step). UNVERIFIED ON MULTI-GPU HARDWARE like --dp")
        p.add_argument("--dp-mode", default="shard", choices=["shard", "replicate"], help="with --dp > 1: shard = ONE micro-batch split over the group (the "
                       "single-GPU trajectory; each GPU sees 1/dp of the tokens); replicate = every rank its own micro-batch (HF DDP: global batch = dp x "
                       "per-device batch, every GPU keeps its full token count)")
        p.add_argument("--dp-transport", default="f32", choices=["f32", "bf16"], help="with --dp > 1 and --train-mode full: wire format of the region-wise "
                       "gradient all-reduce (bf16 = half the xGMI bytes, the precision torch DDP reduces a bf16 model's gradients in)")
        p.add_argument("--dp", type=int, default=1, help="intra-fold data parallelism: groups of this many ranks share a fold (RCCL all-reduce of "
                       "the gradient inside the library; launch with torch.distributed.run, world size a multiple of --dp); one fold per group "
                       "at a time, no stacking. UNVERIFIED ON MULTI-GPU HARDWARE: the 2-rank exchange has only run on CPU stand-ins and with "
                       "1-rank communicators on one MI355X; a rank whose step fails aborts its communicator and exits non-zero")
        p.add_argument("--generate", action="store_true", help="also generate every held-out sample's answer (greedy, KV cache; include/tst_hip.h "
                       "tst_generate_async): the records gain gen (token ids), gen_correct and, with a tokenizer, gen_text. Off: the run is unchanged")
        p.add_argument("--max-new-tokens", type=int, default=8, help="with --generate / --generate-samples: tokens generated per sample (1..256)")
        p.add_argument("--generate-samples", type=int, default=0, metavar="N", help="also draw N (1..64) answers per held-out sample from the model's own "
                       "distribution (include/tst_hip.h tst_sample_async: one prefill, N short decodes on a shared prompt cache): the records gain samples = "
                       "{ids, logp, match (share of draws that start with the reference answer)} and, with a tokenizer, texts and mra (expected VSI-Bench mean "
                       "relative accuracy, numeric references). Independent of --generate; uses --max-new-tokens / --eos-ids. 0: the run is unchanged")
        p.add_argument("--temperature", type=float, default=1.0, help="with --generate-samples: sampling temperature (0.01..100); 1 is the model's distribution")
        p.add_argument("--sample-seed", type=int, default=0, help="with --generate-samples: the run's seed; a QA pair's draws depend on it and the pair's id only")
        p.add_argument("--eos-ids", default=None, help="with --generate / --generate-samples: comma-separated token ids that end an answer; default: eos_token_id of "
                       "<model-dir>/generation_config.json or config.json when present, else none")
        p.add_argument("--candidates", type=int, default=0, metavar="N", help="also score every held-out free-form (\"na\") sample's prompt against the N most "
                       "frequent reference answers of the data set and its own (include/tst_hip.h tst_score_candidates_async: one prefill, every candidate "
                       "token in one extend pass): the records gain cand = {n, rank and p_ref of the reference on that closed set, mass (log of the share of the "
                       "model's distribution the list covers), top, top_p} and, with a tokenizer, top_text and mra_exp (expected mean relative accuracy without "
                       "sampling noise). Independent of the other flags. 0: the run is unchanged")
        p.add_argument("--attribute", action="store_true", help="also attribute every held-out sample's score to its prompt tokens (one more forward + backward "
                       "per held-out batch; include/tst_hip.h tst_attribute_async): the records gain attr = {gxi, gnorm} over the prompt tokens and, with a "
                       "tokenizer, attr_top. Off: the run is unchanged. Not with --dp > 1 or --layout dp-stacked")
        p.add_argument("--attribute-top", type=int, default=5, help="with --attribute: tokens listed in attr_top (largest gradient norm first)")
        p.add_argument("--attribute-ig", type=int, default=0, metavar="STEPS", help="also attribute every held-out sample's score to its prompt tokens by "
                       "integrated gradients over STEPS midpoint steps (1..256; about STEPS forward + backward passes plus two forward passes per held-out batch; include/tst_hip.h "
                       "tst_attribute_ig_async): the prompt tokens are walked from --attribute-baseline-id to their own embeddings, the answer tokens stay; the "
                       "records gain attr_ig = {ig, log_s_base, delta} and, with a tokenizer, attr_ig_top (--attribute-top tokens, largest |ig| first, signed). "
                       "0: off, the run is unchanged. Not with --dp > 1 or --layout dp-stacked")
        p.add_argument("--attribute-baseline-id", type=int, default=None, metavar="ID", help="with --attribute-ig: the token id of the baseline prompt; default: "
                       "the tokenizer's pad id, else the checkpoint's pad_token_id, else its first eos id, else 0 (the choice is recorded in the train log)")
        if name == "prune":
            p.add_argument("--rounds", type=int, default=4)
            p.add_argument("--tau", type=float, default=0.5)
            p.add_argument("--prune-frac", type=float, default=0.1)
    r = sub.add_parser("rf", help="TsT-RF: random forest on non-visual text features, same k-fold split and record schema (CPU, scikit-learn)")
    r.add_argument("--data-file", required=True, help="QA JSONL {id, question, options (optional), answer}")
    r.add_argument("--k", type=int, default=5)
    r.add_argument("--seed", type=int, default=42)
    r.add_argument("--n-estimators", type=int, default=200)
    r.add_argument("--top", type=int, default=10, help="feature importances printed")
    r.add_argument("--out", required=True)
    c = sub.add_parser("convert", help="a local copy of a benchmark table (parquet / json / jsonl / csv) -> the QA JSONL that --data-file reads; text only")
    c.add_argument("--benchmark", required=True, choices=["vsi-bench", "cv-bench", "mmmu", "videomme"])
    c.add_argument("--in", dest="src", required=True)
    c.add_argument("--out", required=True)
    c.add_argument("--columns", default=None, help='JSON object remapping column names, e.g. \'{"ground_truth": "gt"}\'')
    e = sub.add_parser("export")
    e.add_argument("--run", required=True, help="--out directory of a finished `prune` run")
    e.add_argument("--to", required=True)
    e.add_argument("--data-file", default=None, help="the QA JSONL the run was made on: with --to-data, its surviving records are written out")
    e.add_argument("--to-data", default=None, help="debiased benchmark file: the records of --data-file whose id survived, unchanged")
    e.add_argument("--table", default=None, help="the ORIGINAL benchmark table `convert` read (parquet / json / jsonl / csv): with --to-table its surviving rows are written, all columns kept")
    e.add_argument("--to-table", default=None, help="debiased benchmark table (parquet if the name ends in .parquet and --table is parquet, else JSONL)")
    return ap


def apply_config(a, argv):
    """--config YAML: values for options NOT given on the command line (names as in HF TrainingArguments, underscores)."""
    if not getattr(a, "config", None):
        return a
    import yaml
    with open(a.config) as fh:
        conf = yaml.safe_load(fh) or {}
    given = {t.split("=")[0].lstrip("-").replace("-", "_") for t in argv if t.startswith("--")}
    for k, v in conf.items():
        k = k.replace("-", "_")
        if not hasattr(a, k):
            raise SystemExit(f"{a.config}: unknown option {k!r}")
        if k not in given:
            setattr(a, k, type(getattr(a, k))(v) if getattr(a, k) is not None else v)
    return a


def default_eos_ids(model_dir):
    """eos_token_id (an int or a list) of <model-dir>/generation_config.json, else of config.json; () when neither names one"""
    for name in ("generation_config.json", "config.json"):
        path = os.path.join(model_dir, name) if model_dir else None
        if path and os.path.exists(path):
            with open(path) as fh:
                e = json.load(fh).get("eos_token_id")
            if e is not None:
                return tuple(int(x) for x in (e if isinstance(e, (list, tuple)) else [e]))
    return ()


def parse_eos_ids(a):
    """--eos-ids / the YAML key eos_ids: "2,32000", a list, or an int; unset: the checkpoint's own"""
    e = getattr(a, "eos_ids", None)
    if e is None or e == "":
        return default_eos_ids(getattr(a, "model_dir", None))
    if isinstance(e, str):
        return tuple(int(x) for x in e.replace(",", " ").split())
    return tuple(int(x) for x in (e if isinstance(e, (list, tuple)) else [e]))


def default_baseline_id(a):
    """(id, where it came from) of the integrated-gradients baseline prompt when --attribute-baseline-id is not given: the tokenizer's pad id, else pad_token_id
    of the checkpoint's config, else its first eos id, else 0"""
    tok_file = getattr(a, "tokenizer", None) or (os.path.join(a.model_dir, "tokenizer.json") if getattr(a, "model_dir", None) else None)
    if tok_file and os.path.exists(tok_file):
        try:
            from tokenizers import Tokenizer
            pad = Tokenizer.from_file(tok_file).padding
            if pad and pad.get("pad_id") is not None:
                return int(pad["pad_id"]), "tokenizer pad id"
        except ImportError:
            pass
    for name in ("generation_config.json", "config.json"):
        path = os.path.join(a.model_dir, name) if getattr(a, "model_dir", None) else None
        if path and os.path.exists(path):
            with open(path) as fh:
                p = json.load(fh).get("pad_token_id")
            if p is not None:
                return int(p), f"pad_token_id of {name}"
    eos = default_eos_ids(getattr(a, "model_dir", None))
    if eos:
        return int(eos[0]), "eos id"
    return 0, "default"


def _args_to_train(a):
    from .trainer import TrainArgs
    gen = dict(generate=True, max_new_tokens=int(a.max_new_tokens), eos_ids=parse_eos_ids(a)) if getattr(a, "generate", False) else {}
    n_smp = int(getattr(a, "generate_samples", 0) or 0)
    if n_smp != 0:
        if not 1 <= n_smp <= 64:
            raise SystemExit("--generate-samples must be 1..64 draws (0: off)")
        t = float(getattr(a, "temperature", 1.0))
        if not 0.01 <= t <= 100.0:   # (a NaN fails both)
            raise SystemExit("--temperature must lie in [0.01, 100]")
        gen.update(sample_n=n_smp, temperature=t, sample_seed=int(getattr(a, "sample_seed", 0) or 0), max_new_tokens=int(a.max_new_tokens), eos_ids=parse_eos_ids(a))
    n_cand = int(getattr(a, "candidates", 0) or 0)
    if n_cand != 0:
        if not 1 <= n_cand <= 4096:
            raise SystemExit("--candidates must be 1..4096 answers (0: off)")
        gen.update(candidates=n_cand)
    if getattr(a, "attribute", False):
        if getattr(a, "dp", 1) > 1 or getattr(a, "layout", None) == "dp-stacked":
            raise SystemExit("--attribute is not available on the data-parallel layouts (--dp > 1, --layout dp-stacked)")
        if int(a.attribute_top) < 0:
            raise SystemExit("--attribute-top must be >= 0")
        gen.update(attribute=True, attribute_top=int(a.attribute_top))
    if int(getattr(a, "attribute_ig", 0) or 0) != 0:
        if getattr(a, "dp", 1) > 1 or getattr(a, "layout", None) == "dp-stacked":
            raise SystemExit("--attribute-ig is not available on the data-parallel layouts (--dp > 1, --layout dp-stacked)")
        if not 1 <= int(a.attribute_ig) <= 256:
            raise SystemExit("--attribute-ig must be 1..256 steps (0: off)")
        if int(a.attribute_top) < 0:
            raise SystemExit("--attribute-top must be >= 0")
        bid = getattr(a, "attribute_baseline_id", None)
        bid, a.attribute_baseline_source = (int(bid), "--attribute-baseline-id") if bid is not None else default_baseline_id(a)
        if bid < 0:
            raise SystemExit("--attribute-baseline-id must be a token id (>= 0)")
        gen.update(attribute_ig=int(a.attribute_ig), attribute_baseline_id=bid, attribute_top=int(a.attribute_top))
    elif getattr(a, "attribute_baseline_id", None) is not None:
        raise SystemExit("--attribute-baseline-id needs --attribute-ig STEPS")
    return TrainArgs(**gen, learning_rate=a.learning_rate, num_train_epochs=a.num_train_epochs, per_device_train_batch_size=a.per_device_train_batch_size,
                     warmup_steps=a.warmup_steps, weight_decay=a.weight_decay, max_grad_norm=a.max_grad_norm, seed=a.seed, lora_r=a.lora_r,
                     lora_alpha=a.lora_alpha, logging_steps=a.logging_steps, gradient_accumulation_steps=max(1, a.gradient_accumulation_steps))


def fold_layout(cfg, train_mode, k, rank, world, folds_per_gpu=0, stack=0):
    """(resident folds F, folds stacked per context S, contexts) of one rank. A full fine-tune owns its weights: one fold, one context.
    LoRA: this rank's share of the k folds, at most folds_per_gpu at a time, stacked up to three to a context (DESIGN.md sections 2 / 6,
    measured on the 8B shape: 2 folds 89 stacked vs 85 on two streams, 3 folds 100 vs 97, 4 as 2 + 2: 103, k = 5 as 3 + 2: 104,
    6 as 3 + 3: 107 QA-pairs/s); small bases are launch-bound and take deeper stacks (GPT-2-small: 3 + 2 folds 1615, 2 x 8 folds 2742)."""
    if train_mode == "full":
        return 1, 1, 1
    small = cfg["hidden_size"] <= 1536
    mine = len(range(rank, k, world))
    want = folds_per_gpu if folds_per_gpu > 0 else (16 if small else 6 if mine > 3 else 3)
    F = max(1, min(want, mine))
    S = max(1, min(stack if stack > 0 else (8 if small else 3), F, 8))
    return F, S, (F + S - 1) // S


def _make_ctx(a, targs, local_rank, rank=0, world=1, max_answer=4):
    from . import lib
    tied = False
    if a.model_dir:
        from . import io as TIO
        with open(os.path.join(a.model_dir, "config.json")) as fh:
            cfg = TIO.cfg_from_hf(json.load(fh))
        tied = cfg.pop("_tied", False)
    else:
        cfg = MODEL_SHAPES[a.model]
    bs = max(targs.per_device_train_batch_size, targs.per_device_eval_batch_size)
    L = max(128, a.max_len)
    gen_on = targs.generate or targs.sample_n > 0
    if gen_on:   # room for the generated tokens behind the longest prompt: RoPE table / wpe rows (max_tokens, sized from L below, grows with it)
        L += targs.max_new_tokens
    if a.layout == "dp-stacked":   # every rank hosts ALL k folds, laid out as one GPU would lay them out alone
        F, S, nctx = fold_layout(cfg, a.train_mode, a.k, 0, 1, a.folds_per_gpu or a.k, a.stack)
    else:
        F, S, nctx = (1, 1, 1) if a.dp > 1 else fold_layout(cfg, a.train_mode, a.k, rank, world, a.folds_per_gpu, a.stack)
    if gen_on and cfg.get("arch") == "gpt2" and a.max_len + targs.max_new_tokens > cfg["max_position"]:
        raise SystemExit(f"--generate / --generate-samples: --max-len {a.max_len} + --max-new-tokens {targs.max_new_tokens} exceeds the model's {cfg['max_position']} positions")
    draws = targs.per_device_eval_batch_size * S * targs.sample_n   # every draw of a held-out batch is a decode row and a head row (0 without --generate-samples)
    if targs.candidates > 0:
        # every candidate token of a held-out batch is a head row, all but the candidates' last tokens are token rows of the extend pass: N + 1 candidates of
        # at most max_answer (<= TST_CAND_MAX_LEN) tokens per sample; room for a candidate behind the longest prompt (0 without --candidates)
        draws = max(draws, targs.per_device_eval_batch_size * S * (targs.candidates + 1) * min(max(1, max_answer), lib.CAND_MAX_LEN))
        L = max(L, max(128, a.max_len) + lib.CAND_MAX_LEN)
        if cfg.get("arch") == "gpt2" and a.max_len + lib.CAND_MAX_LEN > cfg["max_position"]:
            raise SystemExit(f"--candidates: --max-len {a.max_len} + {lib.CAND_MAX_LEN} candidate tokens exceeds the model's {cfg['max_position']} positions")
    ctx = lib.Context(cfg, device=local_rank, max_tokens=max(bs * L * S, draws), max_seqs=max(bs * S, draws), max_labelled=max(max(4, max_answer) * bs * S, draws),
                      max_position=min(L, cfg["max_position"]) if cfg.get("arch") == "gpt2" else L, lora_r=targs.lora_r,
                      lora_alpha=targs.lora_alpha, lora_targets=targs.lora_targets, beta1=targs.adam_beta1, beta2=targs.adam_beta2,
                      eps=targs.adam_epsilon, weight_decay=targs.weight_decay, max_grad_norm=targs.max_grad_norm, train_mode=a.train_mode, n_stack=S)
    if a.model_dir:
        TIO.load_weights(ctx, a.model_dir, tied)
    else:
        ctx.init_random(seed=a.weights_seed, std=0.02)
    if "TST_BIG_TILE" not in os.environ:
        lib.set_tile_policy(1 if nctx > 1 else 3)   # 256x256 tiles; split-K only when one stream has the GPU to itself
    ctxs = [ctx] + [ctx.fork() for _ in range(nctx - 1)]
    return ctxs, cfg


def main(argv=None):
    a = build_parser().parse_args(argv)
    a = apply_config(a, list(sys.argv[1:] if argv is None else argv))
    rank, world, local_rank = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    if a.cmd == "rf":
        from . import diagnose as DG
        from . import rf as RF
        with open(a.data_file) as fh:
            recs = [json.loads(line) for line in fh if line.strip()]
        scores, imp, nm = RF.diagnose_rf(recs, a.k, a.seed, a.n_estimators, return_names=True)
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "scores_rf.jsonl"), "w") as fh:
            for rec in scores:
                fh.write(json.dumps(rec) + "\n")
        top = [dict(feature=nm[i], importance=float(imp[i])) for i in np.argsort(-imp)[:a.top]]
        with open(os.path.join(a.out, "rf_importances.json"), "w") as fh:
            json.dump(top, fh)
        print(json.dumps(dict(DG.summarize(scores), top_features=[t["feature"] for t in top[:3]])))
        return 0
    if a.cmd == "convert":
        from . import benchmarks as BM
        n, n_mc = BM.convert(a.benchmark, a.src, a.out, json.loads(a.columns) if a.columns else None)
        print(f"wrote {a.out}: {n} text-only QA records ({n_mc} multiple-choice, {n - n_mc} free-form)")
        return 0
    if a.cmd == "export":
        from . import ibp
        with open(os.path.join(a.run, "ibp_final.json")) as fh:
            fin = json.load(fh)
        ibp.export_debiased(a.to, fin["surviving"], fin["history"], meta=fin.get("meta"))
        print(f"wrote {a.to}: {len(fin['surviving'])} samples kept")
        if a.data_file and a.to_data:
            kept, dropped = ibp.filter_records(a.data_file, a.to_data, fin["surviving"])
            print(f"wrote {a.to_data}: {kept} records kept, {dropped} pruned")
        if a.table and a.to_table:
            from . import benchmarks as BM
            kept, dropped = BM.filter_table(a.table, a.to_table, fin["surviving"])
            print(f"wrote {a.to_table}: {kept} rows kept, {dropped} pruned")
        return 0
    from . import data as D
    from . import diagnose as DG
    from . import ibp
    targs = _args_to_train(a)
    samples = None
    if a.data_file:   # real benchmark records: tokenised here, before the context exists (option ids go into the training arguments)
        from . import io as TIO
        tok = a.tokenizer or (os.path.join(a.model_dir, "tokenizer.json") if a.model_dir else None)
        if not tok:
            raise SystemExit("--data-file needs --tokenizer (or --model-dir with a tokenizer.json)")
        samples, opt_ids = TIO.load_qa_jsonl(a.data_file, tok, max_len=a.max_len)
        targs.option_ids = tuple(opt_ids)
    decode = None
    if targs.generate or targs.attribute_ig > 0 or targs.sample_n > 0 or targs.candidates > 0:
        tok_file = a.tokenizer or (os.path.join(a.model_dir, "tokenizer.json") if a.model_dir else None)
        if tok_file and os.path.exists(tok_file):
            from tokenizers import Tokenizer
            _tk = Tokenizer.from_file(tok_file)
            decode = lambda ids: _tk.decode(list(ids))   # noqa: E731
    max_answer = max((len(x.ids) - x.n_prompt for x in samples), default=4) if samples else 4
    ctx, cfg = _make_ctx(a, targs, local_rank, rank, world, max_answer)   # a list: the root context and its resident forks
    if targs.attribute_ig > 0 and targs.attribute_baseline_id >= cfg["vocab_size"]:
        raise SystemExit(f"--attribute-baseline-id {targs.attribute_baseline_id} lies outside the model's vocabulary ({cfg['vocab_size']})")
    if samples is None:
        samples = D.synth_vsi(a.n_samples, cfg["vocab_size"])
    by_id = {s.sid: s for s in samples}
    # what a resumed run must share with the shards already on disk (tst.diagnose.run_fingerprint adds hyper-parameters, k and the samples)
    identity = dict(model=a.model_dir or a.model, weights_seed=None if a.model_dir else a.weights_seed, train_mode=a.train_mode, data=a.data_file or a.data,
                    lora_r=a.lora_r, lora_alpha=a.lora_alpha, dp=a.dp)
    os.makedirs(a.out, exist_ok=True)
    log_fh = open(os.path.join(a.out, f"train_log.rank{rank}.jsonl" if world > 1 else "train_log.jsonl"), "a")

    def log(rec):
        log_fh.write(json.dumps(rec) + "\n")
        log_fh.flush()

    if targs.attribute_ig > 0:   # the run's metadata: which baseline prompt the attr_ig of its records was walked from
        log(dict(event="attribute_ig", steps=targs.attribute_ig, baseline_id=targs.attribute_baseline_id, baseline_from=a.attribute_baseline_source))
    if a.layout == "dp-stacked":
        if a.train_mode != "lora" or a.dp > 1:
            raise SystemExit("--layout dp-stacked is the LoRA layout and excludes --dp")
        from . import ddp
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
            ddp.init_stacked_groups(ctx, rank, world)
        else:
            for c in ctx:
                c.dp_init(c.dp_unique_id(), 1, 0)
        identity["layout"] = "dp-stacked"
        run_diag = lambda smp, rnd: DG.diagnose_dp_stacked(ctx, smp, a.k, targs, rank, world, rnd, a.out, log=log, identity=identity, decode=decode)   # noqa: E731
    elif a.dp > 1:
        # the fold group's communicator: the 128-byte RCCL id travels over a gloo group (CPU); libtst_hip is loaded before torch
        # (the contexts above), so the collectives run on the ROCm runtime the kernels were built against
        import torch.distributed as dist
        from . import ddp
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        g, _, dp_rank, members = ddp.dp_layout(rank, world, a.dp)
        groups = ddp.make_groups(world, a.dp)
        ddp.init_fold_group(ctx[0], groups[g], dp_rank, a.dp, members)
        if a.dp_transport == "bf16":
            ctx[0].dp_set_transport("bf16")
        identity["dp_mode"] = a.dp_mode
        run_diag = lambda smp, rnd: DG.diagnose_dp(ctx[0], smp, a.k, targs, rank, world, a.dp, rnd, a.out, log=log, identity=identity, mode=a.dp_mode, decode=decode)   # noqa: E731
    else:
        run_diag = lambda smp, rnd: DG.diagnose(ctx, smp, a.k, targs, rank, world, rnd, a.out, log=log, identity=identity, decode=decode)   # noqa: E731
    if a.cmd == "diagnose":
        recs, stats = run_diag(samples, 0)
        for st in stats:
            print(json.dumps(dict(rank=rank, **st)), flush=True)
        if rank == 0:
            allr = DG.gather_round(a.out, 0, a.k, len(samples), timeout_s=3600.0 if world > 1 else 0.0)
            with open(os.path.join(a.out, "scores.jsonl"), "w") as fh:
                for r in allr:
                    fh.write(json.dumps(r) + "\n")
            print(json.dumps(DG.summarize(allr)))
        return 0
    # prune: IBP rounds, each a fresh k-fold sweep over the survivors
    def diag(alive_ids, rnd):
        sub = [by_id[i] for i in alive_ids]
        run_diag(sub, rnd)
        return DG.gather_round(a.out, rnd, a.k, len(sub), timeout_s=3600.0 if world > 1 else 0.0)
    alive, hist = ibp.iterative_bias_pruning(diag, [s.sid for s in samples], a.rounds, a.tau, None, a.prune_frac, 1, a.out if rank == 0 else None)
    if rank == 0:
        with open(os.path.join(a.out, "ibp_final.json"), "w") as fh:
            json.dump(dict(surviving=alive, history=hist, meta=dict(model=a.model, k=a.k, rounds=a.rounds, tau=a.tau)), fh)
        print(json.dumps(hist))
    return 0


if __name__ == "__main__":
    sys.exit(main())
