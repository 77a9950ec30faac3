#!/usr/bin/env python3
"""Token attribution (tst_attribute_async): what it costs beside a training forward + backward of the same batch, and whether it finds a planted token.

    python3 tools/attr_bench.py [--model llama3-8b] [--layers 0] [--pairs 16] [--rounds 7] [--skip-cost] [--skip-hits] [--out profiles/attr_bench.json]

Run it on a card with nothing else on it.
Cost: one LoRA context (r = 16, random-initialised base, tile policy 3) and one held-out batch of `pairs` QA pairs of the synthetic VSI length distribution.
Two arms on the same build, ALTERNATING: Context.attribute (forward, backward seeded with log s(x) down to the embedding output, per-token reduction, fetch) and
Context.forward_backward (the training forward + backward; no optimizer step). Every window is bracketed by HIP events on the context's stream (a torch stream
handed to tst_set_stream; torch is used for the stream and the events only, and is initialised before the library is loaded); an untimed warm-up of both arms comes first. Reported: median / min / max ms per arm
and the ratio of the medians.
Hit rate: a small LoRA model (--hit-model, default tiny; the recipe of tests/test_diagnostic_gpu.py) is fine-tuned on synthetic 4-way multiple-choice samples in
which ONE prompt token (position 5) fixes the answer, then fresh samples of the same kind are attributed; reported is how often that token is the prompt's top-1 by gnorm (and by |gxi|), beside the chance
rate 1 / prompt length and the model's accuracy on those samples. Reported, not asserted: no reference value exists.

    python3 tools/attr_bench.py --ig [--ig-steps 16] [--out profiles/attr_ig_bench.json]

The same two measurements for integrated gradients (tst_attribute_ig_async), same harness. Cost: Context.attribute_ig with --ig-steps steps (prompt tokens walked
from token id 0, answer tokens kept) against --ig-steps calls of Context.attribute on the same batch, arms alternating; expected ratio (m + 2/3) / m -- the two
passes without a backward cost about a third of a forward + backward each. Hit rate: on the same trained model, how often the planted token is the prompt's top-1
by |ig|, beside gnorm's and |gxi|'s rates from the same run, and the mean completeness gap |delta| / |log s - log s_base| at --ig-steps and twice as many."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib, score as S  # noqa: E402
from tst.trainer import TrainArgs, attribute_heldout, attribute_ig_heldout, fine_tune, score_heldout  # noqa: E402


def cost(a):
    import torch
    cfg = dict(cli.MODEL_SHAPES[a.model])
    if a.layers:
        cfg["num_layers"] = a.layers
    samples = D.synth_vsi(a.pairs, cfg["vocab_size"], seed=100)
    ids, labels, cu = D.collate(samples)
    kinds = S.attribution_kinds(samples)
    lib.set_tile_policy(3)
    ctx = lib.Context(cfg, max_tokens=a.pairs * 128, max_seqs=a.pairs, max_labelled=4 * a.pairs, max_position=128, lora_r=16, lora_alpha=32.0)
    ctx.init_random(seed=0, std=0.02)
    ctx.reset_trainable(seed=1)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    arms = dict(attribute=lambda: ctx.attribute(ids, labels, cu, kinds, D.OPTION_IDS), forward_backward=lambda: ctx.forward_backward(ids, labels, cu))
    if a.ig:
        base = S.ig_baseline_ids(samples, 0)
        arms = {"attribute_ig": lambda: ctx.attribute_ig(ids, labels, cu, base, a.ig_steps, kinds, D.OPTION_IDS),
                "m_x_attribute": lambda: [ctx.attribute(ids, labels, cu, kinds, D.OPTION_IDS) for _ in range(a.ig_steps)]}
    for fn in arms.values():
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn))
    ctx.set_stream(None)
    ctx.close()
    res = dict(model=a.model, layers=cfg["num_layers"], pairs=a.pairs, tokens=int(len(ids)), labelled=int((labels != -100).sum()), rounds=a.rounds, lora_r=16, tile_policy=3,
               method="HIP events on the context's stream around each call, arms alternating, 2 untimed warm-up calls per arm",
               ms={k: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), windows=[round(x, 3) for x in t]) for k, t in times.items()})
    if a.ig:
        res["ig_steps"] = a.ig_steps
        res["ratio_attribute_ig_over_m_x_attribute"] = res["ms"]["attribute_ig"]["median"] / res["ms"]["m_x_attribute"]["median"]
        res["expected_ratio"] = (a.ig_steps + 2.0 / 3.0) / a.ig_steps
    else:
        res["ratio_attribute_over_forward_backward"] = res["ms"]["attribute"]["median"] / res["ms"]["forward_backward"]["median"]
    return res


def hits(a):
    cfg = dict(cli.MODEL_SHAPES[a.hit_model])
    args = TrainArgs(num_train_epochs=a.hit_epochs, per_device_train_batch_size=16, per_device_eval_batch_size=16, learning_rate=a.hit_lr, logging_steps=0, attribute=True)
    # 4-way multiple choice only: the option letter is a function of prompt token 5 and of nothing else (chance accuracy 0.25)
    mca = lambda n, seed: [x for x in D.synth_vsi(3 * n, cfg["vocab_size"], seed=seed, shortcut_frac=1.0) if x.kind == "mca"][:n]
    train, held = mca(a.hit_train, 11), mca(a.hit_heldout, 12)
    ctx = lib.Context(cfg, max_tokens=16 * 128, max_seqs=16, max_labelled=64, max_position=128, lora_r=args.lora_r, lora_alpha=args.lora_alpha)
    ctx.init_random(seed=0, std=0.05)
    fine_tune(ctx, train, args)
    _, _, correct = score_heldout(ctx, held, args)
    attr = attribute_heldout(ctx, held, args)
    igs = {}
    if a.ig:
        for m in (a.ig_steps, 2 * a.ig_steps):
            args.attribute_ig, args.attribute_baseline_id = m, 0
            igs[m] = attribute_ig_heldout(ctx, held, args)
    ctx.close()
    top_n = np.array([int(np.argmax(x["gnorm"])) for x in attr])
    top_x = np.array([int(np.argmax(np.abs(x["gxi"]))) for x in attr])
    share = np.array([float(x["share"][5]) for x in attr])
    extra = {}
    if a.ig:
        top_i = np.array([int(np.argmax(np.abs(x["ig"]))) for x in igs[a.ig_steps]])
        extra = dict(baseline_id=0, top1_by_abs_ig=float((top_i == 5).mean()),
                     mean_ig_of_planted_token=float(np.mean([x["ig"][5] for x in igs[a.ig_steps]])),
                     mean_abs_delta_over_abs_dJ={str(m): float(np.mean([abs(x["delta"]) / max(abs(x["log_s"] - x["log_s_base"]), 1e-12) for x in v])) for m, v in igs.items()},
                     median_abs_delta_over_abs_dJ={str(m): float(np.median([abs(x["delta"]) / max(abs(x["log_s"] - x["log_s_base"]), 1e-12) for x in v])) for m, v in igs.items()},
                     mean_abs_dJ=float(np.mean([abs(x["log_s"] - x["log_s_base"]) for x in igs[a.ig_steps]])))
    return dict(**extra, model=a.hit_model, train=a.hit_train, heldout=a.hit_heldout, epochs=a.hit_epochs, lr=a.hit_lr, planted_position=5, accuracy=float(np.mean(correct)),
                top1_by_gnorm=float((top_n == 5).mean()), top1_by_abs_gxi=float((top_x == 5).mean()), mean_share_of_planted_token=float(share.mean()),
                chance=float(np.mean([1.0 / s.n_prompt for s in held])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(cli.MODEL_SHAPES))
    ap.add_argument("--layers", type=int, default=0, help="0 = the model's own")
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hit-model", default="tiny", choices=sorted(cli.MODEL_SHAPES))
    ap.add_argument("--hit-train", type=int, default=1600)
    ap.add_argument("--hit-heldout", type=int, default=128)
    ap.add_argument("--hit-epochs", type=int, default=10)
    ap.add_argument("--hit-lr", type=float, default=2e-3)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-hits", action="store_true")
    ap.add_argument("--ig", action="store_true", help="measure integrated gradients (Context.attribute_ig) instead; default --out profiles/attr_ig_bench.json")
    ap.add_argument("--ig-steps", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "attr_ig_bench.json" if a.ig else "attr_bench.json")
    if not a.skip_cost:
        # torch supplies the stream and the events of the cost measurement; its HIP runtime has to be live BEFORE libtst_hip.so is loaded
        # (tests/test_torch_coexist_gpu.py: the library then runs on the runtime torch loaded)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("attr_bench.py measures on the GPU: torch sees no device")
        torch.cuda.init()
    if lib.device_count() < 1:
        raise SystemExit("attr_bench.py measures on the GPU: no device is visible")
    res = {}
    if not a.skip_hits:
        res["planted_token"] = hits(a)
        print(json.dumps(res["planted_token"]))
    if not a.skip_cost:
        res["cost"] = cost(a)
        print(json.dumps(res["cost"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
