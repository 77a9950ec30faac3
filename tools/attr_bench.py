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
rate 1 / prompt length and the model's accuracy on those samples. Reported, not asserted: no reference value exists."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib, score as S  # noqa: E402
from tst.trainer import TrainArgs, attribute_heldout, fine_tune, score_heldout  # noqa: E402


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
    ctx.close()
    top_n = np.array([int(np.argmax(x["gnorm"])) for x in attr])
    top_x = np.array([int(np.argmax(np.abs(x["gxi"]))) for x in attr])
    share = np.array([float(x["share"][5]) for x in attr])
    return dict(model=a.hit_model, train=a.hit_train, heldout=a.hit_heldout, epochs=a.hit_epochs, lr=a.hit_lr, planted_position=5, accuracy=float(np.mean(correct)),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_bench.json"))
    a = ap.parse_args()
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
