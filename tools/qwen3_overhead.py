#!/usr/bin/env python3
"""What the Qwen3 head norm costs end to end: ms per stacked LoRA step of a 5-fold sweep at the Qwen3-8B shape, once as TST_ARCH_QWEN3 and once as
TST_ARCH_LLAMA with identical widths (the same model without q_norm / k_norm), same build, same process, same batches.

    python3 tools/qwen3_overhead.py [--steps 8] [--rounds 5] [--layers 36] [--out profiles/qwen3_head_norm.txt]

One stacked context per arm (5 slots, 16 QA pairs per slot and step: the benchmark's micro-batch), random-initialised base, tile policy 3 (one stream per GPU)
as bench.py runs a single stacked context. Discipline as in bench.py: an untimed warm-up of two steps per arm, then `rounds` timed windows of `steps` steps per
arm, the arms ALTERNATING window by window; a window is a host clock around asynchronous steps that ends in a device synchronise. Reported: the median window
of each arm in ms per step, its min / max (the run-to-run spread), and the ratio of the medians."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib  # noqa: E402


def stacked_batch(samples, k, per_slot):
    ids, labels, cu, slots, off = [], [], [0], [], 0
    for s in range(k):
        i, l, c = D.collate(samples[s * per_slot:(s + 1) * per_slot])
        ids.append(i)
        labels.append(l)
        cu += [off + int(x) for x in c[1:]]
        slots += [s] * (len(c) - 1)
        off += len(i)
    return np.concatenate(ids).astype(np.int32), np.concatenate(labels).astype(np.int32), np.array(cu, np.int32), np.array(slots, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K, BS = args.k, 16
    q3 = dict(cli.MODEL_SHAPES["qwen3-8b"], num_layers=args.layers)
    arms = {"qwen3": q3, "llama-widths": {k: v for k, v in q3.items() if k != "qk_norm"}}
    lib.set_tile_policy(3)
    n_batches = 4
    batches = [stacked_batch(D.synth_vsi(K * BS, q3["vocab_size"], seed=100 + b), K, BS) for b in range(n_batches)]
    ctxs = {}
    for name, cfg in arms.items():
        c = lib.Context(cfg, max_tokens=BS * 128 * K, max_seqs=BS * K, max_labelled=4 * BS * K, max_position=128, lora_r=16, lora_alpha=32.0, n_stack=K)
        c.init_random(seed=0, std=0.02)
        for s in range(K):
            c.select_slot(s)
            c.reset_trainable(seed=s + 1)
        ctxs[name] = c
    lrs = [5e-5] * K

    def window(c, n):
        c.sync()
        t0 = time.perf_counter()
        for i in range(n):
            c.train_step_stacked_async(*batches[i % n_batches], lrs)
        c.sync()
        return (time.perf_counter() - t0) / n * 1e3

    for c in ctxs.values():
        window(c, 2)
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, c in ctxs.items():
            times[name].append(window(c, args.steps))
    for name, c in ctxs.items():
        loss, gn = c.fetch_metrics_stacked()
        assert np.isfinite(loss).all() and (gn > 0).all(), (name, loss, gn)
    tok = int(np.mean([len(b[0]) for b in batches]))
    med = {name: float(np.median(t)) for name, t in times.items()}
    lines = [f"stacked LoRA step, {K} folds x {BS} QA pairs (~{tok} packed tokens), Qwen3-8B widths, {args.layers} layers, r = 16, tile policy 3; "
             f"{args.rounds} windows of {args.steps} steps per arm, arms alternating"]
    for name, t in times.items():
        lines.append(f"  {name:13s} ms_per_step median {med[name]:8.2f}  min {min(t):8.2f}  max {max(t):8.2f}   windows: " + " ".join(f"{x:.2f}" for x in t))
    lines.append(f"  ratio qwen3 / llama-widths = {med['qwen3'] / med['llama-widths']:.4f}  (head norm: {med['qwen3'] - med['llama-widths']:+.2f} ms per step, "
                 f"{(med['qwen3'] - med['llama-widths']) / args.layers * 1e3:+.1f} us per layer, forward + backward)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
