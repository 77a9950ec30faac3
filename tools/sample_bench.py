#!/usr/bin/env python3
"""Sampled generation on a shared prompt cache against what a caller would have to do without it: the prompts replicated n times in the batch.

    python3 tools/sample_bench.py [--model llama3-8b] [--layers 8] [--seqs 64] [--samples 8] [--max-new 8] [--rounds 5] [--parent-lib DIR] [--out FILE.json]

Run it on a card with nothing else on it. One LoRA context (r = 16), random-initialised base, tile policy 3, the model's widths with --layers decoder layers
(the stash of a context grows with max_tokens x layers, and arm B needs n times the prompts' tokens). Prompts: the synthetic VSI length distribution
(tst.data.synth_vsi), as bench.py.
  arm A   Context.sample(prompts, n_samples = n): one prefill over the S prompts, S n decode rows on the shared prefix
  arm B   Context.sample(prompts repeated n times, n_samples = 1): the same S n draws, every one with a prefill and cache rows of its own
Method as bench.py / tools/gen_bench.py: an untimed warm-up of each arm, then `rounds` windows per arm, the arms ALTERNATING; a window is a host clock around
work that ends in a device synchronise. The prefill / decode split of each arm comes from the library's HIP events (tst_profile_intervals: every contraction
launch of ONE generation is bracketed on the stream; a pass ends with the head's contraction; prefill = first start to the end of pass 0's head, decode step =
the mean of the other passes, gaps between passes included). sample_rows alone beside logit_rows (next_token, a launch of one workgroup, is not in the
figure): the lab hooks on S n rows of the model's padded vocabulary, a host clock around 50 launches that end in a device synchronise, kernels alternating.
--parent-lib DIR (a directory holding libtst_hip.so built from the parent commit): the held-out scoring pass (score_rows on the same samples with their
answers) in a context of THAT library and in a context of this one, same process, windows alternating -- a run without the new flag must cost what it cost.
The result is one JSON object (printed; --out FILE.json writes it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib  # noqa: E402
from tst.score import sample_seeds  # noqa: E402
from tst.trainer import collate_prompts  # noqa: E402


def stats(t):
    return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), windows=[round(float(x), 3) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(cli.MODEL_SHAPES))
    ap.add_argument("--layers", type=int, default=8, help="0 = the model's own")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-new", type=int, default=8)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = dict(cli.MODEL_SHAPES[a.model])
    if a.layers:
        cfg["num_layers"] = a.layers
    S, N, M = a.seqs, a.samples, a.max_new
    R = S * N
    samples = D.synth_vsi(S, cfg["vocab_size"], seed=100)
    pid, pcu = collate_prompts(samples)
    plens = np.diff(pcu)
    rep = [x for x in samples for _ in range(N)]
    rid, rcu = collate_prompts(rep)
    seeds = sample_seeds(0, np.arange(S))
    rseeds = sample_seeds(1, np.arange(R))
    lib.set_tile_policy(3)
    dims = dict(max_tokens=int(rcu[-1]) + 64, max_seqs=R, max_labelled=max(4 * S, R), max_position=a.max_len + M, lora_r=16, lora_alpha=32.0)
    ctx = lib.Context(cfg, **dims)
    ctx.init_random(seed=0, std=0.02)
    ctx.reset_trainable(seed=1)

    arms = dict(A=lambda: ctx.sample(pid, pcu, M, N, 1.0, seeds), B=lambda: ctx.sample(rid, rcu, M, 1, 1.0, rseeds))

    def window(run):
        ctx.sync()
        t0 = time.perf_counter()
        run()
        return (time.perf_counter() - t0) * 1e3

    for run in arms.values():
        window(run)
    t = dict(A=[], B=[])
    for _ in range(a.rounds):
        for k, run in arms.items():
            t[k].append(window(run))
    res = dict(model=a.model, layers=cfg["num_layers"], prompts=S, prompt_tokens=int(plens.sum()), longest=int(plens.max()), n_samples=N, max_new=M, rounds=a.rounds,
               arm_A_ms=stats(t["A"]), arm_B_ms=stats(t["B"]), ratio_B_over_A=float(np.median(t["B"]) / np.median(t["A"])))
    # prefill / decode split from HIP events: the contraction launches of one generation, cut at the head's contractions
    vp = -(-cfg["vocab_size"] // 64) * 64
    for k, run, head_rows in (("A", arms["A"], (S, R)), ("B", arms["B"], (R,))):
        pre, dec = [], []
        for _ in range(a.rounds):
            ctx.profile_enable(3)
            run()
            st, en, fl = ctx.profile_intervals(ctx, -1)
            ctx.profile_read(-1, reset=True)
            ctx.profile_enable(0)
            heads = np.flatnonzero(np.isin(fl, [2.0 * r * vp * cfg["hidden_size"] for r in head_rows]))
            assert len(heads) == M, (len(heads), M)
            pre.append(float(en[heads[0]] - st[0]))
            if M > 1:
                dec.append(float(en[heads[-1]] - st[heads[0] + 1]) / (M - 1))
        res[f"arm_{k}_prefill_ms"] = stats(pre)
        if dec:
            res[f"arm_{k}_decode_step_ms"] = stats(dec)
    # sample_rows alone beside logit_rows, on R rows of the padded vocabulary
    lab = lib.load_lab()
    V = cfg["vocab_size"]
    lg_ = lib.dev_f32((1.5 * np.random.default_rng(0).standard_normal((R, vp))).astype(np.float32))
    geo = np.concatenate([[R, M, N]] + [[0, 64, 0]] * R).astype(np.int32)
    geo_, seeds_, tgt_ = lib.DevBuf(geo), lib.DevBuf(np.arange(2 * S, dtype=np.int32)), lib.DevBuf(np.zeros(R, np.int32))
    tok_, lp_, st_ = lib.DevBuf(nbytes=R * M * 4), lib.DevBuf(nbytes=R * M * 4), lib.DevBuf(nbytes=R * 16)
    i1_, i2_, i3_ = (lib.DevBuf(nbytes=R * 4) for _ in range(3))
    kern = dict(sample_rows=lambda: lab.tst_k_sample_rows(lg_.ptr, vp, V, geo_.ptr, seeds_.ptr, R, 1, 1.0, tok_.ptr, lp_.ptr, i1_.ptr, i2_.ptr, i3_.ptr),
                logit_rows=lambda: lab.tst_k_logit_rows(lg_.ptr, vp, tgt_.ptr, R, V, st_.ptr, None, 0, 0.0, None, 0, None))

    def kwindow(fn, n=50):
        lab.tst_dev_sync()
        t0 = time.perf_counter()
        for _ in range(n):
            assert fn() == 0
        lab.tst_dev_sync()
        return (time.perf_counter() - t0) * 1e6 / n

    for fn in kern.values():
        kwindow(fn, 5)
    tk = {k: [] for k in kern}
    for _ in range(a.rounds):
        for k, fn in kern.items():
            tk[k].append(kwindow(fn))
    res["kernel_rows"], res["kernel_vocab_padded"] = R, vp
    for k in kern:
        res[f"{k}_us"] = stats(tk[k])
    if a.parent_lib:
        import ctypes as C
        pl = C.CDLL(os.path.join(a.parent_lib, "libtst_hip.so"))
        for name, (rs, args) in lib.SIGNATURES.items():
            if hasattr(pl, name):
                fn = getattr(pl, name)
                fn.restype, fn.argtypes = rs, args
        pl.tst_set_tile_policy(3)
        mine, lib._lib = lib._lib, pl
        try:
            pctx = lib.Context(cfg, **dims)
        finally:
            lib._lib = mine
        pctx.init_random(seed=0, std=0.02)
        pctx.reset_trainable(seed=1)
        sids, slabels, scu = D.collate(samples)

        def score_window(c, n=4):
            c.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                c.score_rows_async(sids, slabels, scu, ())
                c.score_rows_fetch()
            return (time.perf_counter() - t0) * 1e3 / n

        score_window(pctx, 2)
        score_window(ctx, 2)
        tp, tc = [], []
        for _ in range(a.rounds):
            tp.append(score_window(pctx))
            tc.append(score_window(ctx))
        res["score_parent_ms"], res["score_this_ms"] = stats(tp), stats(tc)
        res["score_ratio_this_over_parent"] = float(np.median(tc) / np.median(tp))
        pctx.close()
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
