#!/usr/bin/env python3
"""Greedy generation with the KV cache against the only alternative without it: max_new full forward_logits passes over the growing batch.

    python3 tools/gen_bench.py [--model llama3-8b] [--layers 32] [--seqs 64] [--max-new 8] [--rounds 5] [--stack 1|3] [--keys 0] [--parent-lib DIR] [--out FILE]

Run it on a card with nothing else on it. One LoRA context (r = 16; --stack 3: a 3-slot stacked context, the prompts dealt to the slots in order),
random-initialised base, tile policy 3. Prompts: the synthetic VSI length distribution (tst.data.synth_vsi), or --keys N: every prompt N tokens long
(the 64 x 1024-key batch of the attn_decode measurement; needs --max-len). Method as bench.py: an untimed warm-up of each arm, then `rounds` windows per
arm, the arms ALTERNATING; a window is a host clock around work that ends in a device synchronise. Reported per arm: median / min / max ms. The split of a
generation into prefill and mean decode step comes from the library's HIP events (tst_profile_intervals: every contraction launch of ONE generation is
bracketed on the stream; a pass ends with the head's contraction, the only launch of its size;
prefill = first start to last end of pass 0, decode step = the mean of the other passes, gaps between passes included).
--parent-lib DIR (a directory holding libtst_hip.so built from the parent commit): the held-out scoring pass (score_rows on the same samples with their
answers) in a context of THAT library and in a context of this one, same process, windows alternating -- a run without --generate must cost what it cost. attn_decode alone: run this script under `rocprofv3 --kernel-trace --stats -- python3 tools/gen_bench.py ...`
in a run of its own and read the attn_decode_kernel row; K + V bytes of one decode step are printed here for the division."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib  # noqa: E402
from tst.trainer import collate_prompts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(cli.MODEL_SHAPES))
    ap.add_argument("--layers", type=int, default=0, help="0 = the model's own")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--max-new", type=int, default=8)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--keys", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stack", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = dict(cli.MODEL_SHAPES[a.model])
    if a.layers:
        cfg["num_layers"] = a.layers
    S, M, K = a.seqs, a.max_new, max(1, a.stack)
    if a.keys:
        rng = np.random.default_rng(1)
        samples = [D.Sample(i, rng.integers(D.FIRST_FREE_ID, cfg["vocab_size"], a.keys + 1).astype(np.int32), a.keys, "na", -1) for i in range(S)]
    else:
        samples = D.synth_vsi(S, cfg["vocab_size"], seed=100)
    max_len = max(a.max_len, a.keys + 1)
    lib.set_tile_policy(3)
    ctx = lib.Context(cfg, max_tokens=S * (max_len + M), max_seqs=S, max_labelled=max(4 * S, S * M), max_position=max_len + M, lora_r=16, lora_alpha=32.0, n_stack=K)
    ctx.init_random(seed=0, std=0.02)
    for s in range(K):
        ctx.select_slot(s)
        ctx.reset_trainable(seed=s + 1)
    ctx.select_slot(0)
    slots = (np.arange(S) * K // S).astype(np.int32) if K > 1 else None
    pid, pcu = collate_prompts(samples)
    plens = np.diff(pcu)

    def gen_window():
        ctx.sync()
        t0 = time.perf_counter()
        tok, _, _ = ctx.generate(pid, pcu, M, (), slots)
        return (time.perf_counter() - t0) * 1e3, tok

    def uncached_window():
        """the parent commit's way to M greedy tokens: M forward_logits passes over the growing batch"""
        seqs = [list(map(int, pid[pcu[i]:pcu[i + 1]])) for i in range(S)]
        ctx.sync()
        t0 = time.perf_counter()
        toks = []
        for _ in range(M):
            ids = np.concatenate([np.asarray(x, np.int32) for x in seqs])
            cu = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int32)
            lg = ctx.forward_logits(ids, cu, cu[1:] - 1, seq_slot=slots)
            t = lg.argmax(-1)
            toks.append(t)
            for i in range(S):
                seqs[i].append(int(t[i]))
        return (time.perf_counter() - t0) * 1e3, np.stack(toks, 1)

    def make_parent_ctx():
        """a context of the parent commit's library beside this one's (the entry points both have; same configuration, same seeds)"""
        import ctypes as C
        pl = C.CDLL(os.path.join(a.parent_lib, "libtst_hip.so"))
        for name, (res, args) in lib.SIGNATURES.items():
            if hasattr(pl, name):
                fn = getattr(pl, name)
                fn.restype, fn.argtypes = res, args
        pl.tst_set_tile_policy(3)
        mine, lib._lib = lib._lib, pl
        try:
            c = lib.Context(cfg, max_tokens=S * (max_len + M), max_seqs=S, max_labelled=max(4 * S, S * M), max_position=max_len + M, lora_r=16, lora_alpha=32.0, n_stack=K)
        finally:
            lib._lib = mine
        c.init_random(seed=0, std=0.02)
        for sl in range(K):
            c.select_slot(sl)
            c.reset_trainable(seed=sl + 1)
        c.select_slot(0)
        return c

    sids, slabels, scu = D.collate(samples)

    def score_window(c, n=4):
        c.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            c.score_rows_async(sids, slabels, scu, (), slots)
            c.score_rows_fetch()
        return (time.perf_counter() - t0) * 1e3 / n

    lines = [f"{a.model} widths, {cfg['num_layers']} layers, LoRA r = 16, {K}-slot context, {S} prompts ({int(plens.sum())} tokens, longest {int(plens.max())}), "
             f"max_new = {M}, tile policy 3; {a.rounds} windows per arm, arms alternating"]
    gen_window()
    uncached_window()
    tg, tu = [], []
    for _ in range(a.rounds):
        ms, tok_g = gen_window()
        tg.append(ms)
        ms, tok_u = uncached_window()
        tu.append(ms)
    agree = float((tok_g == tok_u).mean())
    for name, t in (("generate (KV cache)", tg), (f"{M} x forward_logits", tu)):
        lines.append(f"  {name:22s} ms median {np.median(t):9.2f}  min {min(t):9.2f}  max {max(t):9.2f}   windows: " + " ".join(f"{x:.2f}" for x in t))
    lines.append(f"  ratio uncached / cached = {np.median(tu) / np.median(tg):.2f}; tokens equal between the arms: {agree:.3f} (bf16: near-ties may differ)")
    # prefill / decode split from HIP events on the stream: the contraction launches of one generation, cut into its max_new forward passes
    pre, dec, att = [], [], []
    for _ in range(a.rounds):
        ctx.profile_enable(3)
        ctx.generate(pid, pcu, M, (), slots)
        st, en, fl = ctx.profile_intervals(ctx, -1)
        att_ms, _, att_n = ctx.profile_read(104, reset=False)
        gemm_ms, _, gemm_n = ctx.profile_read(-1, reset=True)
        ctx.profile_enable(0)
        # a pass ends with the head's contraction: [S rows] x [padded vocabulary] x [hidden], the only launch of that size
        heads = np.flatnonzero(np.isclose(fl, 2.0 * S * (-(-cfg["vocab_size"] // 64) * 64) * cfg["hidden_size"], rtol=1e-9))
        assert len(heads) == M, (len(heads), M)
        per = int(heads[0]) + 1
        pre.append(float(en[heads[0]] - st[0]))
        if M > 1:
            dec.append(float(en[heads[-1]] - st[heads[0] + 1]) / (M - 1))
        att.append(att_ms)
    lines.append(f"  HIP events, {a.rounds} generations (event brackets on: each launch pays two event records): prefill median {np.median(pre):.2f} ms (min {min(pre):.2f}); "
                 + (f"mean decode step median {np.median(dec):.3f} ms (min {min(dec):.3f}); " if dec else "")
                 + f"{per} contraction launches in the prefill, contractions {gemm_ms:.2f} ms summed; attention brackets ({att_n}: prefill attn_fwd + attn_decode) {np.median(att):.3f} ms summed")
    esz = 2
    wbytes = cfg["num_layers"] * esz * (cfg["hidden_size"] * (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * cfg["head_dim"] + cfg["num_heads"] * cfg["head_dim"] * cfg["hidden_size"]
                                        + 3 * cfg["hidden_size"] * cfg["intermediate_size"]) + esz * cfg["vocab_size"] * cfg["hidden_size"]
    kvbytes = cfg["num_layers"] * 2 * esz * cfg["num_kv_heads"] * cfg["head_dim"] * float(plens.sum() + S * (M + 1) / 2)
    lines.append(f"  one decode step reads the weights once: {wbytes / 1e9:.2f} GB = {wbytes / 8e12 * 1e3:.2f} ms at 8 TB/s; K + V of all layers: {kvbytes / 1e6:.1f} MB "
                 f"({kvbytes / cfg['num_layers'] / 1e6:.2f} MB per attn_decode launch)")
    if a.parent_lib:
        pctx = make_parent_ctx()
        score_window(pctx, 2)
        score_window(ctx, 2)
        tp, tc = [], []
        for _ in range(a.rounds):
            tp.append(score_window(pctx))
            tc.append(score_window(ctx))
        lines.append(f"  held-out scoring pass ({S} samples, no generation), ms per pass, windows of 4 alternating: parent library median {np.median(tp):.3f} (min {min(tp):.3f}, "
                     f"max {max(tp):.3f}); this library median {np.median(tc):.3f} (min {min(tc):.3f}, max {max(tc):.3f}); ratio {np.median(tc) / np.median(tp):.4f}")
        pctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
