#!/usr/bin/env python3
"""Candidate scoring at one prefill against what a caller would have to do without it: every (prompt, candidate) pair as a sequence of its own through the
scoring pass.

    python3 tools/cand_bench.py [--model llama3-8b] [--layers 8] [--seqs 64] [--cands 32] [--rounds 5] [--parent-lib DIR] [--out FILE.json]

Run it on a card with nothing else on it. One LoRA context (r = 16), random-initialised base, tile policy 3, the model's widths with --layers decoder layers.
Prompts: the synthetic VSI length distribution (tst.data.synth_vsi), as bench.py; candidates: --cands per prompt, lengths and ids drawn from the "na" answers of
the same generator (1 .. 4 tokens).
  arm A   Context.score_candidates(prompts, candidates): one prefill over the S prompts, one extend pass over the sum (L_c - 1) rows
  arm B   the same pairs as S C sequences prompt + candidate, labelled on the candidate tokens, through Context.score_rows, in as many batches as the context's
          max_tokens / max_seqs / max_labelled need (the count is reported)
Method as bench.py / tools/sample_bench.py: an untimed warm-up of each arm, then `rounds` windows per arm, the arms ALTERNATING; a window is a host clock around
work that ends in a device synchronise. The prefill / extend split of arm A comes from the library's HIP events (tst_profile_intervals: every contraction launch
of ONE call is bracketed on the stream; a pass ends with the head's contraction). attn_extend alone against the per-position attn_decode_shared launches it
replaces: the lab hooks on the call's own geometry and a cache of the model's kv width, one layer, a host clock around 20 repetitions that end in a device
synchronise, the two alternating. --parent-lib DIR (a directory holding libtst_hip.so built from the parent commit): the held-out scoring pass (score_rows on
the same samples with their answers) in a context of THAT library and in a context of this one, same process, windows alternating -- a run without the new flag
must cost what it cost. The result is one JSON object (printed; --out FILE.json writes it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import cli, data as D, lib  # noqa: E402
from tst.trainer import collate_prompts  # noqa: E402


def stats(t):
    return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), windows=[round(float(x), 3) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(cli.MODEL_SHAPES))
    ap.add_argument("--layers", type=int, default=8, help="0 = the model's own")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--cands", type=int, default=32)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--max-tokens", type=int, default=16384, help="the context's max_tokens: arm B is cut into batches that fit it")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = dict(cli.MODEL_SHAPES[a.model])
    if a.layers:
        cfg["num_layers"] = a.layers
    S, NC = a.seqs, a.cands
    samples = D.synth_vsi(S, cfg["vocab_size"], seed=100)
    pool = [x.ids[x.n_prompt:] for x in D.synth_vsi(2048, cfg["vocab_size"], seed=101) if x.kind == "na"]
    pick = np.random.default_rng(102).integers(0, len(pool), S * NC)
    cands = [[int(t) for t in pool[i]] for i in pick]
    seq = [s for s in range(S) for _ in range(NC)]
    pid, pcu = collate_prompts(samples)
    plens = np.diff(pcu)
    cid, ccu, cseq = lib.pack_candidates(cands, seq)
    n_tok, R_e = len(cid), len(cid) - len(cands)
    lib.set_tile_policy(3)
    dims = dict(max_tokens=max(a.max_tokens, int(pcu[-1]), R_e), max_seqs=max(R_e, 4 * S), max_labelled=n_tok, max_position=a.max_len + lib.CAND_MAX_LEN,
                lora_r=16, lora_alpha=32.0)
    ctx = lib.Context(cfg, **dims)
    ctx.init_random(seed=0, std=0.02)
    ctx.reset_trainable(seed=1)

    # arm B: the pairs as sequences, cut into batches by the context's three limits
    batches, cur, tok, lab = [], [], 0, 0
    for c, s in zip(cands, seq):
        n = int(plens[s]) + len(c)
        if cur and (tok + n > dims["max_tokens"] or len(cur) + 1 > dims["max_seqs"] or lab + len(c) > dims["max_labelled"]):
            batches.append(cur)
            cur, tok, lab = [], 0, 0
        cur.append((c, s))
        tok += n
        lab += len(c)
    batches.append(cur)
    packed = []
    for b in batches:
        ids = np.concatenate([np.concatenate([pid[pcu[s]:pcu[s + 1]], np.asarray(c, np.int32)]) for c, s in b]).astype(np.int32)
        cu = np.concatenate([[0], np.cumsum([int(plens[s]) + len(c) for c, s in b])]).astype(np.int32)
        labels = np.full(len(ids), -100, np.int32)
        for i, (c, s) in enumerate(b):
            labels[cu[i] + int(plens[s]):cu[i + 1]] = c
        packed.append((ids, labels, cu))

    def arm_b():
        out = []
        for ids, labels, cu in packed:
            ctx.score_rows_async(ids, labels, cu, ())
            out.append(ctx.score_rows_fetch()[0])
        return np.concatenate(out)

    arms = dict(A=lambda: ctx.score_candidates(pid, pcu, cid, ccu, cseq)[0], B=arm_b)

    def window(run):
        ctx.sync()
        t0 = time.perf_counter()
        run()
        return (time.perf_counter() - t0) * 1e3

    got = {k: run() for k, run in arms.items()}   # the untimed warm-up; the two arms compute the same numbers
    t = dict(A=[], B=[])
    for _ in range(a.rounds):
        for k, run in arms.items():
            t[k].append(window(run))
    res = dict(model=a.model, layers=cfg["num_layers"], prompts=S, prompt_tokens=int(plens.sum()), longest=int(plens.max()), cands_per_prompt=NC,
               cand_tokens=n_tok, extend_rows=R_e, arm_A_rows=int(plens.sum()) + R_e, arm_B_tokens=int(sum(len(p[0]) for p in packed)), arm_B_batches=len(packed),
               rounds=a.rounds, max_abs_diff_A_B=float(np.abs(got["A"] - got["B"]).max()), arm_A_ms=stats(t["A"]), arm_B_ms=stats(t["B"]),
               ratio_B_over_A=float(np.median(t["B"]) / np.median(t["A"])))
    # prefill / extend split of arm A from HIP events: the contraction launches of one call, cut at the head's contractions (S rows, then R_e rows)
    vp = -(-cfg["vocab_size"] // 64) * 64
    pre, ext = [], []
    for _ in range(a.rounds):
        ctx.profile_enable(3)
        arms["A"]()
        st, en, fl = ctx.profile_intervals(ctx, -1)
        ctx.profile_read(-1, reset=True)
        ctx.profile_enable(0)
        heads = np.flatnonzero(np.isin(fl, [2.0 * r * vp * cfg["hidden_size"] for r in (S, R_e)]))
        assert len(heads) == 2, len(heads)
        pre.append(float(en[heads[0]] - st[0]))
        ext.append(float(en[heads[1]] - st[heads[0] + 1]))
    res["arm_A_prefill_ms"], res["arm_A_extend_ms"] = stats(pre), stats(ext)
    # attn_extend alone against the per-position attn_decode_shared launches it replaces: one layer, the call's geometry, the model's kv width
    lab_ = lib.load_lab()
    plan = lib.host_plan_candidates(lib.make_model_cfg(cfg, **dims), pid, pcu, cid, ccu, cseq)
    H, Hkv, dh = cfg["num_heads"], cfg["num_kv_heads"], cfg["head_dim"]
    rng = np.random.default_rng(0)
    cap = plan["rows_used"]
    kc_, vc_ = (lib.dev_bf16(rng.standard_normal((cap, Hkv * dh)).astype(np.float32)) for _ in range(2))
    q_ = lib.dev_bf16(rng.standard_normal((R_e, H * dh)).astype(np.float32))
    o_ = lib.DevBuf(nbytes=R_e * H * dh * 2)
    geo = plan["geo"]
    geo_ = lib.DevBuf(geo)
    steps = []
    for p in range(int(geo[:, 4].max())):
        live = np.flatnonzero(geo[:, 4] > p)
        g = np.concatenate([[len(live), 16, 1], geo[live, :3].reshape(-1)]).astype(np.int32)
        # (the per-position launches read their queries where the extend pass does: the rows are not gathered, so row r of the step is candidate live[r]'s
        # first query row -- the same bytes are streamed, only which query meets which keys differs)
        steps.append((lib.DevBuf(g), len(live), p + 1))
    scale = 1.0 / np.sqrt(dh)

    def k_extend():
        assert lab_.tst_k_attn_extend(q_.ptr, H * dh, kc_.ptr, vc_.ptr, geo_.ptr, len(geo), R_e, o_.ptr, H * dh, H, Hkv, dh, scale, cap) == 0

    def k_steps():
        for g_, n, step in steps:
            assert lab_.tst_k_attn_decode_shared(q_.ptr, H * dh, kc_.ptr, vc_.ptr, g_.ptr, n, step, o_.ptr, H * dh, H, Hkv, dh, scale, cap) == 0

    def kwindow(fn, n=20):
        lab_.tst_dev_sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        lab_.tst_dev_sync()
        return (time.perf_counter() - t0) * 1e6 / n

    kern = dict(attn_extend=k_extend, attn_decode_shared_per_position=k_steps)
    for fn in kern.values():
        kwindow(fn, 3)
    tk = {k: [] for k in kern}
    for _ in range(a.rounds):
        for k, fn in kern.items():
            tk[k].append(kwindow(fn))
    res["kernel_candidates"], res["kernel_decode_launches"] = int(len(geo)), len(steps)
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
