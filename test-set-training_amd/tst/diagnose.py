"""TsT diagnostic orchestration (SURVEY.md §3 stack (1)): k-fold sweep -> per-sample bias score s(x).

Fold jobs are independent (no data flows between folds until s(x) is concatenated), so they shard over GPUs with no
collective: fold f runs on rank f % world. A finished fold writes `fold_{f}.jsonl` (one record per
held-out sample); that file is the checkpoint/resume unit (a crashed worker's fold is simply re-run) and the C2
"gather" of the build: rank 0 concatenates the shards. Record schema (frozen, SURVEY §7 hard part 2):
    {"id": int, "fold": int, "round": int, "s": float, "pred": int, "correct": int, "kind": "mca"|"na"}
With TrainArgs.generate every record also carries what the text-only model answers: "gen" (the greedy continuation of the prompt, token ids without the
eos token), "gen_correct" (it starts with the reference answer's ids) and, when the caller hands a `decode` function (the CLI: its tokenizer), "gen_text".
With TrainArgs.sample_n > 0 every record also carries the distribution of those answers: "samples" = {"ids": sample_n id lists (draws from the model's
distribution at TrainArgs.temperature, include/tst_hip.h tst_sample_async, without the eos token), "logp": their summed log-probabilities, "match": the share of
draws that start with the reference answer's ids} and, with a `decode` function, "texts" and -- where the reference answer reads as a number -- "mra", the mean
over the draws of VSI-Bench's mean relative accuracy. A QA pair's draws depend on TrainArgs.sample_seed and the pair's id only.
With TrainArgs.attribute every record also carries which prompt tokens its score rests on: "attr" = {"gxi": [...], "gnorm": [...]} over the prompt tokens
(gradient x input and gradient norm of log s(x) per token, include/tst_hip.h tst_attribute_async) and, with a `decode` function, "attr_top": the
TrainArgs.attribute_top tokens of largest gnorm, as text. Not available on the data-parallel layouts.
With TrainArgs.attribute_ig > 0 every record also carries "attr_ig" = {"ig": [...], "log_s_base": float, "delta": float}: the integrated gradients of log s(x) over
the prompt tokens, walked from a prompt of TrainArgs.attribute_baseline_id tokens in attribute_ig steps (include/tst_hip.h tst_attribute_ig_async), log s of that
baseline prompt, and the completeness gap sum(ig) - (log s - log s_base); with a `decode` function also "attr_ig_top": the attribute_top tokens of largest |ig| as
[text, ig] pairs, signed. Not available on the data-parallel layouts either.
With TrainArgs.candidates > 0 every "na" record also carries the model's exact distribution over the benchmark's own answers: "cand" = {"n": candidates scored (the
TrainArgs.candidates most frequent reference answers of the data set and the record's own), "rank": of the reference among them (1 = the model's top answer),
"p_ref": its probability on that closed set, "mass": log of the share of the model's whole distribution the list covers, "top" / "top_p": the five most probable
candidates (token ids) and their probabilities} (include/tst_hip.h tst_score_candidates_async: one prefill per batch) and, with a `decode` function, "top_text" and
-- where the reference answer reads as a number -- "mra_exp", the expected mean relative accuracy sum_c p_c MRA(text_c, reference), free of sampling noise.
"""
import json
import os
import sys
import time

import numpy as np

from . import kfold
from . import score as S
from .trainer import (ATTRIBUTE, CANDIDATES, GENERATE, IG, SAMPLE, SCORE, TrainArgs, fine_tune, fine_tune_concurrent, fine_tune_dp, fine_tune_stacked, run_heldout,
                      run_heldout_concurrent, run_heldout_stacked)

GEN_ARGS = ("generate", "max_new_tokens", "eos_ids")   # TrainArgs fields that enter the run fingerprint only when generation is on
ATTR_ARGS = ("attribute", "attribute_top")             # TrainArgs settings that enter it only when attribution is on
SAMPLE_ARGS = ("sample_n", "temperature", "sample_seed")   # likewise, when sampled answers are on (max_new_tokens / eos_ids then enter too: they shape the draws)
CAND_ARGS = ("candidates",)                            # likewise, when candidate scoring is on
IG_ARGS = ("attribute_ig", "attribute_baseline_id")    # likewise, when integrated gradients are on (attribute_top then enters too: it sizes attr_ig_top)


def run_fingerprint(samples, k, args, extra=None):
    """identity of a diagnostic run: hyper-parameters, fold count, the sample ids and their token content, and whatever the caller adds
    (model / weights / data identity). Resuming into an --out directory whose shards were produced under another fingerprint would
    silently mix stale fold scores into scores.jsonl."""
    import dataclasses
    import hashlib
    h = hashlib.sha256()
    a = dataclasses.asdict(args) if dataclasses.is_dataclass(args) else dict(args)
    kept = {kk: a[kk] for kk in GEN_ARGS[1:] if kk in a}
    if not a.get("generate"):   # a run without generation is the run it was before the option existed: its directory still resumes
        for kk in GEN_ARGS:
            a.pop(kk, None)
    if getattr(args, "attribute", False):   # likewise the attribution settings (attributes of TrainArgs, not fields: see there)
        a.update({kk: getattr(args, kk) for kk in ATTR_ARGS})
    elif not a.get("attribute"):
        for kk in ATTR_ARGS:
            a.pop(kk, None)
    if int(getattr(args, "attribute_ig", 0) or 0) > 0:
        a.update({kk: getattr(args, kk) for kk in IG_ARGS + ("attribute_top",)})
    else:
        for kk in IG_ARGS:
            a.pop(kk, None)
    if int(getattr(args, "sample_n", 0) or 0) > 0:
        a.update({kk: getattr(args, kk) for kk in SAMPLE_ARGS})
        a.update(kept)
    else:
        for kk in SAMPLE_ARGS:
            a.pop(kk, None)
    if int(getattr(args, "candidates", 0) or 0) > 0:
        a.update({kk: getattr(args, kk) for kk in CAND_ARGS})
    else:
        for kk in CAND_ARGS:
            a.pop(kk, None)
    a.pop("candidate_list", None)   # (derived from the samples, which are hashed below)
    h.update(json.dumps(dict(args={kk: (list(v) if isinstance(v, tuple) else v) for kk, v in sorted(a.items())}, k=int(k), n=len(samples),
                             extra=extra or {}), sort_keys=True).encode())
    for x in samples:
        h.update(np.int64(x.sid).tobytes())
        h.update(np.ascontiguousarray(x.ids, dtype=np.int32).tobytes())
        h.update(np.int32(x.n_prompt).tobytes())
    return h.hexdigest()


def check_fingerprint(out_dir, rnd, fp, rank=0, wait_s=120.0):
    """first writer records the run's fingerprint in the round directory; a resume under a different one is refused"""
    if not out_dir:
        return
    d = os.path.join(out_dir, f"round_{rnd}")
    path = os.path.join(d, "fingerprint.json")
    if rank == 0 and not os.path.exists(path):
        os.makedirs(d, exist_ok=True)
        tmp = path + ".tmp"
        with open(tmp, "w") as fh:
            json.dump(dict(fingerprint=fp), fh)
        os.replace(tmp, path)
        return
    # every other rank checks against what rank 0 recorded: it waits for the file (rank 0 may not have written it yet) instead of passing
    # an existence check that only says "nobody was here before me"
    deadline = time.time() + (0.0 if rank == 0 else wait_s)
    while not os.path.exists(path):
        if time.time() >= deadline:
            raise TimeoutError(f"{path} did not appear within {wait_s:.0f} s: rank 0 has not recorded the run's fingerprint")
        time.sleep(0.05)
    with open(path) as fh:
        old = json.load(fh)["fingerprint"]
    if old != fp:
        raise ValueError(f"{d} holds fold shards of a DIFFERENT run (model, data, k, seed or hyper-parameters changed): refusing to resume into it; "
                         f"use a fresh --out directory or delete the round")


def train_health(recs):
    """what a caller needs to tell a fold that trained from one that silently did not: per-step losses and gradient norms all finite, the gradient
    norm never zero (LoRA: B starts at 0, so dB is non-zero from the first step on; a zero norm means nothing reached the trainables)"""
    if not recs:
        return dict(steps=0, first_loss=None, loss_finite=True, grad_norm_min=None, grad_norm_max=None)
    loss = np.asarray([r["loss"] for r in recs], np.float64)
    gn = np.asarray([r["grad_norm"] for r in recs], np.float64)
    return dict(steps=len(recs), first_loss=float(loss[0]), loss_finite=bool(np.isfinite(loss).all() and np.isfinite(gn).all()),
                grad_norm_min=float(gn.min()), grad_norm_max=float(gn.max()))


def heldout_passes(layout, ctxs, helds, args: TrainArgs):
    """score, then every enabled extra pass (generate, sample, attribute, ig, candidates: in this order) over the held-out folds. layout: "one" (ctxs is one context, helds one fold),
    "concurrent" (a context per fold) or "stacked". Per fold: ((s, pred, correct), extras), extras = {"gen" / "samples" / "attr" / "ig" / "cand": per-sample results} of what ran."""
    run = dict(one=lambda p, c, sets, a: [run_heldout(p, c, sets[0], a)], concurrent=run_heldout_concurrent, stacked=run_heldout_stacked)[layout]
    scored = run(SCORE, ctxs, helds, args)
    enabled = (("gen", GENERATE, args.generate), ("samples", SAMPLE, getattr(args, "sample_n", 0) > 0), ("attr", ATTRIBUTE, args.attribute),
               ("ig", IG, args.attribute_ig > 0), ("cand", CANDIDATES, getattr(args, "candidates", 0) > 0))
    ran = {key: run(p, ctxs, helds, args) for key, p, on in enabled if on}
    return [(sc, {key: got[i] for key, got in ran.items()}) for i, sc in enumerate(scored)]


def set_candidates(samples, args):
    """the data set's candidate answers (tst.score.answer_candidates over ALL samples, held-out ones included: the list is the benchmark's answer vocabulary, not
    something learned) on args.candidate_list, once per run, when candidate scoring is on"""
    if int(getattr(args, "candidates", 0) or 0) > 0 and getattr(args, "candidate_list", None) is None:
        args.candidate_list = S.answer_candidates(samples, args.candidates)


def fold_records(held, f, rnd, s, pred, correct, decode=None, attr_top=5, *, gen=None, attr=None, ig=None, samples=None, cand=None):
    """the records of one scored held-out fold; decode = ids -> text; the extras (heldout_passes' mapping, as keywords): gen = [(gen ids, gen_correct)] per sample
    when generation is on, samples = tst.score.sampled_answers' dict when sampled answers are, attr = tst.score.token_attribution's dict when attribution is on,
    ig = tst.score.token_ig's when integrated gradients are, cand = tst.score.candidate_scores' (None for the samples without candidates) when candidate scoring is"""
    records = [dict(id=int(x.sid), fold=int(f), round=int(rnd), s=float(si), pred=int(pi), correct=int(ci), kind=x.kind)
               for x, si, pi, ci in zip(held, s, pred, correct)]
    if gen is not None:
        for r, (g, gc) in zip(records, gen):
            r["gen"] = [int(t) for t in g]
            r["gen_correct"] = int(gc)
            if decode is not None:
                r["gen_text"] = decode(r["gen"])
    if samples is not None:
        # samples = tst.score.sampled_answers' dict: the draws' ids, their summed log-probabilities and the share that starts with the reference answer; with a
        # tokenizer their texts, and for a reference answer that reads as a number the expected mean relative accuracy over the draws
        from .benchmarks import mean_relative_accuracy, parse_number
        for r, x, sm in zip(records, held, samples):
            r["samples"] = dict(ids=[[int(t) for t in g] for g in sm["ids"]], logp=[float(v) for v in sm["logp"]], match=float(sm["match"]))
            if decode is not None:
                texts = [decode(g) for g in r["samples"]["ids"]]
                r["samples"]["texts"] = texts
                ref = decode([int(t) for t in x.ids[x.n_prompt:]])
                if parse_number(ref) is not None and texts:
                    r["samples"]["mra"] = float(np.mean([mean_relative_accuracy(t, ref) for t in texts]))
    if attr is not None:
        for r, x, a in zip(records, held, attr):
            r["attr"] = dict(gxi=[float(v) for v in a["gxi"]], gnorm=[float(v) for v in a["gnorm"]])
            if decode is not None:
                top = np.argsort(-np.asarray(a["gnorm"], np.float64), kind="stable")[:max(0, int(attr_top))]
                r["attr_top"] = [decode([int(x.ids[t])]) for t in top]
    if ig is not None:
        for r, x, a in zip(records, held, ig):
            r["attr_ig"] = dict(ig=[float(v) for v in a["ig"]], log_s_base=float(a["log_s_base"]), delta=float(a["delta"]))
            if decode is not None:
                top = np.argsort(-np.abs(np.asarray(a["ig"], np.float64)), kind="stable")[:max(0, int(attr_top))]
                r["attr_ig_top"] = [[decode([int(x.ids[t])]), float(a["ig"][t])] for t in top]
    if cand is not None:
        from .benchmarks import mean_relative_accuracy, parse_number
        for r, x, c in zip(records, held, cand):
            if c is None:   # "mca": its restricted softmax over the option letters already is this
                continue
            r["cand"] = dict(n=int(c["n"]), rank=c["rank"], p_ref=c["p_ref"], mass=float(c["mass"]), top=[[int(t) for t in g] for g in c["top"]],
                             top_p=[float(v) for v in c["top_p"]])
            if decode is not None:
                r["cand"]["top_text"] = [decode(g) for g in r["cand"]["top"]]
                ref = decode([int(t) for t in x.ids[x.n_prompt:]])
                if parse_number(ref) is not None:
                    r["cand"]["mra_exp"] = float(sum(float(pc) * mean_relative_accuracy(decode([int(t) for t in g]), ref) for pc, g in zip(c["p"], c["cands"])))
    return records


def fold_path(out_dir, rnd, f):
    return os.path.join(out_dir, f"round_{rnd}", f"fold_{f}.jsonl")


def run_fold(ctx, samples, assign, f, args: TrainArgs, rnd=0, out_dir=None, log=None, decode=None):
    """fine-tune on the k-1 other folds, score the held-out fold; returns the records (and writes the shard)."""
    train_idx, held_idx = kfold.fold_indices(assign, f)
    t0 = time.perf_counter()
    flog = (lambda r: log(dict(r, fold=int(f), round=int(rnd)))) if log else None
    recs_train = fine_tune(ctx, [samples[i] for i in train_idx], args, fold_seed=f, log=flog)
    t1 = time.perf_counter()
    held = [samples[i] for i in held_idx]
    [((s, pred, correct), extras)] = heldout_passes("one", ctx, [held], args)
    t2 = time.perf_counter()
    records = fold_records(held, f, rnd, s, pred, correct, decode, args.attribute_top, **extras)
    if out_dir:
        _write_shard(out_dir, rnd, f, records)
    stats = dict(fold=f, n_train=len(train_idx), n_heldout=len(held_idx), train_s=t1 - t0, score_s=t2 - t1,
                 acc=float(np.mean(correct)) if len(correct) else 0.0, last_loss=recs_train[-1]["loss"] if recs_train else None, **train_health(recs_train))
    return records, stats


def _write_shard(out_dir, rnd, f, records):
    path = fold_path(out_dir, rnd, f)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "w") as fh:
        for r in records:
            fh.write(json.dumps(r) + "\n")
    os.replace(tmp, path)  # atomic: a shard either exists completely or not at all


def run_fold_group(ctxs, samples, assign, fold_ids, args: TrainArgs, rnd=0, out_dir=None, log=None, decode=None):
    """len(fold_ids) <= len(ctxs) folds at once on one GPU (resident folds: contexts forked from one root). Same records and
    shards as run_fold; the timings in the stats are the group's wall time."""
    stacked = any(getattr(c, "n_stack", 1) > 1 for c in ctxs)
    if not stacked:
        ctxs = ctxs[:len(fold_ids)]
    idx = [kfold.fold_indices(assign, f) for f in fold_ids]
    t0 = time.perf_counter()
    flog = (lambda r: log(dict({k: v for k, v in r.items() if k != "slot"}, fold=int(fold_ids[r["slot"]]), round=int(rnd)))) if log else None
    trains = [[samples[i] for i in tr] for tr, _ in idx]
    logs = (fine_tune_stacked if stacked else fine_tune_concurrent)(ctxs, trains, args, list(fold_ids), flog)
    t1 = time.perf_counter()
    helds = [[samples[i] for i in he] for _, he in idx]
    passed = heldout_passes("stacked" if stacked else "concurrent", ctxs, helds, args)
    t2 = time.perf_counter()
    if os.environ.get("TST_PHASE_LOG"):
        print(f"[phase] fold group {list(fold_ids)}: train {t1 - t0:.3f} s, score {t2 - t1:.3f} s", file=sys.stderr)
    all_records, stats = [], []
    for f, (tr, he), held, ((s, pred, correct), extras), lg in zip(fold_ids, idx, helds, passed, logs):
        records = fold_records(held, f, rnd, s, pred, correct, decode, args.attribute_top, **extras)
        if out_dir:
            _write_shard(out_dir, rnd, f, records)
        all_records += records
        stats.append(dict(fold=f, n_train=len(tr), n_heldout=len(he), train_s=t1 - t0, score_s=t2 - t1, resident_folds=len(fold_ids),
                          acc=float(np.mean(correct)) if len(correct) else 0.0, last_loss=lg[-1]["loss"] if lg else None, **train_health(lg)))
    if os.environ.get("TST_PHASE_LOG"):
        print(f"[phase] records + shards {time.perf_counter() - t2:.3f} s", file=sys.stderr)
    return all_records, stats


def diagnose(ctx, samples, k, args: TrainArgs, rank=0, world=1, rnd=0, out_dir=None, resume=True, log=None, identity=None, decode=None):
    """runs this rank's folds; returns (records of this rank, per-fold stats). `ctx` is one context (folds run one after the
    other) or a list of contexts sharing one GPU (root + forks): then that many folds run at once. `identity`: what the caller knows
    about model / weights / data (any JSON-able dict); it goes into the run fingerprint that guards resume. `decode` (ids -> text): with args.generate the
    records also carry "gen_text"."""
    assign = kfold.kfold_assign(len(samples), k, True, args.seed)
    set_candidates(samples, args)
    if out_dir and resume:
        check_fingerprint(out_dir, rnd, run_fingerprint(samples, k, args, identity), rank)
    records, stats, todo = [], [], []
    for f in kfold.folds_for_rank(k, rank, world):
        if resume and out_dir and os.path.exists(fold_path(out_dir, rnd, f)):
            with open(fold_path(out_dir, rnd, f)) as fh:
                records += [json.loads(line) for line in fh]
        else:
            todo.append(f)
    cap = sum(getattr(c, "n_stack", 1) for c in ctx) if isinstance(ctx, (list, tuple)) else getattr(ctx, "n_stack", 1)
    if cap > 1:
        group = list(ctx) if isinstance(ctx, (list, tuple)) else [ctx]
        for g in range(0, len(todo), cap):
            r, st = run_fold_group(group, samples, assign, todo[g:g + cap], args, rnd, out_dir, log, decode)
            records += r
            stats += st
        return records, stats
    one = ctx[0] if isinstance(ctx, (list, tuple)) else ctx
    for f in todo:
        r, st = run_fold(one, samples, assign, f, args, rnd, out_dir, log, decode)
        records += r
        stats.append(st)
    return records, stats


def diagnose_dp(ctx, samples, k, args: TrainArgs, rank, world, dp, rnd=0, out_dir=None, resume=True, log=None, identity=None, mode="shard", decode=None):
    """BASELINE.json config 4: groups of `dp` ranks share a fold (tst/ddp.py; the context has joined its group's communicator,
    ddp.init_fold_group). Fold f goes to group f mod n_groups; the group's ranks fine-tune it together (fine_tune_dp), rank 0 of the
    group scores the held-out fold and writes the shard. Returns (records, stats) of the folds this rank wrote (empty on the
    group's other ranks)."""
    from . import ddp
    if args.attribute or args.attribute_ig > 0:
        raise ValueError("token attribution is not available on data-parallel contexts (include/tst_hip.h tst_attribute_async)")
    g, n_groups, dp_rank, _ = ddp.dp_layout(rank, world, dp)
    assign = kfold.kfold_assign(len(samples), k, True, args.seed)
    set_candidates(samples, args)
    if out_dir and resume:
        check_fingerprint(out_dir, rnd, run_fingerprint(samples, k, args, identity), rank)
    records, stats = [], []
    for f in kfold.folds_for_rank(k, g, n_groups):
        if resume and out_dir and os.path.exists(fold_path(out_dir, rnd, f)):   # every rank of the group sees the same file system
            if dp_rank == 0:
                with open(fold_path(out_dir, rnd, f)) as fh:
                    records += [json.loads(line) for line in fh]
            continue
        tr, he = kfold.fold_indices(assign, f)
        t0 = time.perf_counter()
        flog = (lambda r: log(dict(r, fold=int(f), round=int(rnd)))) if (log and dp_rank == 0) else None
        lg = fine_tune_dp(ctx, [samples[i] for i in tr], args, f, dp_rank, dp, flog, mode)
        t1 = time.perf_counter()
        if dp_rank != 0:
            continue   # the replicas are identical: one of them scores
        held = [samples[i] for i in he]
        [((s, pred, correct), extras)] = heldout_passes("one", ctx, [held], args)
        t2 = time.perf_counter()
        recs = fold_records(held, f, rnd, s, pred, correct, decode, **extras)
        if out_dir:
            _write_shard(out_dir, rnd, f, recs)
        records += recs
        stats.append(dict(fold=f, n_train=len(tr), n_heldout=len(he), train_s=t1 - t0, score_s=t2 - t1, dp=dp,
                          acc=float(np.mean(correct)) if len(correct) else 0.0, last_loss=lg[-1]["loss"] if lg else None, **train_health(lg)))
    return records, stats


def diagnose_dp_stacked(ctxs, samples, k, args: TrainArgs, rank, world, rnd=0, out_dir=None, resume=True, log=None, identity=None, gather=None, decode=None):
    """the dp-stacked layout: EVERY rank hosts all k folds (stacked contexts, the one-GPU layout) and the ranks share every fold's
    fine-tune -- global batches of world x per_device_train_batch_size samples, each rank its own micro-batch, one gradient all-reduce
    per context and step (trainer.fine_tune_stacked(dp=...); the contexts have joined their communicators, ddp.init_stacked_groups).
    All ranks hold the same adapters afterwards, so the held-out scoring is sharded with NO collective: rank r scores samples
    r, r + world, ... of every held-out fold. Returns (records of this rank's part, per-fold stats). With out_dir the parts are brought
    together by `gather(obj) -> list over ranks on rank 0` (default: torch.distributed.gather_object) and rank 0 writes the fold shards."""
    group = list(ctxs) if isinstance(ctxs, (list, tuple)) else [ctxs]
    if args.attribute or args.attribute_ig > 0:
        raise ValueError("token attribution is not available on data-parallel contexts (include/tst_hip.h tst_attribute_async)")
    cap = sum(getattr(c, "n_stack", 1) for c in group)
    assign = kfold.kfold_assign(len(samples), k, True, args.seed)
    set_candidates(samples, args)
    if out_dir and resume:
        check_fingerprint(out_dir, rnd, run_fingerprint(samples, k, args, dict(identity or {}, layout="dp-stacked", world=world)), rank)
    if gather is None and out_dir:
        def gather(obj):
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()) or world == 1:
                return [obj]
            out = [None] * world if rank == 0 else None
            dist.gather_object(obj, out, dst=0)
            return out
    records, stats, todo = [], [], []
    for f in range(k):
        if resume and out_dir and os.path.exists(fold_path(out_dir, rnd, f)):   # (every rank sees the same file system)
            if rank == 0:
                with open(fold_path(out_dir, rnd, f)) as fh:
                    records += [json.loads(line) for line in fh]
        else:
            todo.append(f)
    for g0 in range(0, len(todo), cap):
        fold_ids = todo[g0:g0 + cap]
        idx = [kfold.fold_indices(assign, f) for f in fold_ids]
        t0 = time.perf_counter()
        flog = (lambda r: log(dict({kk: v for kk, v in r.items() if kk != "slot"}, fold=int(fold_ids[r["slot"]]), round=int(rnd)))) if (log and rank == 0) else None
        logs = fine_tune_stacked(group, [[samples[i] for i in tr] for tr, _ in idx], args, list(fold_ids), flog, dp=(rank, world))
        t1 = time.perf_counter()
        helds = [[samples[i] for i in he][rank::world] for _, he in idx]      # this rank's part of every held-out fold
        passed = heldout_passes("stacked", group, helds, args)
        t2 = time.perf_counter()
        for f, (tr, he), held, ((s, pred, correct), extras), lg in zip(fold_ids, idx, helds, passed, logs):
            recs = fold_records(held, f, rnd, s, pred, correct, decode, **extras)
            if out_dir:
                parts = gather(recs)
                if rank == 0:
                    _write_shard(out_dir, rnd, f, sorted((r for p in parts for r in p), key=lambda r: r["id"]))
            records += recs
            stats.append(dict(fold=f, n_train=len(tr), n_heldout=len(he), n_scored_here=len(held), train_s=t1 - t0, score_s=t2 - t1, resident_folds=len(fold_ids),
                              dp_world=world, acc=float(np.mean(correct)) if len(correct) else 0.0, last_loss=lg[-1]["loss"] if lg else None, **train_health(lg)))
    return records, stats


def gather_round(out_dir, rnd, k, n_expected=None, timeout_s=0.0):
    """rank 0: concatenate the k fold shards of a round into s(x) records sorted by sample id."""
    deadline = time.time() + timeout_s
    paths = [fold_path(out_dir, rnd, f) for f in range(k)]
    while not all(os.path.exists(p) for p in paths):
        if time.time() >= deadline:
            missing = [p for p in paths if not os.path.exists(p)]
            raise FileNotFoundError(f"missing fold shards: {missing}")
        time.sleep(0.5)
    recs = []
    for p in paths:
        with open(p) as fh:
            recs += [json.loads(line) for line in fh]
    recs.sort(key=lambda r: r["id"])
    ids = [r["id"] for r in recs]
    if len(set(ids)) != len(ids):
        raise ValueError("a sample was scored in more than one fold")
    if n_expected is not None and len(recs) != n_expected:
        raise ValueError(f"expected {n_expected} scored samples, got {len(recs)}")
    return recs


def summarize(records):
    s = np.array([r["s"] for r in records], np.float64)
    c = np.array([r["correct"] for r in records], np.float64)
    return dict(n=len(records), acc=float(c.mean()) if len(c) else 0.0, mean_s=float(s.mean()) if len(s) else 0.0,
                frac_s_gt_half=float((s > 0.5).mean()) if len(s) else 0.0)
