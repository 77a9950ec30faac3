"""Per-fold fine-tune + held-out scoring loop (SURVEY.md §3 stacks (2) and (3)): the role of HF Trainer.train /
Trainer.predict (HF/trainer.py:1347-1796, 2860-3010) for this one path, driving libtst_hip through the C-ABI.

Hyper-parameter names and defaults mirror HF TrainingArguments (training_args.py:767-856: lr 5e-5, linear schedule,
AdamW 0.9/0.999/1e-8, wd 0, max_grad_norm 1.0, 3 epochs, seed 42) so a future upstream CLI maps 1:1; the per-device
batch of 16 is the value BASELINE.md fixes for the metric."""
import os
import time
from dataclasses import InitVar, dataclass
from typing import Callable, NamedTuple

import numpy as np

from . import data as D
from . import score as S


@dataclass
class TrainArgs:
    learning_rate: float = 5e-5
    num_train_epochs: int = 3
    per_device_train_batch_size: int = 16
    per_device_eval_batch_size: int = 16
    warmup_steps: int = 0
    weight_decay: float = 0.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    max_grad_norm: float = 1.0
    seed: int = 42
    lora_r: int = 16
    lora_alpha: float = 32.0
    lora_targets: tuple = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    logging_steps: int = 50
    gradient_accumulation_steps: int = 1   # HF training_args.py: micro-batches per optimizer update, normalised by ONE num_items_in_batch (trainer.py:1740-1758, 2141-2175)
    option_ids: tuple = D.OPTION_IDS   # token ids of the option letters (synthetic data: reserved ids; real data: from the tokenizer)
    # greedy answer generation on the held-out fold (off by default: a run without it computes and writes exactly what it did before these fields existed,
    # and tst.diagnose.run_fingerprint leaves them out): every record gains what the text-only model says, `gen`, and `gen_correct`
    generate: bool = False
    max_new_tokens: int = 8
    eos_ids: tuple = ()
    # token attribution on the held-out fold (off by default): every record gains `attr`, the gradient of log s(x) per prompt token as gradient x input and
    # gradient norm (include/tst_hip.h tst_attribute_async), and with a tokenizer `attr_top`. The two settings are constructor arguments and attributes but NOT
    # dataclass fields: dataclasses.asdict(args) -- what the run fingerprint of a run without attribution hashes -- lists exactly the fields it always listed, so
    # such a run's directory still resumes; tst.diagnose.run_fingerprint adds them when attribution is on. (dataclasses.replace does not carry them over.)
    attribute: InitVar[bool] = False
    attribute_top: InitVar[int] = 5
    # integrated gradients on the held-out fold (off at 0 steps): every record gains `attr_ig` (include/tst_hip.h tst_attribute_ig_async), the prompt tokens walked
    # from attribute_baseline_id to their own embeddings in attribute_ig midpoint steps, the answer tokens left as they are. Constructor arguments and attributes,
    # NOT dataclass fields, for the reason above.
    attribute_ig: InitVar[int] = 0
    attribute_baseline_id: InitVar[int] = 0
    # sampled answers on the held-out fold (off at 0 samples): every record gains `samples`, sample_n draws of max_new_tokens tokens from the model's own
    # distribution at `temperature` (include/tst_hip.h tst_sample_async; eos_ids end a draw), seeded per QA pair from sample_seed and the pair's id
    # (tst.score.sample_seeds). Independent of `generate`. Constructor arguments and attributes, NOT dataclass fields, for the reason above.
    sample_n: InitVar[int] = 0
    temperature: InitVar[float] = 1.0
    sample_seed: InitVar[int] = 0
    # candidate-answer scoring on the held-out fold (off at 0): every "na" record gains `cand`, the model's exact distribution over the `candidates` most frequent
    # reference answers of the data set plus the record's own (include/tst_hip.h tst_score_candidates_async; tst.score.answer_candidates / candidate_scores).
    # candidate_list is that list: tst.diagnose fills it from the whole data set before the first fold. Attributes, NOT dataclass fields, for the reason above.
    candidates: InitVar[int] = 0

    def __post_init__(self, attribute, attribute_top, attribute_ig, attribute_baseline_id, sample_n, temperature, sample_seed, candidates):
        self.candidates, self.candidate_list = int(candidates), None
        self.attribute, self.attribute_top = bool(attribute), int(attribute_top)
        self.attribute_ig, self.attribute_baseline_id = int(attribute_ig), int(attribute_baseline_id)
        self.sample_n, self.temperature, self.sample_seed = int(sample_n), float(temperature), int(sample_seed)


def linear_lr(step, total, lr0, warmup=0):
    """HF/optimization.py:101-104 (get_linear_schedule_with_warmup); step = optimizer steps already taken."""
    if step < warmup:
        return lr0 * step / max(1, warmup)
    return lr0 * max(0.0, (total - step) / max(1, total - warmup))


def epoch_order(n, seed, epoch):
    """one permutation per epoch (the role of RandomSampler, trainer.py:843)."""
    return np.random.RandomState((seed + 1000003 * epoch) % (2 ** 31)).permutation(n)


def train_plan(samples, args: TrainArgs, fold_seed=0, world=1):
    """the optimizer steps of one fold's fine-tune, in order: yields (step number from 1, total, lr, samples of the update).
    An update consumes gradient_accumulation_steps x world micro-batches of per_device_train_batch_size samples (HF: `world` data-parallel
    ranks each run gradient_accumulation_steps micro-batches per update, trainer.py:1722-1758); with both at 1 that is the micro-batch itself.
    The last update of an epoch takes what is left (trainer.py:1733-1738). micro_batches() cuts an update into one rank's micro-batches."""
    per = args.per_device_train_batch_size * max(1, args.gradient_accumulation_steps) * max(1, world)
    steps_per_epoch = (len(samples) + per - 1) // per
    total = steps_per_epoch * args.num_train_epochs
    step = 0
    for ep in range(args.num_train_epochs):
        order = epoch_order(len(samples), args.seed + fold_seed, ep)
        for b in range(steps_per_epoch):
            lr = linear_lr(step, total, args.learning_rate, args.warmup_steps)
            step += 1
            yield step, total, lr, [samples[i] for i in order[b * per:(b + 1) * per]]


def micro_batches(update, args: TrainArgs, rank=0, world=1):
    """one rank's micro-batches of an update: micro-batch i of rank r is the (i * world + r)-th run of per_device_train_batch_size samples
    (empty runs at the ragged end of an epoch are dropped: that rank then contributes nothing to that micro-step)."""
    bs = args.per_device_train_batch_size
    out = []
    for i in range(max(1, args.gradient_accumulation_steps)):
        mb = update[(i * world + rank) * bs:(i * world + rank + 1) * bs]
        if mb:
            out.append(mb)
    return out


def enqueue_update(ctx, update, lr, args: TrainArgs):
    """one optimizer update of a plain (one-fold) context: a single micro-batch, or gradient_accumulation_steps of them under the
    num_items_in_batch of the WHOLE update (trainer.py:2141-2175)"""
    if args.gradient_accumulation_steps > 1:
        items = D.count_labelled(update)
        for i, mb in enumerate(micro_batches(update, args)):
            ids, labels, cu = D.collate(mb)
            ctx.accumulate_async(ids, labels, cu, items, first=(i == 0))
        ctx.optimizer_step_async(lr)
    else:
        ids, labels, cu = D.collate(update)
        ctx.train_step_async(ids, labels, cu, lr)


def fine_tune(ctx, samples, args: TrainArgs, fold_seed=0, log=None):
    """trains the ctx's adapters on `samples`; returns the list of (step, loss, grad_norm, lr) log records."""
    ctx.reset_trainable(seed=args.seed * 1000 + fold_seed)
    records = []
    for step, total, lr, batch in train_plan(samples, args, fold_seed):
        enqueue_update(ctx, batch, lr, args)
        if args.logging_steps and (step % args.logging_steps == 0 or step == total):
            loss, gn = ctx.fetch_metrics()
            records.append(dict(step=step, loss=loss, grad_norm=gn, lr=lr))
            if log:
                log(records[-1])
    ctx.sync()
    return records


def fine_tune_dp(ctx, samples, args: TrainArgs, fold_seed, dp_rank, dp, log=None, mode="shard"):
    """one fold shared by `dp` ranks (intra-fold data parallelism, tst/ddp.py): every rank of the group walks the SAME plan (same
    seeds, same micro-batches), runs its shard of each micro-batch and joins the gradient all-reduce, so all replicas hold the same
    adapters / weights after every step. Returns the log records (global loss, global gradient norm) like fine_tune()."""
    from . import ddp
    ctx.reset_trainable(seed=args.seed * 1000 + fold_seed)
    records = []
    if args.gradient_accumulation_steps > 1:
        raise ValueError("gradient accumulation with intra-fold data parallelism is not built: enlarge the group's batch instead")
    for step, total, lr, batch in train_plan(samples, args, fold_seed, dp if mode == "replicate" else 1):
        loss, gn = ddp.dp_train_step(ctx, dp_rank, dp, batch, lr, D.collate, mode, per_device_batch=args.per_device_train_batch_size)
        if args.logging_steps and (step % args.logging_steps == 0 or step == total):
            records.append(dict(step=step, loss=loss, grad_norm=gn, lr=lr))
            if log:
                log(records[-1])
    ctx.sync()
    return records


def fine_tune_concurrent(ctxs, sample_sets, args: TrainArgs, fold_seeds, log=None):
    """several folds resident on one GPU (contexts forked from one root, tst_fork): their optimizer steps are enqueued
    round-robin on the folds' own streams, so the hardware interleaves them ("Resident folds"). Each
    fold's trajectory is bit-identical to fine_tune() on that fold alone. Returns one list of log records per fold."""
    plans = []
    for c, smp, fs in zip(ctxs, sample_sets, fold_seeds):
        c.reset_trainable(seed=args.seed * 1000 + fs)
        plans.append(train_plan(smp, args, fs))
    records = [[] for _ in ctxs]
    live = list(range(len(ctxs)))
    while live:
        for j in list(live):
            nxt = next(plans[j], None)
            if nxt is None:
                live.remove(j)
                continue
            step, total, lr, batch = nxt
            enqueue_update(ctxs[j], batch, lr, args)
            if args.logging_steps and (step % args.logging_steps == 0 or step == total):
                loss, gn = ctxs[j].fetch_metrics()
                records[j].append(dict(step=step, loss=loss, grad_norm=gn, lr=lr))
                if log:
                    log(dict(records[j][-1], slot=j))
    for c in ctxs:
        c.sync()
    return records


def collate_prompts(samples):
    """packed prompts (ids[:n_prompt] of every sample): ids, cu_seqlens"""
    ids = np.concatenate([s.ids[:s.n_prompt] for s in samples]).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum([s.n_prompt for s in samples])]).astype(np.int32)
    return ids, cu


# ---------------------------------------------------------------------------------------------- passes over the held-out fold
class HeldoutPass(NamedTuple):
    """one kind of pass over held-out samples, for the three drivers below"""
    enqueue: Callable   # (ctx, samples, args, *seq_slot): collate the flat sample list and enqueue it on the context (seq_slot: stacked contexts only)
    fetch: Callable     # (ctx, samples, args) -> one result per sample of the batch pending on the context
    join: Callable      # (per-sample results of a fold, in input order) -> what the fold's caller gets


def _score_enqueue(ctx, batch, args, *seq_slot):
    ids, labels, cu = D.collate(batch)
    ctx.score_rows_async(ids, labels, cu, args.option_ids, *seq_slot)


def _score_join(rows):
    s, pred, correct = zip(*rows) if rows else ((), (), ())
    return np.array(s, np.float32), np.array(pred, np.int32), np.array(correct, np.int32)


def _generate_enqueue(ctx, batch, args, *seq_slot):
    ids, cu = collate_prompts(batch)
    ctx.generate_async(ids, cu, args.max_new_tokens, args.eos_ids, *seq_slot)


def _generate_fetch(ctx, batch, args):
    tok, _, n_new = ctx.generate_fetch()
    return S.generated_answers(batch, tok, n_new, args.eos_ids)


def _sample_enqueue(ctx, batch, args, *seq_slot):
    ids, cu = collate_prompts(batch)
    ctx.sample_async(ids, cu, args.max_new_tokens, args.sample_n, args.temperature, S.sample_seeds(args.sample_seed, [x.sid for x in batch]), args.eos_ids, *seq_slot)


def _sample_fetch(ctx, batch, args):
    tok, logp, n_new = ctx.sample_fetch()
    return S.sampled_answers(batch, tok, logp, n_new, args.eos_ids)


def _candidates_enqueue(ctx, batch, args, *seq_slot):
    if args.candidate_list is None:
        raise ValueError("TrainArgs.candidate_list is not set: tst.score.answer_candidates(samples, args.candidates) over the whole data set")
    cand_ids, cu_cand, cand_seq = S.pack_candidates(batch, args.candidate_list)
    if len(cand_seq):   # (a batch of "mca" samples only has nothing to score)
        ids, cu = collate_prompts(batch)
        ctx.score_candidates_async(ids, cu, cand_ids, cu_cand, cand_seq, *seq_slot)


def _candidates_fetch(ctx, batch, args):
    if not any(S.sample_candidates(x, args.candidate_list) for x in batch):
        return [None] * len(batch)
    _, logp_cand = ctx.score_candidates_fetch()
    return S.candidate_scores(batch, args.candidate_list, logp_cand)


def _attribute_enqueue(ctx, batch, args, *seq_slot):
    ids, labels, cu = D.collate(batch)
    ctx.attribute_async(ids, labels, cu, S.attribution_kinds(batch), args.option_ids, *seq_slot)   # MCA and open samples in one batch


def _ig_enqueue(ctx, batch, args, *seq_slot):
    ids, labels, cu = D.collate(batch)
    ctx.attribute_ig_async(ids, labels, cu, S.ig_baseline_ids(batch, args.attribute_baseline_id), args.attribute_ig, S.attribution_kinds(batch), args.option_ids,
                           *seq_slot)


# s(x), pred, correct per sample (tst.score.bias_scores): a fold gets three arrays
SCORE = HeldoutPass(_score_enqueue, lambda ctx, batch, args: list(zip(*S.bias_scores(batch, *ctx.score_rows_fetch()))), _score_join)
# greedy continuation of every prompt by args.max_new_tokens tokens: [(gen ids, gen_correct)] (tst.score.generated_answers)
GENERATE = HeldoutPass(_generate_enqueue, _generate_fetch, list)
# args.sample_n draws per prompt from softmax(logits / args.temperature), one prefill per batch: tst.score.sampled_answers' dict per sample. A pair's draws depend
# on args.sample_seed and its id only, not on the fold layout, the batch or the slot
SAMPLE = HeldoutPass(_sample_enqueue, _sample_fetch, list)
# exact log p(candidate | prompt) over args.candidate_list (+ the sample's own reference) for every "na" sample, one prefill per batch:
# tst.score.candidate_scores' dict per sample (None for "mca")
CANDIDATES = HeldoutPass(_candidates_enqueue, _candidates_fetch, list)
# input-gradient attribution of log s(x): tst.score.token_attribution's dict per sample. About one training forward + backward per batch.
ATTRIBUTE = HeldoutPass(_attribute_enqueue, lambda ctx, batch, args: S.token_attribution(batch, *ctx.attribute_fetch()), list)
# integrated gradients of log s(x), args.attribute_ig steps from a prompt of args.attribute_baseline_id: tst.score.token_ig's dict per sample.
# args.attribute_ig forward + backward passes and two forward passes per batch (measured: DESIGN.md section 14)
IG = HeldoutPass(_ig_enqueue, lambda ctx, batch, args: S.token_ig(batch, *ctx.attribute_ig_fetch()), list)


def run_heldout(p: HeldoutPass, ctx, samples, args: TrainArgs):
    """pass p over one context's held-out fold in batches of per_device_eval_batch_size; results in input order"""
    if p is SCORE and not hasattr(ctx, "score_rows_async"):
        ctx = _SyncScorer(ctx)
    bs = args.per_device_eval_batch_size
    out = []
    for b in range(0, len(samples), bs):
        p.enqueue(ctx, samples[b:b + bs], args)
        out += p.fetch(ctx, samples[b:b + bs], args)
    return p.join(out)


def run_heldout_concurrent(p: HeldoutPass, ctxs, sample_sets, args: TrainArgs):
    """pass p over several resident folds, one per context: batch b of every fold is enqueued before batch b-1's results are read."""
    return _run_heldout_groups(p, ctxs, [[(i, None)] for i in range(len(sample_sets))], sample_sets, args)


def run_heldout_stacked(p: HeldoutPass, ctxs, sample_sets, args: TrainArgs):
    """pass p on stacked contexts: batch b of all folds of a context is one pass, every sequence under its own slot's adapters (place_folds decides the
    slots, the batch is concatenated in slot order); returns the joined results per fold, in the order of sample_sets."""
    where = place_folds(len(sample_sets), ctxs)
    return _run_heldout_groups(p, ctxs, [[(i, sl) for i, (jj, sl) in enumerate(where) if jj == j] for j in range(len(ctxs))], sample_sets, args)


def _run_heldout_groups(p, ctxs, mine, sample_sets, args):
    """mine[j]: the (fold position, slot) pairs context j runs; slot None = a plain context, which gets no seq_slot argument. On a context the previous batch
    is fetched right before the next one is enqueued; batch b goes to every context before batch b + 1 goes to any."""
    bs = args.per_device_eval_batch_size
    outs = [[] for _ in sample_sets]
    pending = [None] * len(ctxs)

    def fetch(j):
        if pending[j] is not None:
            parts = pending[j]   # [(fold position, samples)]
            got = p.fetch(ctxs[j], [x for _, xs in parts for x in xs], args)
            o = 0
            for i, xs in parts:
                outs[i] += got[o:o + len(xs)]
                o += len(xs)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, (c, folds) in enumerate(zip(ctxs, mine)):
            fetch(j)
            parts = [(sl, i, sample_sets[i][b * bs:(b + 1) * bs]) for i, sl in folds]
            parts = [(sl, i, xs) for sl, i, xs in parts if xs]
            if parts:
                seq_slot = [] if parts[0][0] is None else [np.concatenate([np.full(len(xs), sl, np.int32) for sl, _, xs in parts])]
                p.enqueue(c, [x for _, _, xs in parts for x in xs], args, *seq_slot)
                pending[j] = [(i, xs) for _, i, xs in parts]
    for j in range(len(ctxs)):
        fetch(j)
    return [p.join(o) for o in outs]


class _SyncScorer:
    """score_rows_async / score_rows_fetch over a model that only has the synchronous score_rows (the oracle models)"""

    def __init__(self, model):
        self.model = model

    def score_rows_async(self, *batch):
        self.rows = self.model.score_rows(*batch)

    def score_rows_fetch(self):
        return self.rows


def score_heldout(ctx, samples, args: TrainArgs):
    """forward-only pass over the held-out fold; returns s(x), pred, correct per sample (batch order = input order)."""
    return run_heldout(SCORE, ctx, samples, args)


def generate_heldout(ctx, samples, args: TrainArgs):
    """greedy continuation of every held-out prompt; returns [(gen ids, gen_correct)] per sample in input order."""
    return run_heldout(GENERATE, ctx, samples, args)


def sample_heldout(ctx, samples, args: TrainArgs):
    """args.sample_n sampled continuations of every held-out prompt; returns tst.score.sampled_answers' dict per sample in input order."""
    return run_heldout(SAMPLE, ctx, samples, args)


def candidates_heldout(ctx, samples, args: TrainArgs):
    """the model's distribution over the candidate answers for every held-out "na" sample; returns tst.score.candidate_scores' dict (None for "mca") per sample."""
    return run_heldout(CANDIDATES, ctx, samples, args)


def attribute_heldout(ctx, samples, args: TrainArgs):
    """input-gradient attribution of log s(x) for every held-out sample; returns tst.score.token_attribution's dict per sample in input order."""
    return run_heldout(ATTRIBUTE, ctx, samples, args)


def attribute_ig_heldout(ctx, samples, args: TrainArgs):
    """integrated gradients of log s(x) for every held-out sample; returns tst.score.token_ig's dict per sample in input order."""
    return run_heldout(IG, ctx, samples, args)


# ---------------------------------------------------------------------------------------------- stacked folds
def place_folds(n, ctxs):
    """n folds over contexts with n_stack slots each, as evenly as the slots allow: [(context index, slot)] per fold."""
    caps = [getattr(c, "n_stack", 1) for c in ctxs]
    if n > sum(caps):
        raise ValueError(f"{n} folds do not fit {sum(caps)} slots")
    take = [0] * len(ctxs)
    for _ in range(n):   # next fold goes to the least-filled context that still has a free slot
        j = min((j for j in range(len(ctxs)) if take[j] < caps[j]), key=lambda j: (take[j], j))
        take[j] += 1
    out, j, sl = [], 0, 0
    for _ in range(n):   # consecutive folds share a context
        while sl >= take[j]:
            j, sl = j + 1, 0
        out.append((j, sl))
        sl += 1
    return out


def collate_stacked(parts):
    """parts: [(slot, samples)] in slot order -> ids, labels, cu, seq_slot of the concatenated micro-batch"""
    flat = [x for _, b in parts for x in b]
    ids, labels, cu = D.collate(flat)
    seq_slot = np.concatenate([np.full(len(b), sl, np.int32) for sl, b in parts])
    return ids, labels, cu, seq_slot


def fine_tune_stacked(ctxs, sample_sets, args: TrainArgs, fold_seeds, log=None, dp=None):
    """the folds' fine-tunes in lockstep on stacked contexts (include/tst_hip.h "stacked folds"): step i of every fold placed
    on a context is ONE device step over the concatenated micro-batches; several contexts (root + forks) are fed round-robin
    like fine_tune_concurrent. Each fold follows the same plan (batches, learning rates, seeds) as fine_tune() on it alone.
    Returns one list of log records per fold.
    dp = (rank, world): the "dp-stacked" layout -- every rank hosts all these folds and walks the SAME plan over global batches of
    world x per_device_train_batch_size samples, runs its own micro-batch of each and joins the context's gradient all-reduce
    (tst_train_step_stacked_dp_async; the contexts have joined their communicators: tst/ddp.py init_stacked_groups)."""
    _t_begin = time.perf_counter()
    rank, world = dp if dp else (0, 1)
    G = max(1, args.gradient_accumulation_steps)
    if dp and G > 1:
        raise ValueError("gradient accumulation inside the dp-stacked layout is not built: enlarge the group instead")
    where = place_folds(len(sample_sets), ctxs)
    plans = [[] for _ in ctxs]   # per context: [(slot, fold position, plan iterator)]
    for i, ((j, sl), smp, fs) in enumerate(zip(where, sample_sets, fold_seeds)):
        ctxs[j].select_slot(sl)
        ctxs[j].reset_trainable(seed=args.seed * 1000 + fs)
        plans[j].append((sl, i, train_plan(smp, args, fs, world)))
    records = [[] for _ in sample_sets]
    pending = [None] * len(ctxs)
    _t_setup = time.perf_counter()

    def fetch(j):
        if pending[j]:
            loss, gn = ctxs[j].fetch_metrics_stacked()
            for sl, i, step, lr in pending[j]:
                records[i].append(dict(step=step, loss=float(loss[sl]), grad_norm=float(gn[sl]), lr=lr))
                if log:
                    log(dict(records[i][-1], slot=i))
        pending[j] = None

    live = True
    while live:
        live = False
        for j, c in enumerate(ctxs):
            parts, lrs, want = [], np.zeros(c.n_stack, np.float32), []
            for sl, i, plan in plans[j]:
                nxt = next(plan, None)
                if nxt is None:
                    continue
                step, total, lr, batch = nxt
                parts.append((sl, batch))
                lrs[sl] = lr
                if args.logging_steps and (step % args.logging_steps == 0 or step == total):
                    want.append((sl, i, step, lr))
            fetch(j)   # metrics of this context's previous step, before the next one overwrites them
            if not parts:
                continue
            live = True
            if dp:
                items = np.zeros(c.n_stack, np.int32)
                for sl, upd in parts:
                    items[sl] = D.count_labelled(upd)          # the slot's labelled tokens over ALL ranks (every rank derives it from the same plan)
                mine = [(sl, mb[0]) for sl, upd in parts for mb in [micro_batches(upd, args, rank, world)] if mb]
                if mine:
                    ids, labels, cu, seq_slot = collate_stacked(mine)
                    c.train_step_stacked_dp_async(ids, labels, cu, seq_slot, lrs, items)
                else:                                          # the ragged end of an epoch left nothing for this rank: it still joins the all-reduce
                    c.train_step_stacked_dp_async(None, None, None, None, lrs, items)
            elif G > 1:
                items = np.zeros(c.n_stack, np.int32)
                mbs = {}
                for sl, upd in parts:
                    items[sl] = D.count_labelled(upd)
                    mbs[sl] = micro_batches(upd, args)
                for m in range(max(len(v) for v in mbs.values())):
                    ids, labels, cu, seq_slot = collate_stacked([(sl, v[m]) for sl, v in sorted(mbs.items()) if m < len(v)])
                    c.accumulate_async(ids, labels, cu, items, first=(m == 0), seq_slot=seq_slot)
                c.optimizer_step_async(lrs)
            else:
                ids, labels, cu, seq_slot = collate_stacked(parts)
                c.train_step_stacked_async(ids, labels, cu, seq_slot, lrs)
            pending[j] = want
    _t_enq = time.perf_counter()
    for j, c in enumerate(ctxs):
        fetch(j)
        c.sync()
        c.select_slot(0)
    if os.environ.get("TST_PHASE_LOG"):
        import sys
        print(f"[phase] fine_tune_stacked: resets + plans {_t_setup - _t_begin:.3f} s, enqueue loop {_t_enq - _t_setup:.3f} s, final sync {time.perf_counter() - _t_enq:.3f} s", file=sys.stderr)
    return records
