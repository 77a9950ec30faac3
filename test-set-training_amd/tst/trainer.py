"""Per-fold fine-tune + held-out scoring loop (SURVEY.md §3 stacks (2) and (3)): the role of HF Trainer.train /
Trainer.predict (HF/trainer.py:1347-1796, 2860-3010) for this one path, driving libtst_hip through the C-ABI.

Hyper-parameter names and defaults mirror HF TrainingArguments (training_args.py:767-856: lr 5e-5, linear schedule,
AdamW 0.9/0.999/1e-8, wd 0, max_grad_norm 1.0, 3 epochs, seed 42) so a future upstream CLI maps 1:1; the per-device
batch of 16 is the value BASELINE.md fixes for the metric."""
import os
import time
from dataclasses import InitVar, dataclass

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

    def __post_init__(self, attribute, attribute_top, attribute_ig, attribute_baseline_id):
        self.attribute, self.attribute_top = bool(attribute), int(attribute_top)
        self.attribute_ig, self.attribute_baseline_id = int(attribute_ig), int(attribute_baseline_id)


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


def score_heldout_concurrent(ctxs, sample_sets, args: TrainArgs):
    """held-out scoring of several resident folds: batch b of every fold is enqueued before batch b-1's results are read."""
    bs = args.per_device_eval_batch_size
    outs = [([], [], []) for _ in ctxs]
    pending = [None] * len(ctxs)

    def fetch(j):
        if pending[j] is not None:
            logp, corr, optl, rseq = ctxs[j].score_rows_fetch()
            s, p, c = S.bias_scores(pending[j], logp, corr, optl, rseq)
            outs[j][0].append(s); outs[j][1].append(p); outs[j][2].append(c)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, (c, smp) in enumerate(zip(ctxs, sample_sets)):
            fetch(j)
            batch = smp[b * bs:(b + 1) * bs]
            if batch:
                ids, labels, cu = D.collate(batch)
                c.score_rows_async(ids, labels, cu, args.option_ids)
                pending[j] = batch
    for j in range(len(ctxs)):
        fetch(j)
    empty_f, empty_i = np.zeros(0, np.float32), np.zeros(0, np.int32)
    return [(np.concatenate(o[0]) if o[0] else empty_f, np.concatenate(o[1]) if o[1] else empty_i, np.concatenate(o[2]) if o[2] else empty_i) for o in outs]


def score_heldout(ctx, samples, args: TrainArgs):
    """forward-only pass over the held-out fold; returns s(x), pred, correct per sample (batch order = input order)."""
    bs = args.per_device_eval_batch_size
    s_all, p_all, c_all = [], [], []
    for b in range(0, len(samples), bs):
        batch = samples[b:b + bs]
        ids, labels, cu = D.collate(batch)
        logp, corr, optl, rseq = ctx.score_rows(ids, labels, cu, args.option_ids)
        s, p, c = S.bias_scores(batch, logp, corr, optl, rseq)
        s_all.append(s); p_all.append(p); c_all.append(c)
    return np.concatenate(s_all), np.concatenate(p_all), np.concatenate(c_all)


# ---------------------------------------------------------------------------------------------- greedy answers of the held-out fold
def collate_prompts(samples):
    """packed prompts (ids[:n_prompt] of every sample): ids, cu_seqlens"""
    ids = np.concatenate([s.ids[:s.n_prompt] for s in samples]).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum([s.n_prompt for s in samples])]).astype(np.int32)
    return ids, cu


def generate_heldout(ctx, samples, args: TrainArgs):
    """greedy continuation of every held-out prompt (Context.generate, batches of per_device_eval_batch_size); returns [(gen ids, gen_correct)]
    per sample in input order (tst.score.generated_answers)."""
    bs = args.per_device_eval_batch_size
    out = []
    for b in range(0, len(samples), bs):
        batch = samples[b:b + bs]
        ids, cu = collate_prompts(batch)
        tok, _, n_new = ctx.generate(ids, cu, args.max_new_tokens, args.eos_ids)
        out += S.generated_answers(batch, tok, n_new, args.eos_ids)
    return out


def generate_heldout_concurrent(ctxs, sample_sets, args: TrainArgs):
    """generate_heldout for several resident folds: batch b of every fold is enqueued before batch b-1's results are read."""
    bs = args.per_device_eval_batch_size
    outs = [[] for _ in ctxs]
    pending = [None] * len(ctxs)

    def fetch(j):
        if pending[j] is not None:
            tok, _, n_new = ctxs[j].generate_fetch()
            outs[j] += S.generated_answers(pending[j], tok, n_new, args.eos_ids)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, (c, smp) in enumerate(zip(ctxs, sample_sets)):
            fetch(j)
            batch = smp[b * bs:(b + 1) * bs]
            if batch:
                ids, cu = collate_prompts(batch)
                c.generate_async(ids, cu, args.max_new_tokens, args.eos_ids)
                pending[j] = batch
    for j in range(len(ctxs)):
        fetch(j)
    return outs


def generate_heldout_stacked(ctxs, sample_sets, args: TrainArgs):
    """generate_heldout on stacked contexts: batch b of all folds of a context is one generation, every sequence under its own slot's adapters;
    returns [(gen ids, gen_correct)] per fold, in the order of sample_sets."""
    where = place_folds(len(sample_sets), ctxs)
    bs = args.per_device_eval_batch_size
    outs = [[] for _ in sample_sets]
    pending = [None] * len(ctxs)
    mine = [[(sl, i) for i, (jj, sl) in enumerate(where) if jj == j] for j in range(len(ctxs))]

    def fetch(j):
        if pending[j] is not None:
            parts = pending[j]   # [(fold position, samples)]
            tok, _, n_new = ctxs[j].generate_fetch()
            got = S.generated_answers([x for _, b in parts for x in b], tok, n_new, args.eos_ids)
            o = 0
            for i, b in parts:
                outs[i] += got[o:o + len(b)]
                o += len(b)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, c in enumerate(ctxs):
            fetch(j)
            parts = [(sl, i, sample_sets[i][b * bs:(b + 1) * bs]) for sl, i in mine[j]]
            parts = [(sl, i, x) for sl, i, x in parts if x]
            if parts:
                ids, cu = collate_prompts([x for _, _, xs in parts for x in xs])
                seq_slot = np.concatenate([np.full(len(xs), sl, np.int32) for sl, _, xs in parts])
                c.generate_async(ids, cu, args.max_new_tokens, args.eos_ids, seq_slot)
                pending[j] = [(i, xs) for _, i, xs in parts]
    for j in range(len(ctxs)):
        fetch(j)
    return outs


# ---------------------------------------------------------------------------------------------- token attribution of the held-out fold
def _attribute_async(ctx, batch, args: TrainArgs, seq_slot=None):
    ids, labels, cu = D.collate(batch)
    ctx.attribute_async(ids, labels, cu, S.attribution_kinds(batch), args.option_ids, seq_slot)   # MCA and open samples in one batch


def _ig_async(ctx, batch, args: TrainArgs, seq_slot=None):
    ids, labels, cu = D.collate(batch)
    ctx.attribute_ig_async(ids, labels, cu, S.ig_baseline_ids(batch, args.attribute_baseline_id), args.attribute_ig, S.attribution_kinds(batch), args.option_ids,
                           seq_slot)


# what the three held-out drivers below run: (enqueue on a context, turn a fetched batch into per-sample dicts)
_ATTR = (_attribute_async, lambda ctx, batch: S.token_attribution(batch, *ctx.attribute_fetch()))
_IG = (_ig_async, lambda ctx, batch: S.token_ig(batch, *ctx.attribute_ig_fetch()))


def attribute_ig_heldout(ctx, samples, args: TrainArgs):
    """integrated gradients of log s(x) for every held-out sample (Context.attribute_ig: args.attribute_ig steps from a prompt of args.attribute_baseline_id);
    returns tst.score.token_ig's dict per sample in input order. args.attribute_ig forward + backward passes and two forward passes per batch (measured: DESIGN.md section 14)."""
    return attribute_heldout(ctx, samples, args, _IG)


def attribute_ig_heldout_concurrent(ctxs, sample_sets, args: TrainArgs):
    """attribute_ig_heldout for several resident folds (as attribute_heldout_concurrent)"""
    return attribute_heldout_concurrent(ctxs, sample_sets, args, _IG)


def attribute_ig_heldout_stacked(ctxs, sample_sets, args: TrainArgs):
    """attribute_ig_heldout on stacked contexts (as attribute_heldout_stacked)"""
    return attribute_heldout_stacked(ctxs, sample_sets, args, _IG)


def attribute_heldout(ctx, samples, args: TrainArgs, how=_ATTR):
    """input-gradient attribution of log s(x) for every held-out sample (Context.attribute, batches of per_device_eval_batch_size); returns
    tst.score.token_attribution's dict per sample in input order. About one training forward + backward per batch."""
    bs = args.per_device_eval_batch_size
    out = []
    for b in range(0, len(samples), bs):
        batch = samples[b:b + bs]
        how[0](ctx, batch, args)
        out += how[1](ctx, batch)
    return out


def attribute_heldout_concurrent(ctxs, sample_sets, args: TrainArgs, how=_ATTR):
    """attribute_heldout for several resident folds: batch b of every fold is enqueued before batch b-1's results are read."""
    bs = args.per_device_eval_batch_size
    outs = [[] for _ in ctxs]
    pending = [None] * len(ctxs)

    def fetch(j):
        if pending[j] is not None:
            outs[j] += how[1](ctxs[j], pending[j])
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, (c, smp) in enumerate(zip(ctxs, sample_sets)):
            fetch(j)
            batch = smp[b * bs:(b + 1) * bs]
            if batch:
                how[0](c, batch, args)
                pending[j] = batch
    for j in range(len(ctxs)):
        fetch(j)
    return outs


def attribute_heldout_stacked(ctxs, sample_sets, args: TrainArgs, how=_ATTR):
    """attribute_heldout on stacked contexts: batch b of all folds of a context is one attribution, every sequence under its own slot's adapters;
    returns the per-sample dicts per fold, in the order of sample_sets."""
    where = place_folds(len(sample_sets), ctxs)
    bs = args.per_device_eval_batch_size
    outs = [[] for _ in sample_sets]
    pending = [None] * len(ctxs)
    mine = [[(sl, i) for i, (jj, sl) in enumerate(where) if jj == j] for j in range(len(ctxs))]

    def fetch(j):
        if pending[j] is not None:
            parts = pending[j]   # [(fold position, samples)]
            got = how[1](ctxs[j], [x for _, b in parts for x in b])
            o = 0
            for i, b in parts:
                outs[i] += got[o:o + len(b)]
                o += len(b)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, c in enumerate(ctxs):
            fetch(j)
            parts = [(sl, i, sample_sets[i][b * bs:(b + 1) * bs]) for sl, i in mine[j]]
            parts = [(sl, i, x) for sl, i, x in parts if x]
            if parts:
                seq_slot = np.concatenate([np.full(len(xs), sl, np.int32) for sl, _, xs in parts])
                how[0](c, [x for _, _, xs in parts for x in xs], args, seq_slot)
                pending[j] = [(i, xs) for _, i, xs in parts]
    for j in range(len(ctxs)):
        fetch(j)
    return outs


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


def score_heldout_stacked(ctxs, sample_sets, args: TrainArgs):
    """held-out scoring on stacked contexts: batch b of all folds of a context is one forward pass; returns (s, pred, correct)
    per fold, in the order of sample_sets."""
    where = place_folds(len(sample_sets), ctxs)
    bs = args.per_device_eval_batch_size
    outs = [([], [], []) for _ in sample_sets]
    pending = [None] * len(ctxs)
    mine = [[(sl, i) for i, (jj, sl) in enumerate(where) if jj == j] for j in range(len(ctxs))]

    def fetch(j):
        if pending[j] is not None:
            parts = pending[j]   # [(fold position, samples)]
            logp, corr, optl, rseq = ctxs[j].score_rows_fetch()
            flat = [x for _, b in parts for x in b]
            s, p, c = S.bias_scores(flat, logp, corr, optl, rseq)
            o = 0
            for i, b in parts:
                outs[i][0].append(s[o:o + len(b)]); outs[i][1].append(p[o:o + len(b)]); outs[i][2].append(c[o:o + len(b)])
                o += len(b)
            pending[j] = None

    nb = max((len(smp) + bs - 1) // bs for smp in sample_sets) if sample_sets else 0
    for b in range(nb):
        for j, c in enumerate(ctxs):
            fetch(j)
            parts = [(sl, i, sample_sets[i][b * bs:(b + 1) * bs]) for sl, i in mine[j]]
            parts = [(sl, i, x) for sl, i, x in parts if x]
            if parts:
                ids, labels, cu, seq_slot = collate_stacked([(sl, x) for sl, _, x in parts])
                c.score_rows_async(ids, labels, cu, args.option_ids, seq_slot)
                pending[j] = [(i, x) for _, i, x in parts]
    for j in range(len(ctxs)):
        fetch(j)
    empty_f, empty_i = np.zeros(0, np.float32), np.zeros(0, np.int32)
    return [(np.concatenate(o[0]) if o[0] else empty_f, np.concatenate(o[1]) if o[1] else empty_i, np.concatenate(o[2]) if o[2] else empty_i) for o in outs]
