"""HF-signature shim over a Context (Python level): the objects an upstream fine-tuning script holds -- a causal-LM
`model(input_ids[B,S], attention_mask[B,S], labels[B,S]) -> (loss, logits)` (HF/models/llama/modeling_llama.py:438-492) and an
`optimizer.step() / zero_grad()` (TORCH/optim/adam.py:215) -- with libtst_hip underneath, so a loop written against HF swaps 1:1:

    model = TstModel(ctx)                        # ctx: tst.lib.Context (weights loaded)
    opt = TstOptimizer(model, lr=5e-5)           # AdamW + global-norm clip live inside the context (cfg: betas, eps, wd, max_grad_norm)
    sched = TstLinearSchedule(opt, total_steps)  # HF/optimization.py:101-104
    for batch in loader:                         # right-padded int tensors / arrays, labels -100 outside the answers
        out = model(**batch)                     # forward AND backward run here (no autograd graph exists to defer it to)
        out.loss.backward()                      # accepted, nothing left to do
        opt.step(); sched.step(); opt.zero_grad()

Differences from torch that a caller can see, all by construction of the engine:
  * in train mode the backward pass runs inside model(...): gradients exist when the call returns; `loss.backward()` is a no-op;
  * several model(...) calls before optimizer.step() accumulate (gradient accumulation), like torch's .grad: pass HF's
    `num_items_in_batch` (trainer.py:2141-2175) to normalise every micro-batch by the whole update's labelled tokens;
  * `out.logits` is computed on first access by an extra forward-only pass (the train step keeps no [B,S,V] tensor: the LM head runs on
    the labelled rows only) and needs max_labelled >= tokens of the batch;
  * tensors are numpy arrays (torch tensors are accepted and converted on the host; logits come back as numpy).
Pad tokens are dropped on the way in (tst.data.from_padded): the packed batch is exact for the real tokens."""
import numpy as np

from . import data as D


def _np(a):
    if a is None:
        return None
    if hasattr(a, "detach"):   # torch tensor
        a = a.detach().cpu().numpy()
    return np.asarray(a)


class TstLoss(float):
    """the loss value; .backward() exists so a torch-style loop runs unchanged (the backward pass already ran inside model(...))"""

    def backward(self):
        return None

    def item(self):
        return float(self)


class TstOutput:
    """the two fields of CausalLMOutputWithPast a fine-tuning loop reads; also unpacks like the (loss, logits) tuple"""

    def __init__(self, loss, logits_fn):
        self.loss = loss
        self._logits_fn, self._logits = logits_fn, None

    @property
    def logits(self):
        if self._logits is None:
            self._logits = self._logits_fn()
        return self._logits

    def __iter__(self):
        yield self.loss
        yield self.logits

    def __getitem__(self, i):
        return (self.loss, self.logits)[i]


class TstModel:
    def __init__(self, ctx):
        self.ctx = ctx
        self.training = True
        self._window_open = False   # gradients of earlier model(...) calls are waiting for optimizer.step()

    # ---- nn.Module surface a training loop touches
    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def zero_grad(self, set_to_none=True):
        self._window_open = False

    def state_dict(self):
        """trainable tensors by name (LoRA: layers.N.<module>.lora_A / lora_B; full fine-tune: HF state_dict names)"""
        return self.ctx.get_trainable()

    def load_state_dict(self, sd):
        self.ctx.set_trainable(sd)

    # ---- forward (+ backward in train mode)
    def __call__(self, input_ids, attention_mask=None, labels=None, num_items_in_batch=None, **_unused):
        input_ids = _np(input_ids)
        if input_ids.ndim != 2:
            raise ValueError("input_ids must be [batch, seq]")
        mask = _np(attention_mask) if attention_mask is not None else np.ones_like(input_ids)
        lab2 = _np(labels) if labels is not None else np.full(input_ids.shape, -100, np.int64)
        ids, lab, cu = D.from_padded(input_ids, mask, lab2)
        loss = None
        if labels is not None and self.training:
            items = int(num_items_in_batch) if num_items_in_batch is not None else _count(lab, cu)
            self.ctx.accumulate_async(ids, lab, cu, items, first=not self._window_open)
            self._window_open = True
            # the loss of THIS micro-batch under the normalisation it was given (what HF's forward returns); the accumulated sum is what
            # optimizer.step() reports through fetch_metrics
            loss = TstLoss(float(self.ctx.fetch_loss()[0]))
        elif labels is not None:
            loss = TstLoss(self._eval_loss(ids, lab, cu, num_items_in_batch))
        B, S = input_ids.shape
        lens = np.diff(cu)

        def logits():
            rows = np.arange(len(ids), dtype=np.int32)
            flat = self.ctx.forward_logits(ids, cu, rows)
            out = np.zeros((B, S, flat.shape[1]), np.float32)
            for b in range(B):
                out[b, :lens[b]] = flat[cu[b]:cu[b + 1]]
            return out

        return TstOutput(loss, logits)

    forward = __call__

    def generate(self, input_ids, attention_mask=None, max_new_tokens=20, eos_token_id=None, pad_token_id=None, **_unused):
        """greedy GenerationMixin.generate for RIGHT-padded inputs (HF/generation/utils.py: do_sample False, num_beams 1): returns the HF-shaped
        [B, S + max_new_tokens] int64 array -- every row its prompt, then its new tokens up to and including the first eos, then padding (pad_token_id,
        default the first eos id, else 0). Unlike HF, whose decoder-only models want LEFT padding, the new tokens follow each row's own end."""
        input_ids = _np(input_ids)
        if input_ids.ndim != 2:
            raise ValueError("input_ids must be [batch, seq]")
        mask = _np(attention_mask) if attention_mask is not None else np.ones_like(input_ids)
        ids, _, cu = D.from_padded(input_ids, mask, np.zeros_like(input_ids))
        eos = () if eos_token_id is None else tuple(int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id]))
        tok, _, n_new = self.ctx.generate(ids, cu, int(max_new_tokens), eos)
        pad = int(pad_token_id) if pad_token_id is not None else (eos[0] if eos else 0)
        B, S = input_ids.shape
        out = np.full((B, S + int(max_new_tokens)), pad, np.int64)
        lens = np.diff(cu)
        for b in range(B):
            out[b, :lens[b]] = input_ids[b, :lens[b]]
            out[b, lens[b]:lens[b] + n_new[b]] = tok[b, :n_new[b]]
        return out

    def _eval_loss(self, ids, lab, cu, num_items):
        logp, _, _, _ = self.ctx.score_rows(ids, lab, cu, ())
        n = int(num_items) if num_items is not None else len(logp)
        return float(-np.sum(logp.astype(np.float64)) / max(1, n))


def _count(lab, cu):
    """labelled tokens of a packed batch after the one-token shift (trainer.py:2141-2175: position p predicts labels[p + 1])"""
    n = 0
    for b in range(len(cu) - 1):
        n += int(np.count_nonzero(lab[cu[b] + 1:cu[b + 1]] != -100))
    return n


class TstOptimizer:
    """AdamW + clip_grad_norm_ as the context runs them (TORCH/optim/adam.py:347-547, clip_grad.py:50-183; hyper-parameters fixed at context
    creation). param_groups[0]["lr"] is read at every step, so any scheduler that writes it works."""

    def __init__(self, model, lr=5e-5):
        self.model = model
        self.param_groups = [dict(lr=float(lr), initial_lr=float(lr))]
        self.last_loss = self.last_grad_norm = None

    def step(self):
        ctx = self.model.ctx
        if not self.model._window_open:
            raise RuntimeError("optimizer.step() without a backward pass since the last step / zero_grad")
        ctx.optimizer_step_async(self.param_groups[0]["lr"])
        self.last_loss, self.last_grad_norm = ctx.fetch_metrics()   # loss = sum over the window's micro-batches, norm = before clipping
        self.model._window_open = False
        return self.last_loss

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad()

    def state_dict(self):
        return self.model.ctx.state()

    def load_state_dict(self, st):
        self.model.ctx.load_state(st)


class TstLinearSchedule:
    """get_linear_schedule_with_warmup (HF/optimization.py:101-104): step() after every optimizer.step()"""

    def __init__(self, optimizer, num_training_steps, num_warmup_steps=0):
        self.opt, self.total, self.warm, self.t = optimizer, int(num_training_steps), int(num_warmup_steps), 0
        self._set()

    def _set(self):
        from .trainer import linear_lr
        g = self.opt.param_groups[0]
        g["lr"] = linear_lr(self.t, self.total, g["initial_lr"], self.warm)

    def step(self):
        self.t += 1
        self._set()

    def get_last_lr(self):
        return [self.opt.param_groups[0]["lr"]]
