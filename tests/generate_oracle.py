"""TEST INFRASTRUCTURE -- the definition of greedy decoding, with no cache: re-run the pinned oracle's forward_logits on the growing sequences and take the
arg-max (first index of the maximum, numpy.argmax). Shared inputs of tests/test_generate_gpu.py and tests/test_generate_cpu.py live here too, and every
reference is computed once per process and kept."""
import functools

import numpy as np

import families as FAM
import golden_inputs as GI
import qwen3_inputs as Q3
from qwen3_oracle import Qwen3Oracle

MAX_NEW = 8
LENS_ROPE = (1, 5, 17, 63, 64, 65, 100, 125, 130)   # length 1, the 64-key boundaries, sequences that cross 128 tokens while decoding
LENS_GPT2 = (1, 5, 17, 33, 63, 64, 65, 100)         # max_position is 128
FAMILIES = {"tiny": GI.TINY_CFG, "tiny2": GI.TINY2_CFG, "qwen": GI.QWEN_CFG, "gpt2": GI.GPT2_CFG, "qwen3": Q3.QWEN3_CFG}


def lens_of(cfg):
    return LENS_GPT2 if cfg.get("arch") == "gpt2" else LENS_ROPE


def make_prompts(cfg):
    rng = np.random.default_rng(31)
    return [rng.integers(0, cfg["vocab_size"], n).astype(np.int32) for n in lens_of(cfg)]


def pack(seqs):
    ids = np.concatenate([np.asarray(s, np.int32) for s in seqs]).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    return ids, cu


@functools.lru_cache(maxsize=None)
def weights(tag):
    return Q3.make_weights() if tag == "qwen3" else GI.make_weights(FAMILIES[tag])


@functools.lru_cache(maxsize=None)
def lora(tag, seed):
    return GI.make_lora(FAMILIES[tag], seed=seed)


def make_oracle(tag, lora_seed=None, bf16=False):
    cfg = FAMILIES[tag]
    args = (cfg, weights(tag)) + ((lora(tag, lora_seed), GI.LORA_R, GI.LORA_ALPHA) if lora_seed is not None else ())
    return Qwen3Oracle(*args, bf16=bf16) if tag == "qwen3" else FAM.oracle(*args, bf16=bf16)


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def greedy(orc, prompts, max_new=MAX_NEW):
    """tokens [n, max_new], logp [n, max_new] (log-softmax at the token), logits [n, max_new, V]: max_new full forwards over the growing batch"""
    seqs = [list(map(int, p)) for p in prompts]
    n = len(seqs)
    tokens, logp, logits = np.zeros((n, max_new), np.int32), np.zeros((n, max_new)), []
    for j in range(max_new):
        ids, cu = pack(seqs)
        lg = np.asarray(orc.forward_logits(ids, cu, cu[1:] - 1), np.float64)
        tok = lg.argmax(-1)
        tokens[:, j] = tok
        logp[:, j] = log_softmax(lg)[np.arange(n), tok]
        logits.append(lg)
        for s in range(n):
            seqs[s].append(int(tok[s]))
    return tokens, logp, np.stack(logits, 1)


@functools.lru_cache(maxsize=None)
def greedy_reference(tag, lora_seed=None):
    """the fp32 oracle's greedy continuation of the shared prompts of a family (base model, or with the LoRA adapters of `lora_seed`)"""
    return greedy(make_oracle(tag, lora_seed), make_prompts(FAMILIES[tag]))


def replay_rows(prompts, tokens):
    """the generated sequences packed, and the rows whose logits chose each generated token: (ids, cu, rows [n * max_new])"""
    seqs = [np.concatenate([p, t]) for p, t in zip(prompts, tokens)]
    ids, cu = pack(seqs)
    m = tokens.shape[1]
    rows = np.concatenate([cu[s] + len(p) - 1 + np.arange(m) for s, p in enumerate(prompts)]).astype(np.int32)
    return ids, cu, rows
