"""Deterministic inputs of the token-attribution fixtures (tests/golden/attr_<tag>.npz), shared by tools/make_golden.py attr (which feeds them to the HF
models) and by the tests (HIP path). Built on tests/golden_inputs.py / tests/qwen3_inputs.py: the same numpy Generator streams; the fixtures hold OUTPUTS only."""
import numpy as np

import golden_inputs as GI
import qwen3_inputs as Q3

LENGTHS, N_ANSWER = (7, 48, 100, 130), (1, 2, 3, 1)   # 130 crosses the 128-token attention path
GPT2_LENGTHS = (7, 33, 64, 100)                       # (wpe has 128 rows)
TAGS = dict(tiny=(GI.TINY_CFG, GI.make_weights), tiny2=(GI.TINY2_CFG, GI.make_weights), qwen=(GI.QWEN_CFG, GI.make_weights),
            qwen3=(Q3.QWEN3_CFG, Q3.make_weights), gpt2=(GI.GPT2_CFG, GI.make_weights))
# two fixture sets: "mix" = the two 1-answer sequences in the option form (kind 1), the others open; "open" = every sequence open
SETS = dict(mix=(1, 0, 0, 1), open=(0, 0, 0, 0))
# adapters: none (all-zero B on the device), and the LoRA sets of seeds 99 and 7 (GI.make_lora)
ADAPTERS = dict(base=None, l99=99, l7=7)
OUTPUTS = ("gxi", "gnorm")


def batch(tag):
    cfg = TAGS[tag][0]
    return GI.make_batch(cfg, GPT2_LENGTHS if cfg.get("arch") == "gpt2" else LENGTHS, N_ANSWER, seed=7)


def option_ids(tag):
    """4 option ids: the targets of the two 1-answer sequences, filled up with the first of 3, 9, 27, 81, 5, 6 that are not among them"""
    ids, labels, cu = batch(tag)
    out = []
    for s in range(len(cu) - 1):
        lab = labels[cu[s]:cu[s + 1]]
        if (lab != -100).sum() == 1 and int(lab[-1]) not in out:
            out.append(int(lab[-1]))
    for c in (3, 9, 27, 81, 5, 6):
        if len(out) < 4 and c not in out:
            out.append(c)
    return np.array(out, np.int32)


def lora(tag, seed):
    return GI.make_lora(TAGS[tag][0], seed=seed)


def zero_lora(tag):
    """the base model as a LoRA context sees it: random A, B = 0"""
    lo = lora(tag, 99)
    return {k: (np.zeros_like(v) if k.endswith("lora_B") else v) for k, v in lo.items()}


def seq_dev(x, ref, cu):
    """per sequence: max_t |x - ref| / max_t |ref|"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return np.array([np.abs(x[cu[s]:cu[s + 1]] - ref[cu[s]:cu[s + 1]]).max() / np.abs(ref[cu[s]:cu[s + 1]]).max() for s in range(len(cu) - 1)])
