"""Deterministic inputs of the integrated-gradients fixtures (tests/golden/ig_<tag>.npz), shared by tools/make_golden.py ig (which feeds them to the HF models)
and by the tests (HIP path). Built on tests/attribution_inputs.py: the same batch, option ids, fixture sets and adapter sets; the fixtures hold OUTPUTS only."""
import numpy as np

import attribution_inputs as AI

STEPS, STEPS_FINE = 16, 64   # the fixtures' step count, and the one of the generator's completeness self-check (ref_ig64, delta_ref64, ref_gap64)
BASELINE_ID = 1
# baseline patterns: "all" = BASELINE_ID on every token; "prompt" = BASELINE_ID on unlabelled positions, the token's own id on labelled ones
PATTERNS = ("all", "prompt")


def baseline_ids(tag, pattern):
    ids, labels, cu = AI.batch(tag)
    base = np.full_like(ids, BASELINE_ID)
    if pattern == "prompt":
        base = np.where(labels != -100, ids, base)
    elif pattern != "all":
        raise KeyError(pattern)
    return base.astype(np.int32)


def alpha(k, m):
    """midpoint k = 1 .. m of the path, in fp32 as the library forms it: (k - 1/2) / m"""
    return (np.float32(k) - np.float32(0.5)) / np.float32(m)


def key(sname, pattern, adapter):
    return f"{sname}/{pattern}/{adapter}/"
