"""Deterministic inputs of the Qwen3 family (per-head q/k RMSNorm, modeling_qwen3.py:237-238, 252-253), shared by tools/make_golden.py (which feeds them to
transformers.Qwen3ForCausalLM) and by the tests (oracle and HIP path). Built on tests/golden_inputs.py: the same numpy Generator streams, plus the two
head-norm vectors of every layer."""
import numpy as np

import golden_inputs as GI

# 4 query heads / 2 key-value heads of head_dim 128 on a hidden size of 256: num_heads * head_dim = 512 != hidden_size, as at several Qwen3 sizes
QWEN3_CFG = dict(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=128, intermediate_size=256,
                 rope_theta=1000000.0, rms_norm_eps=1e-6, qk_norm=True)
LENGTHS, N_ANSWER = (7, 48, 100), (1, 2, 3)


def head_norm_names(cfg):
    return [f"model.layers.{l}.self_attn.{m}.weight" for l in range(cfg["num_layers"]) for m in ("q_norm", "k_norm")]


def _with_head_norms(cfg, w, seed, bf16_exact):
    """q_norm / k_norm ~ 1 + 0.1 N(0, 1), ONE element of each exactly 0 (a zero weight element is legal: the backward must never divide by w)"""
    rng = np.random.default_rng(seed)
    for i, name in enumerate(head_norm_names(cfg)):
        a = (1.0 + 0.1 * rng.standard_normal(cfg["head_dim"])).astype(np.float32)
        a = GI.bf16_round(a) if bf16_exact else a
        a[(17 * i + 5) % cfg["head_dim"]] = 0.0
        w[name] = a
    return w


def make_weights(cfg=QWEN3_CFG, seed=1234, std=0.06, bf16_exact=True):
    return _with_head_norms(cfg, GI.make_weights(cfg, seed, std, bf16_exact), seed + 1, bf16_exact)


def strict_weights(cfg=QWEN3_CFG):
    """the fp32 "strict" fixtures' weights: not bf16-representable"""
    return _with_head_norms(cfg, GI.strict_weights(cfg), 4322, False)
