"""The model's named tensors through the C-ABI, for the five tiny family configurations (Llama x 2, Qwen2, GPT-2, Qwen3): every HF state_dict name is
accepted by tst_set_weight / tst_get_weight and addresses its own storage, names outside the family's list are refused, and a full fine-tune reports its
trainables (tst_trainable_info) in the flat buffer's order with the family's names, offsets, rows and cols.

No tolerance anywhere: the arrays are bf16-representable, so what is read back equals what was set, and the layout is integers.
Extent of a tensor in the flat buffer = rows * cols, except that the token embedding (and an untied lm_head) is stored with its row count padded to a
multiple of 64 (GPT-2's odd vocabulary: 1001 rows reported, 1024 stored); for the four configurations whose vocabulary is a multiple of 64 that is rows * cols."""
import numpy as np
import pytest

import golden_inputs as GI
import qwen3_inputs as Q3
from oracle import gpt2_np, llama_np

pytestmark = pytest.mark.gpu

FAMILIES = [("tiny", GI.TINY_CFG), ("tiny2", GI.TINY2_CFG), ("qwen", GI.QWEN_CFG), ("gpt2", GI.GPT2_CFG), ("qwen3", Q3.QWEN3_CFG)]
IDS = [f[0] for f in FAMILIES]


def is_gpt2(cfg):
    return cfg.get("arch") == "gpt2"


def hf_names_shapes(cfg):
    """the family's HF state_dict: name -> shape (GPT-2 Conv1D weights in the HF [in, out] shape)"""
    if is_gpt2(cfg):
        return {n: gpt2_np.weight_shape(cfg, n) for n in gpt2_np.hf_weight_names(cfg)}
    out = {n: llama_np.weight_shape(cfg, n) for n in llama_np.hf_weight_names(cfg)}
    if cfg.get("qk_norm"):
        out.update({n: (cfg["head_dim"],) for n in Q3.head_norm_names(cfg)})
    return out


def make_ctx(cfg, **kw):
    from tst import lib
    return lib.Context(cfg, max_tokens=128, max_seqs=4, max_labelled=16, max_position=128, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, **kw)


@pytest.mark.parametrize("tag,cfg", FAMILIES, ids=IDS)
def test_names_round_trip(tag, cfg):
    shapes = hf_names_shapes(cfg)
    rng = np.random.default_rng(31)
    given = {n: GI.bf16_round(rng.standard_normal(s).astype(np.float32)) for n, s in shapes.items()}
    ctx = make_ctx(cfg)
    for n, a in given.items():   # all set before any is read: a name that addressed another's storage would show
        ctx.set_weight(n, a)
    for n, a in given.items():
        got = ctx.get_weight(n, shapes[n])
        assert np.array_equal(got, a), n
    if is_gpt2(cfg):   # tied head: an alias of the token embedding
        wte = given["transformer.wte.weight"]
        assert np.array_equal(ctx.get_weight("lm_head.weight", wte.shape), wte)
    ctx.close()


@pytest.mark.parametrize("tag,cfg", FAMILIES, ids=IDS)
def test_unknown_names_refused(tag, cfg):
    from tst.lib import TstError
    L, d = cfg["num_layers"], cfg["hidden_size"]
    bad = ["", f"transformer.h.{L}.ln_1.weight" if is_gpt2(cfg) else f"model.layers.{L}.input_layernorm.weight"]
    if tag in ("tiny", "tiny2"):   # Llama: no head norm, no projection bias
        bad += ["model.layers.0.self_attn.q_norm.weight", "model.layers.0.self_attn.q_proj.bias"]
    if is_gpt2(cfg):
        bad += ["model.embed_tokens.weight"]
    ctx = make_ctx(cfg)
    for n in bad:
        with pytest.raises(TstError, match="unknown weight"):
            ctx.set_weight(n, np.zeros(d, np.float32))
        with pytest.raises(TstError, match="unknown weight"):
            ctx.get_weight(n, (d,))
    norm = "transformer.ln_f.weight" if is_gpt2(cfg) else "model.norm.weight"
    with pytest.raises(TstError, match="numel mismatch"):
        ctx.set_weight(norm, np.zeros(d + 1, np.float32))
    with pytest.raises(TstError, match="numel mismatch"):
        ctx.get_weight(norm, (d - 1,))
    ctx.close()


def full_layout_rule(cfg):
    """[(name, rows, cols)] of a full fine-tune in flat-buffer order, written out from the family's rule"""
    d, F, V, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_layers"]
    out = []
    if is_gpt2(cfg):
        out += [("transformer.wte.weight", V, d), ("transformer.wpe.weight", cfg["max_position"], d)]
        for l in range(L):   # Conv1D matrices in the device layout [out, in]
            p = f"transformer.h.{l}."
            out += [(p + "attn.c_attn.weight", 3 * d, d), (p + "attn.c_proj.weight", d, d), (p + "mlp.c_fc.weight", F, d), (p + "mlp.c_proj.weight", d, F)]
        for l in range(L):   # (tied head: no lm_head entry)
            p = f"transformer.h.{l}."
            out += [(p + "ln_1.weight", 1, d), (p + "ln_1.bias", 1, d), (p + "ln_2.weight", 1, d), (p + "ln_2.bias", 1, d),
                    (p + "attn.c_attn.bias", 1, 3 * d), (p + "attn.c_proj.bias", 1, d), (p + "mlp.c_fc.bias", 1, F), (p + "mlp.c_proj.bias", 1, d)]
        return out + [("transformer.ln_f.weight", 1, d), ("transformer.ln_f.bias", 1, d)]
    dh = cfg["head_dim"]
    dq, dkv = cfg["num_heads"] * dh, cfg["num_kv_heads"] * dh
    out += [("model.embed_tokens.weight", V, d)]
    for l in range(L):
        p = f"model.layers.{l}."
        out += [(p + "self_attn.q_proj.weight", dq, d), (p + "self_attn.k_proj.weight", dkv, d), (p + "self_attn.v_proj.weight", dkv, d),
                (p + "self_attn.o_proj.weight", d, dq), (p + "mlp.gate_proj.weight", F, d), (p + "mlp.up_proj.weight", F, d), (p + "mlp.down_proj.weight", d, F)]
    out += [("lm_head.weight", V, d)]
    for l in range(L):
        p = f"model.layers.{l}."
        out += [(p + "input_layernorm.weight", 1, d), (p + "post_attention_layernorm.weight", 1, d)]
        if cfg.get("qkv_bias"):
            out += [(p + "self_attn.q_proj.bias", 1, dq), (p + "self_attn.k_proj.bias", 1, dkv), (p + "self_attn.v_proj.bias", 1, dkv)]
        if cfg.get("qk_norm"):
            out += [(p + "self_attn.q_norm.weight", 1, dh), (p + "self_attn.k_norm.weight", 1, dh)]
    return out + [("model.norm.weight", 1, d)]


@pytest.mark.parametrize("tag,cfg", FAMILIES, ids=IDS)
def test_full_layout(tag, cfg):
    rule = full_layout_rule(cfg)
    ctx = make_ctx(cfg, train_mode="full")
    layout = ctx.trainable_layout()
    assert list(layout) == [n for n, _, _ in rule]
    vocab_rows = (cfg["vocab_size"] + 63) // 64 * 64   # stored rows of the embedding / head
    off = 0
    for name, rows, cols in rule:
        assert layout[name] == (off, rows, cols), name
        padded = name in ("transformer.wte.weight", "model.embed_tokens.weight", "lm_head.weight")
        off += (vocab_rows if padded else rows) * cols
    assert off == ctx.trainable_numel()
    ctx.close()
