"""Configurations for the construction tests (tests/test_create_cpu.py through libtst_host.so, tests/test_create_gpu.py through tst_create): the ones the
engine accepts, the ones it refuses with the message it must give, and the trainable tables it must report -- all written out here, none read from the code
under test. The messages are the engine's own since before check_cfg existed (csrc/host_logic.h); POSITIVE is the one refusal that came with it."""
import golden_inputs as GI
import qwen3_inputs as Q3

EINVAL = -1
WORKSPACE = dict(max_tokens=256, max_seqs=8, max_labelled=32, max_position=128)
FAMILIES = dict(llama=GI.TINY_CFG, qwen2=GI.QWEN_CFG, qwen3=Q3.QWEN3_CFG, gpt2=GI.GPT2_CFG)
GOLDEN = dict(FAMILIES, tiny2=GI.TINY2_CFG, tiny_rs=GI.TINY_RS_CFG)


def model_cfg(cfg, **kw):
    from tst import lib
    return lib.make_model_cfg(cfg, **dict(WORKSPACE, **kw))


def accepted():
    """(tag, model dict, make_model_cfg keywords, forkable): every family x LoRA / full x bf16 / strict, stacked where allowed (LoRA, bf16), sharded where allowed (full)"""
    out = []
    for fam, cfg in FAMILIES.items():
        for prec in ("bf16", "strict"):
            out.append((f"{fam}-lora-{prec}", cfg, dict(precision=prec), True))
            for z in (None, (1, 0)):
                out.append((f"{fam}-full-{prec}-zero{1 if z else 0}", cfg, dict(precision=prec, train_mode="full", zero=z), False))
        out.append((f"{fam}-lora-bf16-stack3", cfg, dict(n_stack=3), True))
    out.append(("tiny2-lora-bf16-qv-r8", GI.TINY2_CFG, dict(lora_r=8, lora_targets=("q_proj", "v_proj")), True))
    out.append(("tiny_rs-lora-bf16", GI.TINY_RS_CFG, {}, True))
    return out


POSITIVE = "hidden_size/num_layers/num_heads/num_kv_heads/head_dim/intermediate_size/vocab_size must be > 0"
SIZES = "max_tokens/max_seqs/max_labelled/max_position must be > 0"
MULT64 = "hidden/intermediate/head sizes must be multiples of 64"
LORA_R = "lora_r must divide 64"
LLAMA3 = "llama3 rope scaling needs 0 < rope_low_freq_factor < rope_high_freq_factor and rope_original_max_position > 0"
ZERO = "zero_rank must be in [0, zero_ranks), zero_ranks <= 64"
NO_TARGETS = "no trainable parameters (lora_targets empty)"
FORK = "full fine-tune contexts cannot be forked (every fold owns its weights)"

# (base, field, value, message): `base` names a valid configuration of bases(); the refused one differs from it in ONE field
REFUSALS = [
    ("lora", "precision", 2, "precision must be TST_PRECISION_BF16 or TST_PRECISION_STRICT"),
    ("lora", "arch", 4, "unsupported arch"),
    ("lora", "arch", -1, "unsupported arch"),
    ("gpt2", "num_kv_heads", 1, "GPT-2: num_kv_heads must equal num_heads"),
    ("gpt2", "hidden_size", 192, "GPT-2: num_heads * head_dim must equal hidden_size"),
    ("lora", "train_mode", 2, "train_mode must be TST_TRAIN_LORA or TST_TRAIN_FULL"),
    ("lora", "head_dim", 64, "head_dim must be 128 (GPT-2 family: 64 or 128)"),
    ("lora", "hidden_size", 200, MULT64),
    ("lora", "intermediate_size", 257, MULT64),
    ("lora", "num_kv_heads", 3, "num_heads must be a multiple of num_kv_heads"),
    ("lora", "max_tokens", 0, SIZES),
    ("lora", "max_seqs", 0, SIZES),
    ("lora", "max_labelled", -1, SIZES),
    ("lora", "max_position", 0, SIZES),
    ("lora", "lora_r", 0, LORA_R),
    ("lora", "lora_r", 24, LORA_R),
    ("lora", "lora_r", 128, LORA_R),
    ("lora", "rope_scaling", 3, "rope_scaling must be TST_ROPE_DEFAULT, TST_ROPE_LINEAR or TST_ROPE_LLAMA3"),
    ("linear", "rope_factor", 0.0, "rope_factor must be > 0"),
    ("llama3", "rope_low_freq_factor", 0.0, LLAMA3),
    ("llama3", "rope_high_freq_factor", 1.0, LLAMA3),
    ("llama3", "rope_original_max_position", 0, LLAMA3),
    ("lora", "n_stack", 9, "n_stack must be <= 8"),
    ("full", "n_stack", 2, "stacked folds need frozen base weights (LoRA): a full fine-tune owns its weights"),
    ("r4", "n_stack", 2, "stacked folds: lora_r must be a multiple of 8"),
    ("strict", "n_stack", 2, "stacked folds are a bf16-path feature: precision = strict runs one fold per context"),
    ("lora", "zero_ranks", 1, "optimizer-state sharding (zero_ranks >= 1) is for full fine-tunes: LoRA state is 0.2 % of the model"),
    ("full", "zero_ranks", 65, ZERO),
    ("zero2", "zero_rank", 2, ZERO),
    ("zero2", "zero_rank", -1, ZERO),
    ("lora", "lora_targets", 0, NO_TARGETS),
    ("lora", "lora_targets", 128, NO_TARGETS),
    ("gpt2", "lora_targets", 0, NO_TARGETS),
]
# sizes that were undefined behaviour before check_cfg refused them: num_kv_heads = 0 an integer division by zero, num_layers = 0 a read of layers[0]
ZERO_SIZE = [("lora", "num_kv_heads", 0), ("full", "num_layers", 0), ("lora", "num_layers", 0), ("lora", "hidden_size", 0), ("lora", "num_heads", 0),
             ("lora", "head_dim", 0), ("lora", "intermediate_size", 0), ("lora", "vocab_size", 0), ("full", "num_kv_heads", -1), ("gpt2", "vocab_size", -64)]


def bases():
    rs = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64)
    return dict(lora=model_cfg(GI.TINY_CFG), full=model_cfg(GI.TINY_CFG, train_mode="full"), gpt2=model_cfg(GI.GPT2_CFG), r4=model_cfg(GI.TINY_CFG, lora_r=4),
                strict=model_cfg(GI.TINY_CFG, precision="strict"), zero2=model_cfg(GI.TINY_CFG, train_mode="full", zero=(2, 0)),
                linear=model_cfg(dict(GI.TINY_CFG, rope_scaling=dict(rope_type="linear", factor=4.0))), llama3=model_cfg(dict(GI.TINY_CFG, rope_scaling=rs)))


def variant(mc, field, value):
    """a copy of ModelCfg `mc` with one field changed"""
    out = type(mc).from_buffer_copy(mc)
    setattr(out, field, value)
    return out


def lora_table(cfg, r=GI.LORA_R, targets=None):
    """[(name, offset, rows, cols)] of one slot of a LoRA context: per layer and enabled module, lora_A [r, in] then lora_B [out, r], back to back"""
    mods = GI.GPT2_MODS if cfg.get("arch") == "gpt2" else GI.MODS
    out, at = [], 0
    for l in range(cfg["num_layers"]):
        for m in mods:
            if targets is not None and m not in targets:
                continue
            din, dout = GI.mod_dims(cfg, m)
            out.append((f"layers.{l}.{m}.lora_A", at, r, din))
            at += r * din
            out.append((f"layers.{l}.{m}.lora_B", at, dout, r))
            at += dout * r
    return out, at


def full_table(cfg):
    """[(name, offset, rows, cols)] of a full fine-tune: the state_dict tensors in the flat buffer's order [token embedding | (GPT-2: positions) | per layer
    q, k, v, o, gate, up, down (GPT-2: its four Conv1D weights, stored [out, in]) | (untied) lm_head | per layer the norm vectors and biases | final norm];
    the embedding and the head own roundup64(vocab) rows of the buffer and report `vocab`"""
    d, F, V, L, dh = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_layers"], cfg["head_dim"]
    Vp = (V + 63) // 64 * 64
    out, at = [], 0

    def put(name, rows, cols, owns=None):
        nonlocal at
        out.append((name, at, rows, cols))
        at += owns if owns is not None else rows * cols
    if cfg.get("arch") == "gpt2":
        put("transformer.wte.weight", V, d, Vp * d)
        put("transformer.wpe.weight", cfg["max_position"], d)
        for l in range(L):
            for m in GI.GPT2_MODS:
                din, dout = GI.mod_dims(cfg, m)
                put(f"transformer.h.{l}.{m}.weight", dout, din)
        for l in range(L):
            p = f"transformer.h.{l}."
            for n in ("ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias"):
                put(p + n, 1, d)
            for m in GI.GPT2_MODS:
                put(p + m + ".bias", 1, GI.mod_dims(cfg, m)[1])
        put("transformer.ln_f.weight", 1, d)
        put("transformer.ln_f.bias", 1, d)
        return out, at
    dq, dkv = cfg["num_heads"] * dh, cfg["num_kv_heads"] * dh
    put("model.embed_tokens.weight", V, d, Vp * d)
    for l in range(L):
        for m in GI.MODS:
            din, dout = GI.mod_dims(cfg, m)
            put(f"model.layers.{l}.{'mlp' if m in ('gate_proj', 'up_proj', 'down_proj') else 'self_attn'}.{m}.weight", dout, din)
    put("lm_head.weight", V, d, Vp * d)
    for l in range(L):
        p = f"model.layers.{l}."
        put(p + "input_layernorm.weight", 1, d)
        put(p + "post_attention_layernorm.weight", 1, d)
        if cfg.get("qkv_bias"):
            for m, n in (("q_proj", dq), ("k_proj", dkv), ("v_proj", dkv)):
                put(p + f"self_attn.{m}.bias", 1, n)
        if cfg.get("qk_norm"):
            put(p + "self_attn.q_norm.weight", 1, dh)
            put(p + "self_attn.k_norm.weight", 1, dh)
    put("model.norm.weight", 1, d)
    return out, at
