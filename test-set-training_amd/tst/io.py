"""Real-data front end: a local HuggingFace checkpoint directory -> device context, and a QA
JSONL + local tokenizer file -> Samples. Nothing here needs the network, torch or transformers: a safetensors file is an
8-byte little-endian header length, a JSON header {name: {dtype, shape, data_offsets}} and raw little-endian tensor bytes
(https://github.com/huggingface/safetensors, format section), which numpy maps directly; bf16 payloads go to the device as
they are (TST_DTYPE_BF16), fp32 / fp16 are converted on the host.

    ctx = io.from_pretrained("/data/Meta-Llama-3-8B", max_tokens=2048, ...)      # the role of AutoModelForCausalLM.from_pretrained
    samples = io.load_qa_jsonl("vsi_text_only.jsonl", "/data/Meta-Llama-3-8B/tokenizer.json")

Weights, tokenizers and benchmark files are NOT available in the build environment: the tests write tiny
checkpoints / tokenizers / JSONL files themselves and read them back through this module.
"""
import json
import os
import struct

import numpy as np

from . import data as D

_DT = {"F32": (np.float32, 4), "F16": (np.float16, 2), "BF16": (np.uint16, 2), "U16": (np.uint16, 2)}


def read_safetensors_header(path):
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        if n > (1 << 27):
            raise ValueError(f"{path}: implausible safetensors header length {n}")
        hdr = json.loads(f.read(n))
    hdr.pop("__metadata__", None)
    return hdr, 8 + n


def iter_safetensors(path):
    """yields (name, dtype string, shape, numpy view of the payload) without copying (np.memmap)."""
    hdr, base = read_safetensors_header(path)
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    for name, meta in hdr.items():
        if meta["dtype"] not in _DT:
            raise ValueError(f"{path}:{name}: unsupported dtype {meta['dtype']}")
        npdt, size = _DT[meta["dtype"]]
        b0, b1 = meta["data_offsets"]
        count = int(np.prod(meta["shape"])) if meta["shape"] else 1
        if b1 - b0 != count * size:
            raise ValueError(f"{path}:{name}: payload size does not match shape")
        yield name, meta["dtype"], tuple(meta["shape"]), mm[base + b0: base + b1].view(npdt)


def checkpoint_files(model_dir):
    """single-file or sharded (model.safetensors.index.json: weight_map name -> shard file) checkpoints."""
    idx = os.path.join(model_dir, "model.safetensors.index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
        return [os.path.join(model_dir, x) for x in files]
    one = os.path.join(model_dir, "model.safetensors")
    if not os.path.exists(one):
        raise FileNotFoundError(f"{model_dir}: no model.safetensors[.index.json]")
    return [one]


def cfg_from_hf(hf):
    """HF config.json -> the cfg dict of tst.lib.Context (LlamaConfig / Qwen2Config / Qwen3Config / GPT2Config field names)."""
    mt = hf.get("model_type", "llama")
    if mt == "gpt2":
        d, H = hf["n_embd"], hf["n_head"]
        return dict(arch="gpt2", vocab_size=hf["vocab_size"], hidden_size=d, num_layers=hf["n_layer"], num_heads=H, num_kv_heads=H, head_dim=d // H,
                    intermediate_size=hf.get("n_inner") or 4 * d, max_position=hf["n_positions"], layer_norm_eps=hf.get("layer_norm_epsilon", 1e-5))
    if mt not in ("llama", "qwen2", "qwen3"):
        raise ValueError(f"unsupported model_type {mt!r} (llama, qwen2, qwen3, gpt2)")
    if mt == "qwen3":
        # dense Qwen3 with full attention in every layer and no projection bias is what the engine runs (include/tst_hip.h TST_ARCH_QWEN3)
        if hf.get("use_sliding_window"):
            raise ValueError("qwen3: use_sliding_window = true is not supported (sliding-window attention layers are not built)")
        if "sliding_attention" in (hf.get("layer_types") or ()):
            raise ValueError("qwen3: layer_types contains 'sliding_attention' (sliding-window attention layers are not built)")
        if hf.get("attention_bias"):
            raise ValueError("qwen3: attention_bias = true is not supported (q/k/v/o bias together with the q/k head norm is not built)")
    H = hf["num_attention_heads"]
    cfg = dict(vocab_size=hf["vocab_size"], hidden_size=hf["hidden_size"], num_layers=hf["num_hidden_layers"], num_heads=H,
               num_kv_heads=hf.get("num_key_value_heads", H), head_dim=hf.get("head_dim") or hf["hidden_size"] // H,
               intermediate_size=hf["intermediate_size"], rope_theta=float(hf.get("rope_theta", 10000.0)), rms_norm_eps=float(hf.get("rms_norm_eps", 1e-6)))
    if mt == "qwen2":
        cfg["qkv_bias"] = True
    if mt == "qwen3":
        cfg["qk_norm"] = True   # head_dim comes from the config (above): Qwen3 sizes have num_heads * head_dim != hidden_size
    # transformers >= 5 writes "rope_parameters" (which also carries rope_theta), older checkpoints "rope_scaling" + a top-level "rope_theta"
    rs = hf.get("rope_parameters") or hf.get("rope_scaling")
    if rs:
        if "rope_theta" in rs:
            cfg["rope_theta"] = float(rs["rope_theta"])
        kind = rs.get("rope_type", rs.get("type", "default"))
        if kind not in ("default", "linear", "llama3"):
            raise ValueError(f"rope scaling type {kind!r} is not supported (default, linear, llama3)")
        if kind != "default":
            cfg["rope_scaling"] = {k: rs[k] for k in ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings") if k in rs}
            cfg["rope_scaling"]["rope_type"] = kind
    cfg["_tied"] = bool(hf.get("tie_word_embeddings", False))
    return cfg


def load_weights(ctx, model_dir, tied=False):
    """streams every tensor of the checkpoint into the context; returns the number of tensors loaded."""
    from . import lib
    if tied and not ctx.gpt2 and getattr(ctx, "train_mode", "lora") == "full":
        # HF keeps embed_tokens and lm_head ONE parameter (gradients summed, one Adam state); this engine's Llama / Qwen2 layout has two
        # matrices, so a full fine-tune would silently train them apart. LoRA is unaffected (the base is frozen).
        raise ValueError("tie_word_embeddings checkpoints cannot be fully fine-tuned (the tied head would be trained as a separate matrix); "
                         "use --train-mode lora")
    seen = set()
    for path in checkpoint_files(model_dir):
        for name, dt, shape, arr in iter_safetensors(path):
            if name.endswith((".attn.bias", ".attn.masked_bias", "rotary_emb.inv_freq")):
                continue  # buffers some checkpoints carry (GPT-2's causal mask "h.N.attn.bias" -- not "c_attn.bias", a parameter)
            if ctx.gpt2 and not name.startswith(("transformer.", "lm_head.")):
                name = "transformer." + name  # GPT2Model checkpoints (hub "gpt2") omit the LM-head wrapper's prefix
            if dt == "BF16" and not (ctx.gpt2 and name.endswith(lib.CONV1D_SUFFIXES)):
                ctx.set_weight_bf16_bits(name, arr)      # straight to the device, no conversion
            else:
                a = arr.astype(np.float32) if dt != "BF16" else lib.from_bf16_bits(arr)
                ctx.set_weight(name, a.reshape(shape))
            seen.add(name)
    if tied and not ctx.gpt2 and "lm_head.weight" not in seen:   # tie_word_embeddings: the head is the embedding matrix
        V, d = ctx.cfg["vocab_size"], ctx.cfg["hidden_size"]
        ctx.set_weight("lm_head.weight", ctx.get_weight("model.embed_tokens.weight", (V, d)))
        seen.add("lm_head.weight")
    ctx.finalize()
    return len(seen)


def from_pretrained(model_dir, **ctx_kwargs):
    """local HF checkpoint directory (config.json + model.safetensors[.index.json]) -> ready Context."""
    from . import lib
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = cfg_from_hf(json.load(f))
    tied = cfg.pop("_tied", False)
    ctx = lib.Context(cfg, **ctx_kwargs)
    try:
        load_weights(ctx, model_dir, tied)
    except Exception:
        ctx.close()
        raise
    return ctx


# ------------------------------------------------------------------------------------------------ QA data
DEFAULT_TEMPLATE = "{question}\n{options}Answer:"


def format_prompt(rec, template=DEFAULT_TEMPLATE):
    """text-only prompt of one benchmark record: no image / video placeholder (README.md:35 "text-only inputs")."""
    opts = rec.get("options") or []
    letters = "ABCDEFGH"
    otext = "".join(f"{letters[i]}. {o}\n" for i, o in enumerate(opts))
    return template.format(question=rec["question"].strip(), options=otext)


def load_qa_jsonl(path, tokenizer_file, template=DEFAULT_TEMPLATE, max_len=128, option_letters="ABCD"):
    """JSONL records {"id", "question", "options": [...] (optional), "answer": "B" | "3.5"} -> (Samples, option_ids).
    A multiple-choice record's answer is its option letter (one token: kind "mca"); anything else is a free-form answer
    (kind "na"). Prompts are left-truncated to keep the answer within max_len. The tokenizer is a local tokenizers JSON
    (tokenizer.json of the checkpoint directory)."""
    from tokenizers import Tokenizer
    tok = Tokenizer.from_file(tokenizer_file)
    opt_ids = []
    for L in option_letters:
        ids = tok.encode(" " + L, add_special_tokens=False).ids
        opt_ids.append(ids[-1])
    out = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            rec = json.loads(line)
            prompt = tok.encode(format_prompt(rec, template), add_special_tokens=True).ids
            ans_text = str(rec["answer"]).strip()
            is_mca = bool(rec.get("options")) and len(ans_text) == 1 and ans_text.upper() in option_letters[:len(rec["options"])]
            if is_mca:
                gt = option_letters.index(ans_text.upper())
                ans = [opt_ids[gt]]
            else:
                gt = -1
                ans = tok.encode(" " + ans_text, add_special_tokens=False).ids
                if not ans:
                    raise ValueError(f"record {rec.get('id')}: empty answer after tokenisation")
            ans = ans[:max(1, max_len // 4)]
            keep = max_len - len(ans)
            prompt = prompt[-keep:] if len(prompt) > keep else prompt
            if not prompt:
                raise ValueError(f"record {rec.get('id')}: empty prompt")
            out.append(D.Sample(int(rec["id"]), np.array(prompt + ans, np.int32), len(prompt), "mca" if is_mca else "na", gt))
    return out, tuple(opt_ids)
