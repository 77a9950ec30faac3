#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the INSTALLED HuggingFace/torch/sklearn CPU stack (authoring container only).

The upstream repository has no code or fixtures (/root/reference/README.md:38-39); the de-facto reference
arithmetic of the path is HF transformers 5.15.0 + torch 2.10.0 + scikit-learn 1.7.2. This script
imports those libraries, runs them on the deterministic inputs of tests/golden_inputs.py and stores OUTPUTS only.
It never travels to the GPU box as a dependency: tests read the .npz files.

    python tools/make_golden.py            # rewrites tests/golden/*.npz
    python tools/make_golden.py qwen3      # one family only (here: the Qwen3 fixtures, tests/qwen3_inputs.py)
    python tools/make_golden.py attr       # the token-attribution fixtures (tests/attribution_inputs.py)
    python tools/make_golden.py ig         # the integrated-gradients fixtures (tests/ig_inputs.py)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_inputs as GI  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(8)


def hf_model(cfg, weights, dtype=torch.float32):
    if cfg.get("qk_norm"):   # Qwen3: per-head q/k RMSNorm (modeling_qwen3.py:237-238, 252-253); head_dim is its own config field
        from transformers import Qwen3Config, Qwen3ForCausalLM
        hc = Qwen3Config(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                         num_hidden_layers=cfg["num_layers"], num_attention_heads=cfg["num_heads"], num_key_value_heads=cfg["num_kv_heads"],
                         head_dim=cfg["head_dim"], rope_theta=cfg["rope_theta"], rms_norm_eps=cfg["rms_norm_eps"], tie_word_embeddings=False,
                         attention_bias=False, max_position_embeddings=512, use_sliding_window=False)
        assert all(t == "full_attention" for t in hc.layer_types)
        hc._attn_implementation = "eager"
        m = Qwen3ForCausalLM(hc)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()}, strict=False)
        assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
        return m.to(dtype).train()
    if cfg.get("qkv_bias"):
        from transformers import Qwen2Config, Qwen2ForCausalLM
        hc = Qwen2Config(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                         num_hidden_layers=cfg["num_layers"], num_attention_heads=cfg["num_heads"], num_key_value_heads=cfg["num_kv_heads"],
                         rope_theta=cfg["rope_theta"], rms_norm_eps=cfg["rms_norm_eps"], tie_word_embeddings=False, max_position_embeddings=512,
                         use_sliding_window=False)
        assert cfg["hidden_size"] // cfg["num_heads"] == cfg["head_dim"]
        hc._attn_implementation = "eager"
        m = Qwen2ForCausalLM(hc)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()}, strict=False)
        assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
        return m.to(dtype).train()
    from transformers import LlamaConfig, LlamaForCausalLM
    hc = LlamaConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                     num_hidden_layers=cfg["num_layers"], num_attention_heads=cfg["num_heads"], num_key_value_heads=cfg["num_kv_heads"],
                     head_dim=cfg["head_dim"], rope_theta=cfg["rope_theta"], rms_norm_eps=cfg["rms_norm_eps"], tie_word_embeddings=False,
                     attention_bias=False, mlp_bias=False, max_position_embeddings=512,
                     **({"rope_scaling": dict(cfg["rope_scaling"])} if cfg.get("rope_scaling") else {}))
    hc._attn_implementation = "eager"
    m = LlamaForCausalLM(hc)
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    return m.to(dtype).train()


class LoraLinear(torch.nn.Module):
    """LoRA definition (peft is not installed): y = W x + s * B (A x), s = alpha / r, W frozen."""

    def __init__(self, base, A, B, s):
        super().__init__()
        self.base = base
        self.base.weight.requires_grad_(False)
        self.lora_A = torch.nn.Parameter(torch.from_numpy(A.copy()))
        self.lora_B = torch.nn.Parameter(torch.from_numpy(B.copy()))
        self.s = s

    def forward(self, x):
        return self.base(x) + self.s * ((x @ self.lora_A.T) @ self.lora_B.T)


def inject_lora(m, lora, r, alpha):
    for p in m.parameters():
        p.requires_grad_(False)
    params = {}
    for l, layer in enumerate(m.model.layers):
        for mod in GI.MODS:
            key = f"layers.{l}.{mod}"
            if key + ".lora_A" not in lora:
                continue
            parent = layer.self_attn if mod in ("q_proj", "k_proj", "v_proj", "o_proj") else layer.mlp
            wrapped = LoraLinear(getattr(parent, mod), lora[key + ".lora_A"], lora[key + ".lora_B"], alpha / r)
            setattr(parent, mod, wrapped)
            params[key + ".lora_A"] = wrapped.lora_A
            params[key + ".lora_B"] = wrapped.lora_B
    return params


def run_llama(cfg, tag, lengths, n_answer, make_weights=GI.make_weights, split_params=False):
    """split_params: the adapter snapshots p1/ and p3/ go to files of their own (lora_<tag>_p1.npz, lora_<tag>_p3.npz) -- the same keys, every file under 1 MiB"""
    w = make_weights(cfg)
    ids, labels, cu = GI.make_batch(cfg, lengths, n_answer)
    pid, plab, mask = GI.pad_batch(ids, labels, cu)
    m = hf_model(cfg, w)
    out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab))
    out.loss.backward()
    logits = out.logits.detach().numpy()
    packed_logits = np.concatenate([logits[b, : cu[b + 1] - cu[b]] for b in range(len(cu) - 1)])
    res = dict(loss=np.float32(out.loss.item()), logits=packed_logits.astype(np.float32))
    for name, p in m.named_parameters():
        n, head, strided = GI.sample_vec(p.grad.numpy())
        res["gn/" + name], res["gh/" + name], res["gs/" + name] = n, head, strided
    # the reference's OWN bf16 run (model.to(bfloat16), eager attention): its distance to the fp32 logits is the
    # bf16 noise floor that any bf16 implementation of this path sits at (DESIGN.md "Parity protocol")
    mb = hf_model(cfg, w, torch.bfloat16).eval()
    with torch.no_grad():
        lb = mb(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.float().numpy()
    res["logits_hf_bf16"] = np.concatenate([lb[b, : cu[b + 1] - cu[b]] for b in range(len(cu) - 1)]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, f"llama_{tag}.npz"), **res)
    print(f"llama_{tag}: loss {res['loss']:.6f} logits {packed_logits.shape}")

    # ---- LoRA: loss, adapter grads, AdamW trajectory (clip 1.0, wd 0.01, lr 1e-2 linear decay over 5 steps)
    lora = GI.make_lora(cfg)
    m = hf_model(cfg, w)
    params = inject_lora(m, lora, GI.LORA_R, GI.LORA_ALPHA)
    names = list(params.keys())
    opt = torch.optim.AdamW([params[k] for k in names], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, fused=True)
    total = 5
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: max(0.0, (total - s) / total))  # HF/optimization.py:101-104, warmup 0
    res = {}
    losses, gnorms = [], []
    for step in range(total):
        out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab))
        opt.zero_grad()
        out.loss.backward()
        if step == 0:
            res["loss0"] = np.float32(out.loss.item())
            for k in names:
                res["g0/" + k] = params[k].grad.numpy().copy()
        gn = torch.nn.utils.clip_grad_norm_([params[k] for k in names], 1.0)
        losses.append(out.loss.item())
        gnorms.append(gn.item())
        opt.step()
        sched.step()
        if step in (0, 2):
            for k in names:
                res[f"p{step + 1}/" + k] = params[k].detach().numpy().copy()
    res["losses"] = np.array(losses, np.float32)
    res["gnorms"] = np.array(gnorms, np.float32)
    # held-out scoring quantities of the step-5 model on the same batch (definition SURVEY §8 a16)
    m.eval()
    with torch.no_grad():
        lg = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.numpy()
    res["logits_after"] = np.concatenate([lg[b, : cu[b + 1] - cu[b]] for b in range(len(cu) - 1)]).astype(np.float32)
    if split_params:
        for pre in ("p1/", "p3/"):
            np.savez_compressed(os.path.join(OUT, f"lora_{tag}_{pre[:-1]}.npz"), **{k: res.pop(k) for k in [k for k in res if k.startswith(pre)]})
    np.savez_compressed(os.path.join(OUT, f"lora_{tag}.npz"), **res)
    print(f"lora_{tag}: losses {losses} gnorms {gnorms}")


def run_ops():
    """per-op fixtures straight from the HF / torch functions (fp32 CPU)."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm, apply_rotary_pos_emb, eager_attention_forward, LlamaRotaryEmbedding
    from transformers import LlamaConfig
    from transformers.activations import ACT2FN
    from transformers.loss.loss_utils import ForCausalLMLoss
    rng = np.random.default_rng(5)
    res = {}
    # RMSNorm fwd/bwd
    x = torch.tensor(rng.standard_normal((5, 256)).astype(np.float32), requires_grad=True)
    nrm = LlamaRMSNorm(256, eps=1e-5)
    nrm.weight.data = torch.tensor((1 + 0.1 * rng.standard_normal(256)).astype(np.float32))
    dy = torch.tensor(rng.standard_normal((5, 256)).astype(np.float32))
    y = nrm(x)
    y.backward(dy)
    res.update(rms_x=x.detach().numpy(), rms_w=nrm.weight.detach().numpy(), rms_dy=dy.numpy(), rms_y=y.detach().numpy(), rms_dx=x.grad.numpy(),
               rms_dw=nrm.weight.grad.numpy())
    # RoPE
    hc = LlamaConfig(hidden_size=256, num_attention_heads=2, head_dim=128, rope_theta=500000.0, max_position_embeddings=512)
    rot = LlamaRotaryEmbedding(hc)
    q = torch.tensor(rng.standard_normal((1, 2, 9, 128)).astype(np.float32))
    k = torch.tensor(rng.standard_normal((1, 1, 9, 128)).astype(np.float32))
    pos = torch.arange(9)[None]
    cos, sin = rot(q, pos)
    qe, ke = apply_rotary_pos_emb(q, k, cos, sin)
    res.update(rope_q=q.numpy(), rope_k=k.numpy(), rope_qe=qe.numpy(), rope_ke=ke.numpy(), rope_cos=cos.numpy(), rope_sin=sin.numpy())
    # attention fwd/bwd (GQA group 2, one sequence of 70 => two 64-key tiles), eager path of HF
    class _M(torch.nn.Module):
        num_key_value_groups = 2
        training = False
    n = 70
    q = torch.tensor(rng.standard_normal((1, 2, n, 128)).astype(np.float32), requires_grad=True)
    k = torch.tensor(rng.standard_normal((1, 1, n, 128)).astype(np.float32), requires_grad=True)
    v = torch.tensor(rng.standard_normal((1, 1, n, 128)).astype(np.float32), requires_grad=True)
    cm = torch.full((n, n), float("-inf")).triu(1)[None, None]
    o, _ = eager_attention_forward(_M(), q, k, v, cm, scaling=128 ** -0.5, dropout=0.0)  # [1, n, H, dh]
    do = torch.tensor(rng.standard_normal(o.shape).astype(np.float32))
    o.backward(do)
    res.update(att_q=q.detach().numpy(), att_k=k.detach().numpy(), att_v=v.detach().numpy(), att_o=o.detach().numpy(), att_do=do.numpy(),
               att_dq=q.grad.numpy(), att_dk=k.grad.numpy(), att_dv=v.grad.numpy())
    # SwiGLU
    g = torch.tensor(rng.standard_normal((4, 64)).astype(np.float32) * 2, requires_grad=True)
    u = torch.tensor(rng.standard_normal((4, 64)).astype(np.float32), requires_grad=True)
    a = ACT2FN["silu"](g) * u
    da = torch.tensor(rng.standard_normal((4, 64)).astype(np.float32))
    a.backward(da)
    res.update(sw_g=g.detach().numpy(), sw_u=u.detach().numpy(), sw_a=a.detach().numpy(), sw_da=da.numpy(), sw_dg=g.grad.numpy(), sw_du=u.grad.numpy())
    # causal-LM loss with explicit num_items_in_batch
    lg = torch.tensor(rng.standard_normal((2, 6, 50)).astype(np.float32) * 3, requires_grad=True)
    lab = torch.tensor([[-100, -100, -100, 4, 7, -100], [-100, -100, 9, 1, -100, -100]])
    loss = ForCausalLMLoss(lg, lab, vocab_size=50, num_items_in_batch=torch.tensor(7))
    loss.backward()
    res.update(ce_logits=lg.detach().numpy(), ce_labels=lab.numpy(), ce_loss=np.float32(loss.item()), ce_dlogits=lg.grad.numpy())
    # clip + fused AdamW, 3 steps, wd > 0
    p0 = rng.standard_normal(1000).astype(np.float32)
    p = torch.nn.Parameter(torch.tensor(p0.copy()))
    opt = torch.optim.AdamW([p], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, fused=True)
    gs, ps, norms = [], [], []
    for s in range(3):
        gi = (rng.standard_normal(1000) * (3.0 if s == 0 else 0.01)).astype(np.float32)
        p.grad = torch.tensor(gi.copy())
        norms.append(torch.nn.utils.clip_grad_norm_([p], 1.0).item())
        opt.step()
        gs.append(gi)
        ps.append(p.detach().numpy().copy())
    res.update(ad_p0=p0, ad_g=np.stack(gs), ad_p=np.stack(ps), ad_norm=np.array(norms, np.float32))
    np.savez_compressed(os.path.join(OUT, "ops.npz"), **res)
    print("ops: ok")


def run_kfold():
    """sklearn KFold / StratifiedKFold known answers (SK/model_selection/_split.py:516-529)."""
    from sklearn.model_selection import KFold
    res = {}
    for n, k, seed in ((12, 5, 42), (64, 2, 42), (103, 5, 0), (5120, 5, 42), (5120, 8, 42), (17, 4, 7)):
        folds = [te for _, te in KFold(k, shuffle=True, random_state=seed).split(np.arange(n))]
        assign = np.empty(n, np.int32)
        for f, te in enumerate(folds):
            assign[te] = f
        res[f"kf_{n}_{k}_{seed}"] = assign
    folds = [te for _, te in KFold(3, shuffle=False).split(np.arange(10))]
    assign = np.empty(10, np.int32)
    for f, te in enumerate(folds):
        assign[te] = f
    res["kf_10_3_noshuffle"] = assign
    np.savez_compressed(os.path.join(OUT, "kfold.npz"), **res)
    print("kfold: ok", res["kf_12_5_42"])


# ------------------------------------------------------------------------------------------------ GPT-2 family (config 1)
def hf_gpt2(cfg, weights, dtype=torch.float32):
    from transformers import GPT2Config, GPT2LMHeadModel
    hc = GPT2Config(vocab_size=cfg["vocab_size"], n_positions=cfg["max_position"], n_embd=cfg["hidden_size"], n_layer=cfg["num_layers"],
                    n_head=cfg["num_heads"], n_inner=cfg["intermediate_size"], activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0,
                    attn_pdrop=0.0, layer_norm_epsilon=cfg["layer_norm_eps"])
    hc._attn_implementation = "eager"
    m = GPT2LMHeadModel(hc)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()}, strict=False)
    assert not unexpected and all(k == "lm_head.weight" or k.endswith("attn.bias") or k.endswith("masked_bias") for k in missing), (missing, unexpected)
    m.tie_weights()
    assert m.lm_head.weight.data_ptr() == m.transformer.wte.weight.data_ptr()
    return m.to(dtype).train()


class LoraConv1D(torch.nn.Module):
    """LoRA on a Conv1D (peft: fan_in_fan_out=True): y = x W + b + s * (x A^T) B^T, W [in, out] frozen."""

    def __init__(self, base, A, B, s):
        super().__init__()
        self.base = base
        self.lora_A = torch.nn.Parameter(torch.from_numpy(A.copy()))
        self.lora_B = torch.nn.Parameter(torch.from_numpy(B.copy()))
        self.s = s

    def forward(self, x):
        return self.base(x) + self.s * ((x @ self.lora_A.T) @ self.lora_B.T)


def run_gpt2(cfg, tag, lengths, n_answer):
    w = GI.make_weights(cfg)
    ids, labels, cu = GI.make_batch(cfg, lengths, n_answer)
    pid, plab, mask = GI.pad_batch(ids, labels, cu)
    unpack = lambda a: np.concatenate([a[b, : cu[b + 1] - cu[b]] for b in range(len(cu) - 1)]).astype(np.float32)
    m = hf_gpt2(cfg, w)
    out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab))
    out.loss.backward()
    res = dict(loss=np.float32(out.loss.item()), logits=unpack(out.logits.detach().numpy()))
    for name, p in m.named_parameters():  # lm_head.weight is the same Parameter as wte: listed once
        n, head, strided = GI.sample_vec(p.grad.numpy())
        res["gn/" + name], res["gh/" + name], res["gs/" + name] = n, head, strided
    mb = hf_gpt2(cfg, w, torch.bfloat16).eval()
    with torch.no_grad():
        res["logits_hf_bf16"] = unpack(mb(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.float().numpy())
    np.savez_compressed(os.path.join(OUT, f"gpt2_{tag}.npz"), **res)
    print(f"gpt2_{tag}: loss {res['loss']:.6f} logits {res['logits'].shape}")

    lora = GI.make_lora(cfg)
    m = hf_gpt2(cfg, w)
    for p in m.parameters():
        p.requires_grad_(False)
    params = {}
    for l, blk in enumerate(m.transformer.h):
        for mod in GI.GPT2_MODS:
            parent = getattr(blk, mod.split(".")[0])
            leaf = mod.split(".")[1]
            key = f"layers.{l}.{mod}"
            wrapped = LoraConv1D(getattr(parent, leaf), lora[key + ".lora_A"], lora[key + ".lora_B"], GI.LORA_ALPHA / GI.LORA_R)
            setattr(parent, leaf, wrapped)
            params[key + ".lora_A"], params[key + ".lora_B"] = wrapped.lora_A, wrapped.lora_B
    names = list(params.keys())
    opt = torch.optim.AdamW([params[k] for k in names], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, fused=True)
    total = 5
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: max(0.0, (total - s) / total))
    res, losses, gnorms = {}, [], []
    for step in range(total):
        out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab))
        opt.zero_grad()
        out.loss.backward()
        if step == 0:
            res["loss0"] = np.float32(out.loss.item())
            for k in names:
                res["g0/" + k] = params[k].grad.numpy().copy()
        gnorms.append(torch.nn.utils.clip_grad_norm_([params[k] for k in names], 1.0).item())
        losses.append(out.loss.item())
        opt.step()
        sched.step()
        if step in (0, 2):
            for k in names:
                res[f"p{step + 1}/" + k] = params[k].detach().numpy().copy()
    res["losses"], res["gnorms"] = np.array(losses, np.float32), np.array(gnorms, np.float32)
    m.eval()
    with torch.no_grad():
        res["logits_after"] = unpack(m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.numpy())
    np.savez_compressed(os.path.join(OUT, f"lora_gpt2_{tag}.npz"), **res)
    print(f"lora_gpt2_{tag}: losses {losses} gnorms {gnorms}")


def run_ops_gpt2():
    """LayerNorm / gelu_new fixtures from torch.nn.LayerNorm and HF NewGELUActivation (fp32 CPU)."""
    from transformers.activations import ACT2FN
    rng = np.random.default_rng(11)
    res = {}
    x = torch.tensor((rng.standard_normal((6, 128)) * 2 + 0.5).astype(np.float32), requires_grad=True)
    ln = torch.nn.LayerNorm(128, eps=1e-5)
    ln.weight.data = torch.tensor((1 + 0.1 * rng.standard_normal(128)).astype(np.float32))
    ln.bias.data = torch.tensor((0.1 * rng.standard_normal(128)).astype(np.float32))
    dy = torch.tensor(rng.standard_normal((6, 128)).astype(np.float32))
    y = ln(x)
    y.backward(dy)
    res.update(ln_x=x.detach().numpy(), ln_w=ln.weight.detach().numpy(), ln_b=ln.bias.detach().numpy(), ln_dy=dy.numpy(), ln_y=y.detach().numpy(),
               ln_dx=x.grad.numpy(), ln_dw=ln.weight.grad.numpy(), ln_db=ln.bias.grad.numpy())
    g = torch.tensor((rng.standard_normal((4, 64)) * 2).astype(np.float32), requires_grad=True)
    a = ACT2FN["gelu_new"](g)
    da = torch.tensor(rng.standard_normal((4, 64)).astype(np.float32))
    a.backward(da)
    res.update(ge_x=g.detach().numpy(), ge_y=a.detach().numpy(), ge_dy=da.numpy(), ge_dx=g.grad.numpy())
    np.savez_compressed(os.path.join(OUT, "ops_gpt2.npz"), **res)
    print("ops_gpt2: ok")


# ------------------------------------------------------------------------------------------------ fp32 "strict" fixtures (T1/T3)
def _no_decay(name):
    """HF Trainer.get_decay_parameter_names (trainer.py:1181-1196): every parameter gets weight decay except biases and the
    LayerNorm / RMSNorm weights"""
    return name.endswith(".bias") or "norm" in name or ".ln_" in name


def _score_quantities(logits_rows, targets):
    """s(x) ingredients as include/tst_hip.h defines them, from fp32 logits rows: log p(target), argmax == target, option logits"""
    lg = torch.from_numpy(np.ascontiguousarray(logits_rows))
    lp = torch.log_softmax(lg, dim=-1).numpy()
    logp = lp[np.arange(len(targets)), targets]
    correct = (lg.argmax(-1).numpy() == targets).astype(np.int32)
    return logp.astype(np.float32), correct, logits_rows[:, list(GI.STRICT_OPT_IDS)].astype(np.float32)


def run_strict(cfg, tag, strict_weights=GI.strict_weights):
    """fp32 end to end, non-bf16-representable weights: base logits, 20-step LoRA and full-fine-tune trajectories (clip 1.0,
    AdamW wd 0.01 with HF's two parameter groups, linear LR decay) over two alternating micro-batches, and the s(x) ingredients of
    the trained models on a 32-sample held-out set."""
    gpt2 = cfg.get("arch") == "gpt2"
    w = strict_weights(cfg)
    batches = GI.strict_train_batches(cfg)
    hid, hlab, hcu = GI.strict_heldout(cfg)
    build = (lambda: hf_gpt2(cfg, w)) if gpt2 else (lambda: hf_model(cfg, w))
    unpack = lambda a, cu: np.concatenate([a[b, : cu[b + 1] - cu[b]] for b in range(len(cu) - 1)]).astype(np.float32)

    def logits_of(m, ids, labels, cu):
        pid, plab, mask = GI.pad_batch(ids, labels, cu)
        was = m.training
        m.eval()
        with torch.no_grad():
            lg = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.numpy()
        m.train(was)
        return unpack(lg, cu)

    def heldout_rows():
        rows = np.array([hcu[b + 1] - 2 for b in range(len(hcu) - 1)])   # position p predicts labels[p+1]: the row before the answer
        tgt = np.array([hlab[hcu[b + 1] - 1] for b in range(len(hcu) - 1)])
        return rows, tgt

    res = {}
    m = build()
    ids, labels, cu = batches[0]
    res["logits0_rows"] = np.arange(len(ids))[-32:]
    res["logits0"] = logits_of(m, ids, labels, cu)[res["logits0_rows"]]
    rows, tgt = heldout_rows()
    sid, slab, scu = GI.strict_seen(cfg)     # the set on which `correct` is not all zeros (every labelled training position as its own sequence)
    srows = np.array([scu[b + 1] - 2 for b in range(len(scu) - 1)])
    stgt = np.array([slab[scu[b + 1] - 1] for b in range(len(scu) - 1)])
    def score_into(prefix, model):
        lg = logits_of(model, hid, hlab, hcu)[rows]
        res[prefix + "_logp"], res[prefix + "_correct"], res[prefix + "_optl"] = _score_quantities(lg, tgt)
        res[prefix + "_logits"] = lg          # [32, V] fp32: logits parity (1e-4) and argmax agreement are checked on these rows
        res[prefix + "_seen_logp"], res[prefix + "_seen_correct"], _ = _score_quantities(logits_of(model, sid, slab, scu)[srows], stgt)
    score_into("base", m)

    def score_bf16_into(prefix, model):
        """the reference's OWN bf16 run of the same scoring pass (model.to(bfloat16), adapters included): its distance to the fp32 scores is the
        floor any bf16 implementation of the path sits at -- tests/test_strict_gpu.py bounds the product's bf16 path by 1.25 x this"""
        import copy
        mb = copy.deepcopy(model).to(torch.bfloat16).eval()
        pid, plab, mask = GI.pad_batch(hid, hlab, hcu)
        with torch.no_grad():
            lg = unpack(mb(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.float().numpy(), hcu)[rows]
        res[prefix + "_optl_hf_bf16"] = lg[:, list(GI.STRICT_OPT_IDS)].astype(np.float32)
        res[prefix + "_logp_hf_bf16"] = _score_quantities(lg, tgt)[0]
    score_bf16_into("base", m)

    def train(m, params, lr):
        names = list(params)
        dec = [params[k] for k in names if not _no_decay(k)]
        nod = [params[k] for k in names if _no_decay(k)]
        groups = [dict(params=dec, weight_decay=0.01)] + ([dict(params=nod, weight_decay=0.0)] if nod else [])
        opt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8, fused=True)
        total = GI.STRICT_STEPS
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: max(0.0, (total - s) / total))
        losses, gnorms = [], []
        for step in range(total):
            ids, labels, cu = batches[step % 2]
            pid, plab, mask = GI.pad_batch(ids, labels, cu)
            out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab))
            opt.zero_grad()
            out.loss.backward()
            gnorms.append(torch.nn.utils.clip_grad_norm_([params[k] for k in names], 1.0).item())
            losses.append(out.loss.item())
            opt.step()
            sched.step()
        return np.array(losses, np.float64), np.array(gnorms, np.float64)

    # LoRA
    lora = GI.make_lora(cfg)
    m = build()
    if gpt2:
        for p in m.parameters():
            p.requires_grad_(False)
        params = {}
        for l, blk in enumerate(m.transformer.h):
            for mod in GI.GPT2_MODS:
                parent, leaf, key = getattr(blk, mod.split(".")[0]), mod.split(".")[1], f"layers.{l}.{mod}"
                wrapped = LoraConv1D(getattr(parent, leaf), lora[key + ".lora_A"], lora[key + ".lora_B"], GI.LORA_ALPHA / GI.LORA_R)
                setattr(parent, leaf, wrapped)
                params[key + ".lora_A"], params[key + ".lora_B"] = wrapped.lora_A, wrapped.lora_B
    else:
        params = inject_lora(m, lora, GI.LORA_R, GI.LORA_ALPHA)
    res["lora_losses"], res["lora_gnorms"] = train(m, params, GI.STRICT_LR["lora"])
    score_into("lora", m)
    score_bf16_into("lora", m)
    for k, v in params.items():   # the adapters HF ends its 20 fp32 steps with: the bf16 paths (HF's and the product's) score the SAME trained fold
        res["lora_trained/" + k] = v.detach().numpy().astype(np.float32)
    # full fine-tune (tied GPT-2 head: named_parameters lists the shared tensor once)
    m = build()
    params = dict(m.named_parameters())
    res["full_losses"], res["full_gnorms"] = train(m, params, GI.STRICT_LR["full"])
    score_into("full", m)
    res["heldout_rows"], res["heldout_targets"] = rows, tgt
    np.savez_compressed(os.path.join(OUT, f"strict_{tag}.npz"), **res)
    print(f"strict_{tag}: lora losses {res['lora_losses'][[0, 1, 9, 19]]} full losses {res['full_losses'][[0, 1, 9, 19]]} "
          f"acc base/lora/full {res['base_correct'].mean():.2f}/{res['lora_correct'].mean():.2f}/{res['full_correct'].mean():.2f}  "
          f"on the seen set {res['base_seen_correct'].mean():.2f}/{res['lora_seen_correct'].mean():.2f}/{res['full_seen_correct'].mean():.2f}")


def run_accum(cfg, tag):
    """gradient accumulation as HF Trainer runs it (trainer.py:1740-1758, 2141-2175): every optimizer update consumes TWO micro-batches
    (GI.strict_train_batches) under ONE num_items_in_batch = the labelled tokens of both; each micro-batch's loss is
    sum(CE) / num_items_in_batch (loss_utils.py:32-46 with num_items_in_batch given), backward accumulates into .grad, then
    clip_grad_norm_(1.0), fused AdamW (wd 0.01, HF's two parameter groups), linear decay. fp32, non-bf16-representable weights.
    Recorded: per update the summed loss and the gradient norm, LoRA and full fine-tune; held-out log p(answer) of the trained models."""
    gpt2 = cfg.get("arch") == "gpt2"
    w = GI.strict_weights(cfg)
    batches = GI.strict_train_batches(cfg)
    hid, hlab, hcu = GI.strict_heldout(cfg)
    build = (lambda: hf_gpt2(cfg, w)) if gpt2 else (lambda: hf_model(cfg, w))
    n_items = int(sum(sum(1 for b in range(len(cu) - 1) for p in range(cu[b], cu[b + 1] - 1) if labels[p + 1] != -100) for _, labels, cu in batches))
    UPDATES = GI.ACCUM_UPDATES
    rows = np.array([hcu[b + 1] - 2 for b in range(len(hcu) - 1)])
    tgt = np.array([hlab[hcu[b + 1] - 1] for b in range(len(hcu) - 1)])

    def heldout_logp(m):
        pid, plab, mask = GI.pad_batch(hid, hlab, hcu)
        m.eval()
        with torch.no_grad():
            lg = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask)).logits.numpy()
        m.train()
        flat = np.concatenate([lg[b, : hcu[b + 1] - hcu[b]] for b in range(len(hcu) - 1)]).astype(np.float32)[rows]
        return _score_quantities(flat, tgt)[0]

    def train(m, params, lr):
        names = list(params)
        dec = [params[k] for k in names if not _no_decay(k)]
        nod = [params[k] for k in names if _no_decay(k)]
        groups = [dict(params=dec, weight_decay=0.01)] + ([dict(params=nod, weight_decay=0.0)] if nod else [])
        opt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8, fused=True)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s_: max(0.0, (UPDATES - s_) / UPDATES))
        losses, gnorms = [], []
        for _ in range(UPDATES):
            opt.zero_grad()
            tot = 0.0
            for ids, labels, cu in batches:   # the micro-batches of one update
                pid, plab, mask = GI.pad_batch(ids, labels, cu)
                out = m(input_ids=torch.from_numpy(pid), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(plab), num_items_in_batch=n_items)
                out.loss.backward()
                tot += out.loss.item()
            gnorms.append(torch.nn.utils.clip_grad_norm_([params[k] for k in names], 1.0).item())
            losses.append(tot)
            opt.step()
            sched.step()
        return np.array(losses, np.float64), np.array(gnorms, np.float64)

    res = {"num_items": np.array(n_items)}
    lora = GI.make_lora(cfg)
    m = build()
    if gpt2:
        for p_ in m.parameters():
            p_.requires_grad_(False)
        params = {}
        for l, blk in enumerate(m.transformer.h):
            for mod in GI.GPT2_MODS:
                parent, leaf, key = getattr(blk, mod.split(".")[0]), mod.split(".")[1], f"layers.{l}.{mod}"
                wrapped = LoraConv1D(getattr(parent, leaf), lora[key + ".lora_A"], lora[key + ".lora_B"], GI.LORA_ALPHA / GI.LORA_R)
                setattr(parent, leaf, wrapped)
                params[key + ".lora_A"], params[key + ".lora_B"] = wrapped.lora_A, wrapped.lora_B
    else:
        params = inject_lora(m, lora, GI.LORA_R, GI.LORA_ALPHA)
    res["lora_losses"], res["lora_gnorms"] = train(m, params, GI.STRICT_LR["lora"])
    res["lora_logp"] = heldout_logp(m)
    m = build()
    res["full_losses"], res["full_gnorms"] = train(m, dict(m.named_parameters()), GI.STRICT_LR["full"])
    res["full_logp"] = heldout_logp(m)
    np.savez_compressed(os.path.join(OUT, f"accum_{tag}.npz"), **res)
    print(f"accum_{tag}: num_items {n_items} lora losses {res['lora_losses']} full losses {res['full_losses']}")


def run_rope_scaling():
    """inverse frequencies of HF's rotary embedding under the supported scaling types (and the Llama-3.1 published parameters)"""
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    res = {}
    for tag, theta, rs in GI.ROPE_SCALING_CASES:
        hc = LlamaConfig(hidden_size=256, num_attention_heads=2, head_dim=128, rope_theta=theta, max_position_embeddings=131072, rope_scaling=dict(rs))
        rot = LlamaRotaryEmbedding(hc)
        assert float(rot.attention_scaling) == 1.0
        res[f"{tag}_inv_freq"] = rot.inv_freq.numpy().astype(np.float32)
        x = torch.zeros(1, 1, 200, 128)
        cos, sin = rot(x, torch.arange(200)[None])
        res[f"{tag}_cos"], res[f"{tag}_sin"] = cos[0, :, :64].numpy(), sin[0, :, :64].numpy()
    np.savez_compressed(os.path.join(OUT, "rope_scaling.npz"), **res)
    print("rope_scaling:", {k: v.shape for k, v in res.items() if k.endswith("inv_freq")})


# ------------------------------------------------------------------------------------------------ token attribution (include/tst_hip.h tst_attribute_async)
def _inject_lora_any(cfg, m, lora):
    if cfg.get("arch") != "gpt2":
        return inject_lora(m, lora, GI.LORA_R, GI.LORA_ALPHA)
    for p in m.parameters():
        p.requires_grad_(False)
    for l, blk in enumerate(m.transformer.h):
        for mod in GI.GPT2_MODS:
            parent, leaf, key = getattr(blk, mod.split(".")[0]), mod.split(".")[1], f"layers.{l}.{mod}"
            setattr(parent, leaf, LoraConv1D(getattr(parent, leaf), lora[key + ".lora_A"], lora[key + ".lora_B"], GI.LORA_ALPHA / GI.LORA_R))


def _attr_kit(tag):
    """what run_attr and run_ig share: the batch, the HF models of the three precisions (the fp64 one as the reference takes it) and J of one sequence"""
    import types
    import attribution_inputs as AI
    cfg, make_w = AI.TAGS[tag]
    gpt2 = cfg.get("arch") == "gpt2"
    w = make_w(cfg)
    ids, labels, cu = AI.batch(tag)
    opt = torch.from_numpy(AI.option_ids(tag).astype(np.int64))
    S = len(cu) - 1

    def model(adapter, dtype):
        m = (hf_gpt2 if gpt2 else hf_model)(cfg, w)
        if adapter is not None:
            _inject_lora_any(cfg, m, AI.lora(tag, adapter))
        for p in m.parameters():
            p.requires_grad_(False)
        if dtype == torch.float64:
            # HF's eager attention takes its softmax in fp32 whatever the model's dtype (modeling_llama.py eager_attention_forward), which would leave the
            # "fp64" reference with 1e-7 of noise in J; the sdpa path stays in the tensors' dtype. The fp32 / bf16 runs keep the eager path of every other fixture.
            m.config._attn_implementation = "sdpa"
            # likewise HF's RMSNorm modules (layer norms, Qwen3 head norms) run in fp32 whatever they are given (modeling_llama.py LlamaRMSNorm.forward): the
            # reference model takes the same formula in its own dtype
            for mod in m.modules():
                if type(mod).__name__.endswith("RMSNorm"):
                    mod.forward = (lambda x, mod=mod: mod.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + mod.variance_epsilon)))
        return m.to(dtype).eval()

    def J_of(m, x, lab, kind):
        z = m(inputs_embeds=x[None]).logits[0].to(torch.float64 if x.dtype == torch.float64 else torch.float32)
        rows = [p for p in range(len(lab) - 1) if lab[p + 1] != -100]
        tg = torch.tensor([int(lab[p + 1]) for p in rows])
        zr = z[rows]
        if kind == 1:
            assert len(rows) == 1 and int(tg[0]) in opt.tolist()
            return zr[0, tg[0]] - torch.logsumexp(zr[0, opt], 0)
        return torch.log_softmax(zr, -1)[torch.arange(len(rows)), tg].mean()

    def embed_parts(m, s):
        t = torch.from_numpy(ids[cu[s]:cu[s + 1]].astype(np.int64))
        if gpt2:
            return m.transformer.wte.weight[t].detach().clone(), m.transformer.wpe.weight[: len(t)].detach().clone()
        return m.model.embed_tokens.weight[t].detach().clone(), None

    return types.SimpleNamespace(AI=AI, cfg=cfg, gpt2=gpt2, ids=ids, labels=labels, cu=cu, opt=opt, S=S, model=model, J_of=J_of, embed_parts=embed_parts)


def run_attr(tag):
    """attr_<tag>.npz: gradient x input and gradient norm of J = sum_i log s(x_i) w.r.t. the embedding-layer output, from the HF model fed inputs_embeds with
    requires_grad. Per fixture set (AI.SETS) and adapter set (AI.ADAPTERS): ref_* from model.double(), hf32_* / hf_bf16_* from model.float() / .bfloat16(),
    floor32 / floor16 = per output the max over sequences of max_t |x - ref| / max_t |ref|. Sequences run one at a time: they do not interact."""
    kit = _attr_kit(tag)
    AI, gpt2, ids, labels, cu, S, model, J_of, embed_parts = kit.AI, kit.gpt2, kit.ids, kit.labels, kit.cu, kit.S, kit.model, kit.J_of, kit.embed_parts

    def attribute(m, kinds):
        gxi, gnorm, logs = [], [], []
        for s in range(S):
            x, pos = embed_parts(m, s)
            x.requires_grad_(True)
            J = J_of(m, x, labels[cu[s]:cu[s + 1]], kinds[s])
            g, = torch.autograd.grad(J, x)
            e = (x.detach() + pos) if gpt2 else x.detach()   # the embedding-layer output: d J / d e = d J / d x
            gxi.append((g.double() * e.double()).sum(-1).numpy())
            gnorm.append(g.double().norm(dim=-1).numpy())
            logs.append(float(J.detach()))
        return np.concatenate(gxi), np.concatenate(gnorm), np.array(logs)

    res = dict(option_ids=AI.option_ids(tag))
    for aname, adapter in AI.ADAPTERS.items():
        m64, m32, m16 = model(adapter, torch.float64), model(adapter, torch.float32), model(adapter, torch.bfloat16)
        for sname, kinds in AI.SETS.items():
            key = f"{sname}/{aname}/"
            ref = attribute(m64, kinds)
            # the reference against a central difference of J in fp64: scaling token t's embedding output by 1 +- h moves J by +- h gxi[t]
            h, worst = 1e-4, 0.0
            for s, t in ((0, 2), (1, 17), (S - 1, 50)):
                x, pos = embed_parts(m64, s)
                e = x + pos if gpt2 else x
                Jpm = []
                for sign in (1.0, -1.0):
                    e2 = e.clone()
                    e2[t] = e[t] * (1.0 + sign * h)
                    with torch.no_grad():
                        Jpm.append(float(J_of(m64, e2 - pos if gpt2 else e2, labels[cu[s]:cu[s + 1]], kinds[s])))
                fd = (Jpm[0] - Jpm[1]) / (2 * h)
                worst = max(worst, abs(fd - ref[0][cu[s] + t]) / np.abs(ref[0][cu[s]:cu[s + 1]]).max())
            if worst > 1e-6:
                raise SystemExit(f"attr_{tag} {key}: the reference disagrees with the central difference of J ({worst:.3e} relative): nothing written")
            res[key + "fd_check"] = np.float64(worst)
            res[key + "ref_gxi"], res[key + "ref_gnorm"], res[key + "ref_logs"] = ref
            for pre, m in (("hf32", m32), ("hf_bf16", m16)):
                got = attribute(m, kinds)
                res[key + pre + "_gxi"], res[key + pre + "_gnorm"], res[key + pre + "_logs"] = got
                res[key + ("floor32" if pre == "hf32" else "floor16")] = np.array([AI.seq_dev(got[i], ref[i], cu).max() for i in range(2)])
            print(f"attr_{tag} {key}: fd {worst:.2e} floor32 {res[key + 'floor32']} floor16 {res[key + 'floor16']} logs {np.round(ref[2], 4)}")
    # the stacked test tells the two adapter sets apart: per set, output and sequence, the distance of the l7 reference from the l99 one
    for sname in AI.SETS:
        res[f"{sname}/l99_vs_l7"] = np.stack([AI.seq_dev(res[f"{sname}/l7/ref_{o}"], res[f"{sname}/l99/ref_{o}"], cu) for o in AI.OUTPUTS])
        f16 = np.maximum(res[f"{sname}/l99/floor16"], res[f"{sname}/l7/floor16"])
        print(f"attr_{tag} {sname}: l99 vs l7 per output x sequence\n{res[f'{sname}/l99_vs_l7']}\n  4 x floor16 = {4 * f16}")
    np.savez_compressed(os.path.join(OUT, f"attr_{tag}.npz"), **res)


# ------------------------------------------------------------------------------------------------ integrated gradients (include/tst_hip.h tst_attribute_ig_async)
def run_ig(tag):
    """ig_<tag>.npz: integrated gradients of J = sum_i log s(x_i) from a baseline prompt to the real one (midpoint rule, IG.STEPS steps), from the HF models of
    run_attr. Per fixture set, baseline pattern (IG.PATTERNS) and adapter set: ref_ig / ref_logs / ref_logs_base from the fp64 model, hf32_* / hf_bf16_* from
    model.float() / .bfloat16() -- the interpolation in fp32 from the model-dtype table rows, rounded once: the library's contract --, floor32 / floor16 = the max
    over sequences of max_t |ig - ref| / max_t |ref|; ref_ig64 / delta_ref64 / ref_gap64 = the reference at IG.STEPS_FINE steps, its completeness gap
    sum_t ig - (J(e) - J(b)) per sequence, and that gap as a fraction of |J(e) - J(b)| (nan where that is below 0.05).
    Self-check: ref_gap64 <= 2 % everywhere; a case that misses it is checked again at twice the steps (ref_gap128 <= 2 %, stored for that case only), or nothing
    is written."""
    import ig_inputs as IG
    kit = _attr_kit(tag)
    AI, gpt2, ids, labels, cu, S, model, J_of = kit.AI, kit.gpt2, kit.ids, kit.labels, kit.cu, kit.S, kit.model, kit.J_of

    def table(m):
        return (m.transformer.wte if gpt2 else m.model.embed_tokens).weight.detach()

    def ig_of(m, kinds, base_ids, steps):
        """(ig [T], logs [S], logs_base [S]) in float64; the per-step products and the sum over the steps are taken in fp64 whatever the model's dtype"""
        E = table(m)
        wide = torch.float64 if E.dtype == torch.float64 else torch.float32
        out, logs, logs_base = [], [], []
        for s in range(S):
            t = torch.from_numpy(ids[cu[s]:cu[s + 1]].astype(np.int64))
            bt = torch.from_numpy(base_ids[cu[s]:cu[s + 1]].astype(np.int64))
            lab = labels[cu[s]:cu[s + 1]]
            e, b = E[t].clone(), E[bt].clone()
            same = (t == bt)[:, None]
            diff = e.double() - b.double()
            with torch.no_grad():
                logs.append(float(J_of(m, e, lab, kinds[s])))
                logs_base.append(float(J_of(m, b, lab, kinds[s])))
            acc = torch.zeros(len(t), dtype=torch.float64)
            for k in range(1, steps + 1):
                alpha = float(IG.alpha(k, steps))
                x = torch.where(same, e, (b.to(wide) + alpha * (e.to(wide) - b.to(wide))).to(E.dtype)).detach().requires_grad_(True)
                g, = torch.autograd.grad(J_of(m, x, lab, kinds[s]), x)
                acc += (g.double() * diff).sum(-1)
            out.append((acc / steps).numpy())
        return np.concatenate(out), np.array(logs), np.array(logs_base)

    res = dict(option_ids=AI.option_ids(tag))
    for aname, adapter in AI.ADAPTERS.items():
        m64, m32, m16 = model(adapter, torch.float64), model(adapter, torch.float32), model(adapter, torch.bfloat16)
        for sname, kinds in AI.SETS.items():
            for pname in IG.PATTERNS:
                key = f"{sname}/{pname}/{aname}/"
                base_ids = IG.baseline_ids(tag, pname)
                ref = ig_of(m64, kinds, base_ids, IG.STEPS)
                fine = ig_of(m64, kinds, base_ids, IG.STEPS_FINE)
                dJ = fine[1] - fine[2]
                delta = np.array([fine[0][cu[s]:cu[s + 1]].sum() for s in range(S)]) - dJ
                gap = np.where(np.abs(dJ) >= 0.05, np.abs(delta) / np.maximum(np.abs(dJ), 1e-300), np.nan)
                if np.nanmax(gap) > 0.02:   # the quadrature has not converged there yet: the self-check moves to twice the steps, the bound stays
                    finer = ig_of(m64, kinds, base_ids, 2 * IG.STEPS_FINE)
                    delta2 = np.array([finer[0][cu[s]:cu[s + 1]].sum() for s in range(S)]) - dJ
                    gap2 = np.where(np.abs(dJ) >= 0.05, np.abs(delta2) / np.maximum(np.abs(dJ), 1e-300), np.nan)
                    print(f"ig_{tag} {key}: gap at m = {IG.STEPS_FINE} {gap}; at m = {2 * IG.STEPS_FINE} {gap2}")
                    if np.nanmax(gap2) > 0.02:
                        raise SystemExit(f"ig_{tag} {key}: the fp64 reference misses completeness at m = {2 * IG.STEPS_FINE} by {gap2} of |dJ| = {np.abs(dJ)}: nothing written")
                    res[key + "ref_gap128"] = gap2
                res[key + "ref_ig"], res[key + "ref_logs"], res[key + "ref_logs_base"] = ref
                res[key + "ref_ig64"], res[key + "delta_ref64"], res[key + "ref_gap64"] = fine[0], delta, gap
                for pre, m in (("hf32", m32), ("hf_bf16", m16)):
                    got = ig_of(m, kinds, base_ids, IG.STEPS)
                    res[key + pre + "_ig"], res[key + pre + "_logs"], res[key + pre + "_logs_base"] = got
                    res[key + ("floor32" if pre == "hf32" else "floor16")] = np.float64(AI.seq_dev(got[0], ref[0], cu).max())
                print(f"ig_{tag} {key}: gap64 {np.round(gap, 5)} dJ {np.round(dJ, 4)} floor32 {res[key + 'floor32']:.2e} floor16 {res[key + 'floor16']:.4f}", flush=True)
    for sname in AI.SETS:
        for pname in IG.PATTERNS:
            res[f"{sname}/{pname}/l99_vs_l7"] = AI.seq_dev(res[f"{sname}/{pname}/l7/ref_ig"], res[f"{sname}/{pname}/l99/ref_ig"], cu)
            f16 = max(res[f"{sname}/{pname}/l99/floor16"], res[f"{sname}/{pname}/l7/floor16"])
            print(f"ig_{tag} {sname}/{pname}: l99 vs l7 per sequence {res[f'{sname}/{pname}/l99_vs_l7']}; 4 x floor16 = {4 * f16}")
    np.savez_compressed(os.path.join(OUT, f"ig_{tag}.npz"), **res)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = set(sys.argv[1:]) or {"ops", "kfold", "llama", "gpt2", "strict"}   # e.g. `python tools/make_golden.py gpt2` regenerates only that family
    if "ops" in which:
        run_ops()
    if "kfold" in which:
        run_kfold()
    if "llama" in which:
        run_llama(GI.TINY_CFG, "tiny", (7, 48, 100), (1, 2, 3))
        run_llama(GI.TINY2_CFG, "tiny2", (70, 33), (4, 1))
        run_llama(GI.QWEN_CFG, "qwen", (7, 48, 100), (1, 2, 3))
    if "gpt2" in which:
        run_ops_gpt2()
        run_gpt2(GI.GPT2_CFG, "tiny", (7, 48, 100), (1, 2, 3))
    if "strict" in which:
        for tag, cfg in (("tiny", GI.TINY_CFG), ("tiny2", GI.TINY2_CFG), ("qwen", GI.QWEN_CFG), ("gpt2", GI.GPT2_CFG)):
            run_strict(cfg, tag)
    if "qwen3" in which:   # the Qwen3 family's fixtures only (llama_qwen3.npz, lora_qwen3[_p1|_p3].npz, strict_qwen3.npz): not part of the default set, so a plain run
        import qwen3_inputs as Q3   # rewrites exactly the files it always wrote
        run_llama(Q3.QWEN3_CFG, "qwen3", Q3.LENGTHS, Q3.N_ANSWER, make_weights=Q3.make_weights, split_params=True)
        run_strict(Q3.QWEN3_CFG, "qwen3", strict_weights=Q3.strict_weights)
    if "accum" in which:
        for tag, cfg in (("tiny", GI.TINY_CFG), ("tiny2", GI.TINY2_CFG), ("gpt2", GI.GPT2_CFG)):
            run_accum(cfg, tag)
    if "attr" in which:   # the token-attribution fixtures only (attr_<tag>.npz, tests/attribution_inputs.py): not part of the default set
        for tag in ("tiny", "tiny2", "qwen", "qwen3", "gpt2"):
            run_attr(tag)
    if "ig" in which:   # the integrated-gradients fixtures only (ig_<tag>.npz, tests/ig_inputs.py): not part of the default set
        for tag in ("tiny", "tiny2", "qwen", "qwen3", "gpt2"):
            run_ig(tag)
    if "rope" in which or "strict" in which:
        run_rope_scaling()
        run_strict(GI.TINY_RS_CFG, "tiny_rs")
