"""TEST INFRASTRUCTURE -- CPU oracle of the Qwen3 family: oracle.llama_np.LlamaOracle with an RMSNorm over head_dim on every query head and every key head
between the projection and RoPE (modeling_qwen3.py:237-238 q_norm / k_norm = Qwen3RMSNorm(head_dim); :252-253 q_norm(q_proj(x).view(.., head_dim)),
k_norm(k_proj(x).view(.., head_dim)), then apply_rotary_pos_emb). The norm is oracle.ops_np.rmsnorm_fwd / rmsnorm_bwd on the [T * heads, head_dim] view,
with their rounding points in bf16-mirror mode. Pinned by tests/golden/llama_qwen3.npz (transformers.Qwen3ForCausalLM, fp32 CPU)."""
import numpy as np

from oracle import ops_np as O
from oracle.llama_np import LlamaOracle

F32 = np.float32


class Qwen3Oracle(LlamaOracle):
    def _head_norm(self, l, which, y, heads):
        """y [T, heads * dh] -> normed [T, heads, dh], rstd [T * heads]"""
        dh = self.cfg["head_dim"]
        w = self.w[f"model.layers.{l}.self_attn.{which}.weight"]
        yn, rstd = O.rmsnorm_fwd(y.reshape(-1, dh), w, self.cfg["rms_norm_eps"], self.bf16)
        return yn.reshape(len(y), heads, dh), rstd

    def forward(self, ids, cu_seqlens, keep=False):
        c = self.cfg
        H, Hkv, dh, eps = c["num_heads"], c["num_kv_heads"], c["head_dim"], c["rms_norm_eps"]
        T = len(ids)
        pos = np.concatenate([np.arange(cu_seqlens[b + 1] - cu_seqlens[b]) for b in range(len(cu_seqlens) - 1)])
        cos, sin = O.rope_tables(pos, dh, c["rope_theta"], self.bf16, c.get("rope_scaling"))
        x = self.w["model.embed_tokens.weight"][np.asarray(ids)]
        cache = []
        for l in range(c["num_layers"]):
            p = f"model.layers.{l}."
            xn1, rstd1 = O.rmsnorm_fwd(x, self.w[p + "input_layernorm.weight"], eps, self.bf16)
            q_raw, us_q = self._lin(l, "q_proj", xn1)
            k_raw, us_k = self._lin(l, "k_proj", xn1)
            v, us_v = self._lin(l, "v_proj", xn1)
            qn, rstd_q = self._head_norm(l, "q_norm", q_raw, H)
            kn, rstd_k = self._head_norm(l, "k_norm", k_raw, Hkv)
            q = O.rope_apply(qn, cos, sin, self.bf16)
            k = O.rope_apply(kn, cos, sin, self.bf16)
            v = v.reshape(T, Hkv, dh)
            attn, lse = O.attention_fwd(q, k, v, cu_seqlens, self.bf16)
            h, us_o = self._lin(l, "o_proj", attn.reshape(T, H * dh), R=x)
            xn2, rstd2 = O.rmsnorm_fwd(h, self.w[p + "post_attention_layernorm.weight"], eps, self.bf16)
            g, us_g = self._lin(l, "gate_proj", xn2)
            u, us_u = self._lin(l, "up_proj", xn2)
            act = O.swiglu_fwd(g, u, self.bf16)
            x_next, us_d = self._lin(l, "down_proj", act, R=h)
            if keep:
                cache.append(dict(x=x, xn1=xn1, rstd1=rstd1, q=q, k=k, v=v, attn=attn, lse=lse, h=h, xn2=xn2, rstd2=rstd2, g=g, u=u, act=act,
                                  q_raw=q_raw, k_raw=k_raw, rstd_q=rstd_q, rstd_k=rstd_k,
                                  us=dict(q_proj=us_q, k_proj=us_k, v_proj=us_v, o_proj=us_o, gate_proj=us_g, up_proj=us_u, down_proj=us_d)))
            x = x_next
        return x, dict(layers=cache, cos=cos, sin=sin)

    def loss_and_grads(self, ids, labels, cu_seqlens, num_items=None, full=False):
        c, rb = self.cfg, self.rb
        H, Hkv, dh = c["num_heads"], c["num_kv_heads"], c["head_dim"]
        T = len(ids)
        x_final, cache = self.forward(ids, cu_seqlens, keep=True)
        rows, tgts, _ = O.shift_labels(labels, cu_seqlens)
        n = num_items or len(rows)
        logits, xg, xf, rstd_f = self.logits_rows(x_final, rows)
        loss, dlogits, _ = O.ce_rows(logits, tgts, n)
        dlogits = rb(dlogits)
        grads = {}
        dxf = rb(dlogits @ self.w["lm_head.weight"])
        if full:
            grads["lm_head.weight"] = (dlogits.T @ xf).astype(F32)
        dxg, dwn = O.rmsnorm_bwd(dxf, xg, rstd_f, self.w["model.norm.weight"], None, self.bf16)
        if full:
            grads["model.norm.weight"] = dwn
        dX = np.zeros((T, c["hidden_size"]), F32)
        dX[rows] = dxg
        for l in range(c["num_layers"] - 1, -1, -1):
            p = f"model.layers.{l}."
            L = cache["layers"][l]
            dact = self._group_bwd(l, ("down_proj",), (dX,), L["act"], (L["us"]["down_proj"],), grads, full)
            dg, du_ = O.swiglu_bwd(dact, L["g"], L["u"], self.bf16)
            dxn2 = self._group_bwd(l, ("gate_proj", "up_proj"), (dg, du_), L["xn2"], (L["us"]["gate_proj"], L["us"]["up_proj"]), grads, full)
            dH, dw2 = O.rmsnorm_bwd(dxn2, L["h"], L["rstd2"], self.w[p + "post_attention_layernorm.weight"], dX, self.bf16)
            dattn = self._group_bwd(l, ("o_proj",), (dH,), L["attn"].reshape(T, H * dh), (L["us"]["o_proj"],), grads, full)
            dq, dk, dv = O.attention_bwd(L["q"], L["k"], L["v"], L["attn"], dattn.reshape(T, H, dh), L["lse"], cu_seqlens, self.bf16)
            dq = O.rope_apply(dq, cache["cos"], cache["sin"], self.bf16, backward=True)
            dk = O.rope_apply(dk, cache["cos"], cache["sin"], self.bf16, backward=True)
            # head-norm backward on the [T * heads, dh] view; the weight gradients sum over tokens AND heads
            dq, dwq = O.rmsnorm_bwd(dq.reshape(-1, dh), L["q_raw"].reshape(-1, dh), L["rstd_q"], self.w[p + "self_attn.q_norm.weight"], None, self.bf16)
            dk, dwk = O.rmsnorm_bwd(dk.reshape(-1, dh), L["k_raw"].reshape(-1, dh), L["rstd_k"], self.w[p + "self_attn.k_norm.weight"], None, self.bf16)
            dq, dk, dv = dq.reshape(T, H * dh), dk.reshape(T, Hkv * dh), dv.reshape(T, Hkv * dh)
            dxn1 = self._group_bwd(l, ("q_proj", "k_proj", "v_proj"), (dq, dk, dv), L["xn1"],
                                   (L["us"]["q_proj"], L["us"]["k_proj"], L["us"]["v_proj"]), grads, full)
            dX, dw1 = O.rmsnorm_bwd(dxn1, L["x"], L["rstd1"], self.w[p + "input_layernorm.weight"], dH, self.bf16)
            if full:
                grads[p + "post_attention_layernorm.weight"] = dw2
                grads[p + "input_layernorm.weight"] = dw1
                grads[p + "self_attn.q_norm.weight"] = dwq
                grads[p + "self_attn.k_norm.weight"] = dwk
        if full:
            ge = np.zeros_like(self.w["model.embed_tokens.weight"])
            np.add.at(ge, np.asarray(ids), dX)
            grads["model.embed_tokens.weight"] = ge
        return loss, grads
