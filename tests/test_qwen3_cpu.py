"""CPU tests of the Qwen3 family (per-head q/k RMSNorm): the numpy oracle tests/qwen3_oracle.py against the HF fixtures (transformers.Qwen3ForCausalLM, fp32
CPU; tools/make_golden.py qwen3) at the tolerances tests/test_oracle_golden.py uses for the qwen family; the config / preset front end; the full-fine-tune
layout and the ZeRO shard map through libtst_host.so."""
import os

import numpy as np
import pytest

import golden_inputs as GI
import qwen3_inputs as Q3
from oracle import ops_np as O
from qwen3_oracle import Qwen3Oracle

CFG = Q3.QWEN3_CFG


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def test_inputs_carry_a_zero_weight_element():
    for w in (Q3.make_weights(), Q3.strict_weights()):
        names = Q3.head_norm_names(CFG)
        assert len(names) == 2 * CFG["num_layers"]
        for n in names:
            assert w[n].shape == (128,) and int((w[n] == 0).sum()) == 1 and abs(float(np.mean(w[n])) - 1.0) < 0.1
    assert CFG["num_heads"] * CFG["head_dim"] != CFG["hidden_size"]


def test_oracle_forward_backward_matches_hf(golden_dir):
    """logits, loss and EVERY parameter gradient (the head-norm vectors included) of the fp32 oracle against HF fp32 (tolerances of test_llama_forward_backward)"""
    g = load(golden_dir, "llama_qwen3.npz")
    w = Q3.make_weights()
    ids, labels, cu = GI.make_batch(CFG, Q3.LENGTHS, Q3.N_ANSWER)
    orc = Qwen3Oracle(CFG, w)
    close(orc.forward_logits(ids, cu, np.arange(len(ids))), g["logits"], 1e-3, 2e-4)
    loss, grads = orc.loss_and_grads(ids, labels, cu, full=True)
    close(loss, g["loss"], 1e-5, 1e-5)
    names = [n for n, _ in GI.weight_names_shapes(CFG)] + Q3.head_norm_names(CFG)
    assert sorted("gn/" + n for n in names) == sorted(k for k in g.files if k.startswith("gn/"))
    for name in names:
        n, head, strided = GI.sample_vec(grads[name])
        close(n, g["gn/" + name], 2e-3, 1e-6)
        close(head, g["gh/" + name], 5e-3, 2e-5 * float(g["gn/" + name]) + 1e-7)
        close(strided, g["gs/" + name], 5e-3, 2e-5 * float(g["gn/" + name]) + 1e-7)
    # the fixture is discriminating: without the head norm the plain Llama oracle misses it by far
    from oracle.llama_np import LlamaOracle
    plain = LlamaOracle(CFG, w).forward_logits(ids, cu, np.arange(len(ids)))
    assert np.abs(plain - g["logits"]).max() > 1e-2


def test_oracle_lora_trajectory_matches_hf(golden_dir):
    """loss, adapter gradients, clip + AdamW + linear LR over 5 steps (tolerances of test_lora_train_trajectory)"""
    g = load(golden_dir, "lora_qwen3.npz")
    gp = {1: load(golden_dir, "lora_qwen3_p1.npz"), 3: load(golden_dir, "lora_qwen3_p3.npz")}
    w = Q3.make_weights()
    ids, labels, cu = GI.make_batch(CFG, Q3.LENGTHS, Q3.N_ANSWER)
    lora = GI.make_lora(CFG)
    names = sorted(lora.keys())
    m = {k: np.zeros_like(lora[k]) for k in names}
    v = {k: np.zeros_like(lora[k]) for k in names}
    for step in range(5):
        loss, grads = Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA).loss_and_grads(ids, labels, cu)
        if step == 0:
            close(loss, g["loss0"], 1e-5, 1e-5)
            for k in names:
                gn = float(np.sqrt((g["g0/" + k].astype(np.float64) ** 2).sum()))
                close(grads[k], g["g0/" + k], 5e-3, 2e-5 * gn + 1e-7)
        tol = 1e-4 * (10 ** step)
        close(loss, g["losses"][step], tol, tol)
        norm, coef = O.clip_coef(np.concatenate([grads[k].ravel() for k in names]), 1.0)
        close(norm, g["gnorms"][step], 10 * tol, 10 * tol)
        lr = O.linear_lr(step, 5, 1e-2)
        for k in names:
            lora[k], m[k], v[k] = O.adamw_step(lora[k], grads[k] * coef, m[k], v[k], step + 1, lr, wd=0.01)
        if step in (0, 2):
            for k in names:
                diff = np.abs(lora[k].astype(np.float64) - gp[step + 1][f"p{step + 1}/" + k])
                tight = 2e-5 if step == 0 else 2e-3
                assert diff.max() <= 3.2e-2, k
                assert (diff > tight).mean() <= 2e-3, (k, float((diff > tight).mean()))
    close(Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA).forward_logits(ids, cu, np.arange(len(ids))), g["logits_after"], 5e-2, 5e-2)


def test_oracle_fp32_matches_strict_fixture(golden_dir):
    """base logits to 1e-4, held-out s(x) ingredients to 1e-3 / identical `correct` (test_oracle_fp32_matches_strict_fixtures)"""
    g = load(golden_dir, "strict_qwen3.npz")
    orc = Qwen3Oracle(CFG, Q3.strict_weights(), None, bf16=False)
    ids, labels, cu = GI.strict_train_batches(CFG)[0]
    assert np.abs(orc.forward_logits(ids, cu, g["logits0_rows"]) - g["logits0"]).max() <= 1e-4
    hid, hlab, hcu = GI.strict_heldout(CFG)
    logp, correct, optl, rseq = orc.score_rows(hid, hlab, hcu, list(GI.STRICT_OPT_IDS))
    sm = lambda z: np.exp(z - z.max(-1, keepdims=True)) / np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True)
    assert np.abs(sm(optl) - sm(g["base_optl"])).max() <= 1e-3 and np.abs(np.exp(logp) - np.exp(g["base_logp"])).max() <= 1e-3
    np.testing.assert_array_equal(correct, g["base_correct"])
    np.testing.assert_array_equal(rseq, np.arange(32))


def test_fixture_key_sets_match_the_qwen_family(golden_dir):
    """same keys as the qwen family's fixtures, up to the parameter names (no q/k/v bias; two head-norm vectors per layer); the adapter snapshots sit in
    files of their own"""
    ren = lambda keys: {k for k in keys if "bias" not in k and "q_norm" not in k and "k_norm" not in k}
    assert ren(load(golden_dir, "llama_qwen3.npz").files) == ren(load(golden_dir, "llama_qwen.npz").files)
    mine = set(load(golden_dir, "lora_qwen3.npz").files) | set(load(golden_dir, "lora_qwen3_p1.npz").files) | set(load(golden_dir, "lora_qwen3_p3.npz").files)
    assert mine == set(load(golden_dir, "lora_qwen.npz").files)
    assert ren(load(golden_dir, "strict_qwen3.npz").files) == ren(load(golden_dir, "strict_qwen.npz").files)
    for f in os.listdir(golden_dir):
        if "qwen3" in f:
            assert os.path.getsize(os.path.join(golden_dir, f)) < (1 << 20), f


QWEN3_8B_CONFIG = {
    "architectures": ["Qwen3ForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "head_dim": 128, "hidden_act": "silu", "hidden_size": 4096,
    "intermediate_size": 12288, "max_position_embeddings": 40960, "max_window_layers": 36, "model_type": "qwen3", "num_attention_heads": 32,
    "num_hidden_layers": 36, "num_key_value_heads": 8, "rms_norm_eps": 1e-06, "rope_scaling": None, "rope_theta": 1000000, "sliding_window": None,
    "tie_word_embeddings": False, "use_sliding_window": False, "vocab_size": 151936}


def test_cfg_from_hf_qwen3():
    from tst import cli, io, lib
    cfg = io.cfg_from_hf(dict(QWEN3_8B_CONFIG))
    assert cfg.pop("_tied") is False
    assert cfg == cli.MODEL_SHAPES["qwen3-8b"]
    mc = lib.make_model_cfg(cfg)
    assert mc.arch == lib.ARCH_QWEN3 == 3 and mc.head_dim == 128 and abs(mc.rms_norm_eps - 1e-6) < 1e-12 and mc.rope_theta == 1e6
    # head_dim comes from the config, not from hidden_size // heads (Qwen3-0.6B: 1024 / 16 = 64, head_dim 128)
    small = dict(QWEN3_8B_CONFIG, hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, intermediate_size=3072, tie_word_embeddings=True)
    c06 = io.cfg_from_hf(small)
    assert c06.pop("_tied") is True and c06 == cli.MODEL_SHAPES["qwen3-0.6b"] and c06["head_dim"] == 128
    # transformers >= 5 writes rope_parameters (theta inside); layer_types of full attention only is fine
    v5 = {k: v for k, v in QWEN3_8B_CONFIG.items() if k not in ("rope_theta", "rope_scaling")}
    v5.update(rope_parameters={"rope_theta": 1000000.0, "rope_type": "default"}, layer_types=["full_attention"] * 36)
    c5 = io.cfg_from_hf(v5)
    c5.pop("_tied")
    assert c5 == cli.MODEL_SHAPES["qwen3-8b"]
    for bad, word in ((dict(use_sliding_window=True), "use_sliding_window"), (dict(layer_types=["full_attention", "sliding_attention"] * 18), "sliding_attention"),
                      (dict(attention_bias=True), "attention_bias")):
        with pytest.raises(ValueError, match=word):
            io.cfg_from_hf(dict(QWEN3_8B_CONFIG, **bad))
    with pytest.raises(ValueError, match="qk_norm with qkv_bias"):
        lib.make_model_cfg(dict(cfg, qkv_bias=True))
    with pytest.raises(ValueError, match="unsupported model_type"):
        io.cfg_from_hf(dict(QWEN3_8B_CONFIG, model_type="qwen3_moe"))


def test_tied_qwen3_checkpoint_refuses_a_full_fine_tune():
    """tie_word_embeddings (Qwen3-0.6B / 1.7B / 4B) follows the existing rule: LoRA is fine, a full fine-tune is refused before any weight is read"""
    from tst import io

    class Ctx:
        gpt2, train_mode = False, "full"
    with pytest.raises(ValueError, match="tie_word_embeddings"):
        io.load_weights(Ctx(), "/nonexistent", tied=True)


def test_full_layout_qwen3_8b():
    """36 x 192 946 432 per layer (four matrices + two norm vectors + two head-norm vectors) + 2 x 622 329 856 (embedding, head) + 4 096 (final norm)"""
    from tst import cli, lib
    mc = lib.make_model_cfg(cli.MODEL_SHAPES["qwen3-8b"], train_mode="full")
    lay = lib.host_full_layout(mc)
    assert lay["n_train"] == 8190735360 == 36 * 192946432 + 2 * 622329856 + 4096
    assert lay["per_layer"] == 192946432 - 2 * 4096 - 2 * 128          # the decay group's share of a layer: its four matrices
    assert lay["tail"] == lay["n_decay"] == 2 * 622329856 + 36 * lay["per_layer"]
    # the no-decay tail holds exactly the norm vectors and the head-norm vectors
    assert lay["n_train"] - lay["n_decay"] == (2 * 36 + 1) * 4096 + 36 * 2 * 128
    # the same widths as a Llama-family model: the only difference is the head-norm vectors, all of them behind the decay border
    mc_l = lib.make_model_cfg({k: v for k, v in cli.MODEL_SHAPES["qwen3-8b"].items() if k != "qk_norm"}, train_mode="full")
    lay_l = lib.host_full_layout(mc_l)
    assert lay["n_train"] - lay_l["n_train"] == 36 * 256 and lay["n_decay"] == lay_l["n_decay"]
    regs = sorted(lay["regions"])
    at = 0
    for o, n in regs:
        assert o == at and n > 0
        at += n
    assert at == lay["n_train"] and regs[-1] == (lay["tail"], lay["n_train"] - lay["tail"])


@pytest.mark.parametrize("ranks", [2, 3])
def test_shard_map_tiny_qwen3(ranks):
    """ZeRO-1 shard arithmetic of the tiny config: the shards tile the padded vector, and each shard's decay / no-decay split puts the head-norm vectors
    (the last elements of the flat vector are layer 1's k_norm) in the no-decay group"""
    from tst import lib
    mc = lib.make_model_cfg(CFG, train_mode="full")
    lay = lib.host_full_layout(mc)
    d, F, V, L = 256, 256, 256, 2
    per_layer = (512 + 2 * 256) * d + d * 512 + 2 * F * d + d * F
    assert lay["per_layer"] == per_layer and lay["n_decay"] == 2 * V * d + L * per_layer
    assert lay["n_train"] == lay["n_decay"] + (2 * L + 1) * d + L * 2 * 128
    n = lay["n_train"]
    covered, prev = 0, 0
    for r in range(ranks):
        n_pad, shard, lo, hi = lib.host_zero_shard(n, ranks, r)
        assert n_pad % (64 * ranks) == 0 and n_pad >= n and n_pad - n < 64 * ranks and shard == n_pad // ranks and lo == r * shard == prev
        assert hi == min(lo + shard, n)
        prev = lo + shard
        covered += hi - lo
        d_hi, n_lo = lib.host_decay_split(lo, hi, lay["n_decay"])
        dec, nod = max(0, d_hi - lo), max(0, hi - n_lo)
        assert dec + nod == hi - lo
        if r == ranks - 1:   # the tail (norm vectors, head-norm vectors) lies in the last shard for these sizes, all of it without decay
            assert nod == n - lay["n_decay"] and n_lo == lay["n_decay"]
    assert covered == n


def test_lab_signature_table_lists_the_head_norm_hooks():
    from tst import lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tst_hip_lab.h")).read()
    for name in ("tst_k_head_norm_fwd", "tst_k_head_norm_bwd", "tst_k_head_norm_fwd_f32", "tst_k_head_norm_bwd_f32"):
        assert name in lib.LAB_SIGNATURES and f"int {name}(" in hdr
    assert len(lib.LAB_SIGNATURES["tst_k_head_norm_fwd"][1]) == 13 and len(lib.LAB_SIGNATURES["tst_k_head_norm_bwd"][1]) == 15
