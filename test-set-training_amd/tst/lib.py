"""ctypes binding of libtst_hip.so (include/tst_hip.h). Thin by design: plain pointers and sizes, numpy host
buffers, no torch. There is no fallback: if the shared library is missing or no gfx950 device is visible, the
product path raises."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_DIR = os.environ.get("TST_LIB_DIR") or _HERE        # TST_LIB_DIR: another build of the same sources (A/B of two builds on one box, tools/ab.sh arms)
LIB_PATH = os.path.join(_LIB_DIR, "libtst_hip.so")       # product ABI: include/tst_hip.h
LAB_PATH = os.path.join(_LIB_DIR, "libtst_hip_lab.so")   # + test hooks and experimental tiles: include/tst_hip_lab.h
HOST_PATH = os.path.join(_HERE, "libtst_host.so")        # CPU-only: the engine's host arithmetic (csrc/host_logic.h) behind include/tst_host.h

TST_OK = 0
ARCH_LLAMA, ARCH_QWEN2, ARCH_GPT2, ARCH_QWEN3 = 0, 1, 2, 3  # cfg["qkv_bias"] selects the Qwen2 family, cfg["qk_norm"] Qwen3, cfg["arch"] == "gpt2" the GPT-2 family
TRAIN_LORA, TRAIN_FULL = 0, 1
LORA_BITS = {"q_proj": 1, "k_proj": 2, "v_proj": 4, "o_proj": 8, "gate_proj": 16, "up_proj": 32, "down_proj": 64,
             # GPT-2 family: the four Conv1D modules
             "attn.c_attn": 1 | 2 | 4, "attn.c_proj": 8, "mlp.c_fc": 16 | 32, "mlp.c_proj": 64}
CONV1D_SUFFIXES = ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")
LORA_ALL = 127
DTYPE_F32, DTYPE_BF16 = 0, 1
HEAD_NORM_WS_FLOATS = 1024 * 256   # TST_HEAD_NORM_WS_FLOATS (include/tst_hip_lab.h): scratch of the head-norm weight-gradient hooks
PRECISION_BF16, PRECISION_STRICT = 0, 1


@contextlib.contextmanager
def _stdout_to_stderr():
    """file descriptor 1 -> 2 while the block runs (C libraries write to the descriptor, not to sys.stdout)"""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        os.dup2(saved, 1)
        os.close(saved)


class TstError(RuntimeError):
    pass


class ModelCfg(C.Structure):
    _fields_ = [("arch", C.c_int32), ("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
                ("num_kv_heads", C.c_int32), ("head_dim", C.c_int32), ("intermediate_size", C.c_int32), ("rope_theta", C.c_float),
                ("rms_norm_eps", C.c_float), ("max_position", C.c_int32), ("max_tokens", C.c_int32), ("max_seqs", C.c_int32),
                ("max_labelled", C.c_int32), ("train_mode", C.c_int32), ("lora_r", C.c_int32), ("lora_alpha", C.c_float),
                ("lora_targets", C.c_uint32), ("adam_beta1", C.c_float), ("adam_beta2", C.c_float), ("adam_eps", C.c_float),
                ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("n_stack", C.c_int32), ("precision", C.c_int32),
                ("zero_ranks", C.c_int32), ("zero_rank", C.c_int32), ("rope_scaling", C.c_int32), ("rope_factor", C.c_float),
                ("rope_low_freq_factor", C.c_float), ("rope_high_freq_factor", C.c_float), ("rope_original_max_position", C.c_int32)]


ROPE_TYPES = {"default": 0, "linear": 1, "llama3": 2}


def rope_scaling_fields(rs):
    """cfg["rope_scaling"] (HF dict: rope_type / type, factor, low_freq_factor, high_freq_factor, original_max_position_embeddings) -> the five
    tst_model_cfg fields; None / "default" = plain RoPE. Unsupported types raise here, before a context exists."""
    if not rs:
        return 0, 0.0, 0.0, 0.0, 0
    kind = rs.get("rope_type", rs.get("type", "default"))
    if kind not in ROPE_TYPES:
        raise ValueError(f"rope scaling type {kind!r} is not supported (default, linear, llama3)")
    if kind == "default":
        return 0, 0.0, 0.0, 0.0, 0
    if kind == "linear":
        return 1, float(rs["factor"]), 0.0, 0.0, 0
    return 2, float(rs["factor"]), float(rs["low_freq_factor"]), float(rs["high_freq_factor"]), int(rs["original_max_position_embeddings"])


class Batch(C.Structure):
    _fields_ = [("input_ids", C.POINTER(C.c_int32)), ("labels", C.POINTER(C.c_int32)), ("cu_seqlens", C.POINTER(C.c_int32)),
                ("n_seqs", C.c_int32), ("n_tokens", C.c_int32), ("seq_slot", C.POINTER(C.c_int32)), ("flags", C.c_int32)]


_lib = None

# every exported symbol of include/tst_hip.h with its signature (tests check that each one resolves)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "tst_device_count": (C.c_int, []),
    "tst_abi_struct_sizes": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tst_set_tile_policy": (C.c_int, [_I]),
    "tst_set_option": (C.c_int, [_P, C.c_char_p, _I]),
    "tst_clock_probe": (C.c_int, [_I, _I, C.POINTER(_F)]),
    "tst_create": (C.c_int, [C.POINTER(ModelCfg), _I, C.POINTER(_P)]),
    "tst_fork": (C.c_int, [_P, C.POINTER(_P)]),
    "tst_destroy": (C.c_int, [_P]),
    "tst_score_async": (C.c_int, [_P, C.POINTER(Batch), _P, C.c_int32]),
    "tst_score_fetch": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    "tst_last_error": (C.c_char_p, [_P]),
    "tst_sync": (C.c_int, [_P]),
    "tst_set_stream": (C.c_int, [_P, _P, _I]),
    "tst_device_bytes": (C.c_int64, [_P]),
    "tst_set_weight": (C.c_int, [_P, C.c_char_p, _P, _I, _L]),
    "tst_get_weight": (C.c_int, [_P, C.c_char_p, _P, _L]),
    "tst_init_random": (C.c_int, [_P, C.c_uint64, _F]),
    "tst_finalize_weights": (C.c_int, [_P]),
    "tst_trainable_numel": (C.c_int64, [_P]),
    "tst_trainable_count": (C.c_int, [_P]),
    "tst_trainable_info": (C.c_int, [_P, _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L)]),
    "tst_get_trainable": (C.c_int, [_P, _P]),
    "tst_set_trainable": (C.c_int, [_P, _P]),
    "tst_get_grads": (C.c_int, [_P, _P]),
    "tst_get_opt_state": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int32)]),
    "tst_set_opt_state": (C.c_int, [_P, _P, _P, C.c_int32]),
    "tst_grad_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_L)]),
    "tst_dp_unique_id": (C.c_int, [_P, _L]),
    "tst_dp_init": (C.c_int, [_P, _P, _L, _I, _I]),
    "tst_train_step_dp_async": (C.c_int, [_P, C.POINTER(Batch), _F, C.c_int32]),
    "tst_dp_stats": (C.c_int, [_P, C.POINTER(_L), C.POINTER(_L)]),
    "tst_reset_trainable": (C.c_int, [_P, C.c_uint64]),
    "tst_reset_optimizer": (C.c_int, [_P]),
    "tst_forward_backward": (C.c_int, [_P, C.POINTER(Batch), C.c_int32, C.POINTER(_F)]),
    "tst_optimizer_step": (C.c_int, [_P, _F, C.POINTER(_F)]),
    "tst_train_step": (C.c_int, [_P, C.POINTER(Batch), _F, C.POINTER(_F), C.POINTER(_F)]),
    "tst_train_step_async": (C.c_int, [_P, C.POINTER(Batch), _F]),
    "tst_fetch_metrics": (C.c_int, [_P, C.POINTER(_F), C.POINTER(_F)]),
    "tst_stack_size": (C.c_int, [_P]),
    "tst_select_slot": (C.c_int, [_P, _I]),
    "tst_train_step_stacked_async": (C.c_int, [_P, C.POINTER(Batch), _P]),
    "tst_fetch_metrics_stacked": (C.c_int, [_P, _P, _P]),
    "tst_train_step_stacked_dp_async": (C.c_int, [_P, C.POINTER(Batch), _P, _P]),
    "tst_dp_set_transport": (C.c_int, [_P, _I]),
    "tst_accumulate_async": (C.c_int, [_P, C.POINTER(Batch), _P, _I]),
    "tst_optimizer_step_async": (C.c_int, [_P, _P]),
    "tst_fetch_loss": (C.c_int, [_P, _P]),
    "tst_score": (C.c_int, [_P, C.POINTER(Batch), _P, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    "tst_forward_logits": (C.c_int, [_P, C.POINTER(Batch), _P, C.c_int32, _P]),
    "tst_generate_async": (C.c_int, [_P, C.POINTER(Batch), C.c_int32, _P, C.c_int32]),
    "tst_generate_fetch": (C.c_int, [_P, _P, _P, _P]),
    "tst_generate": (C.c_int, [_P, C.POINTER(Batch), C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "tst_sample_async": (C.c_int, [_P, C.POINTER(Batch), C.c_int32, C.c_int32, _F, _P, _P, C.c_int32]),
    "tst_sample_fetch": (C.c_int, [_P, _P, _P, _P]),
    "tst_sample": (C.c_int, [_P, C.POINTER(Batch), C.c_int32, C.c_int32, _F, _P, _P, C.c_int32, _P, _P, _P]),
    "tst_score_candidates_async": (C.c_int, [_P, C.POINTER(Batch), _P, _P, _P, C.c_int32]),
    "tst_score_candidates_fetch": (C.c_int, [_P, _P, _P]),
    "tst_score_candidates": (C.c_int, [_P, C.POINTER(Batch), _P, _P, _P, C.c_int32, _P, _P]),
    "tst_attribute_async": (C.c_int, [_P, C.POINTER(Batch), _P, _P, C.c_int32]),
    "tst_attribute_fetch": (C.c_int, [_P, _P, _P, _P]),
    "tst_attribute": (C.c_int, [_P, C.POINTER(Batch), _P, _P, C.c_int32, _P, _P, _P]),
    "tst_attribute_ig_async": (C.c_int, [_P, C.POINTER(Batch), _P, _P, C.c_int32, _P, C.c_int32]),
    "tst_attribute_ig_fetch": (C.c_int, [_P, _P, _P, _P]),
    "tst_attribute_ig": (C.c_int, [_P, C.POINTER(Batch), _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "tst_profile_enable": (C.c_int, [_P, _I]),
    "tst_profile_read": (C.c_int, [_P, _I, _I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L), _I]),
    "tst_profile_intervals": (C.c_int, [_P, _P, _I, _I, _P, _P, _P, _L, C.POINTER(_L)]),
}

# every exported symbol of include/tst_hip_lab.h (libtst_hip_lab.so also exports all of the above)
LAB_SIGNATURES = {
    "tst_dev_alloc": (C.c_int, [C.POINTER(_P), _L]),
    "tst_dev_free": (C.c_int, [_P]),
    "tst_dev_h2d": (C.c_int, [_P, _P, _L]),
    "tst_dev_d2h": (C.c_int, [_P, _P, _L]),
    "tst_dev_memset": (C.c_int, [_P, _I, _L]),
    "tst_dev_sync": (C.c_int, []),
    "tst_dev_attn_fused_bwd": (C.c_int, [C.c_int]),
    "tst_k_gemm_nt": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _I, _I, _I]),
    "tst_k_gemm_k2slots": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _P, _I]),
    "tst_k_gemm_masked": (C.c_int, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _I, _I, _P, _I, _I]),
    "tst_k_gemm_tn": (C.c_int, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _I, _I]),
    "tst_k_gemm_pp_kmajor": (C.c_int, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tst_k_gemm_tns": (C.c_int, [_P, _L, _I, _P, _L, _I, _P, _L, _I, _F, _I, _I, _I, _P]),
    "tst_k_gemm_ref": (C.c_int, [_P, _L, _L, _P, _L, _L, _P, _L, _I, _I, _I]),
    "tst_k_transpose": (C.c_int, [_P, _L, _P, _L, _I, _I, _I]),
    "tst_k_embed": (C.c_int, [_P, _P, _P, _I, _I, _I]),
    "tst_k_embed_bwd": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, C.POINTER(C.c_float)]),
    "tst_k_rmsnorm_fwd": (C.c_int, [_P, _P, _P, _P, _I, _I, _F]),
    "tst_k_rmsnorm_bwd_dw": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "tst_k_rmsnorm_rank_fwd": (C.c_int, [_P, _P, _P, _P, _I, _I, _F, _P, _L, _P, _I, _F, _I, _I, _P]),
    "tst_k_rmsnorm_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I]),
    "tst_k_rope": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I]),
    "tst_k_head_norm_fwd": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P]),
    "tst_k_head_norm_bwd": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "tst_k_swiglu_fwd": (C.c_int, [_P, _P, _I, _I]),
    "tst_k_swiglu_bwd": (C.c_int, [_P, _P, _P, _I, _I]),
    "tst_k_swiglu_rank_fwd": (C.c_int, [_P, _P, _I, _I, _P, _L, _P, _I, C.c_float, _I, _I, _P]),
    "tst_k_swiglu_rank_bwd": (C.c_int, [_P, _P, _P, _I, _I, _P, _L, _P, _I, C.c_float, _I, _I, _P, _I]),
    "tst_k_layernorm_fwd": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _F]),
    "tst_k_layernorm_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "tst_k_gelu_fwd": (C.c_int, [_P, _P, _L]),
    "tst_k_gelu_bwd": (C.c_int, [_P, _P, _P, _L]),
    "tst_k_embed_pos": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "tst_k_logit_rows": (C.c_int, [_P, _L, _P, _I, _I, _P, _P, _L, _F, _P, _I, _P]),
    "tst_k_attr_seed": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _L]),
    "tst_k_attr_seed_f32": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _L]),
    "tst_k_token_attr": (C.c_int, [_P, _P, _I, _I, _P, _P]),
    "tst_k_token_attr_f32": (C.c_int, [_P, _P, _I, _I, _P, _P]),
    "tst_k_embed_interp": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F]),
    "tst_k_embed_interp_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F]),
    "tst_k_token_ig": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "tst_k_token_ig_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "tst_k_attn_fwd": (C.c_int, [_P, _L, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _F]),
    "tst_k_attn_bwd": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _F]),
    "tst_k_attn_fwd_rope": (C.c_int, [_P, _L, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _F, _P, _P]),
    "tst_k_attn_bwd_rope": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _F, _P, _P]),
    "tst_k_kv_append": (C.c_int, [_P, _L, _I, _P, _P, _P, _I, _I, _I, _L]),
    "tst_k_attn_decode": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_attn_decode_shared": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_attn_decode_shared_f32": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_sample_rows": (C.c_int, [_P, _L, _I, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P]),
    "tst_k_attn_extend": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_attn_extend_f32": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_cand_logp": (C.c_int, [_P, _L, _I, _P, _I, _P, _I, _I, _P]),
    "tst_k_kv_append_f32": (C.c_int, [_P, _L, _I, _P, _P, _P, _I, _I, _I, _L]),
    "tst_k_attn_decode_f32": (C.c_int, [_P, _L, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _F, _L]),
    "tst_k_adamw": (C.c_int, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _I, _P, _P]),
    "tst_k_clip_coef": (C.c_int, [_P, _L, _F, _P, _I, _P]),
    "tst_k_sumsq_partial": (C.c_int, [_P, _L, _P, _I]),
    "tst_k_clip_finalize": (C.c_int, [_P, _I, _F, _P]),
    "tst_k_sum_partials": (C.c_int, [_P, _I, _P]),
    "tst_k_clip_from_sumsq": (C.c_int, [_P, _F, _P]),
    "tst_k_adamw_flat": (C.c_int, [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _I, _P, _I]),
    "tst_k_adamw_matrix": (C.c_int, [_P, _P, _P, _P, _I, _I, _P, _F, _F, _F, _F, _F, _I, _P, _P, _I]),
    "tst_k_grad_accumulate": (C.c_int, [_P, _P, _L, _I]),
    "tst_k_lora_pack": (C.c_int, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "tst_k_lora_unpack_grad": (C.c_int, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "tst_k_tr_probe": (C.c_int, [_P, _I]),
    "tst_k_gemm_pp_stamps": (C.c_int, [_P]),
    "tst_k_gemm_bench": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F)]),
    "tst_k_gemm_bench_masked": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F)]),
    "tst_k_gemm_f32_nt": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _I, _I, _I, _I, _F]),
    "tst_k_gemm_f32_tn": (C.c_int, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _F]),
    "tst_k_attn_fwd_f32": (C.c_int, [_P, _L, _P, _I, _I, _P, _L, _P, _I, _I, _I, _I, _F]),
    "tst_k_attn_bwd_f32": (C.c_int, [_P, _L, _P, _L, _P, _L, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _F]),
    "tst_k_rmsnorm_fwd_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _F]),
    "tst_k_rmsnorm_bwd_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I]),
    "tst_k_rope_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I]),
    "tst_k_head_norm_fwd_f32": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P]),
    "tst_k_head_norm_bwd_f32": (C.c_int, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "tst_k_swiglu_fwd_f32": (C.c_int, [_P, _P, _I, _I]),
    "tst_k_swiglu_bwd_f32": (C.c_int, [_P, _P, _P, _I, _I]),
}


HOST_SIGNATURES = {
    "tst_host_rope_inv_freq": (C.c_float, [_P, _I]),
    "tst_host_zero_shard": (C.c_int, [_L, _I, _I, _P]),
    "tst_host_decay_split": (C.c_int, [_L, _L, _L, _P]),
    "tst_host_full_layout": (C.c_int, [_P, _P, _P, _I, _P]),
    "tst_host_check_cfg": (C.c_int, [_P, _I, _P, _I]),
    "tst_host_lora_layout": (C.c_int, [_P, _P, _P, _I, _P, _I]),
    "tst_host_stage_ints": (_L, [_P]),
    "tst_host_plan_batch": (C.c_int, [_P, _P, _I, _I, _P, _I, _P, _P, _P, _P, _I]),
    "tst_host_plan_generate": (C.c_int, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I]),
    "tst_host_plan_sample": (C.c_int, [_P, _P, _I, _I, _F, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I]),
    "tst_host_plan_candidates": (C.c_int, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "tst_host_cut_at_eos": (C.c_int, [_P, _P, _P, _I, _I, _P, _I]),
    "tst_host_plan_attribute": (C.c_int, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I]),
    "tst_host_untrim_tokens": (C.c_int, [_P, _P, _P, _I, _P]),
    "tst_host_plan_ig": (C.c_int, [_P, _P, _P, _I, _P, _P, _I]),
    "tst_host_trim_tokens": (C.c_int, [_P, _P, _P, _I, _P]),
}


def _open(path, tables):
    if not os.path.exists(path):
        raise TstError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    lib = C.CDLL(path)
    for table in tables:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def load():
    """dlopen libtst_hip.so (the product ABI) and bind every symbol; raises TstError when the library is not built.
    Safe to call in a process that has already initialised torch.cuda (tests/test_torch_coexist_gpu.py): the library then runs on the
    HIP runtime torch loaded, and device pointers / streams of torch tensors can be handed to it."""
    global _lib
    if _lib is None:
        # TST_WHATIF (timing-only ablation, bench diagnostics) exists in the LAB build of the engine only: the product library ignores the variable
        path = LAB_PATH if os.environ.get("TST_WHATIF", "0") not in ("", "0") else LIB_PATH
        lib = _open(path, (SIGNATURES,))
        a, b = C.c_int32(), C.c_int32()
        lib.tst_abi_struct_sizes(C.byref(a), C.byref(b))
        if (a.value, b.value) != (C.sizeof(ModelCfg), C.sizeof(Batch)):
            raise TstError(f"{LIB_PATH} was built with tst_model_cfg / tst_batch of {a.value} / {b.value} bytes, this binding has "
                           f"{C.sizeof(ModelCfg)} / {C.sizeof(Batch)}: rebuild the library or update tst/lib.py")
        _lib = lib
    return _lib


_lab = None


def load_lab():
    """dlopen libtst_hip_lab.so: per-kernel test hooks, raw device helpers, experimental tile families (include/tst_hip_lab.h).
    It carries its own copy of the product entry points; the kernel tests use only its tst_k_* / tst_dev_* symbols."""
    global _lab
    if _lab is None:
        _lab = _open(LAB_PATH, (SIGNATURES, LAB_SIGNATURES))
    return _lab


_host = None


def load_host():
    """dlopen libtst_host.so (include/tst_host.h): the engine's host-side arithmetic compiled by g++ without HIP -- the same header
    (csrc/host_logic.h) libtst_hip.so runs on its hot path. CPU tests only; nothing on the product path loads it."""
    global _host
    if _host is None:
        _host = _open(HOST_PATH, (HOST_SIGNATURES,))
    return _host


def host_zero_shard(n_train, ranks, rank):
    """(n_pad, shard length, lo, hi) of ZeRO shard `rank` of `ranks` -- the product's own shard map"""
    out = (C.c_int64 * 4)()
    if load_host().tst_host_zero_shard(int(n_train), int(ranks), int(rank), out) != 0:
        raise TstError("tst_host_zero_shard: bad arguments")
    return tuple(int(x) for x in out)


def host_decay_split(lo, hi, n_decay):
    out = (C.c_int64 * 2)()
    load_host().tst_host_decay_split(int(lo), int(hi), int(n_decay), out)
    return int(out[0]), int(out[1])


def host_full_layout(mc):
    """flat layout of a full fine-tune of ModelCfg `mc`: dict(n_train, n_decay, per_layer, embed, wpe, lm_head, layer0, tail, regions=[(offset, count)])"""
    out, nreg = (C.c_int64 * 8)(), C.c_int()
    reg = (C.c_int64 * 512)()
    if load_host().tst_host_full_layout(C.byref(mc), out, reg, 256, C.byref(nreg)) != 0:
        raise TstError("tst_host_full_layout failed")
    d = dict(zip(("n_train", "n_decay", "per_layer", "embed", "wpe", "lm_head", "layer0", "tail"), (int(x) for x in out)))
    d["regions"] = [(int(reg[2 * i]), int(reg[2 * i + 1])) for i in range(nreg.value)]
    return d


def host_check_cfg(mc, is_fork=False):
    """tsthost::check_cfg through the CPU library: (rc, message) -- what tst_create (or, is_fork, tst_fork) answers to ModelCfg `mc` before it allocates anything"""
    err = C.create_string_buffer(256)
    rc = load_host().tst_host_check_cfg(C.byref(mc), int(is_fork), err, 256)
    return int(rc), err.value.decode()


def host_lora_layout(mc):
    """tsthost::lora_layout through the CPU library: dict(n1, n_train, entries=[(name, offset, rows, cols)]) -- one slot's trainable table of a LoRA context"""
    cap = 14 * max(0, mc.num_layers)   # two entries for each of at most seven modules per layer
    out, names, ent = (C.c_int64 * 3)(), C.create_string_buffer(128 * max(1, cap)), (C.c_int64 * (3 * max(1, cap)))()
    if load_host().tst_host_lora_layout(C.byref(mc), out, names, 128, ent, cap) != 0:
        raise TstError("tst_host_lora_layout: bad arguments")
    return dict(n1=int(out[0]), n_train=int(out[1]),
                entries=[(names.raw[128 * i:128 * (i + 1)].split(b"\0", 1)[0].decode(), int(ent[3 * i]), int(ent[3 * i + 1]), int(ent[3 * i + 2])) for i in range(out[2])])


def host_plan_batch(mc, ids, labels, cu, seq_slot=None, need_labels=True, trim_last=True, rows=None):
    """tsthost::plan_batch through the CPU library: returns dict(T_dev, S, R, maxlen, slot_t_end, slot_r0, row_end, ids, pos, cu, lab_idx, targets, row_seq);
    raises TstError with the library's message for a refused batch"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    sl = None if seq_slot is None else np.ascontiguousarray(seq_slot, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    b = Batch(ip(ids), ip(lab), ip(cu), len(cu) - 1, len(ids), ip(sl), 0)
    stage = np.zeros(int(L.tst_host_stage_ints(C.byref(mc))), np.int32)
    out, rseq, err = np.zeros(29, np.int32), np.zeros(max(1, mc.max_labelled), np.int32), C.create_string_buffer(256)
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    rc = L.tst_host_plan_batch(C.byref(mc), C.byref(b), int(need_labels), int(trim_last), _ptr(r) if r is not None else None, 0 if r is None else len(r),
                               _ptr(stage), _ptr(out), _ptr(rseq), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_batch rc={rc}")
    T, S, R = int(out[0]), int(out[1]), int(out[2])
    Tm, Sm, Rm = mc.max_tokens, mc.max_seqs, mc.max_labelled
    o_pos, o_cu, o_lab, o_tgt = Tm, 2 * Tm, 2 * Tm + Sm + 1, 2 * Tm + Sm + 1 + Rm
    return dict(T_dev=T, S=S, R=R, maxlen=int(out[3]), slot_t_end=out[4:12].copy(), slot_r0=out[12:21].copy(), row_end=out[21:29].copy(),
                ids=stage[:T].copy(), pos=stage[o_pos:o_pos + T].copy(), cu=stage[o_cu:o_cu + S + 1].copy(), lab_idx=stage[o_lab:o_lab + R].copy(),
                targets=stage[o_tgt:o_tgt + R].copy(), row_seq=rseq[:R].copy())


GEN_MAX_NEW = 256   # TST_GEN_MAX_NEW (include/tst_hip.h)


def host_plan_generate(mc, ids, cu, max_new, eos_ids=(), seq_slot=None):
    """tsthost::plan_generate through the CPU library: dict(S, T, rows_used, cache_rows, slot_s_end, meta, last_rows, prefill_rows, decode_rows [max_new - 1, S]);
    raises TstError with the library's message for a refused generation"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    sl = None if seq_slot is None else np.ascontiguousarray(seq_slot, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    S, T = len(cu) - 1, len(ids)
    b = Batch(ip(ids), None, ip(cu), S, T, ip(sl), 0)
    eos = np.ascontiguousarray(eos_ids, np.int32)
    out, err = np.zeros(12, np.int64), C.create_string_buffer(256)
    meta, last, pre = np.zeros(3 + 2 * max(S, 0), np.int32), np.zeros(max(S, 1), np.int32), np.zeros(max(T, 1), np.int32)
    dec = np.zeros(max(1, (min(max(int(max_new), 1), GEN_MAX_NEW) - 1) * max(S, 0)), np.int32)
    rc = L.tst_host_plan_generate(C.byref(mc), C.byref(b), int(max_new), _ptr(eos) if len(eos) else None, len(eos), _ptr(out), _ptr(meta), _ptr(last), _ptr(pre),
                                  _ptr(dec), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_generate rc={rc}")
    return dict(S=int(out[0]), T=int(out[1]), rows_used=int(out[2]), cache_rows=int(out[3]), slot_s_end=out[4:12].astype(np.int32), meta=meta, last_rows=last[:S],
                prefill_rows=pre[:T], decode_rows=dec[:(int(max_new) - 1) * S].reshape(int(max_new) - 1, S))


SAMPLE_MAX_N = 64   # tsthost::kSampleMaxN


def host_plan_sample(mc, ids, cu, max_new, n_samples, temperature, seq_seeds, eos_ids=(), seq_slot=None):
    """tsthost::plan_sample through the CPU library: dict(S, T, R, rows_used, cache_rows, dev_ints, dev_ints_alloc, slot_r_end, geo [3 + 3 R], seeds [S, 2] (low,
    high word), last_rows, prefill_rows, decode_rows [max_new - 1, R]); seq_seeds = None passes a NULL pointer; raises TstError with the library's message for a
    refused call"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    sl = None if seq_slot is None else np.ascontiguousarray(seq_slot, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    S, T = len(cu) - 1, len(ids)
    b = Batch(ip(ids), None, ip(cu), S, T, ip(sl), 0)
    eos = np.ascontiguousarray(eos_ids, np.int32)
    seeds_in = None if seq_seeds is None else np.ascontiguousarray(seq_seeds, np.uint64)
    if seeds_in is not None and len(seeds_in) != S:
        raise TstError("seq_seeds needs one seed per sequence")
    n_cl, m_cl = min(max(int(n_samples), 1), SAMPLE_MAX_N), min(max(int(max_new), 1), GEN_MAX_NEW)
    R = max(S, 0) * n_cl
    out, err = np.zeros(15, np.int64), C.create_string_buffer(256)
    geo, seeds, last, pre = np.zeros(3 + 3 * R, np.int32), np.zeros(max(2 * S, 2), np.int32), np.zeros(max(S, 1), np.int32), np.zeros(max(T, 1), np.int32)
    dec = np.zeros(max(1, (m_cl - 1) * R), np.int32)
    rc = L.tst_host_plan_sample(C.byref(mc), C.byref(b), int(max_new), int(n_samples), float(temperature), None if seeds_in is None else _ptr(seeds_in),
                                _ptr(eos) if len(eos) else None, len(eos), _ptr(out), _ptr(geo), _ptr(seeds), _ptr(last), _ptr(pre), _ptr(dec), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_sample rc={rc}")
    R = int(out[2])
    return dict(S=int(out[0]), T=int(out[1]), R=R, rows_used=int(out[3]), cache_rows=int(out[4]), dev_ints=int(out[5]), dev_ints_alloc=int(out[6]),
                slot_r_end=out[7:15].astype(np.int32), geo=geo[:3 + 3 * R], seeds=seeds[:2 * S].reshape(S, 2), last_rows=last[:S], prefill_rows=pre[:T],
                decode_rows=dec[:(int(max_new) - 1) * R].reshape(int(max_new) - 1, R))


CAND_MAX_LEN = 16   # TST_CAND_MAX_LEN


def pack_candidates(cands, cand_seq):
    """(cand_ids, cu_cand, cand_seq) int32 arrays of a list of token-id sequences and the prompt index each continues"""
    cu = np.zeros(len(cands) + 1, np.int32)
    for i, c in enumerate(cands):
        cu[i + 1] = cu[i] + len(c)
    ids = np.array([t for c in cands for t in c], np.int32)
    return ids, cu, np.ascontiguousarray(cand_seq, np.int32)


def host_plan_candidates(mc, ids, cu, cand_ids, cu_cand, cand_seq, seq_slot=None):
    """tsthost::plan_candidates through the CPU library: dict(S, T, n_tok, R_e, n_ext, rows_used, cache_rows, dev_ints, slot_r_end, geo [n_ext, 5], ext_rows,
    ext_ids, ext_pos, ext_tgt [R_e], src [n_tok, 2], last_rows [S]); raises TstError with the library's message for a refused call"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    sl = None if seq_slot is None else np.ascontiguousarray(seq_slot, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    S, T = len(cu) - 1, len(ids)
    b = Batch(ip(ids), None, ip(cu), S, T, ip(sl), 0)
    cand_ids = np.ascontiguousarray(cand_ids, np.int32)
    cu_cand = np.ascontiguousarray(cu_cand, np.int32)
    cand_seq = np.ascontiguousarray(cand_seq, np.int32)
    n_cands = len(cu_cand) - 1
    if len(cand_seq) != max(n_cands, 0) or (n_cands >= 1 and len(cand_ids) < int(cu_cand.max())):
        raise TstError("cand_seq needs one entry per candidate and cand_ids cu_cand[-1] tokens")
    n = max(len(cand_ids), 1)
    out, err = np.zeros(16, np.int64), C.create_string_buffer(256)
    geo, rows, eid, epos, etgt = (np.zeros(5 * n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    src, last = np.zeros(2 * n, np.int32), np.zeros(max(S, 1), np.int32)
    rc = L.tst_host_plan_candidates(C.byref(mc), C.byref(b), _ptr(cand_ids) if len(cand_ids) else None, _ptr(cu_cand), _ptr(cand_seq) if n_cands > 0 else None,
                                    int(n_cands), _ptr(out), _ptr(geo), _ptr(rows), _ptr(eid), _ptr(epos), _ptr(etgt), _ptr(src), _ptr(last), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_candidates rc={rc}")
    n_tok, R, n_ext = int(out[2]), int(out[3]), int(out[4])
    return dict(S=int(out[0]), T=int(out[1]), n_tok=n_tok, R_e=R, n_ext=n_ext, rows_used=int(out[5]), cache_rows=int(out[6]), dev_ints=int(out[7]),
                slot_r_end=out[8:16].astype(np.int32), geo=geo[:5 * n_ext].reshape(n_ext, 5), ext_rows=rows[:R], ext_ids=eid[:R], ext_pos=epos[:R], ext_tgt=etgt[:R],
                src=src[:2 * n_tok].reshape(n_tok, 2), last_rows=last[:S])


def host_cut_at_eos(tokens, logp, eos_ids):
    """(tokens, logp, n_new) with every row cut behind its first eos token, as tst_generate_fetch does"""
    tok = np.array(tokens, np.int32, ndmin=2)
    lp = np.array(logp, np.float32, ndmin=2)
    eos = np.ascontiguousarray(eos_ids, np.int32)
    nn = np.zeros(tok.shape[0], np.int32)
    if load_host().tst_host_cut_at_eos(_ptr(tok), _ptr(lp), _ptr(nn), tok.shape[0], tok.shape[1], _ptr(eos) if len(eos) else None, len(eos)) != 0:
        raise TstError("tst_host_cut_at_eos: bad arguments")
    return tok, lp, nn


def host_plan_attribute(mc, ids, labels, cu, seq_kind=None, option_ids=()):
    """tsthost::plan_attribute through the CPU library: (row_w, row_kind, row_seq) of the labelled rows; raises TstError with the library's message for a refusal"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    kind = None if seq_kind is None else np.ascontiguousarray(seq_kind, np.int32)
    opt = np.ascontiguousarray(option_ids, np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    b = Batch(ip(ids), ip(lab), ip(cu), len(cu) - 1, len(ids), None, 0)
    n, cap = C.c_int32(), max(1, len(ids))
    w, k, q, err = np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), C.create_string_buffer(256)
    rc = L.tst_host_plan_attribute(C.byref(mc), C.byref(b), None if kind is None else _ptr(kind), _ptr(opt) if len(opt) else None, len(opt), C.byref(n), _ptr(w),
                                   _ptr(k), _ptr(q), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_attribute rc={rc}")
    return w[:n.value], k[:n.value], q[:n.value]


def host_untrim_tokens(values, cu_dev, cu_src):
    """per-token values of the tokens the device ran -> the caller's token order (a trimmed token gets 0), as tst_attribute_fetch does"""
    src = np.ascontiguousarray(values, np.float32)
    cd, cs = np.ascontiguousarray(cu_dev, np.int32), np.ascontiguousarray(cu_src, np.int32)
    if len(cd) != len(cs) or len(cd) < 1 or len(src) < int(cd[-1]):
        raise TstError("tst_host_untrim_tokens: bad arguments")
    dst = np.full(max(1, int(cs[-1])), np.nan, np.float32)
    if load_host().tst_host_untrim_tokens(_ptr(src), _ptr(cd), _ptr(cs), len(cd) - 1, _ptr(dst)) != 0:
        raise TstError("tst_host_untrim_tokens: bad arguments")
    return dst[:int(cs[-1])]


IG_MAX_STEPS = 256   # TST_IG_MAX_STEPS


def host_plan_ig(mc, ids, cu, baseline_ids, n_steps):
    """tsthost::plan_ig through the CPU library: the n_steps midpoints alpha_k (fp32) of an integrated-gradients call; raises TstError with the library's
    message for a refusal (baseline_ids None, an id outside the vocabulary, n_steps outside 1 .. IG_MAX_STEPS)"""
    L = load_host()
    ids = np.ascontiguousarray(ids, np.int32)
    cu = np.ascontiguousarray(cu, np.int32)
    base = None if baseline_ids is None else np.ascontiguousarray(baseline_ids, np.int32)
    if base is not None and len(base) != len(ids):
        raise TstError("baseline_ids needs one entry per token")
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    b = Batch(ip(ids), None, ip(cu), len(cu) - 1, len(ids), None, 0)
    alpha, err = np.zeros(IG_MAX_STEPS, np.float32), C.create_string_buffer(256)
    rc = L.tst_host_plan_ig(C.byref(mc), C.byref(b), None if base is None else _ptr(base), int(n_steps), _ptr(alpha), err, 256)
    if rc != 0:
        raise TstError(err.value.decode() or f"tst_host_plan_ig rc={rc}")
    return alpha[:int(n_steps)].copy()


def host_trim_tokens(values, cu_dev, cu_src):
    """per-token ids of the caller's batch -> the order the device runs them (a trimmed token is dropped), as tst_attribute_ig_async uploads the baseline ids"""
    src = np.ascontiguousarray(values, np.int32)
    cd, cs = np.ascontiguousarray(cu_dev, np.int32), np.ascontiguousarray(cu_src, np.int32)
    if len(cd) != len(cs) or len(cd) < 1 or len(src) < int(cs[-1]):
        raise TstError("tst_host_trim_tokens: bad arguments")
    dst = np.full(max(1, int(cd[-1])), -1, np.int32)
    if load_host().tst_host_trim_tokens(_ptr(src), _ptr(cd), _ptr(cs), len(cd) - 1, _ptr(dst)) != 0:
        raise TstError("tst_host_trim_tokens: bad arguments")
    return dst[:int(cd[-1])]


def device_count():
    return int(load().tst_device_count())


def clock_probe(device=0, spin_us=50):
    """shader clock held right now, MHz (include/tst_hip.h tst_clock_probe)"""
    out = _F()
    rc = load().tst_clock_probe(int(device), int(spin_us), C.byref(out))
    if rc != 0:
        raise TstError(f"tst_clock_probe failed ({rc})")
    return float(out.value)


class ClockSampler:
    """samples the held shader clock every `period_s` from a side thread (ctypes releases the GIL inside the call) between start() and stop()"""

    def __init__(self, device=0, period_s=0.05, spin_us=50):
        import threading
        self.device, self.period_s, self.spin_us, self.samples = device, period_s, spin_us, []
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append(clock_probe(self.device, self.spin_us))
            except TstError:
                break
            self._stop.wait(self.period_s)

    def start(self):
        self._t.start()
        return self

    def stop(self):
        self._stop.set()
        self._t.join(5.0)
        return self.samples


def set_tile_policy(level):
    """0: 128x128 contraction tiles; 1: 256x256 ping-pong tiles (several resident folds per GPU); 3: the same with split-K
    on the under-filled projections (one fold per GPU). Process-wide."""
    return int(load().tst_set_tile_policy(int(level)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _options(b, option_ids, seq_kind=None):
    """(option-id array, its length, seq_kind array or None) of a scoring / attribution call on batch b (no options: one zero, length 0)"""
    opt_a, _ = _i32(np.asarray(option_ids, np.int32) if len(option_ids) else np.zeros(1, np.int32))
    kind_a = None if seq_kind is None else np.ascontiguousarray(seq_kind, np.int32)
    if kind_a is not None and len(kind_a) != b.n_seqs:
        raise TstError("seq_kind needs one entry per sequence")
    return opt_a, len(option_ids), kind_a


def to_bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) >> np.uint32(16)).astype(np.uint16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


BATCH_DEVICE_IDS = 1


class DeviceIds:
    """input ids that already live in device memory (int32 [n_tokens]), e.g. DeviceIds(t.data_ptr(), t.numel()) for an int32 CUDA
    tensor of a torch process: handed to the library as a device pointer (tst_batch.flags = TST_BATCH_DEVICE_IDS)."""

    def __init__(self, ptr, n_tokens):
        self.ptr, self.n_tokens = int(ptr), int(n_tokens)

    def __len__(self):
        return self.n_tokens


class DevBuf:
    """raw device allocation for the per-kernel tests."""

    def __init__(self, host=None, nbytes=None):
        self.lib = load_lab()
        self.nbytes = int(host.nbytes if host is not None else nbytes)
        p = C.c_void_p()
        if self.lib.tst_dev_alloc(C.byref(p), self.nbytes) != 0:
            raise TstError("tst_dev_alloc failed")
        self.ptr = p
        if host is not None:
            host = np.ascontiguousarray(host)
            if self.lib.tst_dev_h2d(self.ptr, _ptr(host), self.nbytes) != 0:
                raise TstError("tst_dev_h2d failed")
        else:
            self.lib.tst_dev_memset(self.ptr, 0, self.nbytes)

    def get(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if self.lib.tst_dev_d2h(_ptr(out), self.ptr, out.nbytes) != 0:
            raise TstError("tst_dev_d2h failed (a kernel faulted?)")
        return out

    def get_bf16(self, shape):
        return from_bf16_bits(self.get(np.uint16, shape))

    def __del__(self):
        try:
            self.lib.tst_dev_free(self.ptr)
        except Exception:
            pass


def dev_bf16(x):
    return DevBuf(to_bf16_bits(x))


def dev_f32(x):
    return DevBuf(np.ascontiguousarray(x, dtype=np.float32))


def make_model_cfg(cfg, max_tokens=2048, max_seqs=16, max_labelled=64, max_position=128, lora_r=16, lora_alpha=32.0,
                   lora_targets=("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"), beta1=0.9, beta2=0.999, eps=1e-8,
                   weight_decay=0.0, max_grad_norm=1.0, train_mode="lora", n_stack=1, precision="bf16", zero=None):
    """the tst_model_cfg of a model dict (HF config names) and workspace / optimizer settings: what Context hands to tst_create"""
    if cfg.get("arch") == "gpt2":
        # wpe has exactly cfg["max_position"] rows; LayerNorm eps travels in the rms_norm_eps field
        arch, theta, eps_n, max_position = ARCH_GPT2, 0.0, cfg["layer_norm_eps"], cfg["max_position"]
        if tuple(lora_targets) == ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"):
            lora_targets = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
    else:
        if cfg.get("qk_norm") and cfg.get("qkv_bias"):
            raise ValueError("qk_norm with qkv_bias (HF Qwen3Config.attention_bias = True) is not built")
        arch = ARCH_QWEN3 if cfg.get("qk_norm") else (ARCH_QWEN2 if cfg.get("qkv_bias") else ARCH_LLAMA)
        theta, eps_n = cfg["rope_theta"], cfg["rms_norm_eps"]
    mask = 0
    for t in lora_targets:
        mask |= LORA_BITS[t]
    return ModelCfg(arch, cfg["vocab_size"], cfg["hidden_size"], cfg["num_layers"], cfg["num_heads"], cfg["num_kv_heads"], cfg["head_dim"],
                    cfg["intermediate_size"], theta, eps_n, max_position, max_tokens, max_seqs, max_labelled,
                    {"lora": TRAIN_LORA, "full": TRAIN_FULL}[train_mode], lora_r, lora_alpha, mask, beta1, beta2, eps, weight_decay, max_grad_norm, n_stack,
                    {"bf16": PRECISION_BF16, "strict": PRECISION_STRICT}[precision], int(zero[0]) if zero else 0, int(zero[1]) if zero else 0,
                    *rope_scaling_fields(None if cfg.get("arch") == "gpt2" else cfg.get("rope_scaling")))


class Context:
    """One fold worker's device context (weights + adapters + optimizer state + workspace on one GPU)."""

    def __init__(self, cfg: dict, device=0, max_tokens=2048, max_seqs=16, max_labelled=64, max_position=512, lora_r=16, lora_alpha=32.0,
                 lora_targets=("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"), beta1=0.9, beta2=0.999, eps=1e-8,
                 weight_decay=0.0, max_grad_norm=1.0, train_mode="lora", n_stack=1, precision="bf16", zero=None):
        """n_stack > 1 (LoRA): that many folds' adapters live in this context and train in lockstep on concatenated
        micro-batches (include/tst_hip.h "stacked folds"); max_tokens / max_seqs / max_labelled are totals over the slots.
        train_mode: "lora" (frozen base + adapters; forkable) or "full" (every weight trainable: fp32 master, Adam moments
        and gradient for all parameters live in HBM; trainables are then keyed by HF state_dict names).
        precision: "bf16" (product path) or "strict" (every tensor fp32, fp32 MFMA: the reference's fp32 arithmetic; parity mode).
        zero: None, or (ranks, rank) for a full fine-tune whose fp32 master / Adam moments are sharded over the fold's data-parallel group
        (ZeRO stage 1, include/tst_hip.h tst_model_cfg.zero_ranks): this context keeps shard `rank` of `ranks`."""
        self.lib = load()
        self.cfg = dict(cfg)
        self.gpt2 = cfg.get("arch") == "gpt2"
        mc = make_model_cfg(cfg, max_tokens, max_seqs, max_labelled, max_position, lora_r, lora_alpha, lora_targets, beta1, beta2, eps, weight_decay, max_grad_norm,
                            train_mode, n_stack, precision, zero)
        h = C.c_void_p()
        rc = self.lib.tst_create(C.byref(mc), device, C.byref(h))
        if rc != 0:
            raise TstError(f"tst_create failed ({rc}): {self.lib.tst_last_error(None).decode()}")
        self.h = h
        self.vocab = cfg["vocab_size"]
        self.device = device
        self.max_labelled = max_labelled
        self.n_stack = max(1, int(n_stack))
        self.precision = precision
        self.train_mode = train_mode
        self.zero = tuple(zero) if zero else None

    def fork(self):
        """a further fold on the same GPU: shares this context's frozen weights, owns adapters/optimizer/workspace/stream."""
        child = object.__new__(Context)
        child.lib, child.cfg, child.vocab, child.max_labelled, child.gpt2 = self.lib, self.cfg, self.vocab, self.max_labelled, self.gpt2
        child.n_stack = self.n_stack
        child.precision = self.precision
        child.train_mode = self.train_mode
        child.zero = self.zero
        h = C.c_void_p()
        self._check(self.lib.tst_fork(self.h, C.byref(h)), "tst_fork")
        child.h = h
        child.device = self.device
        child._parent = self  # keeps the weight owner alive
        return child

    def _check(self, rc, what):
        if rc != 0:
            raise TstError(f"{what} failed ({rc}): {self.lib.tst_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.tst_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def set_weight(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        self._check(self.lib.tst_set_weight(self.h, name.encode(), _ptr(a), DTYPE_F32, a.size), f"tst_set_weight({name})")

    def set_weight_bf16_bits(self, name, bits):
        """raw bf16 payload (uint16 bit patterns, e.g. straight out of a safetensors file): no host conversion"""
        a = np.ascontiguousarray(bits, dtype=np.uint16)
        self._check(self.lib.tst_set_weight(self.h, name.encode(), _ptr(a), DTYPE_BF16, a.size), f"tst_set_weight({name})")

    def get_weight(self, name, shape):
        out = np.empty(shape, np.float32)
        self._check(self.lib.tst_get_weight(self.h, name.encode(), _ptr(out), out.size), f"tst_get_weight({name})")
        return out

    def load_state_dict(self, sd):
        for k, v in sd.items():
            self.set_weight(k, v)
        self.finalize()

    def finalize(self):
        self._check(self.lib.tst_finalize_weights(self.h), "tst_finalize_weights")

    def init_random(self, seed=0, std=0.02):
        self._check(self.lib.tst_init_random(self.h, seed, std), "tst_init_random")

    def device_bytes(self):
        return int(self.lib.tst_device_bytes(self.h))

    # ---- trainables
    def trainable_layout(self):
        out = {}
        buf = C.create_string_buffer(128)
        off, rows, cols = C.c_int64(), C.c_int64(), C.c_int64()
        for i in range(self.lib.tst_trainable_count(self.h)):
            self._check(self.lib.tst_trainable_info(self.h, i, buf, 128, C.byref(off), C.byref(rows), C.byref(cols)), "tst_trainable_info")
            out[buf.value.decode()] = (off.value, rows.value, cols.value)
        return out

    def trainable_numel(self):
        return int(self.lib.tst_trainable_numel(self.h))

    def _is_conv1d(self, name):
        return self.gpt2 and name.endswith(CONV1D_SUFFIXES)

    def _flat_to_dict(self, flat):
        """name -> array; GPT-2 Conv1D weights are stored [out, in] on the device and handed out in the HF layout [in, out]."""
        out = {}
        for k, (o, r, c) in self.trainable_layout().items():
            a = flat[o:o + r * c].reshape(r, c)
            out[k] = np.ascontiguousarray(a.T) if self._is_conv1d(k) else a.copy()
        return out

    def get_trainable(self):
        flat = np.empty(self.trainable_numel(), np.float32)
        self._check(self.lib.tst_get_trainable(self.h, _ptr(flat)), "tst_get_trainable")
        return self._flat_to_dict(flat)

    def set_trainable(self, d):
        flat = np.zeros(self.trainable_numel(), np.float32)
        for k, (o, r, c) in self.trainable_layout().items():
            a = np.asarray(d[k], np.float32)
            flat[o:o + r * c] = (a.reshape(c, r).T if self._is_conv1d(k) else a).reshape(-1)
        self._check(self.lib.tst_set_trainable(self.h, _ptr(flat)), "tst_set_trainable")

    def get_grads(self):
        flat = np.empty(self.trainable_numel(), np.float32)
        self._check(self.lib.tst_get_grads(self.h, _ptr(flat)), "tst_get_grads")
        return self._flat_to_dict(flat)

    # ---- checkpoint / resume of a fold in progress (flat fp32 vectors in the order of trainable_layout())
    def state(self):
        """{"trainable", "m", "v": flat fp32 arrays, "step": int}: everything a fold needs to continue bit-identically"""
        n = self.trainable_numel()
        p, m, v = (np.empty(n, np.float32) for _ in range(3))
        step = C.c_int32()
        self._check(self.lib.tst_get_trainable(self.h, _ptr(p)), "tst_get_trainable")
        self._check(self.lib.tst_get_opt_state(self.h, _ptr(m), _ptr(v), C.byref(step)), "tst_get_opt_state")
        return dict(trainable=p, m=m, v=v, step=int(step.value))

    def load_state(self, st):
        n = self.trainable_numel()
        p, m, v = (np.ascontiguousarray(st[k], dtype=np.float32) for k in ("trainable", "m", "v"))
        if not (p.size == m.size == v.size == n):
            raise TstError(f"state has {p.size} trainables, this context has {n}")
        self._check(self.lib.tst_set_trainable(self.h, _ptr(p)), "tst_set_trainable")
        self._check(self.lib.tst_set_opt_state(self.h, _ptr(m), _ptr(v), int(st["step"])), "tst_set_opt_state")

    def grad_buffer(self):
        """(device address, numel) of the flat fp32 gradient: what intra-fold data parallelism all-reduces (tst/ddp.py)."""
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.tst_grad_buffer(self.h, C.byref(p), C.byref(n)), "tst_grad_buffer")
        return int(p.value), int(n.value)

    # ---- intra-fold data parallelism (tst/ddp.py drives these)
    @staticmethod
    def dp_unique_id():
        buf = C.create_string_buffer(128)
        if load().tst_dp_unique_id(buf, 128) != 0:
            raise TstError("tst_dp_unique_id failed")
        return buf.raw

    def dp_init(self, uid: bytes, nranks: int, rank: int):
        # RCCL announces itself on the process's STDOUT from inside ncclCommInitRank (version banner, C side): callers whose stdout is a protocol
        # (bench.py: one JSON line; tst.cli: records) must not see it there, so the descriptor points at stderr for the duration of the call
        with _stdout_to_stderr():
            rc = self.lib.tst_dp_init(self.h, C.c_char_p(uid), len(uid), nranks, rank)
        self._check(rc, "tst_dp_init")

    def dp_set_transport(self, dtype="f32"):
        """wire format of a full fine-tune's region-wise gradient reduction: "f32" or "bf16" (half the xGMI bytes; after dp_init)"""
        self._check(self.lib.tst_dp_set_transport(self.h, {"f32": DTYPE_F32, "bf16": DTYPE_BF16}[dtype]), "tst_dp_set_transport")

    def train_step_dp_async(self, ids, labels, cu, lr, num_items_global):
        """ids may be None / empty when this rank's shard has no sequence"""
        if ids is None or len(ids) == 0:
            self._check(self.lib.tst_train_step_dp_async(self.h, None, lr, num_items_global), "tst_train_step_dp_async")
            return
        b, keep = self._batch(ids, labels, cu)
        self._check(self.lib.tst_train_step_dp_async(self.h, C.byref(b), lr, num_items_global), "tst_train_step_dp_async")

    def dp_stats(self):
        """(collectives enqueued, fp32 elements reduced) since dp_init"""
        n, e = C.c_int64(), C.c_int64()
        self._check(self.lib.tst_dp_stats(self.h, C.byref(n), C.byref(e)), "tst_dp_stats")
        return int(n.value), int(e.value)

    def reset_optimizer(self):
        self._check(self.lib.tst_reset_optimizer(self.h), "tst_reset_optimizer")

    def reset_trainable(self, seed=0):
        self._check(self.lib.tst_reset_trainable(self.h, seed), "tst_reset_trainable")

    def set_option(self, name, value):
        """per-context switch (include/tst_hip.h tst_set_option: "last_compact", "trim_last_token", "opt_overlap", "dw_side", "swiglu_rank"); value < 0 queries.
        Returns the setting in force (a bool; the bit mask itself for "swiglu_rank")."""
        rc = int(self.lib.tst_set_option(self.h, name.encode(), int(value)))
        if rc < 0:
            raise RuntimeError(f"tst_set_option({name!r}): unknown option, or it does not apply to this context")
        return rc if name == "swiglu_rank" else bool(rc)

    def set_last_compact(self, on):
        return self.set_option("last_compact", on)

    # ---- stacked folds
    def select_slot(self, slot):
        """the slot addressed by get/set_trainable, get_grads, state/load_state, reset_trainable, reset_optimizer, fetch_metrics"""
        self._check(self.lib.tst_select_slot(self.h, int(slot)), "tst_select_slot")

    def train_step_stacked_async(self, ids, labels, cu, seq_slot, lrs):
        """one lockstep step of the stacked folds: sequences grouped by slot (seq_slot non-decreasing), lrs[slot]"""
        b, keep = self._batch(ids, labels, cu, seq_slot)
        lr_a = np.zeros(self.n_stack, np.float32)
        lr_a[:len(lrs)] = lrs
        self._check(self.lib.tst_train_step_stacked_async(self.h, C.byref(b), _ptr(lr_a)), "tst_train_step_stacked_async")

    def train_step_stacked_dp_async(self, ids, labels, cu, seq_slot, lrs, items_global):
        """one lockstep step of the stacked folds shared with the other ranks of the context's data-parallel group: this rank's part of
        the global batch (ids may be None: nothing of it here), items_global[slot] = labelled tokens of the slot over ALL ranks"""
        lr_a = np.zeros(self.n_stack, np.float32)
        lr_a[:len(lrs)] = lrs
        it_a = np.zeros(self.n_stack, np.int32)
        it_a[:len(items_global)] = items_global
        if ids is None or len(ids) == 0:
            self._check(self.lib.tst_train_step_stacked_dp_async(self.h, None, _ptr(lr_a), _ptr(it_a)), "tst_train_step_stacked_dp_async")
            return
        b, keep = self._batch(ids, labels, cu, seq_slot)
        self._check(self.lib.tst_train_step_stacked_dp_async(self.h, C.byref(b), _ptr(lr_a), _ptr(it_a)), "tst_train_step_stacked_dp_async")

    # ---- gradient accumulation
    def accumulate_async(self, ids, labels, cu, num_items, first, seq_slot=None):
        """forward + backward of one micro-batch of an accumulation window; num_items = labelled tokens of the WHOLE window (an int, or one
        count per slot of a stacked context)"""
        it_a = np.zeros(self.n_stack, np.int32)
        it_a[:] = num_items
        b, keep = self._batch(ids, labels, cu, seq_slot)
        self._check(self.lib.tst_accumulate_async(self.h, C.byref(b), _ptr(it_a), 1 if first else 0), "tst_accumulate_async")

    def fetch_loss(self):
        """per-slot loss of the last forward / backward pass alone (one micro-batch of an accumulation window)"""
        out = np.zeros(max(8, self.n_stack), np.float32)
        self._check(self.lib.tst_fetch_loss(self.h, _ptr(out)), "tst_fetch_loss")
        return out[:self.n_stack]

    def optimizer_step_async(self, lrs):
        lr_a = np.zeros(self.n_stack, np.float32)
        lr_a[:] = lrs
        self._check(self.lib.tst_optimizer_step_async(self.h, _ptr(lr_a)), "tst_optimizer_step_async")

    def fetch_metrics_stacked(self):
        loss, gn = np.zeros(self.n_stack, np.float32), np.zeros(self.n_stack, np.float32)
        self._check(self.lib.tst_fetch_metrics_stacked(self.h, _ptr(loss), _ptr(gn)), "tst_fetch_metrics_stacked")
        return loss, gn

    # ---- steps (packed batches)
    @staticmethod
    def _batch(ids, labels, cu, seq_slot=None):
        flags = 0
        if isinstance(ids, DeviceIds):
            ids_a, ids_p, flags = ids, C.cast(C.c_void_p(ids.ptr), C.POINTER(C.c_int32)), BATCH_DEVICE_IDS
        else:
            ids_a, ids_p = _i32(ids)
        cu_a, cu_p = _i32(cu)
        if labels is not None:
            lab_a, lab_p = _i32(labels)
        else:
            lab_a, lab_p = None, None
        if seq_slot is not None:
            sl_a, sl_p = _i32(seq_slot)
            if len(sl_a) != len(cu_a) - 1:
                raise TstError("seq_slot needs one entry per sequence")
        else:
            sl_a, sl_p = None, None
        b = Batch(ids_p, lab_p, cu_p, len(cu_a) - 1, len(ids_a), sl_p, flags)
        return b, (ids_a, lab_a, cu_a, sl_a)

    def forward_backward(self, ids, labels, cu, num_items=0, seq_slot=None):
        b, keep = self._batch(ids, labels, cu, seq_slot)
        loss = C.c_float()
        self._check(self.lib.tst_forward_backward(self.h, C.byref(b), num_items, C.byref(loss)), "tst_forward_backward")
        return loss.value

    def optimizer_step(self, lr):
        gn = C.c_float()
        self._check(self.lib.tst_optimizer_step(self.h, lr, C.byref(gn)), "tst_optimizer_step")
        return gn.value

    def train_step(self, ids, labels, cu, lr):
        b, keep = self._batch(ids, labels, cu)
        loss, gn = C.c_float(), C.c_float()
        self._check(self.lib.tst_train_step(self.h, C.byref(b), lr, C.byref(loss), C.byref(gn)), "tst_train_step")
        return loss.value, gn.value

    def train_step_async(self, ids, labels, cu, lr):
        b, keep = self._batch(ids, labels, cu)
        self._check(self.lib.tst_train_step_async(self.h, C.byref(b), lr), "tst_train_step_async")

    def fetch_metrics(self):
        loss, gn = C.c_float(), C.c_float()
        self._check(self.lib.tst_fetch_metrics(self.h, C.byref(loss), C.byref(gn)), "tst_fetch_metrics")
        return loss.value, gn.value

    def sync(self):
        self._check(self.lib.tst_sync(self.h), "tst_sync")

    def set_stream(self, hip_stream):
        """run this context's steps on the caller's HIP stream (an integer handle such as torch.cuda.current_stream().cuda_stream;
        0 is the legacy default stream); None returns to the context's own stream."""
        if hip_stream is None:
            self._check(self.lib.tst_set_stream(self.h, None, 0), "tst_set_stream")
        else:
            self._check(self.lib.tst_set_stream(self.h, C.c_void_p(int(hip_stream)), 1), "tst_set_stream")

    def score_rows_async(self, ids, labels, cu, option_ids=(), seq_slot=None):
        """enqueue a held-out scoring pass; results come from score_rows_fetch()."""
        b, keep = self._batch(ids, labels, cu, seq_slot)
        opt_a, n_opt, _ = _options(b, option_ids)
        self._check(self.lib.tst_score_async(self.h, C.byref(b), _ptr(opt_a), n_opt), "tst_score_async")
        self._pending_nopt = n_opt

    def score_rows_fetch(self):
        R, n_opt = self.max_labelled, self._pending_nopt
        logp = np.zeros(R, np.float32)
        correct = np.zeros(R, np.int32)
        optl = np.zeros((R, max(n_opt, 1)), np.float32)
        rseq = np.zeros(R, np.int32)
        n = C.c_int32()
        self._check(self.lib.tst_score_fetch(self.h, _ptr(logp), _ptr(correct), _ptr(optl), _ptr(rseq), C.byref(n)), "tst_score_fetch")
        n = n.value
        return logp[:n], correct[:n], optl.reshape(-1)[: n * n_opt].reshape(n, n_opt), rseq[:n]

    def score_rows(self, ids, labels, cu, option_ids=(), seq_slot=None):
        self.score_rows_async(ids, labels, cu, option_ids, seq_slot)
        return self.score_rows_fetch()

    # ---- greedy generation (include/tst_hip.h tst_generate_async)
    def generate_async(self, ids, cu, max_new_tokens, eos_ids=(), seq_slot=None):
        """enqueue the greedy continuation of the packed prompts (ids, cu) by max_new_tokens tokens each; results come from generate_fetch()."""
        b, keep = self._batch(ids, None, cu, seq_slot)
        eos_a, _ = _i32(np.asarray(eos_ids, np.int32) if len(eos_ids) else np.zeros(1, np.int32))
        self._check(self.lib.tst_generate_async(self.h, C.byref(b), int(max_new_tokens), _ptr(eos_a), len(eos_ids)), "tst_generate_async")
        self._pending_gen = (len(keep[2]) - 1, int(max_new_tokens))

    def generate_fetch(self):
        """(tokens [n_seqs, max_new] int32, logp [n_seqs, max_new], n_new [n_seqs]): rows are cut behind their first eos token (-1 / 0 behind it)"""
        n, m = getattr(self, "_pending_gen", None) or (1, 1)
        tok, logp, n_new = np.full((n, m), -1, np.int32), np.zeros((n, m), np.float32), np.zeros(n, np.int32)
        self._check(self.lib.tst_generate_fetch(self.h, _ptr(tok), _ptr(logp), _ptr(n_new)), "tst_generate_fetch")
        self._pending_gen = None
        return tok, logp, n_new

    def generate(self, ids, cu, max_new_tokens, eos_ids=(), seq_slot=None):
        self.generate_async(ids, cu, max_new_tokens, eos_ids, seq_slot)
        return self.generate_fetch()

    # ---- sampled generation (include/tst_hip.h tst_sample_async)
    def sample_async(self, ids, cu, max_new_tokens, n_samples, temperature, seq_seeds, eos_ids=(), seq_slot=None):
        """enqueue n_samples draws of max_new_tokens tokens from softmax(logits / temperature) for every packed prompt (ids, cu), at one prefill; seq_seeds = one
        uint64 per prompt (a prompt's draws depend on its logits, its seed, the step and the sample index only). Results come from sample_fetch()."""
        b, keep = self._batch(ids, None, cu, seq_slot)
        n_seqs = len(keep[2]) - 1
        seeds = np.ascontiguousarray(seq_seeds, np.uint64).reshape(-1)
        if len(seeds) != n_seqs:
            raise TstError("seq_seeds needs one seed per sequence")
        eos_a, _ = _i32(np.asarray(eos_ids, np.int32) if len(eos_ids) else np.zeros(1, np.int32))
        self._check(self.lib.tst_sample_async(self.h, C.byref(b), int(max_new_tokens), int(n_samples), float(temperature), _ptr(seeds), _ptr(eos_a), len(eos_ids)),
                    "tst_sample_async")
        self._pending_sample = (n_seqs, int(n_samples), int(max_new_tokens))

    def sample_fetch(self):
        """(tokens [n_seqs, n_samples, max_new] int32, logp (same shape), n_new [n_seqs, n_samples]): every draw is cut behind its first eos token (-1 / 0 behind it)"""
        s, n, m = getattr(self, "_pending_sample", None) or (1, 1, 1)
        tok, logp, n_new = np.full((s, n, m), -1, np.int32), np.zeros((s, n, m), np.float32), np.zeros((s, n), np.int32)
        self._check(self.lib.tst_sample_fetch(self.h, _ptr(tok), _ptr(logp), _ptr(n_new)), "tst_sample_fetch")
        self._pending_sample = None
        return tok, logp, n_new

    def sample(self, ids, cu, max_new_tokens, n_samples, temperature, seq_seeds, eos_ids=(), seq_slot=None):
        self.sample_async(ids, cu, max_new_tokens, n_samples, temperature, seq_seeds, eos_ids, seq_slot)
        return self.sample_fetch()

    # ---- candidate scoring (include/tst_hip.h tst_score_candidates_async)
    def score_candidates_async(self, ids, cu, cand_ids, cu_cand, cand_seq, seq_slot=None):
        """enqueue the exact log p(candidate | prompt) of the packed candidates (cand_ids, cu_cand; candidate c continues prompt cand_seq[c], non-decreasing) of
        the packed prompts (ids, cu), at one prefill. Results come from score_candidates_fetch()."""
        b, keep = self._batch(ids, None, cu, seq_slot)
        cu_c = np.ascontiguousarray(cu_cand, np.int32).reshape(-1)
        seq_c = np.ascontiguousarray(cand_seq, np.int32).reshape(-1)
        ids_c = np.ascontiguousarray(cand_ids, np.int32).reshape(-1)
        n_cands = len(cu_c) - 1
        if n_cands < 0 or len(seq_c) != n_cands or (n_cands >= 1 and len(ids_c) < int(cu_c.max())):
            raise TstError("cand_seq needs one entry per candidate and cand_ids cu_cand[-1] tokens")
        if len(ids_c) == 0:
            ids_c = np.zeros(1, np.int32)
        if len(seq_c) == 0:
            seq_c = np.zeros(1, np.int32)
        self._check(self.lib.tst_score_candidates_async(self.h, C.byref(b), _ptr(ids_c), _ptr(cu_c), _ptr(seq_c), n_cands), "tst_score_candidates_async")
        self._pending_cand = (int(cu_c[-1]), n_cands)

    def score_candidates_fetch(self):
        """(logp_tok [n_cand_tokens], logp_cand [n_cands]): the teacher-forced log-probability of every candidate token and their sum per candidate"""
        n_tok, n_c = getattr(self, "_pending_cand", None) or (1, 1)
        lt, lc = np.zeros(max(n_tok, 1), np.float32), np.zeros(max(n_c, 1), np.float32)
        self._check(self.lib.tst_score_candidates_fetch(self.h, _ptr(lt), _ptr(lc)), "tst_score_candidates_fetch")
        self._pending_cand = None
        return lt[:n_tok], lc[:n_c]

    def score_candidates(self, ids, cu, cand_ids, cu_cand, cand_seq, seq_slot=None):
        self.score_candidates_async(ids, cu, cand_ids, cu_cand, cand_seq, seq_slot)
        return self.score_candidates_fetch()

    # ---- token attribution (include/tst_hip.h tst_attribute_async)
    def attribute_async(self, ids, labels, cu, seq_kind=None, option_ids=(), seq_slot=None):
        """enqueue the input-gradient attribution of log s(x) for the packed batch; seq_kind[i] = 0 (open form: mean log-probability of the labelled tokens) or
        1 (option form: the one labelled token against option_ids); None = all open. Results come from attribute_fetch()."""
        b, keep = self._batch(ids, labels, cu, seq_slot)
        opt_a, n_opt, kind_a = _options(b, option_ids, seq_kind)
        self._check(self.lib.tst_attribute_async(self.h, C.byref(b), None if kind_a is None else _ptr(kind_a), _ptr(opt_a), n_opt), "tst_attribute_async")
        self._pending_attr = (len(keep[0]), len(keep[2]) - 1)

    def attribute_fetch(self):
        """(gxi [n_tokens], gnorm [n_tokens], log_s [n_seqs]): gradient x input and gradient norm of every token's embedding output, in the caller's token order"""
        n_tok, n_seq = getattr(self, "_pending_attr", None) or (1, 1)
        gxi, gnorm, logs = np.zeros(n_tok, np.float32), np.zeros(n_tok, np.float32), np.zeros(n_seq, np.float32)
        self._check(self.lib.tst_attribute_fetch(self.h, _ptr(gxi), _ptr(gnorm), _ptr(logs)), "tst_attribute_fetch")
        self._pending_attr = None
        return gxi, gnorm, logs

    def attribute(self, ids, labels, cu, seq_kind=None, option_ids=(), seq_slot=None):
        self.attribute_async(ids, labels, cu, seq_kind, option_ids, seq_slot)
        return self.attribute_fetch()

    # ---- integrated gradients (include/tst_hip.h tst_attribute_ig_async)
    def attribute_ig_async(self, ids, labels, cu, baseline_ids, n_steps, seq_kind=None, option_ids=(), seq_slot=None):
        """enqueue the integrated gradients of log s(x) from the baseline prompt baseline_ids (host ids, one per token; a token whose baseline is its own id is not
        interpolated) to the packed batch, n_steps midpoint steps. seq_kind / option_ids as for attribute_async. Results come from attribute_ig_fetch()."""
        b, keep = self._batch(ids, labels, cu, seq_slot)
        opt_a, n_opt, kind_a = _options(b, option_ids, seq_kind)
        base_a = None if baseline_ids is None else np.ascontiguousarray(baseline_ids, np.int32)
        if base_a is not None and len(base_a) != b.n_tokens:
            raise TstError("baseline_ids needs one entry per token")
        self._check(self.lib.tst_attribute_ig_async(self.h, C.byref(b), None if kind_a is None else _ptr(kind_a), _ptr(opt_a), n_opt,
                                                    None if base_a is None else _ptr(base_a), int(n_steps)), "tst_attribute_ig_async")
        self._pending_attr_ig = (int(b.n_tokens), int(b.n_seqs))

    def attribute_ig_fetch(self):
        """(ig [n_tokens], log_s [n_seqs], log_s_base [n_seqs]): per token the integrated gradient in the caller's token order; per sequence log s(x) of the real
        prompt and of the baseline prompt. The ig of a sequence's tokens sum to log_s - log_s_base up to the quadrature error of n_steps."""
        n_tok, n_seq = getattr(self, "_pending_attr_ig", None) or (1, 1)
        ig, logs, logs_base = np.zeros(n_tok, np.float32), np.zeros(n_seq, np.float32), np.zeros(n_seq, np.float32)
        self._check(self.lib.tst_attribute_ig_fetch(self.h, _ptr(ig), _ptr(logs), _ptr(logs_base)), "tst_attribute_ig_fetch")
        self._pending_attr_ig = None
        return ig, logs, logs_base

    def attribute_ig(self, ids, labels, cu, baseline_ids, n_steps, seq_kind=None, option_ids=(), seq_slot=None):
        self.attribute_ig_async(ids, labels, cu, baseline_ids, n_steps, seq_kind, option_ids, seq_slot)
        return self.attribute_ig_fetch()

    def forward_logits(self, ids, cu, rows, seq_slot=None):
        b, keep = self._batch(ids, None, cu, seq_slot)
        rows_a, _ = _i32(rows)
        out = np.empty((len(rows_a), self.vocab), np.float32)
        self._check(self.lib.tst_forward_logits(self.h, C.byref(b), _ptr(rows_a), len(rows_a), _ptr(out)), "tst_forward_logits")
        return out

    def profile_enable(self, on=True):
        """on: True / 1 = bracket every contraction launch with HIP events; 3 = also the HBM-bound kernel classes (ids 101-104); 0 = off"""
        self._check(self.lib.tst_profile_enable(self.h, int(on)), "tst_profile_enable")

    def profile_intervals(self, ref, variant=-1, unsplit_only=False, cap=1 << 20):
        """(start_ms, end_ms, flop) arrays of the logged launches, times relative to ref.profile_enable()."""
        st, en, fl = (np.zeros(cap, np.float64) for _ in range(3))
        n = C.c_int64()
        self._check(self.lib.tst_profile_intervals(self.h, ref.h, variant, 1 if unsplit_only else 0, _ptr(st), _ptr(en), _ptr(fl), cap, C.byref(n)),
                    "tst_profile_intervals")
        return st[:n.value], en[:n.value], fl[:n.value]

    def profile_read(self, variant=-1, unsplit_only=False, reset=True):
        """(total ms, total FLOP, launches) of the dense-contraction launches logged since profile_enable."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.tst_profile_read(self.h, variant, 1 if unsplit_only else 0, C.byref(ms), C.byref(fl), C.byref(n), 1 if reset else 0),
                    "tst_profile_read")
        return ms.value, fl.value, n.value
