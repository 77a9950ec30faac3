/*
 * libtst_host -- CPU-only C-ABI over the host arithmetic of libtst_hip (test-set-training_amd/csrc/host_logic.h): validation of the configuration and of
 * every batch, the labelled-row map, the flat layout of a full fine-tune and its gradient regions, the trainable table of the LoRA module groups, the ZeRO-1
 * shard map, the RoPE inverse frequencies. It is the SAME code the product
 * library runs on its hot path, compiled by g++ without any HIP dependency, so that it can be driven on a CPU box: by the Python CPU tests (the gloo
 * stand-ins for the multi-rank ZeRO step use the product's own shard map and layout) and, built with -fsanitize=address,undefined, by the self-test
 * csrc/host_selftest.cpp (sanitizers run on the CPU build only). TEST / DIAGNOSTIC surface: a maintainer binds include/tst_hip.h.
 * Upstream interface: none (/root/reference/README.md:38-39); the HF / torch lines each function restates are cited in host_logic.h.
 */
#ifndef TST_HOST_H
#define TST_HOST_H
#include <stdint.h>

#include "tst_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* inverse RoPE frequency i (0 .. head_dim / 2 - 1) of the configuration (modeling_rope_utils.py: default, linear, llama3) */
float tst_host_rope_inv_freq(const tst_model_cfg* cfg, int i);

/* ZeRO stage 1: shard `rank` of `ranks` of a flat trainable vector of n_train elements. out4 = {n_pad, shard length, lo, hi}; the shard owns [lo, hi). */
int tst_host_zero_shard(int64_t n_train, int ranks, int rank, int64_t* out4);
/* HF's decay / no-decay groups inside [lo, hi): out2 = {d_hi, n_lo}: weight decay on [lo, d_hi), none on [n_lo, hi) */
int tst_host_decay_split(int64_t lo, int64_t hi, int64_t n_decay, int64_t* out2);

/* flat layout of a full fine-tune of the configuration. out8 = {n_train, n_decay, per_layer, embed, wpe (-1: none), lm_head, first layer, tail};
 * regions_out (may be NULL) receives up to cap (offset, count) pairs in the order backward finishes them; *n_regions_out their number. */
int tst_host_full_layout(const tst_model_cfg* cfg, int64_t* out8, int64_t* regions_out, int cap, int* n_regions_out);

/* tsthost::check_cfg: every refusal tst_create (is_fork = 0) or tst_fork (is_fork = 1: the parent's configuration) makes from the configuration alone, in the
 * engine's order; err_out / err_cap receive the message tst_last_error would report. Returns TST_OK or TST_EINVAL. */
int tst_host_check_cfg(const tst_model_cfg* cfg, int is_fork, char* err_out, int err_cap);
/* tsthost::lora_layout: the trainable table of ONE slot of a LoRA context of the configuration, as tst_trainable_info reports it. out3 = {n1 (elements per
 * slot), n_train (n1 * max(n_stack, 1)), number of entries}; entry i (up to cap; both arrays may be NULL): names_out[i * name_cap ..] its name,
 * entries_out[3 i ..] = {offset, rows, cols}. */
int tst_host_lora_layout(const tst_model_cfg* cfg, int64_t* out3, char* names_out, int name_cap, int64_t* entries_out, int cap);

/* tsthost::plan_batch on a caller-provided staging buffer of tst_host_stage_ints(...) ints laid out ids[max_tokens] | pos[max_tokens] | cu[max_seqs + 1] |
 * lab_idx[max_labelled] | targets[max_labelled]. out_ints[4 + 8 + 9 + 8] = {T_dev, S, R, maxlen, slot_t_end[8], slot_r0[9], row_end[8]}; row_seq_out
 * [max_labelled]; err_out / err_cap receive the message of a refused batch. Returns TST_OK or TST_EINVAL. */
int64_t tst_host_stage_ints(const tst_model_cfg* cfg);
int tst_host_plan_batch(const tst_model_cfg* cfg, const tst_batch* b, int need_labels, int trim_last, const int32_t* rows, int n_rows, int32_t* stage,
                        int32_t* out_ints, int32_t* row_seq_out, char* err_out, int err_cap);

/* tsthost::plan_generate (greedy generation, include/tst_hip.h tst_generate_async): validation and the KV-cache row map of one generation, on host
 * buffers. out_ints[4 + 8] = {S, T, cache rows this generation uses, cache rows the context allocates for max_new, slot_s_end[8]}; meta_out [3 + 2 S]
 * (S | max_new | cu[0 .. S] | len[0 .. S)), last_rows_out [S], prefill_rows_out [T], decode_rows_out [(max_new - 1) S] may each be NULL; err_out / err_cap
 * receive the message of a refusal. Returns TST_OK or TST_EINVAL. */
int tst_host_plan_generate(const tst_model_cfg* cfg, const tst_batch* b, int max_new, const int32_t* eos_ids, int n_eos, int64_t* out_ints, int32_t* meta_out,
                           int32_t* last_rows_out, int32_t* prefill_rows_out, int32_t* decode_rows_out, char* err_out, int err_cap);
/* tsthost::plan_sample (sampled generation, include/tst_hip.h tst_sample_async): plan_generate's checks, n_samples in 1 .. 64, n_seqs n_samples <=
 * min(max_seqs, max_labelled) and <= max_tokens (a decode step's token rows), temperature in [0.01, 100], seq_seeds non-NULL; and the shared-prefix row map: prompts at cache rows 0 .. T, the tail of decode
 * row r = s n_samples + i at T + r max_new. out_ints[7 + 8] = {S, T, R = S n_samples, cache rows used, cache rows the context allocates for max_new, ints of the
 * device image, ints allocated for it, slot_r_end[8]}; geo_out [3 + 3 R] (R | max_new | n_samples | {pre_row0, len, tail_row0} per row), seeds_out [2 S] (low,
 * high word per sequence), last_rows_out [S], prefill_rows_out [T], decode_rows_out [(max_new - 1) R] may each be NULL. Returns TST_OK or TST_EINVAL. */
int tst_host_plan_sample(const tst_model_cfg* cfg, const tst_batch* b, int max_new, int n_samples, float temperature, const uint64_t* seq_seeds,
                         const int32_t* eos_ids, int n_eos, int64_t* out_ints, int32_t* geo_out, int32_t* seeds_out, int32_t* last_rows_out, int32_t* prefill_rows_out,
                         int32_t* decode_rows_out, char* err_out, int err_cap);
/* tsthost::plan_candidates (candidate scoring, include/tst_hip.h tst_score_candidates_async): every refusal of that call but the host ids of the prompts, and
 * the extend row map. out_ints[8 + 8] = {S, T, n_cand_tokens, R_e, candidates with at least two tokens, cache rows used (T + R_e), cache rows the context
 * allocates (max_tokens + max_seqs), ints of the call's device image at capacity, slot_r_end[8]}; geo_out [5 n_ext] ({pre_row0, len, tail_row0, q_row0, n_pos} per
 * candidate with at least two tokens), ext_rows_out / ext_ids_out / ext_pos_out / ext_tgt_out [R_e], src_out [2 n_cand_tokens] ({row, tok} per candidate token:
 * {prompt, c_0} for a first token, {extend row, -1} for a later one), last_rows_out [S] may each be NULL. Returns TST_OK or TST_EINVAL. */
int tst_host_plan_candidates(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int n_cands,
                             int64_t* out_ints, int32_t* geo_out, int32_t* ext_rows_out, int32_t* ext_ids_out, int32_t* ext_pos_out, int32_t* ext_tgt_out,
                             int32_t* src_out, int32_t* last_rows_out, char* err_out, int err_cap);
/* the fetch side of a generation: rows of tokens / logp [n_seqs, max_new] are cut behind their first token that is in eos_ids (tokens -1, logp 0 behind it;
 * n_new_out[s] counts the eos token), in place */
int tst_host_cut_at_eos(int32_t* tokens, float* logp, int32_t* n_new_out, int n_seqs, int max_new, const int32_t* eos_ids, int n_eos);

/* tsthost::plan_attribute (token attribution, include/tst_hip.h tst_attribute_async): the checks an attribution adds to a batch's own, and for every labelled
 * row -- by sequence, then by position -- its weight 1 / n_i, its kind and its sequence. The three outputs hold one entry per labelled token of the batch and
 * may each be NULL; err_out / err_cap receive the message of a refusal. Returns TST_OK or TST_EINVAL. */
int tst_host_plan_attribute(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int n_opt, int32_t* n_rows_out,
                            float* row_w_out, int32_t* row_kind_out, int32_t* row_seq_out, char* err_out, int err_cap);
/* the fetch side of an attribution: per-token values of the tokens the device ran (sequence s at [cu_dev[s], cu_dev[s + 1])) into the caller's token order
 * (sequence s at [cu_src[s], cu_src[s + 1])); a token the device did not run (trim_last_token) gets 0. TST_EINVAL when a sequence is longer on the device. */
int tst_host_untrim_tokens(const float* src, const int32_t* cu_dev, const int32_t* cu_src, int n_seqs, float* dst);
/* tsthost::plan_ig (integrated gradients, include/tst_hip.h tst_attribute_ig_async): the checks the call adds to tst_host_plan_attribute's -- baseline_ids (one per
 * token of the caller's batch, inside the vocabulary) and n_steps (1 .. TST_IG_MAX_STEPS). alpha_out, when not NULL, receives the n_steps midpoints
 * (k - 1/2) / n_steps in fp32 as the engine passes them to its kernels. err_out / err_cap receive the message of a refusal. Returns TST_OK or TST_EINVAL. */
int tst_host_plan_ig(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* baseline_ids, int n_steps, float* alpha_out, char* err_out, int err_cap);
/* the upload side: per-token ids of the caller's batch into the order the device runs them (the inverse of tst_host_untrim_tokens; a trimmed token is dropped) */
int tst_host_trim_tokens(const int32_t* src, const int32_t* cu_dev, const int32_t* cu_src, int n_seqs, int32_t* dst);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
