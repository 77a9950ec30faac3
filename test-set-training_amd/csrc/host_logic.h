// Host-only arithmetic of the engine -- validation of the configuration and of every batch, the labelled-row map, the flat layout of a full fine-tune and
// its gradient regions, the trainable table of the LoRA module groups, the ZeRO-1 shard map, the RoPE inverse frequencies. No HIP type appears here: the
// same header is compiled into libtst_hip.so by hipcc (engine.hip calls these functions on the product path) and, by g++ with
// -fsanitize=address,undefined, into the self-test csrc/host_selftest.cpp and the CPU-only library libtst_host.so (include/tst_host.h) that the CPU
// tests drive (SURVEY.md section 5 "sanitizers": run on the CPU build only).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tst_hip.h"

namespace tsthost {

constexpr int kMaxStack = 8;   // == TST_MAX_STACK (kernels.h; engine.hip static_asserts the two agree)

inline int roundup(int a, int b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------------------------------------------ RoPE
// inverse frequency i of the rotary embedding, fp32 arithmetic in the reference's operation order
// (transformers/modeling_rope_utils.py: _compute_default_rope_parameters, _compute_linear_scaling_rope_parameters, _compute_llama3_parameters)
inline float rope_inv_freq(const tst_model_cfg& c, int i, int dh) {
  const float inv_freq = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)dh);
  if (c.rope_scaling == TST_ROPE_LINEAR) return inv_freq / c.rope_factor;
  if (c.rope_scaling != TST_ROPE_LLAMA3) return inv_freq;
  const float old_len = (float)c.rope_original_max_position;
  const float low_wavelen = old_len / c.rope_low_freq_factor, high_wavelen = old_len / c.rope_high_freq_factor;
  const float wavelen = 6.283185307179586f / inv_freq;
  float f = wavelen > low_wavelen ? inv_freq / c.rope_factor : inv_freq;
  if (!(wavelen < high_wavelen) && !(wavelen > low_wavelen)) {
    const float smooth = (old_len / wavelen - c.rope_low_freq_factor) / (c.rope_high_freq_factor - c.rope_low_freq_factor);
    f = (1.0f - smooth) * f / c.rope_factor + smooth * f;
  }
  return f;
}

// ------------------------------------------------------------------------------------------------ ZeRO stage 1 shard map
// The flat trainable vector of n_train elements, padded to a multiple of 64 * ranks, is cut into `ranks` equal contiguous shards; rank r keeps the fp32
// master / m / v of elements [lo, hi) (hi clipped to n_train: the last shard may be ragged or, for tiny vectors, empty).
struct ZeroShard {
  int64_t n_pad, shard, lo, hi;
};
inline ZeroShard zero_shard(int64_t n_train, int ranks, int rank) {
  ZeroShard z;
  z.n_pad = (n_train + 64LL * ranks - 1) / (64LL * ranks) * (64LL * ranks);
  z.shard = z.n_pad / ranks;
  z.lo = (int64_t)rank * z.shard;
  z.hi = z.lo + z.shard < n_train ? z.lo + z.shard : n_train;
  if (z.hi < z.lo) z.hi = z.lo;
  return z;
}
// HF's two parameter groups (trainer.py:1181-1196) inside a shard: weight decay on [lo, d_hi) (matrices: the flat vector's first n_decay elements), none
// on [n_lo, hi) (norm vectors, biases). Either range may be empty (d_hi <= lo / hi <= n_lo).
struct DecaySplit {
  int64_t d_hi, n_lo;
};
inline DecaySplit decay_split(int64_t lo, int64_t hi, int64_t n_decay) {
  DecaySplit s;
  s.d_hi = hi < n_decay ? hi : n_decay;
  s.n_lo = lo > n_decay ? lo : n_decay;
  return s;
}

// ------------------------------------------------------------------------------------------------ flat layout of a full fine-tune
// ONE flat vector in the order [token embedding | (GPT-2: learned positions) | per layer Wqkv, Wo, Wgu, Wd | (Llama / Qwen2: lm_head) | norm vectors and
// biases (Qwen3: and the q_norm / k_norm head-norm vectors, per layer behind its two norm vectors)]: matrices first (= HF's decay group), vectors last. `regions` = the gradient regions in the order backward finishes them: lm_head (untied),
// layers L-1 .. 0, the embedding side, the vector tail -- the units of the region-wise data-parallel reduction.
struct ModelDims {
  int d, L, F, Fgu, V /* padded to 64 */, dq, dkv, dqkv, dattn, npos;
  bool gpt2, qkv_bias;
  bool qk_norm;   // Qwen3: two [dh] head-norm vectors per layer
  int dh;
};
inline ModelDims model_dims(const tst_model_cfg& c) {
  ModelDims m;
  m.d = c.hidden_size; m.L = c.num_layers; m.F = c.intermediate_size;
  m.gpt2 = c.arch == TST_ARCH_GPT2;
  m.qkv_bias = c.arch == TST_ARCH_QWEN2 || m.gpt2;
  m.qk_norm = c.arch == TST_ARCH_QWEN3;
  m.dh = c.head_dim;
  m.V = roundup(c.vocab_size, 64);
  m.Fgu = m.gpt2 ? m.F : 2 * m.F;
  m.npos = c.max_position;
  m.dq = c.num_heads * c.head_dim; m.dkv = c.num_kv_heads * c.head_dim; m.dqkv = m.dq + 2 * m.dkv; m.dattn = m.dq;
  return m;
}
// a layer's four projections [dout, din]: q|k|v, o, gate|up (GPT-2: c_fc), down -- the order of the flat buffer, the optimizer and the module groups
inline void proj_dims(const ModelDims& m, int dout[4], int din[4]) {
  const int pd[4][2] = {{m.dqkv, m.d}, {m.d, m.dattn}, {m.Fgu, m.d}, {m.d, m.F}};
  for (int p = 0; p < 4; ++p) { dout[p] = pd[p][0]; din[p] = pd[p][1]; }
}
struct FullLayout {
  int64_t n_decay = 0, n_train = 0, per_layer = 0;
  int64_t embed = 0, wpe = -1, lm_head = -1, layer0 = 0;   // offsets (lm_head = embed when tied)
  int64_t tail = 0;                                         // first element of the no-decay group
  std::vector<std::pair<int64_t, int64_t>> regions;         // (offset, count), launch order of the region-wise reduction
};
inline FullLayout full_layout(const ModelDims& m) {
  FullLayout f;
  const int64_t V = m.V, d = m.d;
  f.per_layer = (int64_t)m.dqkv * d + (int64_t)d * m.dattn + (int64_t)m.Fgu * d + (int64_t)d * m.F;
  f.n_decay = (m.gpt2 ? V * d + (int64_t)m.npos * d : 2 * V * d) + m.L * f.per_layer;
  f.n_train = f.n_decay + (m.gpt2 ? (int64_t)m.L * (4 * d + m.dqkv + d + m.Fgu + d) + 2 * d : (int64_t)(2 * m.L + 1) * d + (m.qkv_bias ? (int64_t)m.L * m.dqkv : 0) + (m.qk_norm ? (int64_t)m.L * 2 * m.dh : 0));
  int64_t o = 0;
  f.embed = o; o += V * d;
  if (m.gpt2) { f.wpe = o; o += (int64_t)m.npos * d; }
  f.layer0 = o; o += m.L * f.per_layer;
  if (m.gpt2) f.lm_head = f.embed; else { f.lm_head = o; o += V * d; }
  f.tail = o;
  if (!m.gpt2) f.regions.push_back({f.lm_head, V * d});
  for (int l = m.L - 1; l >= 0; --l) f.regions.push_back({f.layer0 + l * f.per_layer, f.per_layer});
  f.regions.push_back({0, f.layer0});
  f.regions.push_back({f.tail, f.n_train - f.tail});
  return f;
}

// ------------------------------------------------------------------------------------------------ the configuration: what tst_create / tst_fork refuse
// Every refusal the engine makes from the tst_model_cfg alone, BEFORE anything is allocated; TST_OK, or TST_EINVAL with `err` set. is_fork: the configuration
// of a context about to be forked (tst_fork). The order is part of the interface: a configuration with several faults reports the first.
inline int check_cfg(const tst_model_cfg& c, bool is_fork, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (c.precision != TST_PRECISION_BF16 && c.precision != TST_PRECISION_STRICT) return fail("precision must be TST_PRECISION_BF16 or TST_PRECISION_STRICT");
  const bool gpt2 = c.arch == TST_ARCH_GPT2, full = c.train_mode == TST_TRAIN_FULL;
  if (c.arch != TST_ARCH_LLAMA && c.arch != TST_ARCH_QWEN2 && c.arch != TST_ARCH_QWEN3 && !gpt2) return fail("unsupported arch");
  if (c.hidden_size <= 0 || c.num_layers <= 0 || c.num_heads <= 0 || c.num_kv_heads <= 0 || c.head_dim <= 0 || c.intermediate_size <= 0 || c.vocab_size <= 0)
    return fail("hidden_size/num_layers/num_heads/num_kv_heads/head_dim/intermediate_size/vocab_size must be > 0");
  const ModelDims m = model_dims(c);
  if (gpt2 && c.num_kv_heads != c.num_heads) return fail("GPT-2: num_kv_heads must equal num_heads");
  if (gpt2 && m.dq != m.d) return fail("GPT-2: num_heads * head_dim must equal hidden_size");
  if (c.train_mode != TST_TRAIN_LORA && !full) return fail("train_mode must be TST_TRAIN_LORA or TST_TRAIN_FULL");
  if (full && is_fork) return fail("full fine-tune contexts cannot be forked (every fold owns its weights)");
  if (m.dh != 128 && !(gpt2 && m.dh == 64)) return fail("head_dim must be 128 (GPT-2 family: 64 or 128)");
  if (m.d % 64 || m.F % 64 || m.dq % 64 || m.dkv % 64) return fail("hidden/intermediate/head sizes must be multiples of 64");
  if (c.num_heads % c.num_kv_heads) return fail("num_heads must be a multiple of num_kv_heads");
  if (c.max_tokens <= 0 || c.max_seqs <= 0 || c.max_labelled <= 0 || c.max_position <= 0) return fail("max_tokens/max_seqs/max_labelled/max_position must be > 0");
  if (!full && (c.lora_r <= 0 || c.lora_r > 64 || (64 % c.lora_r) != 0)) return fail("lora_r must divide 64");
  if (!gpt2 && c.rope_scaling != TST_ROPE_DEFAULT) {
    if (c.rope_scaling != TST_ROPE_LINEAR && c.rope_scaling != TST_ROPE_LLAMA3) return fail("rope_scaling must be TST_ROPE_DEFAULT, TST_ROPE_LINEAR or TST_ROPE_LLAMA3");
    if (!(c.rope_factor > 0.f)) return fail("rope_factor must be > 0");
    if (c.rope_scaling == TST_ROPE_LLAMA3 && (!(c.rope_low_freq_factor > 0.f) || !(c.rope_high_freq_factor > c.rope_low_freq_factor) || c.rope_original_max_position <= 0))
      return fail("llama3 rope scaling needs 0 < rope_low_freq_factor < rope_high_freq_factor and rope_original_max_position > 0");
  }
  const bool stacked = c.n_stack > 1, zero_on = c.zero_ranks >= 1;
  if (c.n_stack > kMaxStack) return fail("n_stack must be <= 8");
  if (stacked && full) return fail("stacked folds need frozen base weights (LoRA): a full fine-tune owns its weights");
  if (stacked && (c.lora_r & 7)) return fail("stacked folds: lora_r must be a multiple of 8");
  if (stacked && c.precision == TST_PRECISION_STRICT) return fail("stacked folds are a bf16-path feature: precision = strict runs one fold per context");
  if (zero_on && !full) return fail("optimizer-state sharding (zero_ranks >= 1) is for full fine-tunes: LoRA state is 0.2 % of the model");
  if (zero_on && (c.zero_rank < 0 || c.zero_rank >= c.zero_ranks || c.zero_ranks > 64)) return fail("zero_rank must be in [0, zero_ranks), zero_ranks <= 64");
  if (!full && !(c.lora_targets & TST_LORA_ALL)) return fail("no trainable parameters (lora_targets empty)");   // (both families' tables below cover every bit)
  return TST_OK;
}

// ------------------------------------------------------------------------------------------------ LoRA module groups and their trainable table
// A layer has one module group per projection (P_QKV .. P_D, proj_dims' order): the peft modules that share the projection's input, each owning a row range of
// its output. Per naming family: the modules of the four groups and the target bit(s) that enable each; module j's rows end at split[j], the last one's at dout.
// GPT-2's peft targets are its four Conv1D modules: c_attn (any of Q/K/V), attn.c_proj (O), c_fc (GATE/UP), mlp.c_proj (DOWN).
struct LoraModule { const char* name; unsigned bits; };
struct LoraGroupSpec { int nmod; LoraModule mod[3]; };
constexpr LoraGroupSpec kLoraLlama[4] = {{3, {{"q_proj", TST_LORA_Q}, {"k_proj", TST_LORA_K}, {"v_proj", TST_LORA_V}}}, {1, {{"o_proj", TST_LORA_O}}},
                                         {2, {{"gate_proj", TST_LORA_GATE}, {"up_proj", TST_LORA_UP}}}, {1, {{"down_proj", TST_LORA_DOWN}}}};
constexpr LoraGroupSpec kLoraGpt2[4] = {{1, {{"attn.c_attn", TST_LORA_Q | TST_LORA_K | TST_LORA_V}}}, {1, {{"attn.c_proj", TST_LORA_O}}},
                                        {1, {{"mlp.c_fc", TST_LORA_GATE | TST_LORA_UP}}}, {1, {{"mlp.c_proj", TST_LORA_DOWN}}}};
// The flat trainable vector of ONE slot: per layer, per group, per enabled module lora_A [r, din] then lora_B [rows, r]; slot s of a stacked context holds the
// same table shifted by s * n1. group[4 l + p] = the enabled modules of layer l's projection p: their row ranges and the offsets of A and B.
struct TrainableEntry { std::string name; int64_t offset, rows, cols; };
struct LoraGroupLayout { int nseg = 0, row0[3], row1[3]; int64_t a_off[3], b_off[3]; };
struct LoraLayout { int64_t n1 = 0, n_train = 0; std::vector<TrainableEntry> entries; std::vector<LoraGroupLayout> group; };
inline LoraLayout lora_layout(const ModelDims& m, int r, unsigned targets, int n_stack) {
  LoraLayout out;
  int dout[4], din[4];
  proj_dims(m, dout, din);
  const int split[4][2] = {{m.dq, m.dq + m.dkv}, {0, 0}, {m.F, 0}, {0, 0}};
  out.group.resize((size_t)(m.L > 0 ? m.L : 0) * 4);
  for (int l = 0; l < m.L; ++l)
    for (int p = 0; p < 4; ++p) {
      const LoraGroupSpec& spec = (m.gpt2 ? kLoraGpt2 : kLoraLlama)[p];
      LoraGroupLayout& g = out.group[(size_t)4 * l + p];
      for (int j = 0, row = 0; j < spec.nmod; ++j) {
        const int end = j + 1 < spec.nmod ? split[p][j] : dout[p];
        if (targets & spec.mod[j].bits) {
          const std::string pre = "layers." + std::to_string(l) + "." + spec.mod[j].name;
          g.row0[g.nseg] = row; g.row1[g.nseg] = end;
          g.a_off[g.nseg] = out.n1;
          out.entries.push_back({pre + ".lora_A", out.n1, r, din[p]});
          out.n1 += (int64_t)r * din[p];
          g.b_off[g.nseg++] = out.n1;
          out.entries.push_back({pre + ".lora_B", out.n1, end - row, r});
          out.n1 += (int64_t)(end - row) * r;
        }
        row = end;
      }
    }
  out.n_train = out.n1 * (n_stack > 1 ? n_stack : 1);
  return out;
}

// ------------------------------------------------------------------------------------------------ batch validation + the labelled-row map
// The pinned staging buffer of a context (and its device mirror) is ONE int array laid out ids[Tmax] | pos[Tmax] | cu[Smax + 1] | lab_idx[Rmax] |
// targets[Rmax] | order[Smax]; plan_batch fills it from the caller's packed batch and returns what the step needs to know about it.
// order = the sequence indices by DECREASING device-side length (ties: lower index first): the attention backward launches one workgroup per (sequence,
// KV head) whose cost grows with length^2, and workgroups are dispatched in grid order -- heaviest first ends the launch on the lightest ones instead of on a
// straggler (78.7 -> 60.0 us alone on the benchmark's micro-batch, profiles/r04_attention_launch_order.txt). Pure scheduling: no output depends on it.
struct BatchLimits {
  int Tmax, Smax, Rmax, V, max_position, ns;
};
inline size_t stage_ints(const BatchLimits& l) { return (size_t)2 * l.Tmax + (size_t)(l.Smax + 1) + 2 * (size_t)l.Rmax + (size_t)l.Smax; }
struct BatchPlan {
  int T_dev = 0, S = 0, R = 0, maxlen = 0;
  double sumsq_len = 0;            // sum over the sequences of length^2 (attention work)
  int slot_t_end[kMaxStack];       // tokens of slot s end here
  int slot_r0[kMaxStack + 1];      // labelled rows of slot s are [slot_r0[s], slot_r0[s + 1])
  int row_end[kMaxStack];          // the same as ends (the compacted last layer's row boundaries)
  bool lc_batch_ok = true;         // false: caller-chosen rows on a stacked context (the last layer stays whole)
};
// need_labels: labels -> rows (position p predicts labels[p + 1], loss_utils.py:59-63). trim_last: the last token of every sequence is not run (it
// predicts nothing and nothing attends to it). rows != nullptr: caller-chosen rows instead (tst_forward_logits). dev_ids: input_ids is a DEVICE pointer --
// never dereferenced here; with trim the ids slot receives the SOURCE INDEX of every kept token (gathered on the device).
// Returns TST_OK, or TST_EINVAL with `err` set; row_seq receives the sequence of every labelled row.
inline int plan_batch(const tst_batch* b, const BatchLimits& lim, bool need_labels, bool trim_last, const int32_t* rows, int n_rows, int* stage, BatchPlan& out,
                      std::vector<int>& row_seq, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (!b) return fail("null batch");
  const int T = b->n_tokens, S = b->n_seqs;
  if (T <= 0 || S <= 0 || T > lim.Tmax || S > lim.Smax) return fail("batch exceeds max_tokens/max_seqs or is empty");
  if (!b->input_ids || !b->cu_seqlens) return fail("null batch pointers");
  if (b->cu_seqlens[0] != 0 || b->cu_seqlens[S] != T) return fail("cu_seqlens must start at 0 and end at n_tokens");
  int* h_ids = stage;
  int* h_pos = h_ids + lim.Tmax;
  int* h_cu = h_pos + lim.Tmax;
  int* h_lab = h_cu + (lim.Smax + 1);
  int* h_tgt = h_lab + lim.Rmax;
  int* h_ord = h_tgt + lim.Rmax;
  int maxlen = 0, R = 0;
  double sumsq_len = 0;
  row_seq.clear();
  const bool trim = trim_last && need_labels && !rows;
  const bool dev_ids = (b->flags & TST_BATCH_DEVICE_IDS) != 0;
  // stacked folds: sequences are grouped by slot (seq_slot non-decreasing); slot boundaries in tokens and labelled rows
  int cur_slot = 0, o = 0;   // o = first device-side token of the sequence
  for (int q = 0; q < kMaxStack; ++q) out.slot_r0[q + 1] = 0;
  out.slot_r0[0] = 0;
  for (int s = 0; s < S; ++s) {
    const int s0 = b->cu_seqlens[s], s1 = b->cu_seqlens[s + 1];
    if (s0 < 0 || s1 > T || s1 < s0) return fail("cu_seqlens must be non-decreasing and within n_tokens");
    const int len = s1 - s0;
    if (b->seq_slot) {
      const int sl = b->seq_slot[s];
      if (sl < cur_slot || sl >= lim.ns) return fail("seq_slot must be non-decreasing and < n_stack");
      for (; cur_slot < sl; ++cur_slot) { out.slot_t_end[cur_slot] = o; out.slot_r0[cur_slot + 1] = R; }
    }
    if (len <= 0 || len > lim.max_position) return fail("sequence length out of range (1..max_position)");
    const int keep = (trim && len >= 2) ? len - 1 : len;
    if (keep > maxlen) maxlen = keep;
    sumsq_len += (double)keep * keep;
    h_cu[s] = o;
    for (int p = 0; p < keep; ++p) h_pos[o + p] = p;
    if (!dev_ids) {
      // ids outside the vocabulary would be clamped by the embedding kernels: a tokenizer with added tokens must fail loudly instead (the trimmed token too)
      for (int p = 0; p < len; ++p)
        if (b->input_ids[s0 + p] < 0 || b->input_ids[s0 + p] >= lim.V) return fail("input id out of vocabulary");
      memcpy(h_ids + o, b->input_ids + s0, sizeof(int) * (size_t)keep);
    } else if (trim) {
      for (int p = 0; p < keep; ++p) h_ids[o + p] = s0 + p;   // source index of the device-side token (ids_gather)
    }
    if (need_labels) {
      if (!b->labels) return fail("labels required");
      for (int p = 0; p + 1 < len; ++p) {
        const int tgt = b->labels[s0 + p + 1];
        if (tgt != -100) {
          if (tgt < 0 || tgt >= lim.V) return fail("label out of vocabulary");
          if (R >= lim.Rmax) return fail("more labelled tokens than max_labelled");
          h_lab[R] = o + p;
          h_tgt[R] = tgt;
          row_seq.push_back(s);
          ++R;
        }
      }
    }
    o += keep;
  }
  h_cu[S] = o;
  const int T_dev = o;   // tokens the model runs (== T unless trimmed)
  {   // launch order of the per-sequence attention workgroups: longest first (counting sort over the lengths 1 .. max_position, stable)
    std::vector<int> first((size_t)maxlen + 2, 0);
    for (int s = 0; s < S; ++s) first[(size_t)(maxlen - (h_cu[s + 1] - h_cu[s])) + 1] += 1;
    for (int l = 0; l <= maxlen; ++l) first[(size_t)l + 1] += first[(size_t)l];
    for (int s = 0; s < S; ++s) h_ord[first[(size_t)(maxlen - (h_cu[s + 1] - h_cu[s]))]++] = s;
  }
  for (int q = cur_slot; q < kMaxStack; ++q) out.slot_t_end[q] = T_dev;
  for (; cur_slot < kMaxStack; ++cur_slot) out.slot_r0[cur_slot + 1] = R;
  for (int q = 0; q < kMaxStack; ++q) out.row_end[q] = out.slot_r0[q + 1];
  if (rows) {
    if (n_rows > lim.Rmax || n_rows < 0) return fail("more rows than max_labelled");
    for (int r = 0; r < n_rows; ++r) {
      if (rows[r] < 0 || rows[r] >= T) return fail("row index out of range");
      h_lab[r] = rows[r];
      h_tgt[r] = 0;
    }
    R = n_rows;
    for (int q = 0; q < kMaxStack; ++q) out.row_end[q] = R;   // (caller-chosen rows carry no slot order: a stacked context keeps the last layer whole)
  }
  out.lc_batch_ok = !(rows && lim.ns > 1);
  out.T_dev = T_dev; out.S = S; out.R = R; out.maxlen = maxlen; out.sumsq_len = sumsq_len;
  return TST_OK;
}

// ------------------------------------------------------------------------------------------------ greedy generation: validation + the cache row map
// A generation continues the packed prompts of `b` by max_new tokens each. The KV cache of a layer is [rows, Hkv dh] with the row of (sequence s, position p)
// = cu[s] + s max_new + p: the packed prompts with room for the new tokens behind each; it holds max_tokens + max_seqs max_new rows (gen_cache_rows).
// plan_generate refuses what the engine cannot run BEFORE anything is launched and fills the staging image of the generation's device array:
//   meta         [3 + 2 S]        S | max_new | cu[0 .. S] | len[0 .. S)                       (what attn_decode / next_token read, csrc/decode.hip)
//   last_rows    [S]              packed index of every prompt's last token: the rows the prefill's head runs on
//   prefill_rows [T]              cache row of every prompt token
//   decode_rows  [(max_new-1) S]  cache row of the token decode step j = 1 .. max_new - 1 appends for sequence s, at [(j - 1) S + s]
//   slot_s_end   [kMaxStack]      sequences of slots 0 .. q (a decode step's "tokens" are its sequences: these are its slot boundaries)
// input_ids is never dereferenced (it may be a device pointer); ids and lengths 1 .. max_position are plan_batch's to check.
constexpr int kGenMaxNew = 256;   // == TST_GEN_MAX_NEW
constexpr int kGenMaxEos = 16;
inline long gen_cache_rows(const BatchLimits& l, int max_new) { return (long)l.Tmax + (long)l.Smax * max_new; }
// ints of the device array at capacity: meta | prefill_rows | decode_rows
inline size_t gen_dev_ints(const BatchLimits& l, int max_new) { return (size_t)(3 + 2 * l.Smax) + (size_t)l.Tmax + (size_t)l.Smax * (size_t)max_new; }
struct GenPlan {
  int S = 0, T = 0, max_new = 0;
  long rows_used = 0;   // rows of the cache this generation touches (<= gen_cache_rows)
  std::vector<int> meta, last_rows, prefill_rows, decode_rows;
  int slot_s_end[kMaxStack];
};
inline int plan_generate(const tst_batch* b, const BatchLimits& lim, int max_new, const int32_t* eos_ids, int n_eos, GenPlan& out, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (!b) return fail("null batch");
  if (max_new < 1 || max_new > kGenMaxNew) return fail("max_new_tokens out of range (1..TST_GEN_MAX_NEW)");
  if (n_eos < 0 || n_eos > kGenMaxEos || (n_eos > 0 && !eos_ids)) return fail("more than 16 eos ids (or a null list)");
  for (int i = 0; i < n_eos; ++i)
    if (eos_ids[i] < 0 || eos_ids[i] >= lim.V) return fail("eos id out of vocabulary");
  const int T = b->n_tokens, S = b->n_seqs;
  if (T <= 0 || S <= 0 || T > lim.Tmax || S > lim.Smax) return fail("batch exceeds max_tokens/max_seqs or is empty");
  if (S > lim.Rmax) return fail("more sequences than max_labelled: the head runs on one row per sequence");
  if (!b->input_ids || !b->cu_seqlens) return fail("null batch pointers");
  if (b->cu_seqlens[0] != 0 || b->cu_seqlens[S] != T) return fail("cu_seqlens must start at 0 and end at n_tokens");
  out.S = S; out.T = T; out.max_new = max_new;
  out.meta.assign((size_t)3 + 2 * (size_t)S, 0);
  out.last_rows.assign((size_t)S, 0);
  out.prefill_rows.assign((size_t)T, 0);
  out.decode_rows.assign((size_t)(max_new - 1) * (size_t)S, 0);
  out.meta[0] = S; out.meta[1] = max_new;
  int cur_slot = 0;
  for (int s = 0; s < S; ++s) {
    const int s0 = b->cu_seqlens[s], s1 = b->cu_seqlens[s + 1];
    if (s0 < 0 || s1 > T || s1 < s0) return fail("cu_seqlens must be non-decreasing and within n_tokens");
    const int len = s1 - s0;
    if (len <= 0) return fail("sequence length out of range (1..max_position)");
    if ((long)len + max_new > lim.max_position) return fail("prompt length + max_new_tokens exceeds max_position");
    if (b->seq_slot) {
      const int sl = b->seq_slot[s];
      if (sl < cur_slot || sl >= lim.ns) return fail("seq_slot must be non-decreasing and < n_stack");
      for (; cur_slot < sl; ++cur_slot) out.slot_s_end[cur_slot] = s;
    }
    out.meta[(size_t)2 + s] = s0;
    out.meta[(size_t)3 + S + s] = len;
    out.last_rows[(size_t)s] = s1 - 1;
    const int row0 = s0 + s * max_new;
    for (int p = 0; p < len; ++p) out.prefill_rows[(size_t)s0 + p] = row0 + p;
    for (int j = 1; j < max_new; ++j) out.decode_rows[(size_t)(j - 1) * S + s] = row0 + len + j - 1;
  }
  out.meta[(size_t)2 + S] = T;
  for (; cur_slot < kMaxStack; ++cur_slot) out.slot_s_end[cur_slot] = S;
  out.rows_used = (long)T + (long)S * max_new;
  return TST_OK;
}
// ------------------------------------------------------------------------------------------------ sampled generation: validation + the shared-prefix row map
// tst_sample_async draws n_samples continuations of every prompt at one prefill: decode row r = s n_samples + i (s-major, so a stacked context's slot order is
// kept) attends to its prompt's cache rows, which the n samples share, and then to its own tail. The prompts are packed at cache rows 0 .. T; the tail of decode row
// r starts at T + r max_new. That fits gen_cache_rows because S n_samples <= max_seqs. A decode step is a forward pass over S n_samples token rows, so that
// product is held to max_tokens as well. plan_sample refuses what the engine cannot run BEFORE anything is launched
// and fills the staging image of the generation's device array (offsets: sample_off_*):
//   geo          [3 + 3 R]        R | max_new | n_samples | {pre_row0, len, tail_row0} per decode row    (what attn_decode_shared / sample_rows read)
//   seeds        [2 S]            low, high 32 bits of seq_seeds[s]: the Philox key of sequence s (a small device array of its own: geo | prefill_rows |
//                                 decode_rows fill exactly the ints a greedy generation's image has, gen_dev_ints)
//   last_rows    [S]              packed index of every prompt's last token: the rows the prefill's head runs on
//   prefill_rows [T]              cache row of every prompt token (its packed index)
//   decode_rows  [(max_new-1) R]  cache row of the token decode step j = 1 .. max_new - 1 appends for decode row r (the one step j - 1 drew), at [(j - 1) R + r]
//   slot_r_end   [kMaxStack]      decode rows of slots 0 .. q: plan_generate's slot_s_end times n_samples
constexpr int kSampleMaxN = 64;
constexpr float kSampleMinTemp = 0.01f, kSampleMaxTemp = 100.0f;
inline size_t sample_off_prefill(const BatchLimits& l) { return (size_t)3 + 3 * (size_t)l.Smax; }
inline size_t sample_off_decode(const BatchLimits& l) { return sample_off_prefill(l) + (size_t)l.Tmax; }
// ints of a sampled generation's image at capacity (== gen_dev_ints)
inline size_t sample_dev_ints(const BatchLimits& l, int max_new) { return sample_off_decode(l) + (size_t)l.Smax * (size_t)(max_new - 1); }
struct SamplePlan {
  int S = 0, T = 0, R = 0, max_new = 0, n_samples = 0;
  long rows_used = 0;   // rows of the cache this generation touches (<= gen_cache_rows)
  std::vector<int> geo, seeds, last_rows, prefill_rows, decode_rows;
  int slot_r_end[kMaxStack];
};
inline int plan_sample(const tst_batch* b, const BatchLimits& lim, int max_new, int n_samples, float temperature, const uint64_t* seq_seeds, const int32_t* eos_ids,
                       int n_eos, SamplePlan& out, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  GenPlan g;
  if (const int rc = plan_generate(b, lim, max_new, eos_ids, n_eos, g, err)) return rc;
  if (n_samples < 1 || n_samples > kSampleMaxN) return fail("n_samples out of range (1..64)");
  const long R = (long)g.S * n_samples;
  if (R > lim.Smax || R > lim.Rmax) return fail("n_seqs * n_samples exceeds max_seqs or max_labelled: every draw is a decode row");
  // a decode step runs the model over R token rows: the activation buffers, ids and positions hold max_tokens of them (a greedy step has n_seqs <= n_tokens rows)
  if (R > lim.Tmax) return fail("n_seqs * n_samples exceeds max_tokens: every draw is a token row of a decode step");
  if (!(temperature >= kSampleMinTemp && temperature <= kSampleMaxTemp)) return fail("temperature must be finite and in [0.01, 100]");   // (a NaN fails both)
  if (!seq_seeds) return fail("null seq_seeds");
  const int S = g.S, T = g.T;
  out.S = S; out.T = T; out.R = (int)R; out.max_new = max_new; out.n_samples = n_samples;
  out.geo.assign((size_t)3 + 3 * (size_t)R, 0);
  out.seeds.assign(2 * (size_t)S, 0);
  out.last_rows = g.last_rows;
  out.prefill_rows.assign((size_t)T, 0);
  out.decode_rows.assign((size_t)(max_new - 1) * (size_t)R, 0);
  out.geo[0] = (int)R; out.geo[1] = max_new; out.geo[2] = n_samples;
  for (int t = 0; t < T; ++t) out.prefill_rows[(size_t)t] = t;
  for (int s = 0; s < S; ++s) {
    out.seeds[2 * (size_t)s] = (int)(uint32_t)(seq_seeds[s] & 0xffffffffu);
    out.seeds[2 * (size_t)s + 1] = (int)(uint32_t)(seq_seeds[s] >> 32);
    for (int i = 0; i < n_samples; ++i) {
      const size_t r = (size_t)s * n_samples + i;
      const int tail0 = T + (int)r * max_new;
      out.geo[3 + 3 * r] = g.meta[(size_t)2 + s];
      out.geo[4 + 3 * r] = g.meta[(size_t)3 + S + s];
      out.geo[5 + 3 * r] = tail0;
      for (int j = 1; j < max_new; ++j) out.decode_rows[(size_t)(j - 1) * R + r] = tail0 + j - 1;
    }
  }
  for (int q = 0; q < kMaxStack; ++q) out.slot_r_end[q] = g.slot_s_end[q] * n_samples;
  out.rows_used = (long)T + R * max_new;
  return TST_OK;
}
// ------------------------------------------------------------------------------------------------ candidate scoring: validation + the extend row map
// tst_score_candidates_async scores n_cands given continuations of the packed prompts at ONE prefill: candidate c = tokens [cu_cand[c], cu_cand[c + 1]) continues
// prompt cand_seq[c]. Its first token is read from the prompt's one logits row; every later token c_{p + 1} needs the model's output behind c_p, so candidate c
// adds L_c - 1 "extend rows" (c, p), p = 0 .. L_c - 2, ordered c-major (cand_seq is non-decreasing: the rows keep the prompts' slot order). Row (c, p) is fed c_p at
// position len + p and its k | v go to cache row T + (cu_cand[c] - c) + p: the tails packed behind the prompts at rows 0 .. T, a one-token candidate taking none.
// That fits the cache of a one-token generation (gen_cache_rows(l, 1) = max_tokens + max_seqs) because R_e <= max_seqs. plan_candidates refuses what the engine
// cannot run BEFORE anything is allocated or launched and fills the images:
//   geo          [5 n_ext]   {pre_row0, len, tail_row0, q_row0, n_pos} per candidate with L_c >= 2, in candidate order   (what attn_extend reads)
//   ext_rows     [R_e]       cache row of every extend row (what kv_append reads)
//   src          [2 n_tok]   {row, tok} per candidate token, what cand_logp reads: first tokens {prompt s, c_0}, later ones {extend row of (c, p - 1), -1}
//   ext_ids / ext_pos / ext_tgt [R_e]   input id, position and head target c_{p + 1} of every extend row
//   last_rows    [S]         packed index of every prompt's last token;   prefill_rows [T] = 0 .. T - 1
//   slot_r_end   [kMaxStack] extend rows of the prompts in slots 0 .. q
// b->input_ids is never dereferenced (it may be a device pointer); the candidates' ids are host memory.
constexpr int kCandMaxLen = 16;   // == TST_CAND_MAX_LEN
inline int cand_ext_cap(const BatchLimits& l) { return std::min(l.Tmax, std::min(l.Smax, l.Rmax)); }
inline size_t cand_off_rows(const BatchLimits& l) { return 5 * (size_t)cand_ext_cap(l); }
inline size_t cand_off_src(const BatchLimits& l) { return 6 * (size_t)cand_ext_cap(l); }
// ints of the call's own device image at capacity: geo | ext_rows | src
inline size_t cand_dev_ints(const BatchLimits& l) { return cand_off_src(l) + 2 * (size_t)l.Rmax; }
struct CandPlan {
  int S = 0, T = 0, n_cands = 0, n_tok = 0, R_e = 0, n_ext = 0;
  long rows_used = 0;   // rows of the cache this call touches: T + R_e (<= gen_cache_rows(l, 1))
  std::vector<int> geo, ext_rows, src, ext_ids, ext_pos, ext_tgt, last_rows, prefill_rows;
  int slot_r_end[kMaxStack];
};
inline int plan_candidates(const tst_batch* b, const BatchLimits& lim, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int n_cands,
                           CandPlan& out, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (!b) return fail("null batch");
  const int T = b->n_tokens, S = b->n_seqs;
  if (T <= 0 || S <= 0 || T > lim.Tmax || S > lim.Smax) return fail("batch exceeds max_tokens/max_seqs or is empty");
  if (S > lim.Rmax) return fail("more sequences than max_labelled: the head runs on one row per sequence");
  if (!b->input_ids || !b->cu_seqlens) return fail("null batch pointers");
  if (b->cu_seqlens[0] != 0 || b->cu_seqlens[S] != T) return fail("cu_seqlens must start at 0 and end at n_tokens");
  if (n_cands < 1) return fail("n_cands must be at least 1");
  if (!cand_ids || !cu_cand || !cand_seq) return fail("null candidate pointers");
  out = CandPlan();
  out.S = S; out.T = T; out.n_cands = n_cands;
  out.last_rows.assign((size_t)S, 0);
  out.prefill_rows.assign((size_t)T, 0);
  for (int t = 0; t < T; ++t) out.prefill_rows[(size_t)t] = t;
  std::vector<int> slot_of((size_t)S, 0);
  int cur_slot = 0;
  for (int s = 0; s < S; ++s) {
    const int s0 = b->cu_seqlens[s], s1 = b->cu_seqlens[s + 1];
    if (s0 < 0 || s1 > T || s1 < s0) return fail("cu_seqlens must be non-decreasing and within n_tokens");
    const int len = s1 - s0;
    if (len <= 0 || len > lim.max_position) return fail("sequence length out of range (1..max_position)");
    if (b->seq_slot) {
      const int sl = b->seq_slot[s];
      if (sl < cur_slot || sl >= lim.ns) return fail("seq_slot must be non-decreasing and < n_stack");
      cur_slot = sl;
      slot_of[(size_t)s] = sl;
    }
    out.last_rows[(size_t)s] = s1 - 1;
  }
  if (cu_cand[0] != 0) return fail("cu_cand must start at 0 and increase strictly");
  const long ext_cap = cand_ext_cap(lim);
  long n_tok = 0, R_e = 0;
  int prev_seq = 0;
  for (int c = 0; c < n_cands; ++c) {
    const long L = (long)cu_cand[c + 1] - (long)cu_cand[c];
    if (L < 1) return fail("cu_cand must start at 0 and increase strictly");
    if (L > kCandMaxLen) return fail("a candidate is longer than TST_CAND_MAX_LEN (16) tokens");
    n_tok += L;
    if (n_tok > lim.Rmax) return fail("the candidates' tokens exceed max_labelled");
    const int s = cand_seq[c];
    if (s < 0 || s >= S) return fail("cand_seq out of range (0..n_seqs-1)");
    if (s < prev_seq) return fail("cand_seq must be non-decreasing");
    prev_seq = s;
    const int len = b->cu_seqlens[s + 1] - b->cu_seqlens[s];
    if ((long)len + L - 1 > lim.max_position) return fail("prompt length + candidate length - 1 exceeds max_position");
    for (long p = 0; p < L; ++p) {
      const int id = cand_ids[cu_cand[c] + p];
      if (id < 0 || id >= lim.V) return fail("candidate id out of vocabulary");
    }
    R_e += L - 1;
    if (R_e > ext_cap) return fail("the candidates' extend rows (sum of length - 1) exceed min(max_tokens, max_seqs, max_labelled)");
  }
  out.n_tok = (int)n_tok; out.R_e = (int)R_e;
  out.src.assign(2 * (size_t)n_tok, 0);
  out.ext_rows.assign((size_t)R_e, 0);
  out.ext_ids.assign((size_t)R_e, 0);
  out.ext_pos.assign((size_t)R_e, 0);
  out.ext_tgt.assign((size_t)R_e, 0);
  for (int q = 0; q < kMaxStack; ++q) out.slot_r_end[q] = 0;
  int r = 0;
  for (int c = 0; c < n_cands; ++c) {
    const int c0 = cu_cand[c], L = cu_cand[c + 1] - c0, s = cand_seq[c];
    const int s0 = b->cu_seqlens[s], len = b->cu_seqlens[s + 1] - s0;
    const int tail0 = T + (c0 - c);
    out.src[2 * (size_t)c0] = s;
    out.src[2 * (size_t)c0 + 1] = cand_ids[c0];
    if (L >= 2) {
      const int g[5] = {s0, len, tail0, r, L - 1};
      out.geo.insert(out.geo.end(), g, g + 5);
      ++out.n_ext;
    }
    for (int p = 0; p + 1 < L; ++p, ++r) {
      out.ext_rows[(size_t)r] = tail0 + p;
      out.ext_ids[(size_t)r] = cand_ids[c0 + p];
      out.ext_pos[(size_t)r] = len + p;
      out.ext_tgt[(size_t)r] = cand_ids[c0 + p + 1];
      out.src[2 * (size_t)(c0 + p + 1)] = r;
      out.src[2 * (size_t)(c0 + p + 1) + 1] = -1;
    }
    for (int q = slot_of[(size_t)s]; q < kMaxStack; ++q) out.slot_r_end[q] = r;
  }
  out.rows_used = (long)T + R_e;
  return TST_OK;
}
// the fetch side: row s of tokens / logp [S, max_new] is cut behind its first token that is in eos_ids -- n_new[s] counts that token, the entries behind
// it become -1 / 0; without a hit n_new[s] = max_new. In place.
inline void cut_at_eos(int32_t* tokens, float* logp, int32_t* n_new, int S, int max_new, const int32_t* eos_ids, int n_eos) {
  for (int s = 0; s < S; ++s) {
    int n = max_new;
    for (int j = 0; j < max_new && n == max_new; ++j)
      for (int e = 0; e < n_eos; ++e)
        if (tokens[(size_t)s * max_new + j] == eos_ids[e]) { n = j + 1; break; }
    for (int j = n; j < max_new; ++j) {
      tokens[(size_t)s * max_new + j] = -1;
      if (logp) logp[(size_t)s * max_new + j] = 0.0f;
    }
    if (n_new) n_new[s] = n;
  }
}

// ------------------------------------------------------------------------------------------------ token attribution: validation, row weights, the fetch side
// An attribution (include/tst_hip.h tst_attribute_async) differentiates J = sum_i J_i, J_i = log s(x_i): the mean log-probability of sequence i's labelled rows
// (kind 0, the open form) or logit[target] - logsumexp over option_ids on its ONE labelled row (kind 1, the option form). plan_attribute refuses what the engine
// cannot run BEFORE anything is launched and gives every labelled row -- in plan_batch's order: by sequence, then by position -- its weight 1 / n_i and its kind.
// Ids, labels and lengths against the vocabulary / max_position and the context's capacities stay plan_batch's to check; input_ids is never dereferenced.
constexpr int kAttrMaxOpt = 256;
struct AttrPlan {
  int R = 0;
  std::vector<float> row_w;
  std::vector<int> row_kind, row_seq;
};
inline int plan_attribute(const tst_batch* b, const BatchLimits& lim, const int32_t* seq_kind, const int32_t* option_ids, int n_opt, AttrPlan& out, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (!b) return fail("null batch");
  if (n_opt < 0 || n_opt > kAttrMaxOpt || (n_opt > 0 && !option_ids)) return fail("n_opt out of range (0..256), or a null option list");
  for (int j = 0; j < n_opt; ++j)
    if (option_ids[j] < 0 || option_ids[j] >= lim.V) return fail("option id out of vocabulary");
  const int T = b->n_tokens, S = b->n_seqs;
  if (T <= 0 || S <= 0 || T > lim.Tmax || S > lim.Smax) return fail("batch exceeds max_tokens/max_seqs or is empty");
  if (!b->input_ids || !b->cu_seqlens) return fail("null batch pointers");
  if (!b->labels) return fail("labels required");
  if (b->cu_seqlens[0] != 0 || b->cu_seqlens[S] != T) return fail("cu_seqlens must start at 0 and end at n_tokens");
  out.R = 0;
  out.row_w.clear(); out.row_kind.clear(); out.row_seq.clear();
  for (int s = 0; s < S; ++s) {
    const int s0 = b->cu_seqlens[s], s1 = b->cu_seqlens[s + 1];
    if (s0 < 0 || s1 > T || s1 < s0) return fail("cu_seqlens must be non-decreasing and within n_tokens");
    const int kind = seq_kind ? seq_kind[s] : 0;
    if (kind != 0 && kind != 1) return fail("seq_kind must be 0 (open form) or 1 (option form)");
    if (kind == 1 && n_opt == 0) return fail("an option-form sequence needs option ids (n_opt == 0)");
    int n = 0, tgt = -1;
    for (int p = s0 + 1; p < s1; ++p)
      if (b->labels[p] != -100) { ++n; tgt = b->labels[p]; }
    if (kind == 1) {
      if (n != 1) return fail("an option-form sequence must have exactly one labelled token");
      bool found = false;
      for (int j = 0; j < n_opt && !found; ++j) found = option_ids[j] == tgt;
      if (!found) return fail("the target of an option-form sequence is not one of the option ids");
    }
    for (int q = 0; q < n; ++q) {
      out.row_w.push_back(kind == 1 ? 1.0f : 1.0f / (float)n);
      out.row_kind.push_back(kind);
      out.row_seq.push_back(s);
    }
    out.R += n;
  }
  if (out.R == 0) return fail("batch has no labelled tokens");
  return TST_OK;
}
// J_i of every sequence from the rows the seed kernel leaves, stats[r] = {lse, logit[target], option logsumexp, max}: sequences without a labelled row get 0
inline void attr_logs(const float* stats, const AttrPlan& p, int S, float* logs_out) {
  std::vector<double> acc((size_t)S, 0.0);
  for (int r = 0; r < p.R; ++r) {
    const float* st = stats + (size_t)r * 4;
    const double j = p.row_kind[(size_t)r] ? (double)st[1] - (double)st[2] : (double)st[1] - (double)st[0];
    acc[(size_t)p.row_seq[(size_t)r]] += (double)p.row_w[(size_t)r] * j;
  }
  for (int s = 0; s < S; ++s) logs_out[s] = (float)acc[(size_t)s];
}
// Per-token results back into the caller's token order: the device ran the tokens [cu_dev[s], cu_dev[s + 1]) of sequence s, the caller's batch holds it at
// [cu_src[s], cu_src[s + 1]) (trim_last_token: one token more, the last one); a token the device did not run gets 0. TST_EINVAL when the two maps do not fit.
inline int untrim_tokens(const float* src, const int32_t* cu_dev, const int32_t* cu_src, int S, float* dst) {
  if (!src || !cu_dev || !cu_src || !dst || S < 0) return TST_EINVAL;
  for (int s = 0; s < S; ++s) {
    const int nd = cu_dev[s + 1] - cu_dev[s], ns = cu_src[s + 1] - cu_src[s];
    if (cu_dev[s] < 0 || cu_src[s] < 0 || nd < 0 || ns < nd) return TST_EINVAL;
  }
  for (int s = 0; s < S; ++s) {
    const int nd = cu_dev[s + 1] - cu_dev[s], ns = cu_src[s + 1] - cu_src[s];
    for (int p = 0; p < ns; ++p) dst[cu_src[s] + p] = p < nd ? src[cu_dev[s] + p] : 0.0f;
  }
  return TST_OK;
}

// ------------------------------------------------------------------------------------------------ integrated gradients: what they add to an attribution
// tst_attribute_ig_async walks the embedding-layer output from b[t] = embed_tokens[baseline_ids[t]] to the real e[t] in n_steps midpoint steps. plan_ig refuses,
// BEFORE anything is allocated or launched, what plan_attribute and plan_batch do not look at: the baseline ids (host memory, one per token of the caller's batch,
// inside the vocabulary) and the step count. The batch is only read for n_tokens, which plan_attribute has checked by then.
constexpr int kIgMaxSteps = 256;   // == TST_IG_MAX_STEPS
inline int plan_ig(const tst_batch* b, const BatchLimits& lim, const int32_t* baseline_ids, int n_steps, std::string& err) {
  auto fail = [&](const char* m) { err = m; return TST_EINVAL; };
  if (!b) return fail("null batch");
  if (n_steps < 1 || n_steps > kIgMaxSteps) return fail("n_steps out of range (1..256)");
  if (!baseline_ids) return fail("null baseline_ids");
  if (b->n_tokens <= 0 || b->n_tokens > lim.Tmax) return fail("batch exceeds max_tokens/max_seqs or is empty");
  for (int t = 0; t < b->n_tokens; ++t)
    if (baseline_ids[t] < 0 || baseline_ids[t] >= lim.V) return fail("baseline id out of vocabulary");
  return TST_OK;
}
// alpha of midpoint step k = 1 .. m, in fp32 as the engine passes it to embed_interp
inline float ig_alpha(int k, int m) { return ((float)k - 0.5f) / (float)m; }
// The inverse of untrim_tokens for per-token inputs: the caller's tokens (sequence s at [cu_src[s], cu_src[s + 1])) into the order the device runs them
// (sequence s at [cu_dev[s], cu_dev[s + 1]), its first tokens; trim_last_token drops the last one). The baseline ids follow the input ids through it.
inline int trim_tokens_i32(const int32_t* src, const int32_t* cu_dev, const int32_t* cu_src, int S, int32_t* dst) {
  if (!src || !cu_dev || !cu_src || !dst || S < 0) return TST_EINVAL;
  for (int s = 0; s < S; ++s) {
    const int nd = cu_dev[s + 1] - cu_dev[s], ns = cu_src[s + 1] - cu_src[s];
    if (cu_dev[s] < 0 || cu_src[s] < 0 || nd < 0 || ns < nd) return TST_EINVAL;
  }
  for (int s = 0; s < S; ++s) {
    const int nd = cu_dev[s + 1] - cu_dev[s];
    for (int p = 0; p < nd; ++p) dst[cu_dev[s] + p] = src[cu_src[s] + p];
  }
  return TST_OK;
}

}  // namespace tsthost
