// libtst_host.so: the C-ABI of include/tst_host.h over host_logic.h (g++, no HIP). See the header.
#include "../../include/tst_host.h"

#include "host_logic.h"

extern "C" {

float tst_host_rope_inv_freq(const tst_model_cfg* cfg, int i) { return cfg ? tsthost::rope_inv_freq(*cfg, i, cfg->head_dim) : 0.0f; }

int tst_host_zero_shard(int64_t n_train, int ranks, int rank, int64_t* out4) {
  if (!out4 || ranks < 1 || rank < 0 || rank >= ranks || n_train < 0) return TST_EINVAL;
  const tsthost::ZeroShard z = tsthost::zero_shard(n_train, ranks, rank);
  out4[0] = z.n_pad; out4[1] = z.shard; out4[2] = z.lo; out4[3] = z.hi;
  return TST_OK;
}

int tst_host_decay_split(int64_t lo, int64_t hi, int64_t n_decay, int64_t* out2) {
  if (!out2) return TST_EINVAL;
  const tsthost::DecaySplit s = tsthost::decay_split(lo, hi, n_decay);
  out2[0] = s.d_hi; out2[1] = s.n_lo;
  return TST_OK;
}

int tst_host_full_layout(const tst_model_cfg* cfg, int64_t* out8, int64_t* regions_out, int cap, int* n_regions_out) {
  if (!cfg || !out8) return TST_EINVAL;
  const tsthost::FullLayout f = tsthost::full_layout(tsthost::model_dims(*cfg));
  out8[0] = f.n_train; out8[1] = f.n_decay; out8[2] = f.per_layer; out8[3] = f.embed; out8[4] = f.wpe; out8[5] = f.lm_head; out8[6] = f.layer0; out8[7] = f.tail;
  if (n_regions_out) *n_regions_out = (int)f.regions.size();
  if (regions_out)
    for (int i = 0; i < (int)f.regions.size() && i < cap; ++i) { regions_out[2 * i] = f.regions[(size_t)i].first; regions_out[2 * i + 1] = f.regions[(size_t)i].second; }
  return TST_OK;
}

int tst_host_check_cfg(const tst_model_cfg* cfg, int is_fork, char* err_out, int err_cap) {
  if (!cfg) return TST_EINVAL;
  std::string err;
  const int rc = tsthost::check_cfg(*cfg, is_fork != 0, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  return rc;
}

int tst_host_lora_layout(const tst_model_cfg* cfg, int64_t* out3, char* names_out, int name_cap, int64_t* entries_out, int cap) {
  if (!cfg || !out3 || cfg->num_layers < 0 || cfg->lora_r < 0) return TST_EINVAL;
  const tsthost::LoraLayout l = tsthost::lora_layout(tsthost::model_dims(*cfg), cfg->lora_r, cfg->lora_targets, cfg->n_stack);
  out3[0] = l.n1; out3[1] = l.n_train; out3[2] = (int64_t)l.entries.size();
  for (int i = 0; i < (int)l.entries.size() && i < cap; ++i) {
    const tsthost::TrainableEntry& e = l.entries[(size_t)i];
    if (names_out && name_cap > 0) {
      strncpy(names_out + (size_t)i * name_cap, e.name.c_str(), (size_t)name_cap - 1);
      names_out[(size_t)i * name_cap + name_cap - 1] = 0;
    }
    if (entries_out) { entries_out[3 * i] = e.offset; entries_out[3 * i + 1] = e.rows; entries_out[3 * i + 2] = e.cols; }
  }
  return TST_OK;
}

static tsthost::BatchLimits limits_of(const tst_model_cfg& c) {
  return {c.max_tokens, c.max_seqs, c.max_labelled, c.vocab_size, c.max_position, c.n_stack > 1 ? c.n_stack : 1};
}

int64_t tst_host_stage_ints(const tst_model_cfg* cfg) { return cfg ? (int64_t)tsthost::stage_ints(limits_of(*cfg)) : 0; }

int tst_host_plan_batch(const tst_model_cfg* cfg, const tst_batch* b, int need_labels, int trim_last, const int32_t* rows, int n_rows, int32_t* stage,
                        int32_t* out_ints, int32_t* row_seq_out, char* err_out, int err_cap) {
  if (!cfg || !stage || !out_ints) return TST_EINVAL;
  tsthost::BatchPlan plan;
  std::vector<int> row_seq;
  std::string err;
  const int rc = tsthost::plan_batch(b, limits_of(*cfg), need_labels != 0, trim_last != 0, rows, n_rows, stage, plan, row_seq, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  int32_t* o = out_ints;
  *o++ = plan.T_dev; *o++ = plan.S; *o++ = plan.R; *o++ = plan.maxlen;
  for (int q = 0; q < tsthost::kMaxStack; ++q) *o++ = plan.slot_t_end[q];
  for (int q = 0; q <= tsthost::kMaxStack; ++q) *o++ = plan.slot_r0[q];
  for (int q = 0; q < tsthost::kMaxStack; ++q) *o++ = plan.row_end[q];
  if (row_seq_out)
    for (size_t i = 0; i < row_seq.size(); ++i) row_seq_out[i] = row_seq[i];
  return TST_OK;
}

int tst_host_plan_generate(const tst_model_cfg* cfg, const tst_batch* b, int max_new, const int32_t* eos_ids, int n_eos, int64_t* out_ints, int32_t* meta_out,
                           int32_t* last_rows_out, int32_t* prefill_rows_out, int32_t* decode_rows_out, char* err_out, int err_cap) {
  if (!cfg || !out_ints) return TST_EINVAL;
  tsthost::GenPlan g;
  std::string err;
  const tsthost::BatchLimits lim = limits_of(*cfg);
  const int rc = tsthost::plan_generate(b, lim, max_new, eos_ids, n_eos, g, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  int64_t* o = out_ints;
  *o++ = g.S; *o++ = g.T; *o++ = g.rows_used; *o++ = tsthost::gen_cache_rows(lim, max_new);
  for (int q = 0; q < tsthost::kMaxStack; ++q) *o++ = g.slot_s_end[q];
  auto put = [](int32_t* dst, const std::vector<int>& v) {
    if (dst)
      for (size_t i = 0; i < v.size(); ++i) dst[i] = v[i];
  };
  put(meta_out, g.meta); put(last_rows_out, g.last_rows); put(prefill_rows_out, g.prefill_rows); put(decode_rows_out, g.decode_rows);
  return TST_OK;
}

int tst_host_plan_sample(const tst_model_cfg* cfg, const tst_batch* b, int max_new, int n_samples, float temperature, const uint64_t* seq_seeds,
                         const int32_t* eos_ids, int n_eos, int64_t* out_ints, int32_t* geo_out, int32_t* seeds_out, int32_t* last_rows_out, int32_t* prefill_rows_out,
                         int32_t* decode_rows_out, char* err_out, int err_cap) {
  if (!cfg || !out_ints) return TST_EINVAL;
  tsthost::SamplePlan g;
  std::string err;
  const tsthost::BatchLimits lim = limits_of(*cfg);
  const int rc = tsthost::plan_sample(b, lim, max_new, n_samples, temperature, seq_seeds, eos_ids, n_eos, g, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  int64_t* o = out_ints;
  *o++ = g.S; *o++ = g.T; *o++ = g.R; *o++ = g.rows_used; *o++ = tsthost::gen_cache_rows(lim, max_new);
  *o++ = (int64_t)tsthost::sample_dev_ints(lim, max_new); *o++ = (int64_t)tsthost::gen_dev_ints(lim, max_new);
  for (int q = 0; q < tsthost::kMaxStack; ++q) *o++ = g.slot_r_end[q];
  auto put = [](int32_t* dst, const std::vector<int>& v) {
    if (dst)
      for (size_t i = 0; i < v.size(); ++i) dst[i] = v[i];
  };
  put(geo_out, g.geo); put(seeds_out, g.seeds); put(last_rows_out, g.last_rows); put(prefill_rows_out, g.prefill_rows); put(decode_rows_out, g.decode_rows);
  return TST_OK;
}

int tst_host_plan_candidates(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int n_cands,
                             int64_t* out_ints, int32_t* geo_out, int32_t* ext_rows_out, int32_t* ext_ids_out, int32_t* ext_pos_out, int32_t* ext_tgt_out,
                             int32_t* src_out, int32_t* last_rows_out, char* err_out, int err_cap) {
  if (!cfg || !out_ints) return TST_EINVAL;
  tsthost::CandPlan g;
  std::string err;
  const tsthost::BatchLimits lim = limits_of(*cfg);
  const int rc = tsthost::plan_candidates(b, lim, cand_ids, cu_cand, cand_seq, n_cands, g, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  int64_t* o = out_ints;
  *o++ = g.S; *o++ = g.T; *o++ = g.n_tok; *o++ = g.R_e; *o++ = g.n_ext; *o++ = g.rows_used; *o++ = tsthost::gen_cache_rows(lim, 1);
  *o++ = (int64_t)tsthost::cand_dev_ints(lim);
  for (int q = 0; q < tsthost::kMaxStack; ++q) *o++ = g.slot_r_end[q];
  auto put = [](int32_t* dst, const std::vector<int>& v) {
    if (dst)
      for (size_t i = 0; i < v.size(); ++i) dst[i] = v[i];
  };
  put(geo_out, g.geo); put(ext_rows_out, g.ext_rows); put(ext_ids_out, g.ext_ids); put(ext_pos_out, g.ext_pos); put(ext_tgt_out, g.ext_tgt);
  put(src_out, g.src); put(last_rows_out, g.last_rows);
  return TST_OK;
}

int tst_host_cut_at_eos(int32_t* tokens, float* logp, int32_t* n_new_out, int n_seqs, int max_new, const int32_t* eos_ids, int n_eos) {
  if (!tokens || n_seqs < 0 || max_new < 1 || n_eos < 0 || (n_eos > 0 && !eos_ids)) return TST_EINVAL;
  tsthost::cut_at_eos(tokens, logp, n_new_out, n_seqs, max_new, eos_ids, n_eos);
  return TST_OK;
}

int tst_host_plan_attribute(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int n_opt, int32_t* n_rows_out,
                            float* row_w_out, int32_t* row_kind_out, int32_t* row_seq_out, char* err_out, int err_cap) {
  if (!cfg) return TST_EINVAL;
  tsthost::AttrPlan p;
  std::string err;
  const int rc = tsthost::plan_attribute(b, limits_of(*cfg), seq_kind, option_ids, n_opt, p, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  if (n_rows_out) *n_rows_out = p.R;
  for (int r = 0; r < p.R; ++r) {
    if (row_w_out) row_w_out[r] = p.row_w[(size_t)r];
    if (row_kind_out) row_kind_out[r] = p.row_kind[(size_t)r];
    if (row_seq_out) row_seq_out[r] = p.row_seq[(size_t)r];
  }
  return TST_OK;
}

int tst_host_untrim_tokens(const float* src, const int32_t* cu_dev, const int32_t* cu_src, int n_seqs, float* dst) {
  return tsthost::untrim_tokens(src, cu_dev, cu_src, n_seqs, dst);
}

int tst_host_plan_ig(const tst_model_cfg* cfg, const tst_batch* b, const int32_t* baseline_ids, int n_steps, float* alpha_out, char* err_out, int err_cap) {
  if (!cfg) return TST_EINVAL;
  std::string err;
  const int rc = tsthost::plan_ig(b, limits_of(*cfg), baseline_ids, n_steps, err);
  if (err_out && err_cap > 0) {
    strncpy(err_out, err.c_str(), (size_t)err_cap - 1);
    err_out[err_cap - 1] = 0;
  }
  if (rc != TST_OK) return rc;
  for (int k = 1; alpha_out && k <= n_steps; ++k) alpha_out[k - 1] = tsthost::ig_alpha(k, n_steps);
  return TST_OK;
}

int tst_host_trim_tokens(const int32_t* src, const int32_t* cu_dev, const int32_t* cu_src, int n_seqs, int32_t* dst) {
  return tsthost::trim_tokens_i32(src, cu_dev, cu_src, n_seqs, dst);
}

}  // extern "C"
