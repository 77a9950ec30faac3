// Self-test of host_logic.h, built by g++ with -fsanitize=address,undefined (tests/test_host_sanitized.py builds and runs it on the CPU box; GPU
// AddressSanitizer is not available on the pool, and this is exactly the code that walks caller-provided buffers). Exit code 0 = every check held and
// neither sanitizer reported. Every buffer handed to plan_batch is heap-allocated at its EXACT size, so an out-of-range read or write is an ASan report.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>

#include "host_logic.h"

using namespace tsthost;

static int g_fail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

struct Batch {
  std::unique_ptr<int32_t[]> ids, labels, cu, slot;
  tst_batch b;
};

// a random ragged batch; every array exactly as long as the batch says
static Batch make_batch(std::mt19937& rng, int S, int max_len, int V, int n_slots, bool with_labels) {
  Batch x;
  std::vector<int> len((size_t)S);
  int T = 0;
  for (int s = 0; s < S; ++s) { len[(size_t)s] = 1 + (int)(rng() % (unsigned)max_len); T += len[(size_t)s]; }
  x.ids.reset(new int32_t[(size_t)T]);
  x.labels.reset(new int32_t[(size_t)T]);
  x.cu.reset(new int32_t[(size_t)S + 1]);
  x.slot.reset(new int32_t[(size_t)S]);
  int o = 0;
  for (int s = 0; s < S; ++s) {
    x.cu[(size_t)s] = o;
    x.slot[(size_t)s] = (int32_t)((long)s * n_slots / S);
    const int na = 1 + (int)(rng() % 3u);
    for (int p = 0; p < len[(size_t)s]; ++p) {
      x.ids[(size_t)(o + p)] = (int32_t)(rng() % (unsigned)V);
      x.labels[(size_t)(o + p)] = (p >= len[(size_t)s] - na) ? (int32_t)(rng() % (unsigned)V) : -100;
    }
    o += len[(size_t)s];
  }
  x.cu[(size_t)S] = o;
  memset(&x.b, 0, sizeof(x.b));
  x.b.input_ids = x.ids.get(); x.b.labels = with_labels ? x.labels.get() : nullptr; x.b.cu_seqlens = x.cu.get();
  x.b.n_seqs = S; x.b.n_tokens = T; x.b.seq_slot = n_slots > 1 ? x.slot.get() : nullptr; x.b.flags = 0;
  return x;
}

static void test_plan_batch() {
  std::mt19937 rng(20251121u);
  for (int it = 0; it < 400; ++it) {
    const int ns = (it % 3 == 0) ? 1 + (int)(rng() % 4u) : 1;
    const int S = 1 + (int)(rng() % 24u), max_len = 1 + (int)(rng() % 40u), V = 50 + (int)(rng() % 1000u);
    Batch x = make_batch(rng, S, max_len, V, ns, true);
    const int T = x.b.n_tokens;
    BatchLimits lim = {T + (int)(rng() % 3u), S + (int)(rng() % 2u), 3 * S + 1, V, max_len, ns};
    const bool trim = (it & 1) != 0;
    std::unique_ptr<int[]> stage(new int[stage_ints(lim)]);
    BatchPlan plan;
    std::vector<int> row_seq;
    std::string err;
    const int rc = plan_batch(&x.b, lim, true, trim, nullptr, 0, stage.get(), plan, row_seq, err);
    CHECK(rc == TST_OK);
    if (rc != TST_OK) { fprintf(stderr, "  (%s)\n", err.c_str()); continue; }
    // reference restatement: walk the sequences independently
    const int* h_ids = stage.get();
    const int* h_pos = h_ids + lim.Tmax;
    const int* h_cu = h_pos + lim.Tmax;
    const int* h_lab = h_cu + (lim.Smax + 1);
    const int* h_tgt = h_lab + lim.Rmax;
    const int* h_ord = h_tgt + lim.Rmax;
    int o = 0, R = 0, maxlen = 0;
    for (int s = 0; s < S; ++s) {
      const int s0 = x.cu[(size_t)s], len = x.cu[(size_t)s + 1] - s0;
      const int keep = (trim && len >= 2) ? len - 1 : len;
      CHECK(h_cu[s] == o);
      for (int p = 0; p < keep; ++p) { CHECK(h_ids[o + p] == x.ids[(size_t)(s0 + p)]); CHECK(h_pos[o + p] == p); }
      for (int p = 0; p + 1 < len; ++p)
        if (x.labels[(size_t)(s0 + p + 1)] != -100) {
          CHECK(h_lab[R] == o + p && h_tgt[R] == x.labels[(size_t)(s0 + p + 1)] && row_seq[(size_t)R] == s);
          CHECK(o + p < o + keep);   // a labelled row is never the trimmed token
          ++R;
        }
      o += keep;
      if (keep > maxlen) maxlen = keep;
    }
    CHECK(h_cu[S] == o && plan.T_dev == o && plan.R == R && plan.maxlen == maxlen && plan.S == S && (int)row_seq.size() == R);
    {   // the launch order: a permutation of the sequences, lengths non-increasing, equal lengths in index order
      std::vector<int> seen((size_t)S, 0);
      for (int q = 0; q < S; ++q) {
        CHECK(h_ord[q] >= 0 && h_ord[q] < S);
        if (h_ord[q] >= 0 && h_ord[q] < S) seen[(size_t)h_ord[q]] += 1;
        if (q > 0) {
          const int la = h_cu[h_ord[q - 1] + 1] - h_cu[h_ord[q - 1]], lb = h_cu[h_ord[q] + 1] - h_cu[h_ord[q]];
          CHECK(la > lb || (la == lb && h_ord[q - 1] < h_ord[q]));
        }
      }
      for (int q = 0; q < S; ++q) CHECK(seen[(size_t)q] == 1);
    }
    // slot boundaries: non-decreasing, end at T_dev / R, and every sequence's tokens lie inside its slot's range
    for (int q = 0; q + 1 < kMaxStack; ++q) CHECK(plan.slot_t_end[q] <= plan.slot_t_end[q + 1] && plan.slot_r0[q] <= plan.slot_r0[q + 1]);
    CHECK(plan.slot_t_end[kMaxStack - 1] == o && plan.slot_r0[kMaxStack] == R);
    if (ns > 1)
      for (int s = 0; s < S; ++s) {
        const int sl = x.slot[(size_t)s], lo = sl ? plan.slot_t_end[sl - 1] : 0;
        CHECK(h_cu[s] >= lo && h_cu[s + 1] <= plan.slot_t_end[sl]);
      }
  }
  // refusals: each must come back as TST_EINVAL with a message, never as a read beyond a buffer
  std::mt19937 r2(7u);
  Batch x = make_batch(r2, 6, 20, 300, 1, true);
  const int T = x.b.n_tokens;
  BatchLimits lim = {T, 6, 64, 300, 20, 1};
  std::unique_ptr<int[]> stage(new int[stage_ints(lim)]);
  BatchPlan plan;
  std::vector<int> rs;
  std::string err;
  auto refused = [&](const tst_batch& b, const BatchLimits& l, const int32_t* rows = nullptr, int n_rows = 0) {
    err.clear();
    const int rc = plan_batch(&b, l, rows == nullptr, true, rows, n_rows, stage.get(), plan, rs, err);
    return rc == TST_EINVAL && !err.empty();
  };
  { tst_batch b = x.b; b.n_tokens = T + 1; CHECK(refused(b, lim)); }                                        // exceeds max_tokens
  { BatchLimits l = lim; l.Tmax = T + 8; std::unique_ptr<int[]> st2(new int[stage_ints(l)]); tst_batch b = x.b; b.n_tokens = T + 1;
    err.clear(); CHECK(plan_batch(&b, l, true, true, nullptr, 0, st2.get(), plan, rs, err) == TST_EINVAL); }  // cu_seqlens does not end at n_tokens
  { BatchLimits l = lim; l.max_position = 4 * T;   // (long sequences allowed: only the offset check stands between this batch and a read past input_ids)
    const int32_t keep = x.cu[3]; x.cu[3] = T + 5; CHECK(refused(x.b, l)); x.cu[3] = keep; }                // a middle offset beyond n_tokens: refused BEFORE any id is read
  { const int32_t keep = x.cu[2]; x.cu[2] = x.cu[1] - 1 < 0 ? 0 : x.cu[1]; CHECK(refused(x.b, lim)); x.cu[2] = keep; }   // empty / decreasing sequence
  { const int32_t keep = x.ids[5]; x.ids[5] = 300; CHECK(refused(x.b, lim)); x.ids[5] = -1; CHECK(refused(x.b, lim)); x.ids[5] = keep; }   // id out of vocabulary
  { BatchLimits l = lim; l.Rmax = 2; CHECK(refused(x.b, l)); }                                               // more labelled tokens than max_labelled
  { BatchLimits l = lim; l.max_position = 3; CHECK(refused(x.b, l)); }                                       // sequence longer than max_position
  { tst_batch b = x.b; b.labels = nullptr; CHECK(refused(b, lim)); }                                         // labels required
  { int32_t rows[2] = {0, T}; CHECK(refused(x.b, lim, rows, 2)); }                                           // row index out of range
  { std::unique_ptr<int32_t[]> sl(new int32_t[6]{0, 1, 0, 1, 1, 1}); tst_batch b = x.b; b.seq_slot = sl.get(); BatchLimits l = lim; l.ns = 2; CHECK(refused(b, l)); }   // slots not grouped
  { int32_t rows[3] = {0, T - 1, 3}; err.clear(); CHECK(plan_batch(&x.b, lim, false, true, rows, 3, stage.get(), plan, rs, err) == TST_OK && plan.R == 3 && plan.T_dev == T); }
  // device ids: the pointer must never be dereferenced (hand over a poisoned address)
  { tst_batch b = x.b; b.input_ids = (const int32_t*)(uintptr_t)0x10; b.flags = TST_BATCH_DEVICE_IDS; err.clear();
    CHECK(plan_batch(&b, lim, true, true, nullptr, 0, stage.get(), plan, rs, err) == TST_OK);
    CHECK(stage[0] == 0 && plan.T_dev == T - 6); }                                                            // source indices of the kept tokens
}

static void test_zero_and_layout() {
  for (int64_t n : {1LL, 63LL, 64LL, 65LL, 191LL, 100000LL, 8030261248LL})
    for (int R : {1, 2, 3, 5, 8, 64}) {
      int64_t covered = 0, prev_hi = 0;
      for (int r = 0; r < R; ++r) {
        const ZeroShard z = zero_shard(n, R, r);
        CHECK(z.n_pad % (64LL * R) == 0 && z.n_pad >= n && z.n_pad - n < 64LL * R && z.shard * R == z.n_pad);
        CHECK(z.lo == (int64_t)r * z.shard && z.hi >= z.lo && z.hi <= (n > z.lo ? n : z.lo) && z.hi - z.lo <= z.shard && z.hi <= z.n_pad);
        CHECK(z.lo >= prev_hi || z.hi == z.lo);
        covered += z.hi - z.lo;
        prev_hi = z.hi > prev_hi ? z.hi : prev_hi;
        for (int64_t nd : {(int64_t)0, n / 3, n}) {
          const DecaySplit s = decay_split(z.lo, z.hi, nd);
          const int64_t dec = s.d_hi > z.lo ? s.d_hi - z.lo : 0, nod = z.hi > s.n_lo ? z.hi - s.n_lo : 0;
          CHECK(dec + nod == z.hi - z.lo);   // the two groups tile the shard
        }
      }
      CHECK(covered == n);   // the shards tile the vector
    }
  // layouts: Llama-3-8B (8,030,261,248 parameters), Qwen2.5-7B (7,615,616,512), GPT-2-small (124,439,808), tiny shapes
  auto cfg = [](int arch, int V, int d, int L, int H, int Hkv, int dh, int F, int pos) {
    tst_model_cfg c;
    memset(&c, 0, sizeof(c));
    c.arch = arch; c.vocab_size = V; c.hidden_size = d; c.num_layers = L; c.num_heads = H; c.num_kv_heads = Hkv; c.head_dim = dh; c.intermediate_size = F; c.max_position = pos;
    return c;
  };
  const FullLayout l3 = full_layout(model_dims(cfg(TST_ARCH_LLAMA, 128256, 4096, 32, 32, 8, 128, 14336, 128)));
  CHECK(l3.n_train == 8030261248LL);
  const FullLayout q7 = full_layout(model_dims(cfg(TST_ARCH_QWEN2, 152064, 3584, 28, 28, 4, 128, 18944, 128)));
  CHECK(q7.n_train == 7615616512LL);
  const tst_model_cfg g2 = cfg(TST_ARCH_GPT2, 50257, 768, 12, 12, 12, 64, 3072, 1024);
  const FullLayout gl = full_layout(model_dims(g2));
  CHECK(gl.n_train == 124439808LL + (50304LL - 50257LL) * 768);   // the vocabulary is padded to a multiple of 64 with zero rows
  // Qwen3-8B (8,190,735,360): no q/k/v bias, two [128] head-norm vectors per layer in the no-decay tail
  const FullLayout q3 = full_layout(model_dims(cfg(TST_ARCH_QWEN3, 151936, 4096, 36, 32, 8, 128, 12288, 128)));
  CHECK(q3.n_train == 8190735360LL);
  CHECK(q3.n_train - q3.n_decay == (2LL * 36 + 1) * 4096 + 36LL * 2 * 128);
  // Qwen3-0.6B's widths: num_heads * head_dim (2048) != hidden_size (1024)
  const FullLayout q06 = full_layout(model_dims(cfg(TST_ARCH_QWEN3, 151936, 1024, 28, 16, 8, 128, 3072, 128)));
  CHECK(q06.per_layer == (2048LL + 2 * 1024) * 1024 + 1024LL * 2048 + 3LL * 3072 * 1024);
  for (const FullLayout* f : {&l3, &q7, &gl, &q3, &q06}) {
    // the regions tile [0, n_train) exactly once
    std::vector<std::pair<int64_t, int64_t>> r = f->regions;
    std::sort(r.begin(), r.end());
    int64_t at = 0;
    for (auto& x : r) { CHECK(x.first == at && x.second > 0); at += x.second; }
    CHECK(at == f->n_train && f->tail >= f->n_decay - 0 && f->n_decay <= f->n_train && f->tail == f->n_decay);
  }
  // RoPE: default = theta^(-2i/dh); linear divides by the factor; llama3 leaves the short wavelengths alone and divides the long ones
  tst_model_cfg c = cfg(TST_ARCH_LLAMA, 1000, 256, 2, 2, 1, 128, 512, 256);
  c.rope_theta = 500000.0f;
  for (int i = 0; i < 64; ++i) CHECK(fabsf(rope_inv_freq(c, i, 128) - 1.0f / powf(500000.0f, (float)(2 * i) / 128.0f)) <= 1e-12f);
  tst_model_cfg cl = c; cl.rope_scaling = TST_ROPE_LINEAR; cl.rope_factor = 4.0f;
  for (int i = 0; i < 64; ++i) CHECK(rope_inv_freq(cl, i, 128) == rope_inv_freq(c, i, 128) / 4.0f);
  tst_model_cfg c3 = c; c3.rope_scaling = TST_ROPE_LLAMA3; c3.rope_factor = 8.0f; c3.rope_low_freq_factor = 1.0f; c3.rope_high_freq_factor = 4.0f; c3.rope_original_max_position = 8192;
  CHECK(rope_inv_freq(c3, 0, 128) == rope_inv_freq(c, 0, 128));
  CHECK(rope_inv_freq(c3, 63, 128) == rope_inv_freq(c, 63, 128) / 8.0f);
  for (int i = 1; i < 64; ++i) CHECK(rope_inv_freq(c3, i, 128) <= rope_inv_freq(c3, i - 1, 128));
}

// plan_generate: the cache row map is injective, inside the cache, in prompt order with room behind every prompt; decode rows continue each prompt;
// every refusal of include/tst_hip.h is refused. Random ragged prompt batches, arrays at their exact sizes.
static void test_plan_generate() {
  std::mt19937 rng(31u);
  for (int it = 0; it < 300; ++it) {
    const int ns = (it % 3 == 0) ? 1 + (int)(rng() % 4u) : 1;
    const int S = ns + (int)(rng() % 12u), max_len = 1 + (int)(rng() % 40u), V = 50, max_new = 1 + (int)(rng() % 9u);
    Batch x = make_batch(rng, S, max_len, V, ns, false);
    x.b.input_ids = (const int32_t*)(uintptr_t)16;   // never dereferenced: the ids may live on the device
    const BatchLimits lim = {x.b.n_tokens + (int)(rng() % 3u), S + (int)(rng() % 3u), S, V, max_len + max_new, ns};
    const int32_t eos[2] = {0, V - 1};
    GenPlan g;
    std::string err;
    CHECK(plan_generate(&x.b, lim, max_new, eos, 2, g, err) == TST_OK);
    const long cap = gen_cache_rows(lim, max_new);
    CHECK(g.S == S && g.T == x.b.n_tokens && g.rows_used <= cap && g.rows_used == (long)x.b.n_tokens + (long)S * max_new);
    CHECK((int)g.meta.size() == 3 + 2 * S && g.meta[0] == S && g.meta[1] == max_new && (int)g.decode_rows.size() == (max_new - 1) * S);
    CHECK(gen_dev_ints(lim, max_new) >= (size_t)(3 + 2 * lim.Smax) + (size_t)lim.Tmax + g.decode_rows.size());
    std::vector<char> seen((size_t)cap, 0);
    for (int s = 0; s < S; ++s) {
      const int s0 = x.cu[(size_t)s], len = x.cu[(size_t)s + 1] - s0;
      CHECK(g.meta[(size_t)2 + s] == s0 && g.meta[(size_t)3 + S + s] == len && g.last_rows[(size_t)s] == s0 + len - 1);
      for (int p = 0; p < len + max_new - 1; ++p) {
        const int row = p < len ? g.prefill_rows[(size_t)s0 + p] : g.decode_rows[(size_t)(p - len) * S + s];
        CHECK(row == s0 + s * max_new + p && row >= 0 && row < g.rows_used);
        if (row >= 0 && row < cap) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; }
      }
    }
    CHECK(g.meta[(size_t)2 + S] == x.b.n_tokens);
    for (int q = 0; q < kMaxStack; ++q) {
      int want = 0;
      for (int s = 0; s < S; ++s) want += (ns > 1 ? x.slot[(size_t)s] : 0) <= q;
      CHECK(g.slot_s_end[q] == want);
    }
    // refusals
    GenPlan r;
    CHECK(plan_generate(&x.b, lim, 0, eos, 2, r, err) == TST_EINVAL && err.find("max_new_tokens") != std::string::npos);
    CHECK(plan_generate(&x.b, lim, kGenMaxNew + 1, eos, 2, r, err) == TST_EINVAL && err.find("max_new_tokens") != std::string::npos);
    const int32_t bad_eos[1] = {V};
    CHECK(plan_generate(&x.b, lim, max_new, bad_eos, 1, r, err) == TST_EINVAL && err.find("eos id") != std::string::npos);
    int32_t many[kGenMaxEos + 1] = {0};
    CHECK(plan_generate(&x.b, lim, max_new, many, kGenMaxEos + 1, r, err) == TST_EINVAL && err.find("16 eos") != std::string::npos);
    CHECK(plan_generate(&x.b, lim, max_new, many, kGenMaxEos, r, err) == TST_OK);
    BatchLimits few = lim; few.Rmax = S - 1;
    CHECK(plan_generate(&x.b, few, max_new, nullptr, 0, r, err) == TST_EINVAL && err.find("max_labelled") != std::string::npos);
    int longest = 0;
    for (int s = 0; s < S; ++s) longest = std::max(longest, x.cu[(size_t)s + 1] - x.cu[(size_t)s]);
    BatchLimits shortpos = lim; shortpos.max_position = longest + max_new - 1;
    CHECK(plan_generate(&x.b, shortpos, max_new, nullptr, 0, r, err) == TST_EINVAL && err.find("max_position") != std::string::npos);
    shortpos.max_position = longest + max_new;
    CHECK(plan_generate(&x.b, shortpos, max_new, nullptr, 0, r, err) == TST_OK);
    CHECK(plan_generate(nullptr, lim, max_new, nullptr, 0, r, err) == TST_EINVAL);
  }
  // the fetch side: rows cut behind the first eos token
  int32_t tok[3 * 4] = {5, 6, 7, 8, 9, 2, 9, 2, 1, 1, 1, 3};
  float lp[3 * 4];
  for (float& v : lp) v = -1.0f;
  int32_t n_new[3];
  const int32_t eos[2] = {2, 3};
  cut_at_eos(tok, lp, n_new, 3, 4, eos, 2);
  CHECK(n_new[0] == 4 && n_new[1] == 2 && n_new[2] == 4);
  CHECK(tok[3] == 8 && tok[4] == 9 && tok[5] == 2 && tok[6] == -1 && tok[7] == -1 && lp[5] == -1.0f && lp[6] == 0.0f && lp[7] == 0.0f && tok[11] == 3 && lp[11] == -1.0f);
  cut_at_eos(tok, nullptr, n_new, 3, 4, nullptr, 0);
  CHECK(n_new[1] == 4);
}

// plan_sample: prompts at rows 0 .. T, one tail of max_new rows per decode row behind them -- inside the cache, no tail overlapping another or a prompt; the
// device image inside what gen_reserve allocates; slot boundaries times n_samples; every refusal. Random ragged prompt batches, arrays at their exact sizes.
static void test_plan_sample() {
  std::mt19937 rng(47u);
  for (int it = 0; it < 300; ++it) {
    const int ns = (it % 3 == 0) ? 1 + (int)(rng() % 4u) : 1;
    const int S = ns + (int)(rng() % 6u), max_len = 1 + (int)(rng() % 40u), V = 50, max_new = 1 + (int)(rng() % 9u), n = 1 + (int)(rng() % 8u);
    Batch x = make_batch(rng, S, max_len, V, ns, false);
    x.b.input_ids = (const int32_t*)(uintptr_t)16;   // never dereferenced
    const int R = S * n;
    const BatchLimits lim = {std::max(x.b.n_tokens, R) + (int)(rng() % 3u), R + (int)(rng() % 3u), R, V, max_len + max_new, ns};
    const int32_t eos[2] = {0, V - 1};
    std::vector<uint64_t> seeds((size_t)S);
    for (auto& v : seeds) v = ((uint64_t)rng() << 32) | rng();
    SamplePlan g;
    std::string err;
    CHECK(plan_sample(&x.b, lim, max_new, n, 1.0f, seeds.data(), eos, 2, g, err) == TST_OK);
    const long cap = gen_cache_rows(lim, max_new);
    const int T = x.b.n_tokens;
    CHECK(g.S == S && g.T == T && g.R == R && R <= lim.Tmax && g.rows_used <= cap && g.rows_used == (long)T + (long)R * max_new);
    CHECK((int)g.geo.size() == 3 + 3 * R && g.geo[0] == R && g.geo[1] == max_new && g.geo[2] == n && (int)g.decode_rows.size() == (max_new - 1) * R);
    CHECK((int)g.seeds.size() == 2 * S && (int)g.prefill_rows.size() == T && (int)g.last_rows.size() == S);
    // the image fits what the context allocates, every part at its offset
    CHECK(sample_dev_ints(lim, max_new) == gen_dev_ints(lim, max_new));
    CHECK(g.geo.size() <= sample_off_prefill(lim));
    CHECK(sample_off_prefill(lim) + g.prefill_rows.size() <= sample_off_decode(lim) && sample_off_decode(lim) + g.decode_rows.size() <= sample_dev_ints(lim, max_new));
    std::vector<char> seen((size_t)cap, 0);
    for (int t = 0; t < T; ++t) {
      const int row = g.prefill_rows[(size_t)t];
      CHECK(row == t);
      if (row >= 0 && row < cap) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; }
    }
    for (int s = 0; s < S; ++s) {
      const int s0 = x.cu[(size_t)s], len = x.cu[(size_t)s + 1] - s0;
      CHECK(g.last_rows[(size_t)s] == s0 + len - 1);
      CHECK((uint32_t)g.seeds[2 * (size_t)s] == (uint32_t)seeds[(size_t)s] && (uint32_t)g.seeds[2 * (size_t)s + 1] == (uint32_t)(seeds[(size_t)s] >> 32));
      for (int i = 0; i < n; ++i) {
        const int r = s * n + i;
        const int pre0 = g.geo[3 + 3 * (size_t)r], tail0 = g.geo[5 + 3 * (size_t)r];
        CHECK(pre0 == s0 && g.geo[4 + 3 * (size_t)r] == len && tail0 == T + r * max_new && (long)tail0 + max_new <= g.rows_used);
        for (int j = 0; j < max_new; ++j) {   // the whole tail is the row's own (its last row is reserved, never written: max_new - 1 appends)
          const int row = tail0 + j;
          if (j + 1 < max_new) CHECK(g.decode_rows[(size_t)j * R + r] == row);
          if (row >= 0 && row < cap) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; }
        }
      }
    }
    for (int q = 0; q < kMaxStack; ++q) {
      int want = 0;
      for (int s = 0; s < S; ++s) want += (ns > 1 ? x.slot[(size_t)s] : 0) <= q;
      CHECK(g.slot_r_end[q] == want * n);
    }
    // refusals: plan_generate's own, then what sampling adds
    SamplePlan r;
    CHECK(plan_sample(&x.b, lim, 0, n, 1.0f, seeds.data(), eos, 2, r, err) == TST_EINVAL && err.find("max_new_tokens") != std::string::npos);
    const int32_t bad_eos[1] = {V};
    CHECK(plan_sample(&x.b, lim, max_new, n, 1.0f, seeds.data(), bad_eos, 1, r, err) == TST_EINVAL && err.find("eos id") != std::string::npos);
    BatchLimits shortpos = lim; shortpos.max_position = 1;
    CHECK(plan_sample(&x.b, shortpos, max_new, n, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("max_position") != std::string::npos);
    CHECK(plan_sample(nullptr, lim, max_new, n, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL);
    CHECK(plan_sample(&x.b, lim, max_new, 0, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("n_samples") != std::string::npos);
    CHECK(plan_sample(&x.b, lim, max_new, kSampleMaxN + 1, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("n_samples") != std::string::npos);
    BatchLimits few = lim; few.Rmax = R - 1;
    if (few.Rmax >= S) CHECK(plan_sample(&x.b, few, max_new, n, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("n_seqs * n_samples") != std::string::npos);
    few = lim; few.Smax = R - 1;
    if (few.Smax >= S) CHECK(plan_sample(&x.b, few, max_new, n, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("n_seqs * n_samples") != std::string::npos);
    few = lim; few.Tmax = R - 1;   // rows fit max_seqs and max_labelled, not max_tokens (possible where the prompts are shorter than n_samples tokens)
    if (few.Tmax >= x.b.n_tokens) CHECK(plan_sample(&x.b, few, max_new, n, 1.0f, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("exceeds max_tokens") != std::string::npos);
    for (float bad : {0.0f, 0.009f, 100.5f, -1.0f, (float)INFINITY, (float)NAN})
      CHECK(plan_sample(&x.b, lim, max_new, n, bad, seeds.data(), nullptr, 0, r, err) == TST_EINVAL && err.find("temperature") != std::string::npos);
    CHECK(plan_sample(&x.b, lim, max_new, n, 0.01f, seeds.data(), nullptr, 0, r, err) == TST_OK);
    CHECK(plan_sample(&x.b, lim, max_new, n, 100.0f, seeds.data(), nullptr, 0, r, err) == TST_OK);
    CHECK(plan_sample(&x.b, lim, max_new, n, 1.0f, nullptr, nullptr, 0, r, err) == TST_EINVAL && err.find("seq_seeds") != std::string::npos);
  }
}

// plan_candidates: prompts at rows 0 .. T, the candidates' tails packed behind them in c-major order -- the row map injective and inside the cache, a one-token
// candidate taking no row; ids / positions / targets of every extend row; the {row, tok} source of every candidate token; slot boundaries; every refusal with its
// message. Random ragged prompt batches and candidate lists, arrays at their exact sizes.
static void test_plan_candidates() {
  std::mt19937 rng(53u);
  for (int it = 0; it < 300; ++it) {
    const int ns = (it % 3 == 0) ? 1 + (int)(rng() % 4u) : 1;
    const int S = ns + (int)(rng() % 6u), max_len = 1 + (int)(rng() % 40u), V = 50;
    Batch x = make_batch(rng, S, max_len, V, ns, false);
    x.b.input_ids = (const int32_t*)(uintptr_t)16;   // never dereferenced
    const int T = x.b.n_tokens;
    // 0 .. 4 candidates per prompt (at least one over all), lengths 1 .. 16 with every third one a single token
    std::vector<int32_t> cseq, ccu(1, 0), cids;
    for (int s = 0; s < S; ++s) {
      const int nc = (int)(rng() % 5u) + (s == S - 1 && cseq.empty() ? 1 : 0);
      for (int i = 0; i < nc; ++i) {
        const int L = (rng() % 3u == 0) ? 1 : 1 + (int)(rng() % (unsigned)kCandMaxLen);
        for (int p = 0; p < L; ++p) cids.push_back((int32_t)(rng() % (unsigned)V));
        ccu.push_back((int32_t)cids.size());
        cseq.push_back(s);
      }
    }
    const int NC = (int)cseq.size(), N = (int)cids.size(), R = N - NC;
    std::unique_ptr<int32_t[]> e_ids(new int32_t[(size_t)N]), e_cu(new int32_t[(size_t)NC + 1]), e_seq(new int32_t[(size_t)NC]);
    std::copy(cids.begin(), cids.end(), e_ids.get());
    std::copy(ccu.begin(), ccu.end(), e_cu.get());
    std::copy(cseq.begin(), cseq.end(), e_seq.get());
    const int big = std::max(std::max(T, S), std::max(R, 1));
    const BatchLimits lim = {big + (int)(rng() % 3u), big + (int)(rng() % 3u), std::max(N, S), V, max_len + kCandMaxLen - 1, ns};
    CandPlan g;
    std::string err;
    CHECK(plan_candidates(&x.b, lim, e_ids.get(), e_cu.get(), e_seq.get(), NC, g, err) == TST_OK);
    const long cap = gen_cache_rows(lim, 1);
    CHECK(g.S == S && g.T == T && g.n_cands == NC && g.n_tok == N && g.R_e == R && g.rows_used == (long)T + R && g.rows_used <= cap);
    CHECK((int)g.ext_rows.size() == R && (int)g.ext_ids.size() == R && (int)g.ext_pos.size() == R && (int)g.ext_tgt.size() == R && (int)g.src.size() == 2 * N);
    CHECK((int)g.geo.size() == 5 * g.n_ext && (int)g.last_rows.size() == S && (int)g.prefill_rows.size() == T);
    // the image fits what the context allocates, every part at its offset
    CHECK(g.geo.size() <= cand_off_rows(lim) && cand_off_rows(lim) + g.ext_rows.size() <= cand_off_src(lim) && cand_off_src(lim) + g.src.size() <= cand_dev_ints(lim));
    std::vector<char> seen((size_t)cap, 0);
    for (int t = 0; t < T; ++t) {
      CHECK(g.prefill_rows[(size_t)t] == t);
      seen[(size_t)t] = 1;
    }
    int r = 0, e = 0;
    for (int c = 0; c < NC; ++c) {
      const int c0 = ccu[(size_t)c], L = ccu[(size_t)c + 1] - c0, s = cseq[(size_t)c];
      const int s0 = x.cu[(size_t)s], len = x.cu[(size_t)s + 1] - s0;
      CHECK(g.src[2 * (size_t)c0] == s && g.src[2 * (size_t)c0 + 1] == cids[(size_t)c0]);
      if (L >= 2) {
        const int* q = g.geo.data() + 5 * (size_t)e++;
        CHECK(q[0] == s0 && q[1] == len && q[2] == T + r && q[3] == r && q[4] == L - 1);   // tails packed in c-major order: the tail starts where the last one ended
      }
      for (int p = 0; p + 1 < L; ++p, ++r) {
        const int row = g.ext_rows[(size_t)r];
        CHECK(row == T + (c0 - c) + p && row == T + r && row >= T && row < cap);
        if (row >= 0 && row < cap) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; }
        CHECK(g.ext_ids[(size_t)r] == cids[(size_t)c0 + p] && g.ext_pos[(size_t)r] == len + p && g.ext_tgt[(size_t)r] == cids[(size_t)c0 + p + 1]);
        CHECK(g.src[2 * (size_t)(c0 + p + 1)] == r && g.src[2 * (size_t)(c0 + p + 1) + 1] == -1);
      }
    }
    CHECK(r == R && e == g.n_ext);
    for (int s = 0; s < S; ++s) CHECK(g.last_rows[(size_t)s] == x.cu[(size_t)s + 1] - 1);
    for (int q = 0; q < kMaxStack; ++q) {
      int want = 0;
      for (int c = 0; c < NC; ++c)
        if ((ns > 1 ? x.slot[(size_t)cseq[(size_t)c]] : 0) <= q) want += ccu[(size_t)c + 1] - ccu[(size_t)c] - 1;
      CHECK(g.slot_r_end[q] == want);
    }
    // refusals
    CandPlan rr;
    auto refused = [&](const BatchLimits& l, const int32_t* ids, const int32_t* cu, const int32_t* seq, int n, const char* what) {
      err.clear();
      return plan_candidates(&x.b, l, ids, cu, seq, n, rr, err) == TST_EINVAL && err.find(what) != std::string::npos;
    };
    CHECK(plan_candidates(nullptr, lim, e_ids.get(), e_cu.get(), e_seq.get(), NC, rr, err) == TST_EINVAL);
    CHECK(refused(lim, e_ids.get(), e_cu.get(), e_seq.get(), 0, "n_cands"));
    CHECK(refused(lim, nullptr, e_cu.get(), e_seq.get(), NC, "null candidate"));
    { std::vector<int32_t> cu2(ccu); cu2[0] = 1; CHECK(refused(lim, e_ids.get(), cu2.data(), e_seq.get(), NC, "cu_cand")); }
    { std::vector<int32_t> cu2(ccu); cu2[(size_t)NC] = cu2[(size_t)NC - 1]; CHECK(refused(lim, e_ids.get(), cu2.data(), e_seq.get(), NC, "cu_cand")); }
    {
      // one candidate of 17 tokens
      std::vector<int32_t> ids2((size_t)kCandMaxLen + 1, 1);
      const int32_t cu2[2] = {0, kCandMaxLen + 1}, seq2[1] = {0};
      BatchLimits roomy = lim; roomy.Tmax = roomy.Smax = roomy.Rmax = std::max(big, 64); roomy.max_position = max_len + 64;
      CHECK(refused(roomy, ids2.data(), cu2, seq2, 1, "TST_CAND_MAX_LEN"));
      const int32_t cu3[2] = {0, kCandMaxLen};
      err.clear();
      CHECK(plan_candidates(&x.b, roomy, ids2.data(), cu3, seq2, 1, rr, err) == TST_OK);
    }
    { std::vector<int32_t> ids2(cids); ids2[(size_t)N - 1] = V; CHECK(refused(lim, ids2.data(), e_cu.get(), e_seq.get(), NC, "candidate id")); }
    { std::vector<int32_t> ids2(cids); ids2[0] = -1; CHECK(refused(lim, ids2.data(), e_cu.get(), e_seq.get(), NC, "candidate id")); }
    { std::vector<int32_t> seq2(cseq); seq2[(size_t)NC - 1] = S; CHECK(refused(lim, e_ids.get(), e_cu.get(), seq2.data(), NC, "cand_seq out of range")); }
    { std::vector<int32_t> seq2(cseq); seq2[0] = -1; CHECK(refused(lim, e_ids.get(), e_cu.get(), seq2.data(), NC, "cand_seq out of range")); }
    if (NC >= 2 && cseq[0] != cseq[(size_t)NC - 1]) {
      std::vector<int32_t> seq2(cseq); std::swap(seq2[0], seq2[(size_t)NC - 1]);
      CHECK(refused(lim, e_ids.get(), e_cu.get(), seq2.data(), NC, "non-decreasing"));
    }
    {
      int need = 0;   // the largest len + L - 1 over the candidates
      for (int c = 0; c < NC; ++c) need = std::max(need, x.cu[(size_t)cseq[(size_t)c] + 1] - x.cu[(size_t)cseq[(size_t)c]] + ccu[(size_t)c + 1] - ccu[(size_t)c] - 1);
      int longest = 0;
      for (int s = 0; s < S; ++s) longest = std::max(longest, x.cu[(size_t)s + 1] - x.cu[(size_t)s]);
      BatchLimits shortpos = lim; shortpos.max_position = need - 1;
      if (need - 1 >= longest) CHECK(refused(shortpos, e_ids.get(), e_cu.get(), e_seq.get(), NC, "exceeds max_position"));
      shortpos.max_position = std::max(need, longest);
      err.clear();
      CHECK(plan_candidates(&x.b, shortpos, e_ids.get(), e_cu.get(), e_seq.get(), NC, rr, err) == TST_OK);
    }
    { BatchLimits few = lim; few.Rmax = N - 1; if (few.Rmax >= S) CHECK(refused(few, e_ids.get(), e_cu.get(), e_seq.get(), NC, "exceed max_labelled")); }
    if (R >= 1) {
      BatchLimits few = lim; few.Smax = R - 1;
      if (few.Smax >= S) CHECK(refused(few, e_ids.get(), e_cu.get(), e_seq.get(), NC, "extend rows"));
      few = lim; few.Tmax = R - 1;
      if (few.Tmax >= T) CHECK(refused(few, e_ids.get(), e_cu.get(), e_seq.get(), NC, "extend rows"));
    }
    { BatchLimits few = lim; few.Rmax = S - 1; CHECK(refused(few, e_ids.get(), e_cu.get(), e_seq.get(), NC, "more sequences than max_labelled")); }
  }
}

// token attribution: the row weights / kinds of plan_attribute, its refusals, and the un-trim of the fetch side
static void test_attribute() {
  // three sequences of 1, 2 and 5 tokens; labels on the last token of the second and on the last three of the third
  const int32_t cu[4] = {0, 1, 3, 8};
  const int32_t ids[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  const int32_t lab[8] = {9, -100, 7, -100, -100, 3, 4, 5};   // (a label on a sequence's first token predicts nothing: not a row)
  tst_batch b;
  memset(&b, 0, sizeof(b));
  b.input_ids = ids; b.labels = lab; b.cu_seqlens = cu; b.n_seqs = 3; b.n_tokens = 8;
  const BatchLimits lim = {16, 4, 8, 50, 16, 1};
  const int32_t opt[3] = {2, 7, 11};
  const int32_t kind[3] = {0, 1, 0};
  AttrPlan p;
  std::string err;
  CHECK(plan_attribute(&b, lim, kind, opt, 3, p, err) == TST_OK);
  CHECK(p.R == 4 && p.row_w.size() == 4 && p.row_kind.size() == 4 && p.row_seq.size() == 4);
  if (p.R == 4) {
    CHECK(p.row_seq[0] == 1 && p.row_kind[0] == 1 && p.row_w[0] == 1.0f);
    for (int r = 1; r < 4; ++r) CHECK(p.row_seq[(size_t)r] == 2 && p.row_kind[(size_t)r] == 0 && p.row_w[(size_t)r] == 1.0f / 3.0f);
    const float stats[16] = {5.f, 2.f, 3.f, 0.f, 4.f, 1.f, 0.f, 0.f, 4.f, 2.f, 0.f, 0.f, 4.f, 3.f, 0.f, 0.f};
    float logs[3] = {-1.f, -1.f, -1.f};
    attr_logs(stats, p, 3, logs);
    CHECK(logs[0] == 0.0f && logs[1] == -1.0f && fabsf(logs[2] - (-2.0f)) < 1e-6f);
  }
  CHECK(plan_attribute(&b, lim, nullptr, nullptr, 0, p, err) == TST_OK && p.R == 4 && p.row_kind[0] == 0);
  // refusals
  CHECK(plan_attribute(&b, lim, kind, opt, 0, p, err) == TST_EINVAL && err.find("n_opt == 0") != std::string::npos);
  CHECK(plan_attribute(&b, lim, kind, opt, kAttrMaxOpt + 1, p, err) == TST_EINVAL && err.find("n_opt") != std::string::npos);
  CHECK(plan_attribute(&b, lim, kind, opt, -1, p, err) == TST_EINVAL);
  const int32_t bad_opt[2] = {2, 50};
  CHECK(plan_attribute(&b, lim, kind, bad_opt, 2, p, err) == TST_EINVAL && err.find("option id") != std::string::npos);
  const int32_t miss[2] = {2, 11};
  CHECK(plan_attribute(&b, lim, kind, miss, 2, p, err) == TST_EINVAL && err.find("not one of the option ids") != std::string::npos);
  const int32_t kind3[3] = {0, 0, 1};
  CHECK(plan_attribute(&b, lim, kind3, opt, 3, p, err) == TST_EINVAL && err.find("exactly one") != std::string::npos);
  const int32_t kind0[3] = {1, 0, 0};
  CHECK(plan_attribute(&b, lim, kind0, opt, 3, p, err) == TST_EINVAL && err.find("exactly one") != std::string::npos);
  const int32_t kindx[3] = {0, 2, 0};
  CHECK(plan_attribute(&b, lim, kindx, opt, 3, p, err) == TST_EINVAL && err.find("seq_kind") != std::string::npos);
  const int32_t nolab[8] = {9, -100, -100, -100, -100, -100, -100, -100};
  tst_batch e = b;
  e.labels = nolab;
  CHECK(plan_attribute(&e, lim, nullptr, nullptr, 0, p, err) == TST_EINVAL && err.find("no labelled") != std::string::npos);
  e.labels = nullptr;
  CHECK(plan_attribute(&e, lim, nullptr, nullptr, 0, p, err) == TST_EINVAL && err.find("labels required") != std::string::npos);
  CHECK(plan_attribute(nullptr, lim, nullptr, nullptr, 0, p, err) == TST_EINVAL);
  // un-trim: lengths 1 (never trimmed), 2 and 5, trimmed and untrimmed
  const float src[6] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f};
  const int32_t cu_trim[4] = {0, 1, 2, 6};
  float dst[8];
  for (float& v : dst) v = -7.f;
  CHECK(untrim_tokens(src, cu_trim, cu, 3, dst) == TST_OK);
  const float want[8] = {1.f, 2.f, 0.f, 3.f, 4.f, 5.f, 6.f, 0.f};
  for (int t = 0; t < 8; ++t) CHECK(dst[t] == want[t]);
  const float src8[8] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
  CHECK(untrim_tokens(src8, cu, cu, 3, dst) == TST_OK);
  for (int t = 0; t < 8; ++t) CHECK(dst[t] == src8[t]);
  const int32_t cu1[2] = {0, 1}, cu2[2] = {0, 2};
  float one[2] = {-7.f, -7.f};
  CHECK(untrim_tokens(src, cu1, cu1, 1, one) == TST_OK && one[0] == 1.f && one[1] == -7.f);
  CHECK(untrim_tokens(src, cu1, cu2, 1, one) == TST_OK && one[0] == 1.f && one[1] == 0.f);
  CHECK(untrim_tokens(src, cu2, cu1, 1, one) == TST_EINVAL);   // longer on the device than in the caller's batch
  CHECK(untrim_tokens(src, cu1, cu1, 0, one) == TST_OK);
  CHECK(untrim_tokens(nullptr, cu1, cu1, 1, one) == TST_EINVAL);
}

// integrated gradients: plan_ig's refusals, the midpoints, and the baseline ids' way onto the device
static void test_ig() {
  const int32_t cu[4] = {0, 1, 3, 8};
  const int32_t ids[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  tst_batch b;
  memset(&b, 0, sizeof(b));
  b.input_ids = ids; b.cu_seqlens = cu; b.n_seqs = 3; b.n_tokens = 8;
  const BatchLimits lim = {16, 4, 8, 50, 16, 1};
  const int32_t base[8] = {1, 1, 1, 1, 1, 49, 0, 8};
  std::string err;
  CHECK(plan_ig(&b, lim, base, 1, err) == TST_OK);
  CHECK(plan_ig(&b, lim, base, kIgMaxSteps, err) == TST_OK);
  CHECK(plan_ig(&b, lim, base, 0, err) == TST_EINVAL && err.find("n_steps") != std::string::npos);
  CHECK(plan_ig(&b, lim, base, kIgMaxSteps + 1, err) == TST_EINVAL && err.find("n_steps") != std::string::npos);
  CHECK(plan_ig(&b, lim, nullptr, 4, err) == TST_EINVAL && err.find("null baseline_ids") != std::string::npos);
  CHECK(plan_ig(nullptr, lim, base, 4, err) == TST_EINVAL);
  { int32_t bad[8]; memcpy(bad, base, sizeof(bad)); bad[7] = 50; CHECK(plan_ig(&b, lim, bad, 4, err) == TST_EINVAL && err.find("baseline id") != std::string::npos);
    bad[7] = 8; bad[0] = -1; CHECK(plan_ig(&b, lim, bad, 4, err) == TST_EINVAL && err.find("baseline id") != std::string::npos); }
  { tst_batch e = b; e.n_tokens = 17; CHECK(plan_ig(&e, lim, base, 4, err) == TST_EINVAL); e.n_tokens = 0; CHECK(plan_ig(&e, lim, base, 4, err) == TST_EINVAL); }
  // (the baseline ids are read up to n_tokens and no further: an exactly sized heap array under the sanitizer)
  { std::unique_ptr<int32_t[]> hb(new int32_t[8]); memcpy(hb.get(), base, sizeof(base)); CHECK(plan_ig(&b, lim, hb.get(), 16, err) == TST_OK); }
  CHECK(ig_alpha(1, 1) == 0.5f && ig_alpha(1, 16) == 0.03125f && ig_alpha(16, 16) == 0.96875f && ig_alpha(8, 16) == 0.46875f);
  for (int m = 1; m <= kIgMaxSteps; ++m) CHECK(ig_alpha(1, m) > 0.0f && ig_alpha(m, m) < 1.0f);
  // trim: lengths 1 (never trimmed), 2 and 5
  const int32_t cu_trim[4] = {0, 1, 2, 6};
  std::unique_ptr<int32_t[]> dst(new int32_t[6]);
  CHECK(trim_tokens_i32(base, cu_trim, cu, 3, dst.get()) == TST_OK);
  const int32_t want[6] = {1, 1, 1, 1, 49, 0};
  for (int t = 0; t < 6; ++t) CHECK(dst[(size_t)t] == want[t]);
  std::unique_ptr<int32_t[]> dst8(new int32_t[8]);
  CHECK(trim_tokens_i32(base, cu, cu, 3, dst8.get()) == TST_OK);
  for (int t = 0; t < 8; ++t) CHECK(dst8[(size_t)t] == base[t]);
  // trim, then un-trim of a per-token result: the round trip of a token's value, 0 where the device did not run it
  { float f[6], back[8]; for (int t = 0; t < 6; ++t) f[t] = (float)dst[(size_t)t];
    CHECK(untrim_tokens(f, cu_trim, cu, 3, back) == TST_OK);
    for (int t = 0; t < 8; ++t) CHECK(back[t] == ((t == 2 || t == 7) ? 0.0f : (float)base[t])); }
  const int32_t cu1[2] = {0, 1}, cu2[2] = {0, 2};
  CHECK(trim_tokens_i32(base, cu2, cu1, 1, dst.get()) == TST_EINVAL);   // longer on the device than in the caller's batch
  CHECK(trim_tokens_i32(nullptr, cu1, cu1, 1, dst.get()) == TST_EINVAL);
  CHECK(trim_tokens_i32(base, cu1, cu1, 0, dst.get()) == TST_OK);
}

// one valid configuration per naming family and train mode (the tiny shapes of tests/golden_inputs.py)
static tst_model_cfg valid_cfg(int arch, int train_mode) {
  tst_model_cfg c;
  memset(&c, 0, sizeof(c));
  c.arch = arch; c.vocab_size = 256; c.hidden_size = 256; c.num_layers = 2; c.num_heads = 2; c.num_kv_heads = 1; c.head_dim = 128; c.intermediate_size = 256;
  if (arch == TST_ARCH_GPT2) { c.vocab_size = 1001; c.hidden_size = 128; c.num_kv_heads = 2; c.head_dim = 64; c.intermediate_size = 512; }
  c.rope_theta = 10000.0f; c.rms_norm_eps = 1e-5f; c.max_position = 128; c.max_tokens = 256; c.max_seqs = 8; c.max_labelled = 32;
  c.train_mode = train_mode; c.lora_r = 16; c.lora_alpha = 32.0f; c.lora_targets = TST_LORA_ALL; c.n_stack = 1; c.precision = TST_PRECISION_BF16;
  return c;
}

// check_cfg: every refusal tst_create / tst_fork make from the configuration, each on a configuration that differs from a valid one in ONE field
static void test_check_cfg() {
  std::string err;
  for (int arch : {TST_ARCH_LLAMA, TST_ARCH_QWEN2, TST_ARCH_GPT2, TST_ARCH_QWEN3})
    for (int mode : {TST_TRAIN_LORA, TST_TRAIN_FULL}) {
      tst_model_cfg c = valid_cfg(arch, mode);
      err = "stale";
      CHECK(check_cfg(c, false, err) == TST_OK);
      CHECK(check_cfg(c, mode == TST_TRAIN_LORA, err) == TST_OK);   // (a LoRA context may be forked)
      c.precision = TST_PRECISION_STRICT;
      CHECK(check_cfg(c, false, err) == TST_OK);
      if (mode == TST_TRAIN_LORA) { c.precision = TST_PRECISION_BF16; c.n_stack = kMaxStack; CHECK(check_cfg(c, false, err) == TST_OK); }
      if (mode == TST_TRAIN_FULL) { c.zero_ranks = 64; c.zero_rank = 63; CHECK(check_cfg(c, false, err) == TST_OK); }
    }
  const tst_model_cfg lora = valid_cfg(TST_ARCH_LLAMA, TST_TRAIN_LORA), full = valid_cfg(TST_ARCH_LLAMA, TST_TRAIN_FULL), gpt2 = valid_cfg(TST_ARCH_GPT2, TST_TRAIN_LORA);
  tst_model_cfg linear = lora; linear.rope_scaling = TST_ROPE_LINEAR; linear.rope_factor = 4.0f;
  tst_model_cfg l3 = lora; l3.rope_scaling = TST_ROPE_LLAMA3; l3.rope_factor = 8.0f; l3.rope_low_freq_factor = 1.0f; l3.rope_high_freq_factor = 4.0f; l3.rope_original_max_position = 64;
  tst_model_cfg r4 = lora; r4.lora_r = 4;
  tst_model_cfg strict = lora; strict.precision = TST_PRECISION_STRICT;
  CHECK(check_cfg(linear, false, err) == TST_OK && check_cfg(l3, false, err) == TST_OK && check_cfg(r4, false, err) == TST_OK);
  int n = 0;
  auto refused = [&](tst_model_cfg c, const char* msg, bool is_fork = false) {
    err.clear();
    const int rc = check_cfg(c, is_fork, err);
    if (rc != TST_EINVAL || err != msg) { fprintf(stderr, "refusal %d: rc=%d \"%s\", expected \"%s\"\n", n, rc, err.c_str(), msg); ++g_fail; }
    ++n;
  };
#define WITH(base, stmt) [&] { tst_model_cfg c = base; stmt; return c; }()
  const char* positive = "hidden_size/num_layers/num_heads/num_kv_heads/head_dim/intermediate_size/vocab_size must be > 0";
  const char* sizes = "max_tokens/max_seqs/max_labelled/max_position must be > 0";
  const char* l3msg = "llama3 rope scaling needs 0 < rope_low_freq_factor < rope_high_freq_factor and rope_original_max_position > 0";
  const char* zmsg = "zero_rank must be in [0, zero_ranks), zero_ranks <= 64";
  refused(WITH(lora, c.precision = 2), "precision must be TST_PRECISION_BF16 or TST_PRECISION_STRICT");
  refused(WITH(lora, c.arch = 4), "unsupported arch");
  refused(WITH(lora, c.arch = -1), "unsupported arch");
  // the zero-size cases: num_kv_heads = 0 was an integer division by zero, num_layers = 0 a read of layers[0]
  refused(WITH(lora, c.num_kv_heads = 0), positive);
  refused(WITH(full, c.num_layers = 0), positive);
  refused(WITH(lora, c.num_layers = 0), positive);
  refused(WITH(lora, c.hidden_size = 0), positive);
  refused(WITH(lora, c.num_heads = 0), positive);
  refused(WITH(lora, c.head_dim = 0), positive);
  refused(WITH(lora, c.intermediate_size = 0), positive);
  refused(WITH(lora, c.vocab_size = 0), positive);
  refused(WITH(full, c.num_kv_heads = -1), positive);
  refused(WITH(gpt2, c.vocab_size = -64), positive);
  refused(WITH(gpt2, c.num_kv_heads = 1), "GPT-2: num_kv_heads must equal num_heads");
  refused(WITH(gpt2, c.hidden_size = 192), "GPT-2: num_heads * head_dim must equal hidden_size");
  refused(WITH(lora, c.train_mode = 2), "train_mode must be TST_TRAIN_LORA or TST_TRAIN_FULL");
  refused(full, "full fine-tune contexts cannot be forked (every fold owns its weights)", true);
  refused(WITH(lora, c.head_dim = 64), "head_dim must be 128 (GPT-2 family: 64 or 128)");
  refused(WITH(gpt2, c.head_dim = 32), "GPT-2: num_heads * head_dim must equal hidden_size");
  refused(WITH(lora, c.hidden_size = 200), "hidden/intermediate/head sizes must be multiples of 64");
  refused(WITH(lora, c.intermediate_size = 257), "hidden/intermediate/head sizes must be multiples of 64");
  refused(WITH(lora, c.num_kv_heads = 3), "num_heads must be a multiple of num_kv_heads");
  refused(WITH(lora, c.max_tokens = 0), sizes);
  refused(WITH(lora, c.max_seqs = 0), sizes);
  refused(WITH(lora, c.max_labelled = -1), sizes);
  refused(WITH(lora, c.max_position = 0), sizes);
  refused(WITH(lora, c.lora_r = 0), "lora_r must divide 64");
  refused(WITH(lora, c.lora_r = 24), "lora_r must divide 64");
  refused(WITH(lora, c.lora_r = 128), "lora_r must divide 64");
  refused(WITH(lora, c.rope_scaling = 3), "rope_scaling must be TST_ROPE_DEFAULT, TST_ROPE_LINEAR or TST_ROPE_LLAMA3");
  refused(WITH(linear, c.rope_factor = 0.0f), "rope_factor must be > 0");
  refused(WITH(l3, c.rope_low_freq_factor = 0.0f), l3msg);
  refused(WITH(l3, c.rope_high_freq_factor = 1.0f), l3msg);
  refused(WITH(l3, c.rope_original_max_position = 0), l3msg);
  refused(WITH(lora, c.n_stack = 9), "n_stack must be <= 8");
  refused(WITH(full, c.n_stack = 2), "stacked folds need frozen base weights (LoRA): a full fine-tune owns its weights");
  refused(WITH(r4, c.n_stack = 2), "stacked folds: lora_r must be a multiple of 8");
  refused(WITH(strict, c.n_stack = 2), "stacked folds are a bf16-path feature: precision = strict runs one fold per context");
  refused(WITH(lora, c.zero_ranks = 1), "optimizer-state sharding (zero_ranks >= 1) is for full fine-tunes: LoRA state is 0.2 % of the model");
  refused(WITH(full, c.zero_ranks = 65), zmsg);
  refused(WITH(WITH(full, c.zero_ranks = 2), c.zero_rank = 2), zmsg);
  refused(WITH(WITH(full, c.zero_ranks = 2), c.zero_rank = -1), zmsg);
  refused(WITH(lora, c.lora_targets = 0), "no trainable parameters (lora_targets empty)");
  refused(WITH(lora, c.lora_targets = 128u), "no trainable parameters (lora_targets empty)");
  refused(WITH(gpt2, c.lora_targets = 0), "no trainable parameters (lora_targets empty)");
  // several faults: the first in the engine's order is the one reported
  refused(WITH(WITH(lora, c.precision = 9), c.arch = 9), "precision must be TST_PRECISION_BF16 or TST_PRECISION_STRICT");
  refused(WITH(WITH(lora, c.head_dim = 0), c.train_mode = 9), positive);
  refused(WITH(WITH(lora, c.lora_targets = 0), c.n_stack = 9), "n_stack must be <= 8");
  // a GPT-2 context has no RoPE: its scaling fields are not looked at; a full fine-tune has no rank or targets
  CHECK(check_cfg(WITH(gpt2, c.rope_scaling = 3), false, err) == TST_OK);
  CHECK(check_cfg(WITH(WITH(full, c.lora_r = 0), c.lora_targets = 0), false, err) == TST_OK);
#undef WITH
}

// lora_layout: slot 0's table is contiguous, in (layer, group, module) order, n1 = the sum of r (din + rows) over the enabled modules; every single target
// bit, the full mask, and GPT-2's mapping of the seven bits onto its four Conv1D modules
static void test_lora_layout() {
  struct Mod { const char* name; unsigned bits; int din, rows; };
  for (int arch : {TST_ARCH_LLAMA, TST_ARCH_QWEN3, TST_ARCH_GPT2}) {
    tst_model_cfg c = valid_cfg(arch, TST_TRAIN_LORA);
    if (arch == TST_ARCH_QWEN3) { c.num_heads = 4; c.num_kv_heads = 2; c.num_layers = 3; c.intermediate_size = 384; }   // num_heads * head_dim != hidden_size
    const int d = c.hidden_size, F = c.intermediate_size, dq = c.num_heads * c.head_dim, dkv = c.num_kv_heads * c.head_dim;
    const std::vector<Mod> mods = arch == TST_ARCH_GPT2
        ? std::vector<Mod>{{"attn.c_attn", TST_LORA_Q | TST_LORA_K | TST_LORA_V, d, 3 * d}, {"attn.c_proj", TST_LORA_O, d, d}, {"mlp.c_fc", TST_LORA_GATE | TST_LORA_UP, d, F}, {"mlp.c_proj", TST_LORA_DOWN, F, d}}
        : std::vector<Mod>{{"q_proj", TST_LORA_Q, d, dq}, {"k_proj", TST_LORA_K, d, dkv}, {"v_proj", TST_LORA_V, d, dkv}, {"o_proj", TST_LORA_O, dq, d},
                           {"gate_proj", TST_LORA_GATE, d, F}, {"up_proj", TST_LORA_UP, d, F}, {"down_proj", TST_LORA_DOWN, F, d}};
    std::vector<unsigned> masks = {TST_LORA_ALL, TST_LORA_Q | TST_LORA_V, TST_LORA_K | TST_LORA_UP | TST_LORA_DOWN, 0u};
    for (unsigned b = 1; b <= TST_LORA_DOWN; b <<= 1) masks.push_back(b);
    for (unsigned mask : masks)
      for (int r : {8, 16})
        for (int ns : {1, 3}) {
          const LoraLayout lay = lora_layout(model_dims(c), r, mask, ns);
          int64_t at = 0;
          size_t e = 0;
          for (int l = 0; l < c.num_layers; ++l)
            for (const Mod& m : mods) {
              if (!(mask & m.bits)) continue;
              CHECK(e + 2 <= lay.entries.size());
              if (e + 2 > lay.entries.size()) return;
              const TrainableEntry &A = lay.entries[e], &B = lay.entries[e + 1];
              const std::string pre = "layers." + std::to_string(l) + "." + m.name;
              CHECK(A.name == pre + ".lora_A" && A.offset == at && A.rows == r && A.cols == m.din);
              at += (int64_t)r * m.din;
              CHECK(B.name == pre + ".lora_B" && B.offset == at && B.rows == m.rows && B.cols == r);
              at += (int64_t)m.rows * r;
              e += 2;
            }
          CHECK(e == lay.entries.size() && lay.n1 == at && lay.n_train == at * ns && (int)lay.group.size() == 4 * c.num_layers);
          // the groups: their segments tile the enabled modules' rows in order, and point at the same offsets as the entries
          int dout[4], din[4];
          proj_dims(model_dims(c), dout, din);
          size_t seen = 0;
          for (size_t g = 0; g < lay.group.size(); ++g) {
            const LoraGroupLayout& G = lay.group[g];
            CHECK(G.nseg >= 0 && G.nseg <= 3);
            for (int q = 0; q < G.nseg; ++q, seen += 2) {
              CHECK(G.row0[q] >= 0 && G.row0[q] < G.row1[q] && G.row1[q] <= dout[g % 4] && (q == 0 || G.row0[q] >= G.row1[q - 1]));
              CHECK(G.a_off[q] == lay.entries[seen].offset && G.b_off[q] == lay.entries[seen + 1].offset);
              CHECK(lay.entries[seen].cols == din[g % 4] && lay.entries[seen + 1].rows == G.row1[q] - G.row0[q]);
            }
          }
          CHECK(seen == lay.entries.size());
        }
  }
}

int main() {
  test_plan_generate();
  test_plan_sample();
  test_plan_candidates();
  test_attribute();
  test_ig();
  test_plan_batch();
  test_zero_and_layout();
  test_check_cfg();
  test_lora_layout();
  if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
  printf("host_selftest: ok\n");
  return 0;
}
