// Host-side engine behind the C-ABI (include/tst_hip.h): owns device memory, schedules the hand-written
// kernels of one train / score step on one HIP stream. No autograd, no tracing: the backward pass is
// scheduled explicitly in the reverse order of the forward (SURVEY.md §3 stack (2)).
//
// HBM layout (all row-major, bf16 unless noted):
//   weights   Wqkv[(H+2Hkv)*dh, d] Wo[d, H*dh] Wgu[2F, d] Wd[d, F] per layer, each also transposed (W^T) for dX;
//             embed[V, d], lm_head[V, d] (+^T), norm vectors [d]
//   adapters  flat fp32 masters/grads/moments (logical A[r,in], B[out,r]); packed bf16 operands per module group
//   stash     per layer: x_in, xn1, qkv, attn, h_mid, xn2, gu, act [T, .], us_* [T, RP], rstd1/2 [T] f32, lse [H, T] f32
//   backward  shared scratch: dX, dH, dxn, dattn, dqkv, dact, dgu, transposed operands, split-K slabs
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/tst_hip.h"
#include "common.h"
#include "host_logic.h"
#include "kernels.h"

static_assert(tsthost::kMaxStack == TST_MAX_STACK, "host_logic.h and kernels.h disagree about the stack size");
static_assert(tsthost::kIgMaxSteps == TST_IG_MAX_STEPS, "host_logic.h and tst_hip.h disagree about the step limit of integrated gradients");

namespace {

thread_local std::string g_create_err;

// CU-masked streams: one per (device, CU count), shared by the contexts that ask for that mask, created on first use and destroyed by an exit handler.
// Two behaviours of this runtime (ROCm 7.2 on gfx950) shape that, both reproduced WITHOUT any code of this library (tools/probes/, records under profiles/r05_cumask_*):
//  (1) after hipStreamDestroy of a CU-masked stream while other user streams of the device are alive, the next hipStreamDestroy of a PLAIN stream -- even one
//      created afterwards -- never returns (cumask_probe.hip modes 0, 2, 7: the call stops inside the runtime's queue release, last log line rocdevice.cpp
//      "Free hsa memory"); destroying the masked stream after every plain stream is clean, also for contexts created one after the other (modes 5, 9).
//      This is what round 4 saw as "tst_destroy hangs behind its hipFree calls": the stop was the hipStreamDestroy(own_stream) behind them.
//      So a context never destroys a masked stream: other contexts', the caller's or torch's streams may be alive.
//  (2) a CU-masked stream that is still alive when the process exits makes `rocprofv3 --kernel-trace -- python3 ...` die with SIGSEGV in __cxa_finalize after
//      the tool has written its output (cumask_exit.py `leak`, 25 lines of ctypes on libamdhip64; a leaked plain stream, or a masked stream destroyed before
//      exit, ends rc 0). So the streams are destroyed by an atexit handler -- registered when the first one is created, i.e. after the HIP runtime's own
//      initialisation, so that it runs before the runtime's teardown -- as the last HIP calls this library makes.
// Bits 0 .. n-1 set = n / 8 CUs of every XCD (the driver deals the bits round-robin over the XCDs).
struct MaskedStreams {
  std::mutex mu;
  std::vector<std::pair<std::pair<int, int>, hipStream_t>> cache;
  bool hooked = false;
};
inline MaskedStreams& masked_streams() {
  static MaskedStreams* m = new MaskedStreams();   // (never freed: the exit handler below may run after this library's static destructors)
  return *m;
}
inline void masked_streams_atexit() {
  MaskedStreams& m = masked_streams();
  std::lock_guard<std::mutex> lk(m.mu);
  for (auto& e : m.cache) {
    if (hipSetDevice(e.first.first) != hipSuccess) continue;
    (void)hipStreamSynchronize(e.second);
    (void)hipStreamDestroy(e.second);
  }
  m.cache.clear();
}
inline hipStream_t masked_stream(int device, int n_cus) {
  MaskedStreams& m = masked_streams();
  std::lock_guard<std::mutex> lk(m.mu);
  for (auto& e : m.cache) if (e.first.first == device && e.first.second == n_cus) return e.second;
  uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n_cus && i < 256; ++i) mask[i >> 5] |= 1u << (i & 31);
  hipStream_t s = nullptr;
  if (hipExtStreamCreateWithCUMask(&s, 8, mask) != hipSuccess) return nullptr;
  if (!m.hooked) { m.hooked = true; (void)atexit(masked_streams_atexit); }
  m.cache.push_back({{device, n_cus}, s});
  return s;
}

// every TST_* integer / boolean switch of this file: unset = the default, else atoi
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt) != 0; }
// the attention kernels take a sequence's workgroups longest sequence first (plan_batch's order vector); TST_ATTN_ORDER=0: batch order (A/B switch; no output depends on it)
inline bool attn_order_on() {
  static const bool on = env_flag("TST_ATTN_ORDER", true);
  return on;
}

struct DevPool {
  std::vector<void*> ptrs;
  int64_t bytes = 0;
  void* alloc(int64_t n) {
    if (n <= 0) n = 16;
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)n) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, (size_t)n) != hipSuccess) { (void)hipFree(p); return nullptr; }  // stale rows must be finite
    ptrs.push_back(p);
    bytes += n;
    return p;
  }
  // one allocation back (the KV cache of a generation that grows): the caller has synchronised every stream that may still touch it
  void free_one(void* p, int64_t n) {
    for (size_t i = 0; i < ptrs.size(); ++i)
      if (ptrs[i] == p) {
        (void)hipFree(p);
        ptrs.erase(ptrs.begin() + (long)i);
        bytes -= n <= 0 ? 16 : n;
        return;
      }
  }
  void release() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
    bytes = 0;
  }
};

// AT = element type of every weight / activation / packed-adapter tensor: bf16_t on the product path, float in the fp32 "strict"
// parity mode (cfg.precision = TST_PRECISION_STRICT). Trainable masters, gradients, Adam moments, logits and statistics are fp32 in both.
template <typename AT>
struct LoraGroupT {
  bool on = false;
  LoraGroupDescT<AT> d;
  int index = -1;  // position in ctx->descs
};

// one of a layer's four projections y = x . W^T, in the order the flat buffer of a full fine-tune, the optimizer and tst_init_random visit them
enum { P_QKV = 0, P_O = 1, P_GU = 2, P_D = 3 };
template <typename AT>
struct ProjT {
  AT *W = nullptr, *WT = nullptr;   // [dout, din] and its transpose for dX (nullptr: dX contracts against W itself, tst_ctx::kmajor bit 0)
  int dout = 0, din = 0;
  const LoraGroupT<AT>* g = nullptr;   // the module group on it (in the same LayerT)
  int64_t numel() const { return (int64_t)dout * din; }
};

template <typename AT>
struct LayerT {
  AT *attn_norm, *mlp_norm;
  AT* bqkv = nullptr;  // Qwen2 / GPT-2: bias of the fused q|k|v projection [dqkv]
  // Qwen3: per-head RMSNorm of q and k over head_dim (modeling_qwen3.py:237-238, 252-253): one [128] vector for all query heads, one for all key heads
  AT *q_norm = nullptr, *k_norm = nullptr;
  bool q_norm_set = false, k_norm_set = false;   // tst_finalize_weights refuses a Qwen3 context whose head-norm vectors were never given
  AT* qk_raw = nullptr;        // stash [T, (H + Hkv) 128]: q|k as the projection wrote them (the head norm runs in place; its backward re-forms x_hat from this)
  float* rstd_qk = nullptr;    // [T, H + Hkv]
  AT *attn_norm_b = nullptr, *mlp_norm_b = nullptr, *bo = nullptr, *bgu = nullptr, *bd = nullptr;  // GPT-2: LayerNorm and Conv1D biases
  ProjT<AT> proj[4];
  LoraGroupT<AT> g_qkv, g_o, g_gu, g_d;
  // stash
  AT *x_in, *xn1, *qkv, *attn, *hmid, *xn2, *gu, *act;
  AT *us_qkv, *us_o, *us_gu, *us_d;
  float *rstd1, *rstd2, *lse;
};

using TrainableInfo = tsthost::TrainableEntry;   // (name, offset, rows, cols): host_logic.h states the LoRA table

}  // namespace

struct tst_ctx {
  virtual ~tst_ctx() {}
  bool strict = false;   // cfg.precision == TST_PRECISION_STRICT: this is a CtxT<float>, else a CtxT<bf16_t>
  bool has_parent = false;
  tst_model_cfg cfg;
  int device;
  hipStream_t stream = nullptr;       // the stream every step is enqueued on: own_stream, or the caller's (tst_set_stream)
  hipStream_t own_stream = nullptr;
  std::string err;
  DevPool pool;
  bool finalized = false;

  int d, L, H, Hkv, dh, F, V, dq, dkv, dqkv, dattn;
  int proj_dout[4] = {0}, proj_din[4] = {0};   // widths of a layer's four projections (P_QKV .. P_D)
  // GPT-2 family (TST_ARCH_GPT2): LayerNorm with bias, learned positions wpe, biased Conv1D linears, gelu_new MLP (one
  // fc projection of width F instead of gate|up), no RoPE, head tied to the token embedding.
  // intra-fold data parallelism: one RCCL communicator per fold group, collectives enqueued on this ctx's stream
  ncclComm_t dp_comm = nullptr;
  int dp_ranks = 1;
  // full fine-tune + data parallelism: the flat gradient is reduced region by region (lm_head, then layer L-1 .. 0, then the
  // embedding side and the norm / bias tail) on a communication stream while backward is still producing the earlier layers'
  // gradients (TORCH/nn/parallel/distributed.py:828-834: bucketed all-reduce overlapped with backward); regions in launch order
  hipStream_t dp_stream = nullptr;
  hipEvent_t dp_ev = nullptr, dp_done = nullptr;
  std::vector<std::pair<int64_t, int64_t>> dp_regions;   // (offset, count) into tg
  // bf16 transport of the region-wise reduction (tst_dp_set_transport): a region is rounded to bf16 into dp_stage, all-reduced as
  // ncclBfloat16 (half the bytes on the xGMI link: 15 instead of 30 GB per step for an 8B full fine-tune) and widened back into tg
  bool dp_bf16 = false;
  unsigned short* dp_stage = nullptr;
  int64_t dp_stage_elems = 0;
  size_t dp_next = 0;
  // the region table of a full fine-tune, built with the context (tst_dp_init copies it into dp_regions). Taking each region's sum
  // of squares for the gradient norm on a side stream the same way was measured and dropped: 485 -> 521 ms per bench step, the
  // memory-bound norm kernels slow the contractions they run beside by more than the 24 ms they take off the critical path.
  std::vector<std::pair<int64_t, int64_t>> gn_regions;
  // full fine-tune: the weight-gradient contractions leave per-workgroup sums of squares of what they store (GemmParams.sumsq), so
  // the global norm needs no second pass over the 28 GB of layer gradients: only the embedding, the head and the small vectors
  // are summed afterwards. Fixed slots, zeroed at the start of backward: reproducible.
  float* gn_partial = nullptr;
  int64_t gn_cap = 0, gn_used = 0;
  float* colred_ws = nullptr;   // full fine-tune: slice sums of the norm-weight / bias gradient reductions (two launches, no atomics: kernels.h colred_ws_floats)
  bool gn_fused = false;          // the slots describe the gradient now in tg (not after a data-parallel reduction / a caller's own)
  int last_variant = -1, last_sk = 1;   // tile family and split of the last run_gemm
  int64_t dp_n_coll = 0, dp_n_elems = 0;   // collectives enqueued / fp32 elements reduced since tst_dp_init (tst_dp_stats)
  // optimizer-state sharding (cfg.zero_ranks > 1, full fine-tune): tp / tm / tv hold the elements [z_lo, z_hi) of the flat trainable vector
  // only (index i of the vector lives at tp[i - z_lo]); tg and the compute copy wb are full length, padded to n_pad = zero_ranks * z_shard
  bool zero_on = false;   // cfg.zero_ranks >= 1 (1 = a single shard: the sharded step with 1-rank collectives, for one-GPU tests)
  int zero = 1, zero_rank = 0;
  int64_t z_lo = 0, z_hi = 0, z_shard = 0, n_pad = 0;
  float* z_sumsq = nullptr;   // device [1]: the shard's sum of squares, all-reduced over the group
  // Full fine-tune: the optimizer step off the critical path. AdamW over 8 G parameters is 45 ms of HBM streaming per step and needs the clip
  // coefficient, i.e. the END of backward, so it cannot hide under backward; but the NEXT forward needs the updated weights layer by layer, and its
  // contractions (80-tile grids at one micro-batch) leave most CUs and nearly all of the HBM bandwidth idle. So the per-matrix AdamW launches go to
  // opt_stream in FORWARD order -- norm / bias tail and embedding side, layers 0 .. L-1, head -- one event each, and every forward (train or score) makes
  // its stream wait for event i just before it touches those weights (opt_need). Every other reader / writer of weights, masters, moments or the
  // gradient joins the whole optimizer first (opt_join: all host waits go through ctx_sync, which does). Same arithmetic per element as the serial step.
  hipStream_t opt_stream = nullptr;
  bool side_shared = false;         // (TST_DW_CUS) the side stream is a CU-masked stream from the process-wide cache: never destroyed by a context
  bool opt_stream_shared = false;   // a CU-masked stream from the process-wide cache (masked_stream): never destroyed
  hipEvent_t opt_go = nullptr;
  std::vector<hipEvent_t> opt_ev;   // [0] tail + embedding side, [1 + l] layer l, [L + 1] head
  size_t opt_joined = 0;            // events of the pending optimizer step the context's stream already waits for
  bool opt_pending = false;
  bool opt_overlap = env_flag("TST_OPT_OVERLAP", true);   // "opt_overlap" (tst_set_option)
  bool gpt2 = false;
  bool qk_norm = false;    // TST_ARCH_QWEN3: head norm between the q|k|v projection and RoPE (csrc/head_norm.hip)
  float* hn_ws = nullptr;  // full fine-tune: partial sums of the head-norm weight gradients (HEAD_NORM_WS_FLOATS)
  int Vp = 0;    // vocabulary padded to a multiple of 64 (GPT-2: 50257 -> 50304): row count of embed / lm_head, ld of the logits
  int Fgu = 0;   // output width of the first MLP projection: 2F (gate|up) or F (c_fc)
  int npos = 0;  // rows of wpe
  int Tmax, Smax, Rmax, Tpad_max;

  float *cosT = nullptr, *sinT = nullptr;

  // full fine-tune (TST_TRAIN_FULL): every weight is trainable. wb = bf16 compute copy of all weights in ONE flat buffer
  // laid out exactly like the fp32 master tp (matrices first = decay group, then norm vectors = no-decay group), so the
  // optimizer kernel refreshes it element for element; wb0 = pristine snapshot restored at the start of each fold.
  bool full = false;
  int64_t n_decay = 0, per_layer = 0;   // (host_logic.h full_layout: the decay group's length, one layer's four matrices)
  tsthost::ModelDims md;                // host_logic.h model_dims of cfg: what the fields above restate, and qkv_bias
  // trainables
  int64_t n_train = 0;
  float *tp = nullptr, *tg = nullptr, *tm = nullptr, *tv = nullptr;
  // stacked folds (cfg.n_stack > 1, LoRA only): ns adapter sets with their own optimizer state in ONE context. Slot s owns
  // trainables [s*n1, (s+1)*n1) and the rank columns [s*nmod*r, (s+1)*nmod*r) of every module group; the frozen projections
  // see the tokens of all slots as one contraction (M = sum of the folds' micro-batches), the adapters are kept apart by
  // zeroing, per token, the rank columns of the other slots (rank_mask).
  int ns = 1, sel_slot = 0;
  int64_t n1 = 0;                        // trainables per slot (n_train = ns * n1)
  int opt_steps[TST_MAX_STACK] = {0};
  SlotEnds slot_ends;                    // current batch: tokens of slot s end at slot_ends.t_end[s]
  SlotEnds row_ends;                     // current batch: labelled rows of slot s end at row_ends.t_end[s] (slot boundaries of the compacted last layer's rows)
  bool trim_last = env_flag("TST_TRIM_LAST", true);   // "trim_last_token" (include/tst_hip.h tst_set_option; env TST_TRIM_LAST=0 starts with it off)
  int swr = env_int("TST_SWR", 3) & 3;   // "swiglu_rank": bit 0 the forward, bit 1 the backward fused SwiGLU + rank kernel (env TST_SWR)
  bool lc_have = false, lc_on = false, lc_used = false, lc_batch_ok = true;   // last-layer compaction (see lc_attn below): workspace there / switched on / this batch
  int slot_r0[TST_MAX_STACK + 1] = {0};  // current batch: labelled rows of slot s are [slot_r0[s], slot_r0[s+1])
  std::vector<TrainableInfo> tinfo;
  long pack_max_elems = 0, pack_max_long = 0;
  float *clip_out = nullptr, *clip_partial = nullptr;  // device [2], [4096]
  // Which slots take an optimizer step and what their loss is normalised by. Default: a slot steps when it has labelled rows in the
  // batch and is normalised by that count. Gradient accumulation (tst_accumulate_async) and the stacked data-parallel step
  // (tst_train_step_stacked_dp_async) give the count of the WHOLE accumulated / global batch per slot (backward()'s slot_items) instead.
  bool slot_steps[TST_MAX_STACK] = {false};
  // gradient accumulation (HF/trainer.py:1740-1758): tacc = running sum of the micro-batches' flat gradients, d_loss_acc = of their losses;
  // allocated by the first tst_accumulate_async of the context (LoRA: n_train floats; full fine-tune: another 4 B / parameter)
  float *tacc = nullptr, *d_loss_acc = nullptr;
  bool acc_active = false;

  // batch (device) + pinned host staging
  int *d_ids = nullptr, *d_pos = nullptr, *d_cu = nullptr, *d_lab_idx = nullptr, *d_targets = nullptr, *d_opt_ids = nullptr;
  int* d_order = nullptr;   // sequences by decreasing length: launch order of the attention backward's workgroups (host_logic.h plan_batch)
  int* h_stage[2] = {nullptr, nullptr};  // pinned, double-buffered: ids | pos | cu | lab_idx | targets
  hipEvent_t stage_evt[2] = {nullptr, nullptr};
  int stage_idx = 0;
  int* cur_stage = nullptr;
  int* d_idflag = nullptr;     // device [1]: set by ids_check when a TST_BATCH_DEVICE_IDS batch held an id outside the vocabulary
  int* h_idflag = nullptr;     // pinned [1]: copied behind every such batch; reported (and cleared) by the next host wait
  float* h_metrics = nullptr;  // pinned [8 + 16]: loss per slot | {gnorm, clip coef} per slot (async fetch)
  float* h_score = nullptr;    // pinned [Rmax*4 + Rmax*256]: row stats | option logits of the pending tst_score_async
  int* h_opt_ids = nullptr;    // pinned [256]
  int score_R = -1, score_nopt = 0;
  hipEvent_t score_evt = nullptr;  // recorded behind the result copies of tst_score_async: tst_score_fetch waits for it, not for the stream
  std::vector<int> score_tgt, score_row_seq;
  // Greedy generation (tst_generate_async; kernels in decode.hip, row map in host_logic.h plan_generate). Allocated by the first generation of the context,
  // for gen_cap_new new tokens per sequence; re-allocated behind a stream sync when a later call asks for more. gen_kv = K then V of layer 0, layer 1, ...:
  // [gen_rows, Hkv dh] each in the activation dtype. gen_dev = meta | prefill_rows [Tmax] | decode_rows; gen_tok / gen_logp = the steps' outputs [S, max_new].
  // forward() takes the pass of a generation as its GenPass argument (below).
  void* gen_kv = nullptr;
  int64_t gen_kv_bytes = 0, gen_dev_bytes = 0, gen_out_bytes = 0;
  long gen_rows = 0;
  int gen_cap_new = 0;
  int *gen_dev = nullptr, *gen_tok = nullptr;
  float* gen_logp = nullptr;
  int* h_gen = nullptr;         // pinned: staging image of gen_dev | tokens [Smax, cap_new] | logp [Smax, cap_new] of the pending generation
  hipEvent_t gen_evt = nullptr; // recorded behind the result copies: tst_generate_fetch waits for it, not for the stream
  int gen_S = -1, gen_new = 0;  // pending generation (-1: none); a sampled one (tst_sample_async) shares the slot: gen_S counts its decode rows
  int gen_samples = 0;          // 0: the pending generation is greedy; n >= 1: sampled with n draws per prompt
  int *smp_seeds = nullptr, *h_smp_seeds = nullptr;   // sampled generations: low | high word of every sequence's seed [2 Smax] and its pinned staging image (first tst_sample_async)
  std::vector<int> gen_eos;
  // Candidate scoring (tst_score_candidates_async; kernels in decode.hip, row map in host_logic.h plan_candidates): the generation's cache and pending slot, and a
  // block of its own allocated by the first such call of the context: cand_dev = geo | ext_rows | src (cand_dev_ints) | logp_tok [Rmax]; h_cand = the pinned
  // staging image of the first three, then ids | pos | lab_idx | targets of the extend rows [4 x cand_ext_cap] and logp_tok [Rmax] of the pending call.
  int* cand_dev = nullptr;
  int* h_cand = nullptr;
  int cand_n_ext = 0;           // candidates with at least two tokens of the call being enqueued: attn_extend's workgroups per kv head
  int gen_cand = 0;             // n >= 1: the pending generation is a tst_score_candidates_async over n candidates (gen_S counts their tokens)
  std::vector<int> cand_cu;
  // Token attribution (tst_attribute_async; kernels in attribute.hip, row weights and the fetch side in host_logic.h). Allocated by the first attribution of the
  // context. attr_dev = row weights [Rmax] | row kinds [Rmax] | option ids [256] | gxi [Tmax] | gnorm [Tmax] (4-byte words); h_attr = the pinned staging image of the
  // first three, then gxi | gnorm | row statistics [Rmax * 4] of the pending attribution. forward() and backward() take the pass of an attribution as their AttrPass
  // argument (below). grad_stale: the flat gradient no longer holds a training step's gradient.
  float* attr_dev = nullptr;
  float* h_attr = nullptr;
  hipEvent_t attr_evt = nullptr;   // recorded behind the result copies: tst_attribute_fetch waits for it, not for the stream
  int attr_S = -1, attr_nopt = 0;  // pending attribution (-1: none)
  bool grad_stale = false;
  tsthost::AttrPlan attr_plan;
  std::vector<int> attr_cu_dev, attr_cu_src;
  // Integrated gradients (tst_attribute_ig_async): the same pending slot as an attribution, attr_ig telling the two kinds apart. Allocated by the first such call of
  // the context. ig_dev = baseline ids in device token order [Tmax] | ig [Tmax] (4-byte words); h_ig = the pinned staging of the baseline ids [Tmax], then ig [Tmax] |
  // row statistics at the baseline [Rmax * 4] | at the real prompt [Rmax * 4] of the pending call.
  float* ig_dev = nullptr;
  float* h_ig = nullptr;
  bool attr_ig = false;
  float* d_loss = nullptr;
  int cur_T = 0, cur_S = 0, cur_R = 0, cur_maxlen = 0, cur_items = 0;
  double cur_sumsq_len = 0;   // sum over the batch's sequences of length^2 (attention work)
  std::vector<int> row_seq;

  // head / loss workspace
  float *rstd_f = nullptr, *logits = nullptr, *stats = nullptr, *optl = nullptr;
  // backward scratch
  // LoRA: the adapter-gradient contractions (dB = dy^T.us, dA = s du^T.x) of a module group are not on the dX chain, so they
  // run on a side stream with their own split-K slab; du has one buffer per module group of a layer (the side stream reads it
  // while the main stream moves on). Joined once per layer (before dX is overwritten) and before the optimizer.
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool dw_side = env_flag("TST_FULL_DW_SIDE", true);   // "dw_side" (tst_set_option)
  // full fine-tune, bf16 path: the K-major members of the 256x256 ping-pong tile (gemm_pp.hip TA / TB). Bit 0 (fixed at tst_create, env TST_KMAJOR): dX = dY . W from
  // the ONE stored W (NN) -- no W^T copies in HBM, AdamW writes 30 instead of 32 B / param; bit 1 ("kmajor_dw"): dW = dy^T . x straight from the row-major
  // activations (TN) -- no transposed activation copies. "kmajor" (tst_set_option) reads both bits
  int kmajor = 0;
  int nbdw = env_int("TST_NBDW", 1);   // "norm_bwd_dw" (tst_set_option): full fine-tune, RMSNorm backward + its weight gradient in one pass
  int nrk = env_int("TST_NRK", 1);   // "norm_rank" (tst_set_option): RMSNorm forward fused with the rank-axis contraction behind it
  // "ndw_side" (tst_set_option): a full fine-tune's norm-weight reductions beside the weight gradients on the side stream. OFF by default: measured -1.1 %
  // (24.12 -> 23.85 QA-pairs/s, two interleaved rounds, profiles/r05_full_ndw_side_ab.txt) -- as in round 4, when the side stream was the longer one
  bool ndw_side = env_flag("TST_NDW_SIDE", false);
  bool ndw_open[2] = {false, false};
  hipEvent_t ev_ndw[2] = {nullptr, nullptr};
  float* colred_ws_side = nullptr;
  bool in_backward = false;    // (between the entry and the exit of backward(): the tile policy of a full fine-tune may differ by pass)
  bool dw_side_open = false;   // full fine-tune: weight-gradient work of the current layer is in flight on the side stream (joined per layer)
  float* side_slab = nullptr;
  size_t side_slab_bytes = 0;
  float* delta = nullptr;
  float* slab = nullptr;
  size_t slab_bytes = 0;

  // profiling of the dense contractions
  bool prof = false;
  bool prof_hbm = false;   // tst_profile_enable(ctx, 2 | 1): also bracket the HBM-bound kernel classes (variant ids >= 100)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  hipEvent_t prof_ref = nullptr;  // recorded at tst_profile_enable(1): time origin of tst_profile_intervals
  struct ProfMeta { int variant, splitk; double flop; };
  std::vector<ProfMeta> prof_meta;
};

// the typed half of a context: every tensor whose element type depends on the precision mode
template <typename AT>
struct CtxT : tst_ctx {
  const CtxT<AT>* parent = nullptr;  // set by tst_fork: frozen weights are borrowed from it (it must outlive this ctx)
  AT *wpe = nullptr, *final_norm_b = nullptr;
  AT *embed = nullptr, *lm_head = nullptr, *lm_headT = nullptr, *final_norm = nullptr;
  std::vector<LayerT<AT>> layers;
  // every tensor the model's state_dict names, built once at the end of build_ctx: tst_set_weight / tst_get_weight look a name up here, and the trainables of a
  // full fine-tune (tst_trainable_info) are the entries that lie inside wb. rows / cols describe the device layout (a GPT-2 Conv1D weight: [out, in], the
  // transpose of the HF tensor); alias: a second name of storage another entry owns (GPT-2's tied lm_head)
  struct Named { std::string name; AT* ptr; int64_t rows, cols; bool conv1d, alias; };
  std::vector<Named> named;
  AT* x_last = nullptr;  // output of the last layer
  // full fine-tune: wb = compute copy of all weights in ONE flat buffer laid out exactly like the fp32 master tp; wb0 = pristine snapshot
  AT *wb = nullptr, *wb0 = nullptr;
  std::vector<LoraGroupDescT<AT>> descs;
  LoraGroupDescT<AT>* descs_dev = nullptr;
  // head / loss workspace
  AT *xg = nullptr, *xf = nullptr, *dxf = nullptr, *dxg = nullptr, *dlogits = nullptr;
  // backward scratch
  AT *dX = nullptr, *dH = nullptr, *dxn = nullptr, *dattn_b = nullptr, *dqkv_b = nullptr, *dact = nullptr, *dgu = nullptr;
  AT *du = nullptr, *dyT = nullptr, *xT = nullptr;
  AT* du4[4] = {nullptr, nullptr, nullptr, nullptr};
  // Last-layer compaction (LoRA; TST_LAST_COMPACT, default on): behind the last layer's attention only the rows the head reads (labelled / selected rows,
  // d_lab_idx) are ever used -- o projection, MLP and their backward are row-wise -- so those run on the R gathered rows instead of all T tokens
  // (88 % of one layer's projection FLOPs, forward and backward). lc_* = that layer's compact stash and backward scratch, [roundup64(Rmax), .] rows.
  AT *lc_attn = nullptr, *lc_xin = nullptr, *lc_hmid = nullptr, *lc_xn2 = nullptr, *lc_gu = nullptr, *lc_act = nullptr;
  AT *lc_us_o = nullptr, *lc_us_gu = nullptr, *lc_us_d = nullptr;
  AT *lc_dact = nullptr, *lc_dgu = nullptr, *lc_dxn = nullptr, *lc_dH = nullptr, *lc_dattn = nullptr;
  float* lc_rstd2 = nullptr;
  // LoRA: the adapter-gradient contractions of a layer's four module groups are collected here and issued as ONE grouped launch
  // at the end of the layer's backward (gemm_tn_grouped: no split-K, no slab reduces); needs one du buffer per group (du4)
  std::vector<GemmParamsT<AT>> tn_pending;
  double tn_pending_flop = 0;
  // the same contractions for gemm_tns_grouped (bf16 path): restricted to each slot's tokens and rank block, 64-wide rank tiles
  std::vector<TnsProblem> tns_pending;
};

namespace {

#define CTX_HIP(call)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
      return TST_EHIP;                                                                    \
    }                                                                                     \
  } while (0)

#define CTX_RC(call)                                                        \
  do {                                                                      \
    int rc_ = (call);                                                       \
    if (rc_ != TST_OK) {                                                    \
      if (ctx->err.empty()) {                                               \
        hipError_t le_ = hipGetLastError();                                 \
        ctx->err = std::string(#call) + " failed rc=" + std::to_string(rc_) + \
                   (le_ != hipSuccess ? std::string(": ") + hipGetErrorString(le_) : std::string()); \
      }                                                                     \
      return rc_;                                                           \
    }                                                                       \
  } while (0)

int fail(tst_ctx* ctx, int rc, const std::string& msg) {
  ctx->err = msg;
  return rc;
}

inline uint16_t host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float host_bf2f(uint16_t b) {
  uint32_t u = ((uint32_t)b) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

template <typename T>
T* palloc(tst_ctx* ctx, int64_t count) {
  return (T*)ctx->pool.alloc(count * (int64_t)sizeof(T));
}

int roundup(int a, int b) { return (a + b - 1) / b * b; }

// inverse frequency i of the rotary embedding: host_logic.h (HF's fp32 operation order, linear and llama3 scaling)
using tsthost::rope_inv_freq;

// every data-parallel collective goes through here (in-place fp32 sum): counted, so a test can check that a rank without rows issues
// exactly the sequence of a rank with rows (a mismatch would hang the group)
int dp_allreduce(tst_ctx* ctx, float* buf, size_t n, hipStream_t st) {
  ctx->dp_n_coll += 1;
  ctx->dp_n_elems += (int64_t)n;
  if (ncclAllReduce(buf, buf, n, ncclFloat, ncclSum, ctx->dp_comm, st) != ncclSuccess) {
    ctx->err = "ncclAllReduce failed";
    return TST_EHIP;
  }
  return TST_OK;
}
// A failed data-parallel step must not leave the peers waiting inside the step's collectives for ever: the communicator is aborted
// (ncclCommAbort), the caller gets the error and is expected to exit non-zero (tst.cli does; torch.distributed.run then ends the job)
void dp_abort(tst_ctx* ctx, const char* why) {
  if (!ctx->dp_comm) return;
  (void)ncclCommAbort(ctx->dp_comm);
  ctx->dp_comm = nullptr;
  ctx->dp_ranks = 1;
  ctx->err += std::string(" [data-parallel group aborted: ") + why + "]";
}
// bounded wait for a data-parallel context's stream: a peer that died leaves this rank's all-reduce kernel spinning. Polls the stream and
// the communicator's asynchronous error state; after TST_DP_TIMEOUT_S seconds (default 600) the communicator is aborted.
template <typename Q>
int dp_poll(tst_ctx* ctx, Q&& query) {
  static const double limit_s = [] { const char* e = getenv("TST_DP_TIMEOUT_S"); return e ? atof(e) : 600.0; }();
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = query();
    if (q == hipSuccess) return TST_OK;
    if (q != hipErrorNotReady) { ctx->err = std::string("stream / event query: ") + hipGetErrorString(q); dp_abort(ctx, "stream error"); return TST_EHIP; }
    ncclResult_t ae = ncclSuccess;
    if (ctx->dp_comm && (ncclCommGetAsyncError(ctx->dp_comm, &ae) != ncclSuccess || ae != ncclSuccess)) {
      ctx->err = std::string("RCCL asynchronous error: ") + ncclGetErrorString(ae);
      dp_abort(ctx, "communicator error");
      return TST_EHIP;
    }
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
      ctx->err = "data-parallel step did not finish within TST_DP_TIMEOUT_S: a peer rank failed or stalled";
      dp_abort(ctx, "timeout");
      return TST_EHIP;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}
int dp_wait(tst_ctx* ctx, hipStream_t st) {
  return dp_poll(ctx, [&] { return hipStreamQuery(st); });
}
// overlapped optimizer step of a full fine-tune: the context's stream waits for the first `upto` events of the pending step (no-ops otherwise)
int opt_need(tst_ctx* ctx, size_t upto) {
  if (!ctx->opt_pending) return TST_OK;
  if (upto > ctx->opt_ev.size()) upto = ctx->opt_ev.size();
  for (; ctx->opt_joined < upto; ++ctx->opt_joined) {
    const hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->opt_ev[ctx->opt_joined], 0);
    if (e != hipSuccess) { ctx->err = std::string("hipStreamWaitEvent (optimizer stream): ") + hipGetErrorString(e); return TST_EHIP; }
  }
  if (ctx->opt_joined == ctx->opt_ev.size()) ctx->opt_pending = false;
  return TST_OK;
}
// ... for all of it (the optimizer stream is in order: its last event covers the others)
int opt_join(tst_ctx* ctx) {
  if (!ctx->opt_pending) return TST_OK;
  ctx->opt_joined = ctx->opt_ev.size() - 1;
  return opt_need(ctx, ctx->opt_ev.size());
}
// EVERY host wait of a context goes through these two: a context that has joined a data-parallel group never blocks without a bound
// (a peer that died inside a collective leaves this rank's kernel spinning), any other context simply synchronises
int ctx_sync(tst_ctx* ctx) {
  { const int jrc = opt_join(ctx); if (jrc != TST_OK) return jrc; }   // the stream waits for a pending optimizer step, the host for the stream
  if (ctx->dp_comm) {
    const int rc = dp_wait(ctx, ctx->stream);
    if (rc != TST_OK) return rc;
  } else {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); return TST_EHIP; }
  }
  if (ctx->h_idflag && *ctx->h_idflag) {   // a device-id batch since the last wait held an id outside the vocabulary: its results are void
    *ctx->h_idflag = 0;
    (void)hipMemsetAsync(ctx->d_idflag, 0, sizeof(int), ctx->stream);
    ctx->err = "input id out of vocabulary in a TST_BATCH_DEVICE_IDS batch (checked on the device): the results of the steps since the last wait are invalid";
    return TST_EINVAL;
  }
  return TST_OK;
}
int ctx_event_sync(tst_ctx* ctx, hipEvent_t ev) {
  if (ctx->dp_comm) return dp_poll(ctx, [&] { return hipEventQuery(ev); });
  const hipError_t e = hipEventSynchronize(ev);
  if (e != hipSuccess) { ctx->err = std::string("hipEventSynchronize: ") + hipGetErrorString(e); return TST_EHIP; }
  return TST_OK;
}

// TIMING-ONLY ablation (env TST_WHATIF, bit mask; never set in a real run: results are then WRONG by construction). It answers "what would the sweep gain if
// this kernel class cost nothing?" BEFORE a fusion is built, by not launching the class at all (its consumers read stale buffers of the right shape):
//   1 = the layers' forward norms (the projections read the un-normed stream)   2 = attention forward + backward   4 = SwiGLU forward + backward
//   8 = the rank-axis contractions u = x.Ag^T / du = dy.Bg                       16 = the adapter-gradient launch
// bench.py marks a line produced under it as a diagnostic (profiles/r04_whatif_*.txt).
// The first 12 forward passes of a context run everything, so that the buffers the ablated classes would have written hold REAL values afterwards (a
// zero-filled operand raises the clock of every contraction that reads it: MI355X_MICROARCH.md "DVFS give-back").
// Compiled into the LAB library only (-DTST_BUILD_LAB: libtst_hip_lab.so, which bench.py loads when TST_WHATIF is set): in the product library whatif() is the
// constant 0 and the variable is never read, so no environment setting can make libtst_hip.so skip work and still return TST_OK.
#ifdef TST_BUILD_LAB
std::atomic<int> g_whatif_live{0};   // (contexts may step from several host threads)
inline int whatif() {
  static const int m = env_int("TST_WHATIF", 0);
  return g_whatif_live.load(std::memory_order_relaxed) >= 12 ? m : 0;
}
inline void whatif_tick() { if (g_whatif_live.load(std::memory_order_relaxed) < 12) g_whatif_live.fetch_add(1, std::memory_order_relaxed); }
#else
constexpr int whatif() { return 0; }
inline void whatif_tick() {}
#endif

// HBM-bound kernel classes of the measurement hooks (tst_profile_read variant ids): work = algorithmic bytes of the launch
enum { PROF_ADAMW = 101, PROF_SWIGLU = 102, PROF_NORM = 103, PROF_ATTN = 104 };
// event bracket around one or more launches on `st`: prof_begin returns the slot (or -1 when not profiling)
int prof_begin(tst_ctx* ctx, hipStream_t st, bool on) {
  if (!on) return -1;
  if (ctx->prof_used == ctx->prof_events.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
    ctx->prof_events.push_back({a, b});
  }
  (void)hipEventRecord(ctx->prof_events[ctx->prof_used].first, st);
  return (int)ctx->prof_used;
}
void prof_end(tst_ctx* ctx, hipStream_t st, int slot, int variant, int splitk, double work) {
  if (slot < 0) return;
  (void)hipEventRecord(ctx->prof_events[(size_t)slot].second, st);
  if (ctx->prof_meta.size() <= (size_t)slot) ctx->prof_meta.resize((size_t)slot + 1);
  ctx->prof_meta[(size_t)slot] = {variant, splitk, work};
  ctx->prof_used = (size_t)slot + 1;
}

// ---- dense contraction wrapper (optionally timed with HIP events on the ctx stream) ----
template <typename AT>
int run_gemm(CtxT<AT>* ctx, GemmParamsT<AT> p, bool on_side = false) {
  hipStream_t gst = on_side ? ctx->side : ctx->stream;
  const int slot = prof_begin(ctx, gst, ctx->prof);
  int used[2] = {0, 1};
  // a full fine-tune never has the GPU to one stream: the weight gradients run beside the dX chain, AdamW beside the next forward. The tail split (fp32 partials
  // of the last partial wave of tiles + a reduce launch) then only adds traffic: 22.9 -> 23.4 QA-pairs/s without it (profiles/r05_full_tail_split_ab.txt)
  if (ctx->full) {
    p.no_tail = 1;
    static const int fsk = env_int("TST_FULL_SPLITK", 2);   // A/B: bit 0 = split-K in the forward (under AdamW the slabs add HBM traffic to the saturated side), bit 1 = in the backward; 2: profiles/r05_full_splitk_ab.txt
    if (!(fsk & (ctx->in_backward ? 2 : 1))) p.no_splitk = 1;
  }
  int rc = gemm_nt(gst, p, on_side ? ctx->side_slab : ctx->slab, on_side ? ctx->side_slab_bytes : ctx->slab_bytes, -1, -1, used);
  ctx->last_variant = used[0]; ctx->last_sk = used[1];
  double flop = 2.0 * p.M * p.N * (double)(p.K + p.K2);
  if (p.k2_w > 0 && used[0] == 5 && used[1] == 1) {   // the ping-pong tile ran only the K2 k-tiles of its rows' slots: count what ran
    flop = 2.0 * p.M * p.N * (double)p.K;
    for (int r_lo = 0; r_lo < p.M; r_lo += 256) {
      const int r_hi = (r_lo + 256 < p.M ? r_lo + 256 : p.M) - 1;
      int s_lo = 0, s_hi = 0;
      for (int q = 0; q + 1 < p.mask_nslot; ++q) { s_lo += r_lo >= p.mask_ends.t_end[q]; s_hi += r_hi >= p.mask_ends.t_end[q]; }
      int last = ((s_hi + 1) * p.k2_w + 63) >> 6;
      if (last > (p.K2 >> 6)) last = p.K2 >> 6;
      flop += 2.0 * (r_hi - r_lo + 1) * p.N * 64.0 * (last - ((s_lo * p.k2_w) >> 6));
    }
  }
  prof_end(ctx, gst, slot, used[0], used[1], flop);
  if (rc != TST_OK && ctx->err.empty())
    ctx->err = "gemm_nt rc=" + std::to_string(rc) + " M=" + std::to_string(p.M) + " N=" + std::to_string(p.N) + " K=" + std::to_string(p.K) +
               " K2=" + std::to_string(p.K2);
  return rc;
}

// C[M,N] (fp32) = alpha * sum_{t<T} P[t,M] * Q[t,N]
template <typename AT>
int run_gemm_tn(CtxT<AT>* ctx, const AT* P, long ldp, const AT* Q, long ldq, float* C, long ldc, int M, int N, int T, float alpha, bool on_side = false) {
  hipStream_t st = on_side ? ctx->side : ctx->stream;
  float* slab = on_side ? ctx->side_slab : ctx->slab;
  const size_t slab_bytes = on_side ? ctx->side_slab_bytes : ctx->slab_bytes;
  GemmParamsT<AT> p;
  memset(&p, 0, sizeof(p));
  p.A = P; p.lda = ldp; p.B = Q; p.ldb = ldq; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = roundup(T, 64); p.kvalid = T;
  p.alpha = alpha; p.out_f32 = 1;
  const int slot = prof_begin(ctx, st, ctx->prof);
  int used[2] = {3, 1};
  int rc = gemm_tn(st, p, slab, slab_bytes, used);
  prof_end(ctx, st, slot, 3, used[1], 2.0 * M * N * (double)T);
  if (rc != TST_OK && ctx->err.empty()) ctx->err = "gemm_tn rc=" + std::to_string(rc);
  return rc;
}

// the K-major members of the 256x256 ping-pong tile (gemm_pp.hip; bf16 path): TN for dW = dy^T . x, NN for dX = dy . W. `site` names the caller in the error text
inline int run_gemm_kmajor(tst_ctx* ctx, const GemmParams& p, bool on_side, int split, double flop, const char* site, bool shape_in_err = false) {
  hipStream_t st = on_side ? ctx->side : ctx->stream;
  const int slot = prof_begin(ctx, st, ctx->prof);
  int used[2] = {5, 1};
  const int rc = gemm_pp_kmajor(st, p, on_side ? ctx->side_slab : ctx->slab, on_side ? ctx->side_slab_bytes : ctx->slab_bytes, split, used);
  prof_end(ctx, st, slot, used[0], used[1], flop);
  if (rc != TST_OK && ctx->err.empty()) {
    ctx->err = std::string("gemm_pp_kmajor (") + site + ") rc=" + std::to_string(rc);
    if (shape_in_err) ctx->err += " M=" + std::to_string(p.M) + " N=" + std::to_string(p.N) + " K=" + std::to_string(p.K);
  }
  return rc;
}

// the rows a contraction runs over: the batch's token rows (slot boundaries slot_ends), or the compact labelled rows of the last layer (row_ends)
struct Rows {
  int n;
  const SlotEnds* ends;
  bool compact;
};
inline Rows token_rows(const tst_ctx* ctx) { return {ctx->cur_T, &ctx->slot_ends, false}; }
inline Rows compact_rows(const tst_ctx* ctx) { return {ctx->cur_R, &ctx->row_ends, true}; }

// the slot mask of a rank-axis operand: row t keeps the rank block (nmod * r columns) of its slot only. Stacked folds always; with one_slot_too (the fused norm /
// SwiGLU rank kernels) also an unstacked context whose block is a multiple of 16 and <= 64 wide: one slot, the columns behind it are the packed operands' zero padding
template <typename AT>
void slot_mask(const tst_ctx* ctx, const LoraGroupT<AT>& g, const Rows& rows, bool one_slot_too, int& width, int& nslot, SlotEnds& ends) {
  const int w = g.d.nmod * g.d.r;
  if (ctx->ns > 1 || (one_slot_too && (w & 15) == 0 && w <= 64)) { width = w; nslot = ctx->ns > 1 ? ctx->ns : 1; }
  if (ctx->ns > 1) ends = *rows.ends;
}

// stacked folds: u / du rows are zero outside their slot's rank block -- tell the projection tile, which then skips the K2 k-tiles of other slots
// (TST_K2_SLOTS=0: A/B switch, every K2 k-tile runs)
template <typename AT>
void k2_slots(const tst_ctx* ctx, GemmParamsT<AT>& p, const LoraGroupT<AT>& g, const Rows& rows) {
  static const bool on = env_flag("TST_K2_SLOTS", true);
  if (on && sizeof(AT) == 2) slot_mask(ctx, g, rows, false, p.k2_w, p.mask_nslot, p.mask_ends);
}

template <typename AT>
GemmParamsT<AT> gp(const AT* A, long lda, const AT* B, long ldb, void* C, long ldc, int M, int N, int K) {
  GemmParamsT<AT> p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.alpha = 1.0f;
  return p;
}

// SwiGLU fused with the rank-axis contraction that reads its result (swiglu_rank.hip): bf16 LoRA path with [gate | up] layout. ctx->swr (tst_set_option
// "swiglu_rank", env TST_SWR): bit 0 the forward (act and us of the down projection), bit 1 the backward (dgu and du of the gate|up projection); default both;
// 0 = the elementwise kernel + gemm_rank / gemm_nt
template <typename AT>
bool swr_setup(CtxT<AT>* ctx, const LoraGroupT<AT>& g, bool backward, const Rows& rows, AT* C, SwiRank& r) {
  if constexpr (sizeof(AT) != 2) return false;
  else {
    if (!(ctx->swr & (backward ? 2 : 1)) || ctx->gpt2 || ctx->full || !g.on || whatif()) return false;
    memset(&r, 0, sizeof(r));
    r.B = backward ? g.d.BgT : g.d.Ag; r.ldb = backward ? 2L * ctx->F : (long)ctx->F; r.C = C; r.N = g.d.RP;
    r.alpha = backward ? 1.0f : g.d.scale;
    slot_mask(ctx, g, rows, true, r.mask_width, r.mask_nslot, r.mask_ends);
    // gate|up group: module 0 owns the gate rows, module 1 the up rows -- Bg is block diagonal, half of BgT's entries in a slot's rank block are zeros by construction
    r.block_diag = backward && r.mask_width && g.d.nmod == 2 && g.d.seg_row0[0] == 0 && g.d.seg_row1[0] == ctx->F && g.d.seg_row0[1] == ctx->F &&
                   g.d.seg_row1[1] == 2 * ctx->F;
    return swiglu_rank_supported(rows.n, ctx->F, r);
  }
}

// y[rows, dout] = x.W^T (+ us.Bg^T) (+R)
template <typename AT>
int linear_fwd(CtxT<AT>* ctx, const AT* x, const ProjT<AT>& P, AT* us, const AT* R, AT* y, const Rows& rows, const AT* bias = nullptr, bool us_done = false) {
  const LoraGroupT<AT>& g = *P.g;
  const int T = rows.n, din = P.din, dout = P.dout;
  if (g.on && !us_done) {   // us_done: the kernel that produced x has formed us = s x . Ag^T on the way (swiglu_rank_fwd)
    GemmParamsT<AT> q = gp<AT>(x, din, g.d.Ag, din, us, g.d.RP, T, g.d.RP, din);
    q.alpha = g.d.scale;
    slot_mask(ctx, g, rows, false, q.mask_width, q.mask_nslot, q.mask_ends);   // applied where the output is rounded
    if (!(whatif() & 8)) CTX_RC(run_gemm(ctx, q));
  }
  GemmParamsT<AT> p = gp<AT>(x, din, P.W, din, y, dout, T, dout, din);
  if (g.on) { p.A2 = us; p.lda2 = g.d.RP; p.B2 = g.d.Bg; p.ldb2 = g.d.RP; p.K2 = g.d.RP; k2_slots(ctx, p, g, rows); }
  p.R = R; p.ldr = dout;
  p.bias = bias;
  return run_gemm(ctx, p);
}

// adapter gradients of one module group + du; then dx[T,din] = dy.W (+ du.(sA))
// where linear_bwd puts du = dy . Bg of module group `slot` of a layer (0 down, 1 gate|up, 2 o, 3 q|k|v): with the layer's adapter gradients grouped into one
// launch (or on the side stream) every group keeps its own buffer until that launch has run
template <typename AT>
AT* du_target(CtxT<AT>* ctx, const LoraGroupT<AT>& g, int slot, bool* grouped_out = nullptr, bool* on_side_out = nullptr) {
  static const bool group_env = env_flag("TST_TN_GROUPED", true);   // A/B switch
  const bool grouped = group_env && sizeof(AT) == 2 && g.on && ctx->du4[0] != nullptr;
  // the side stream pays only when the fold has the GPU to itself (tile policy 3: +3.5 % at one fold per GPU); with resident
  // folds the extra streams cost 14 % (97.2 -> 83.4 QA-pairs/s with three folds), like a fourth fold does
  const bool on_side = !grouped && ctx->side != nullptr && gemm_big_tile_level(-1) == 3;
  if (grouped_out) *grouped_out = grouped;
  if (on_side_out) *on_side_out = on_side;
  return (on_side || grouped) ? ctx->du4[slot] : ctx->du;
}

// sums-of-squares slots of one weight-gradient matrix (tst_ctx::gn_partial): one per 256x256 tile + 16 per possible tail tile (at most 128)
inline int64_t gn_slots(int dout, int din) { return (int64_t)tst_ceil_div(dout, 256) * tst_ceil_div(din, 256) + 2048; }

template <typename AT>
int linear_bwd(CtxT<AT>* ctx, const AT* dy, const AT* x, const ProjT<AT>& P, const AT* us, AT* dx, const Rows& rows, float* dW = nullptr, int slot = 0,
               bool need_dx = true, bool du_done = false) {
  const LoraGroupT<AT>& g = *P.g;
  const int T = rows.n, din = P.din, dout = P.dout;
  // full fine-tune: dW[dout,din] = dy^T . x (fp32, written straight into the flat gradient buffer). Both factors are large and the contraction axis
  // (tokens) is short. Round 5: the TN member of the 256x256 ping-pong tile contracts the row-major activations as they are (rows >= T of the last k-tile
  // are out of range of its buffer descriptor and read as zeros). Before (ctx->kmajor bit 1 off, strict mode): both activations transposed into zero-padded
  // [cols, Tp] copies (~0.3 GB of traffic per layer) + the NT member on them; the 128x128 TN tiles of gemm.hip reach only ~320 TFLOP/s on these shapes.
  if (dW) {
    const int64_t slots = gn_slots(dout, din);
    float* ssq = (ctx->gn_fused && ctx->gn_used + slots <= ctx->gn_cap) ? ctx->gn_partial + ctx->gn_used : nullptr;
    if (!ssq) ctx->gn_fused = false;
    ctx->gn_used += slots;
    bool in_epilogue = false;
    // The weight gradient is not on the dX chain: it runs on the SIDE stream (transposes, contraction, its sums of squares) while the main stream goes on
    // with dX -- whose 80-tile grids at one micro-batch leave two thirds of the CUs idle -- and is joined once per layer, before the layer's dy buffers are
    // overwritten (backward()). Same kernels on the same operands: bit-identical to the single-stream order (TST_FULL_DW_SIDE=0).
    const bool ws = ctx->dw_side && ctx->full && ctx->side != nullptr;
    hipStream_t wst = ws ? ctx->side : ctx->stream;
    if (ws) {
      CTX_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));          // dy is complete (x has been since the forward)
      CTX_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
      ctx->dw_side_open = true;
    }
    bool tn_done = false;
    if constexpr (sizeof(AT) == 2) {
      if ((ctx->kmajor & 2) && T > 256) {
        GemmParams w = gp<AT>(dy, dout, x, din, dW, din, dout, din, roundup(T, 64));
        w.ta = 1; w.tb = 1; w.kvalid = T; w.out_f32 = 1; w.sumsq = ssq; w.no_tail = 1;
        if (gemm_pp_kmajor_supported(w)) {
          CTX_RC(run_gemm_kmajor(ctx, w, ws, 1, 2.0 * dout * din * (double)T, "TN"));
          tn_done = true;
          in_epilogue = true;   // (unsplit: the tile epilogues wrote the sums of squares)
        }
      }
    }
    if (tn_done) {
    } else if (ctx->dyT && T > 256) {
      const int Tp = roundup(T, 64);
      CTX_RC(transpose_mat<AT>(wst, dy, dout, ctx->dyT, Tp, T, dout, Tp));
      CTX_RC(transpose_mat<AT>(wst, x, din, ctx->xT, Tp, T, din, Tp));
      GemmParamsT<AT> w = gp<AT>(ctx->dyT, Tp, ctx->xT, Tp, dW, din, dout, din, Tp);
      w.out_f32 = 1;
      w.sumsq = ssq;
      CTX_RC(run_gemm(ctx, w, ws));
      in_epilogue = ctx->last_variant == 5 && ctx->last_sk == 1 && gemm_pp_supported(w);   // else gemm_pp falls back to a kernel without the sums
    } else {
      CTX_RC(run_gemm_tn<AT>(ctx, dy, dout, x, din, dW, din, dout, din, T, 1.0f, ws));
    }
    if (ssq && !in_epilogue) CTX_RC(sumsq_partial(wst, dW, (long)dout * din, ssq, 256));   // another tile family wrote dW
  }
  bool grouped, on_side;
  AT* du = du_target(ctx, g, slot, &grouped, &on_side);
  if (g.on) {
    const int RP = g.d.RP;
    // du[T,RP] = dy . Bg  (on the dX chain: it is the second K segment of the dX contraction); du_done: the kernel that produced dy has formed it (swiglu_rank_bwd)
    GemmParamsT<AT> b = gp<AT>(dy, dout, g.d.BgT, dout, du, RP, T, RP, dout);
    slot_mask(ctx, g, rows, false, b.mask_width, b.mask_nslot, b.mask_ends);
    if (!du_done && !(whatif() & 8)) CTX_RC(run_gemm(ctx, b));
    // adapter gradients contract over the token axis of both operands: TN form, no transposed copies; off the dX chain
    if (on_side) {
      CTX_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));          // dy and du are complete
      CTX_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    }
    // dBg[dout,RP] = dy^T . us ;  dAg[RP,din] = s * du^T . x
    // the slot-restricted launch (gemm_tns.hip) instead of general 128 x 128 TN tiles over all tokens and all RP columns; TST_TN_SLOT=0 restores those
    // (A/B, profiles/r03_ab_tn_slot.txt: +0.4 ... +0.8 % with two streams, +1.4 % with one)
    static const bool tns_env = env_flag("TST_TN_SLOT", true);
    bool tns = false;
    if constexpr (sizeof(AT) == 2) {
      if (grouped && tns_env && ((g.d.nmod * g.d.r) & 7) == 0) {
        TnsProblem pb, pa;
        memset(&pb, 0, sizeof(pb));
        pb.rk = us; pb.ldr = RP; pb.rp = RP; pb.wd = dy; pb.ldw = dout; pb.wn = dout; pb.c = g.d.dBg; pb.ldc = RP; pb.w = g.d.nmod * g.d.r; pb.alpha = 1.0f; pb.kind = 1;
        pb.rows_pad = ctx->Tpad_max;
        pa = pb;
        pa.rk = du; pa.wd = x; pa.ldw = din; pa.wn = din; pa.c = g.d.dAg; pa.ldc = din; pa.alpha = g.d.scale; pa.kind = 0;
        if (gemm_tns_supported(pa) && gemm_tns_supported(pb)) {
          ctx->tns_pending.push_back(pb);
          ctx->tns_pending.push_back(pa);
          ctx->tn_pending_flop += 2.0 * T * RP * ((double)dout + din);
          tns = true;
        }
      }
    }
    if (tns) {
    } else if (grouped) {   // issued with the layer's other groups' in one launch (flush_tn): dy, du4[slot], us, x stay valid until then
      GemmParamsT<AT> b1 = gp<AT>(dy, dout, us, RP, g.d.dBg, RP, dout, RP, 0), a1 = gp<AT>(du, RP, x, din, g.d.dAg, din, RP, din, 0);
      b1.kvalid = T; b1.out_f32 = 1; b1.alpha = 1.0f;
      a1.kvalid = T; a1.out_f32 = 1; a1.alpha = g.d.scale;
      ctx->tn_pending.push_back(b1);
      ctx->tn_pending.push_back(a1);
      ctx->tn_pending_flop += 2.0 * T * RP * ((double)dout + din);
    } else {
      CTX_RC(run_gemm_tn<AT>(ctx, dy, dout, us, RP, g.d.dBg, RP, dout, RP, T, 1.0f, on_side));
      CTX_RC(run_gemm_tn<AT>(ctx, du, RP, x, din, g.d.dAg, din, RP, din, T, g.d.scale, on_side));
    }
  }
  if (!need_dx) return TST_OK;   // (the first layer of a LoRA fine-tune: nothing trainable lies below its q|k|v projection)
  if constexpr (sizeof(AT) == 2) {
    if (!P.WT) {   // full fine-tune without W^T copies (ctx->kmajor bit 0): dx = dy . W on the NN member, W[dout][din] as it is stored
      GemmParams q = gp<AT>(dy, dout, P.W, din, dx, din, T, din, dout);
      q.tb = 1; q.no_tail = 1;
      static const int fsk = env_int("TST_FULL_SPLITK", 2);
      if (!(fsk & 2)) q.no_splitk = 1;
      return run_gemm_kmajor(ctx, q, false, -1, 2.0 * T * din * (double)dout, "NN", true);
    }
  }
  GemmParamsT<AT> p = gp<AT>(dy, dout, P.WT, dout, dx, din, T, din, dout);
  if (g.on) { p.A2 = du; p.lda2 = g.d.RP; p.B2 = g.d.AgT; p.ldb2 = g.d.RP; p.K2 = g.d.RP; k2_slots(ctx, p, g, rows); }
  return run_gemm(ctx, p);
}

// what a batch of this context may hold (host_logic.h: plan_batch, plan_generate and the staging / cache layouts)
inline tsthost::BatchLimits batch_limits(const tst_ctx* ctx) { return {ctx->Tmax, ctx->Smax, ctx->Rmax, ctx->V, ctx->cfg.max_position, ctx->ns}; }

int upload_batch(tst_ctx* ctx, const tst_batch* b, bool need_labels, const int32_t* rows, int n_rows) {
  // validation, trimmed token list, positions, labelled-row map and slot boundaries: tsthost::plan_batch (host_logic.h; pure host arithmetic on the caller's
  // buffers, run under AddressSanitizer / UBSan by the CPU self-test). Only the cheap size checks come first: the staging buffer may still be in flight.
  if (!b) return fail(ctx, TST_EINVAL, "null batch");
  if (b->n_tokens <= 0 || b->n_seqs <= 0 || b->n_tokens > ctx->Tmax || b->n_seqs > ctx->Smax) return fail(ctx, TST_EINVAL, "batch exceeds max_tokens/max_seqs or is empty");
  const int T = b->n_tokens;
  ctx->stage_idx ^= 1;
  int* hs = ctx->h_stage[ctx->stage_idx];
  CTX_RC(ctx_event_sync(ctx, ctx->stage_evt[ctx->stage_idx]));  // the copies that last used this buffer have left it
  ctx->cur_stage = hs;
  int* h_ids = hs;
  int* h_pos = h_ids + ctx->Tmax;
  const tsthost::BatchLimits lim = batch_limits(ctx);
  tsthost::BatchPlan plan;
  {
    std::string perr;
    if (tsthost::plan_batch(b, lim, need_labels, ctx->trim_last, rows, n_rows, hs, plan, ctx->row_seq, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
  }
  const bool trim = ctx->trim_last && need_labels && !rows;
  const bool dev_ids = (b->flags & TST_BATCH_DEVICE_IDS) != 0;
  for (int q = 0; q < TST_MAX_STACK; ++q) { ctx->slot_ends.t_end[q] = plan.slot_t_end[q]; ctx->row_ends.t_end[q] = plan.row_end[q]; }
  for (int q = 0; q <= TST_MAX_STACK; ++q) ctx->slot_r0[q] = plan.slot_r0[q];
  ctx->lc_batch_ok = plan.lc_batch_ok;
  const int T_dev = plan.T_dev, S = plan.S, R = plan.R, maxlen = plan.maxlen;
  const double sumsq_len = plan.sumsq_len;
  // ONE host-to-device copy per batch: the device buffers d_ids | d_pos | d_cu | d_lab_idx | d_targets are one allocation laid out like
  // the pinned staging buffer (five small copies per step were five blit dispatches on the context's queue)
  const size_t stage_ints = tsthost::stage_ints(lim);
  if (dev_ids) {
    if (trim) {
      CTX_HIP(hipMemcpyAsync(ctx->d_ids, h_ids, sizeof(int) * stage_ints, hipMemcpyHostToDevice, ctx->stream));   // d_ids = source indices for now
      CTX_RC(ids_gather(ctx->stream, b->input_ids, ctx->d_ids, T_dev, T));
    } else {
      CTX_HIP(hipMemcpyAsync(ctx->d_ids, b->input_ids, sizeof(int) * T, hipMemcpyDeviceToDevice, ctx->stream));
      CTX_HIP(hipMemcpyAsync(ctx->d_pos, h_pos, sizeof(int) * (stage_ints - ctx->Tmax), hipMemcpyHostToDevice, ctx->stream));
    }
    // the host cannot see these ids: validate them (all of the caller's, trimmed ones too) on the device; the flag travels back behind the batch and
    // the next host wait reports it
    CTX_RC(ids_check(ctx->stream, b->input_ids, T, ctx->V, ctx->d_idflag));
    CTX_HIP(hipMemcpyAsync(ctx->h_idflag, ctx->d_idflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    CTX_HIP(hipMemcpyAsync(ctx->d_ids, h_ids, sizeof(int) * stage_ints, hipMemcpyHostToDevice, ctx->stream));
  }
  CTX_HIP(hipEventRecord(ctx->stage_evt[ctx->stage_idx], ctx->stream));
  ctx->cur_T = T_dev; ctx->cur_S = S; ctx->cur_R = R; ctx->cur_maxlen = maxlen; ctx->cur_sumsq_len = sumsq_len;
  return TST_OK;
}

// RMSNorm (Llama / Qwen2; stats = rstd[T]) or LayerNorm (GPT-2; stats = {mean, rstd}[T])
template <typename AT>
int norm_fwd(CtxT<AT>* ctx, const AT* x, const AT* w, const AT* b, AT* y, float* stats, int T) {
  const int slot = prof_begin(ctx, ctx->stream, ctx->prof_hbm);
  const int rc = ctx->gpt2 ? layernorm_fwd<AT>(ctx->stream, x, w, b, y, stats, T, ctx->d, ctx->cfg.rms_norm_eps)
                           : rmsnorm_fwd<AT>(ctx->stream, x, w, y, stats, T, ctx->d, ctx->cfg.rms_norm_eps);
  prof_end(ctx, ctx->stream, slot, PROF_NORM, 1, 2.0 * T * ctx->d * sizeof(AT));   // read x, write y
  return rc;
}
template <typename AT>
int norm_bwd(CtxT<AT>* ctx, const AT* dy, const AT* x, const float* stats, const AT* w, const AT* dres, AT* dx, int T) {
  const int slot = prof_begin(ctx, ctx->stream, ctx->prof_hbm);
  const int rc = ctx->gpt2 ? layernorm_bwd<AT>(ctx->stream, dy, x, stats, w, dres, dx, T, ctx->d) : rmsnorm_bwd<AT>(ctx->stream, dy, x, stats, w, dres, dx, T, ctx->d);
  prof_end(ctx, ctx->stream, slot, PROF_NORM, 1, (dres ? 4.0 : 3.0) * T * ctx->d * sizeof(AT));   // read dy, x (, dres), write dx
  return rc;
}
// RMSNorm forward with the rank-axis contraction of the module group that reads the normed stream (norm_rank.hip: u = s . xn . Ag^T in the norm's own pass).
// Returns true when the fused kernel ran (the caller then passes us_done to linear_fwd). ctx->nrk ("norm_rank", env TST_NRK): 1 = on (default), 0 = the norm and
// gemm_rank as two launches; xn and rstd are bit-identical either way (rmsnorm_fwd routes the same widths through the same kernel), us sums the same products in another order
template <typename AT>
bool norm_rank_fwd(CtxT<AT>* ctx, const AT* x, const AT* w, AT* y, float* stats, const Rows& rows, const LoraGroupT<AT>& g, AT* us, int* rc_out) {
  *rc_out = TST_OK;
  if constexpr (sizeof(AT) != 2) return false;
  else {
    if (!ctx->nrk || ctx->gpt2 || ctx->full || !g.on || whatif()) return false;
    NormRank r;
    memset(&r, 0, sizeof(r));
    r.B = g.d.Ag; r.ldb = ctx->d; r.C = us; r.N = g.d.RP; r.alpha = g.d.scale;
    const int T = rows.n;
    slot_mask(ctx, g, rows, true, r.mask_width, r.mask_nslot, r.mask_ends);
    if (ctx->ns == 1) r.mask_ends.t_end[0] = T;   // (one slot: all rows)
    if (!rmsnorm_rank_supported(T, ctx->d, &r)) return false;
    const int slot = prof_begin(ctx, ctx->stream, ctx->prof_hbm);
    *rc_out = rmsnorm_rank_fwd(ctx->stream, x, w, y, stats, T, ctx->d, ctx->cfg.rms_norm_eps, &r);
    prof_end(ctx, ctx->stream, slot, PROF_NORM, 1, 2.0 * T * ctx->d * sizeof(AT));
    return true;
  }
}
// (the norm-weight gradients stay on the main stream: beside the weight gradients on the side stream they made IT the longer one, profiles/r04_full_overlap_ab.txt block 7)
// which = 0 (MLP norm) / 1 (attention norm): with "ndw_side" (env TST_NDW_SIDE; an A/B switch, off by default: measured negative again in round 5) the layer's two
// norm-weight reductions (two launches each) run beside the weight gradients on the side stream, with scratch of their own. dy of both is ctx->dxn: ev_ndw[which] tells the main stream when the
// side stream has read it (backward() waits right before the next contraction that overwrites dxn). which < 0: on the main stream (final norm).
template <typename AT>
int norm_dw(CtxT<AT>* ctx, const AT* dy, const AT* x, const float* stats, float* dw, float* db, int T, int which = -1) {
  hipStream_t st = ctx->stream;
  float* ws = ctx->colred_ws;
  const bool side = which >= 0 && ctx->ndw_side && ctx->full && ctx->dw_side && ctx->side != nullptr && ctx->colred_ws_side != nullptr;
  if (side) {
    CTX_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));   // dy (dxn) is complete
    CTX_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    st = ctx->side;
    ws = ctx->colred_ws_side;
  }
  const int rc = ctx->gpt2 ? layernorm_dwdb<AT>(st, dy, x, stats, dw, db, T, ctx->d, ws) : rmsnorm_dw<AT>(st, dy, x, stats, dw, T, ctx->d, ws);
  if (side && rc == TST_OK) {
    CTX_HIP(hipEventRecord(ctx->ev_ndw[which], ctx->side));
    ctx->ndw_open[which] = true;
  }
  return rc;
}
// full fine-tune, bf16, RMSNorm: the norm backward and the norm-weight gradient as ONE pass over dy and x (norm_rank.hip rmsnorm_bwd_dw) + the ordered finish, instead
// of rmsnorm_dw_kernel + colred_finish + rmsnorm_bwd_kernel. Returns true when it ran. "norm_bwd_dw" (env TST_NBDW), default on; not with "ndw_side".
template <typename AT>
bool norm_bwd_dw(CtxT<AT>* ctx, const AT* dy, const AT* x, const float* stats, const AT* w, const AT* dres, AT* dx, float* dw, int T, int* rc_out) {
  *rc_out = TST_OK;
  if constexpr (sizeof(AT) != 2) return false;
  else {
    if (!ctx->nbdw || !ctx->full || ctx->gpt2 || ctx->ndw_side || !dw || !rmsnorm_rank_width_ok(ctx->d)) return false;
    const int slot = prof_begin(ctx, ctx->stream, ctx->prof_hbm);
    *rc_out = rmsnorm_bwd_dw(ctx->stream, dy, x, stats, w, dres, dx, dw, T, ctx->d, ctx->colred_ws);
    prof_end(ctx, ctx->stream, slot, PROF_NORM, 1, (dres ? 4.0 : 3.0) * T * ctx->d * sizeof(AT));
    return true;
  }
}
// the main stream is about to overwrite ctx->dxn: the side stream's norm-weight reduction `which` must have read it
template <typename AT>
int ndw_wait(CtxT<AT>* ctx, int which) {
  if (!ctx->ndw_open[which]) return TST_OK;
  CTX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_ndw[which], 0));
  ctx->ndw_open[which] = false;
  return TST_OK;
}

// RoPE inside the attention kernels for this batch? (bf16 path only: the fp32 strict kernels keep the stand-alone pass)
template <typename AT>
bool rope_fused(const CtxT<AT>* ctx) {
  if constexpr (sizeof(AT) == 2) return attn_rope_fusable(ctx->cur_maxlen, ctx->dh);
  return false;
}

// The half of a layer behind the attention -- o projection, MLP norm, gate|up projection, SwiGLU / GELU, down projection -- runs on the layer's token rows or,
// for the compacted last layer, on the gathered labelled rows: the same schedule on another set of buffers.
template <typename AT>
struct TailBufsT {
  AT *attn, *x_in, *hmid, *xn2, *gu, *act, *us_o, *us_gu, *us_d;   // stash
  float* rstd2;
  AT* out;                                  // forward: the layer's output rows
  AT *dout, *dact, *dgu, *dxn, *dH, *dattn; // backward: gradient of the output rows (read) and the scratch down to the attention output's gradient
};
template <typename AT>
TailBufsT<AT> token_tail(CtxT<AT>* ctx, LayerT<AT>& A, AT* x_in = nullptr, AT* x_out = nullptr) {   // (backward reads neither x_in nor out)
  return {A.attn, x_in, A.hmid, A.xn2, A.gu, A.act, A.us_o, A.us_gu, A.us_d, A.rstd2, x_out, ctx->dX, ctx->dact, ctx->dgu, ctx->dxn, ctx->dH, ctx->dattn_b};
}
// compact rows: the layer's output lands in xg, where head_forward / the final norm's backward expect the head's input rows, and dxg IS the gradient of those rows
template <typename AT>
TailBufsT<AT> compact_tail(CtxT<AT>* ctx) {
  return {ctx->lc_attn, ctx->lc_xin, ctx->lc_hmid, ctx->lc_xn2, ctx->lc_gu, ctx->lc_act, ctx->lc_us_o, ctx->lc_us_gu, ctx->lc_us_d, ctx->lc_rstd2, ctx->xg,
          ctx->dxg, ctx->lc_dact, ctx->lc_dgu, ctx->lc_dxn, ctx->lc_dH, ctx->lc_dattn};
}

// hmid = x_in + o(attn); out = hmid + down(act(gate|up(norm(hmid))))
template <typename AT>
int tail_fwd(CtxT<AT>* ctx, LayerT<AT>& W, const Rows& rows, const TailBufsT<AT>& B) {
  hipStream_t st = ctx->stream;
  const int n = rows.n;
  CTX_RC(linear_fwd<AT>(ctx, B.attn, W.proj[P_O], B.us_o, B.x_in, B.hmid, rows, W.bo));
  bool u_gu = false;
  if (!rows.compact) {   // compact rows: always the plain norm kernel followed by the rank contraction (the fused kernel there is an unmeasured question)
    int nrc = TST_OK;
    u_gu = norm_rank_fwd<AT>(ctx, B.hmid, W.mlp_norm, B.xn2, B.rstd2, rows, W.g_gu, B.us_gu, &nrc);   // xn2 AND the gate|up group's u
    CTX_RC(nrc);
  }
  if (!u_gu && !(whatif() & 1)) CTX_RC(norm_fwd<AT>(ctx, B.hmid, W.mlp_norm, W.mlp_norm_b, B.xn2, B.rstd2, n));
  CTX_RC(linear_fwd<AT>(ctx, B.xn2, W.proj[P_GU], B.us_gu, nullptr, B.gu, rows, W.bgu, u_gu));
  bool us_done = false;
  if (ctx->gpt2) CTX_RC(gelu_fwd<AT>(st, B.gu, B.act, (long)n * ctx->F));
  else {
    const int slot = prof_begin(ctx, st, ctx->prof_hbm && !rows.compact);   // compact rows: no bracket (the SwiGLU class of the measurement hooks counts token-row launches)
    SwiRank sr;
    if (swr_setup<AT>(ctx, W.g_d, false, rows, B.us_d, sr)) {   // act AND the down projection's us = s act . Ag^T in one pass over gate | up
      if constexpr (sizeof(AT) == 2) CTX_RC(swiglu_rank_fwd(st, B.gu, B.act, n, ctx->F, sr));
      us_done = true;
    } else if (!(whatif() & 4)) CTX_RC(swiglu_fwd<AT>(st, B.gu, B.act, n, ctx->F));
    prof_end(ctx, st, slot, PROF_SWIGLU, 1, 3.0 * n * ctx->F * sizeof(AT));   // read gate, up; write act
  }
  return linear_fwd<AT>(ctx, B.act, W.proj[P_D], B.us_d, B.hmid, B.out, rows, W.bd, us_done);
}

// what a generation asks of forward(): mode 0 = the graph every other entry point runs; 1 = the prefill (RoPE as its own pass, k | v of every layer appended to
// the cache); 2 = decode step `step` (one row per sequence, positions from d_pos, attn_decode against the cache). shared: a sampled generation -- gen_dev
// holds plan_sample's image, a decode row attends to its prompt's shared rows and its own tail (attn_decode_shared)
// mode 3 = the extend pass of a candidate scoring: a decode step over the rows "candidate c, position p", k | v rows and geometry from cand_dev, all positions
// of a candidate in one attention launch (attn_extend)
struct GenPass {
  int mode = 0, step = 0;
  bool shared = false;
};

// what an attribution asks of its passes. backward: true = backward() is seeded by attr_seed instead of the loss gradient, forms the gradient of layer 0's input in
// LoRA contexts too and no embedding gradient. interp: forward() writes layer 0's input with embed_interp at alpha, on the path from the baseline prompt's
// embeddings (ig_dev) to the real ones (the passes of tst_attribute_ig_async), instead of the embedding gather.
struct AttrPass {
  bool backward = false, interp = false;
  float alpha = 1.0f;
};

// forward through the decoder stack; stash=true keeps per-layer activations for the backward pass
template <typename AT>
int forward(CtxT<AT>* ctx, bool stash, GenPass gen = {}, AttrPass ap = {}) {
  const int T = ctx->cur_T, d = ctx->d;
  hipStream_t st = ctx->stream;
  const float scale = 1.0f / sqrtf((float)ctx->dh);
  const Rows rows = token_rows(ctx);
  LayerT<AT>& L0 = ctx->layers[0];
  // (R rows of ~T / 40 in the diagnostic's batches; a batch labelled on most of its tokens gains nothing from the gathers)
  ctx->lc_used = ctx->lc_on && ctx->lc_batch_ok && ctx->cur_R > 0 && 2 * ctx->cur_R <= T;
  whatif_tick();   // (process-wide: the bench's contexts step in turn)
  CTX_RC(opt_need(ctx, 1));   // norm vectors / biases and the embedding side of a pending optimizer step
  // (an integrated-gradients pass enters the stack on the path from the baseline prompt's embeddings to the real ones; everything behind the embedding is unchanged)
  if (ap.interp) CTX_RC(embed_interp<AT>(st, ctx->d_ids, (const int*)ctx->ig_dev, ctx->d_pos, ctx->embed, ctx->gpt2 ? ctx->wpe : (const AT*)nullptr, L0.x_in, T, d, ctx->V,
                                         ctx->npos, ap.alpha));
  else if (ctx->gpt2) CTX_RC(embed_pos_fwd<AT>(st, ctx->d_ids, ctx->d_pos, ctx->embed, ctx->wpe, L0.x_in, T, d, ctx->V, ctx->npos));
  else CTX_RC(embed_fwd<AT>(st, ctx->d_ids, ctx->embed, L0.x_in, T, d, ctx->V));
  for (int l = 0; l < ctx->L; ++l) {
    LayerT<AT>& W = ctx->layers[l];
    LayerT<AT>& A = stash ? ctx->layers[l] : ctx->layers[0];  // activation slots
    AT* x_in = stash ? W.x_in : (l & 1 ? ctx->x_last : L0.x_in);
    AT* x_out = stash ? (l + 1 < ctx->L ? ctx->layers[l + 1].x_in : ctx->x_last) : (l & 1 ? L0.x_in : ctx->x_last);
    CTX_RC(opt_need(ctx, 2 + (size_t)l));   // this layer's matrices
    bool u_qkv = false;
    {
      int nrc = TST_OK;
      u_qkv = norm_rank_fwd<AT>(ctx, x_in, W.attn_norm, A.xn1, A.rstd1, rows, W.g_qkv, A.us_qkv, &nrc);   // xn1 AND the q|k|v group's u in one pass
      CTX_RC(nrc);
    }
    if (!u_qkv && !(whatif() & 1)) CTX_RC(norm_fwd<AT>(ctx, x_in, W.attn_norm, W.attn_norm_b, A.xn1, A.rstd1, T));
    CTX_RC(linear_fwd<AT>(ctx, A.xn1, W.proj[P_QKV], A.us_qkv, nullptr, A.qkv, rows, W.bqkv, u_qkv));
    // RoPE: inside the attention kernels where they can (bf16 path, sequences <= 128 tokens: q and k then stay UN-rotated in the stash and
    // the backward kernel rotates dq / dk back itself), else as a pass of its own over q and k
    // (a generation keeps the rotation a pass of its own: the cache takes k as attention reads it, and kv_append stays a copy)
    const bool rope_in = !ctx->gpt2 && !gen.mode && rope_fused(ctx);
    if (ctx->qk_norm) {
      // Qwen3: head norm in place on q|k, and the rotation in the same traversal whenever RoPE is a pass of its own (q|k read and written once, not twice)
      const int slot = prof_begin(ctx, st, ctx->prof_hbm);
      CTX_RC(head_norm_fwd<AT>(st, A.qkv, ctx->dqkv, W.q_norm, W.k_norm, A.rstd_qk, stash ? A.qk_raw : nullptr, T, ctx->H, ctx->Hkv, ctx->cfg.rms_norm_eps,
                               rope_in ? nullptr : ctx->d_pos, ctx->cosT, ctx->sinT));
      prof_end(ctx, st, slot, PROF_NORM, 1, (stash ? 3.0 : 2.0) * T * (ctx->dq + ctx->dkv) * sizeof(AT));
    } else
    if (!ctx->gpt2 && !rope_in) CTX_RC(rope_apply<AT>(st, A.qkv, ctx->d_pos, ctx->cosT, ctx->sinT, T, ctx->H + ctx->Hkv, ctx->dh, ctx->dqkv, 0));
    if (gen.mode) {
      // generation: this layer's k | v rows join the cache here -- behind the head norm and RoPE, before the activation slot is reused by the next layer
      const long wkv = (long)ctx->Hkv * ctx->dh;
      AT* kc = (AT*)ctx->gen_kv + (long)l * 2 * ctx->gen_rows * wkv;
      AT* vc = kc + ctx->gen_rows * wkv;
      const int S = ctx->cur_S;
      const long o_pre = gen.shared ? (long)tsthost::sample_off_prefill(batch_limits(ctx)) : 3 + 2 * ctx->Smax;
      const int* krows = gen.mode == 3 ? ctx->cand_dev + (long)tsthost::cand_off_rows(batch_limits(ctx))
                                       : ctx->gen_dev + o_pre + (gen.mode == 1 ? 0L : ctx->Tmax + (long)(gen.step - 1) * S);
      CTX_RC(kv_append<AT>(st, A.qkv, ctx->dqkv, ctx->dq, krows, kc, vc, T, ctx->Hkv, ctx->dh, ctx->gen_rows));
      if (gen.mode == 2) {
        const int slot = prof_begin(ctx, st, ctx->prof_hbm);
        if (gen.shared)
          CTX_RC(attn_decode_shared<AT>(st, A.qkv, ctx->dqkv, kc, vc, ctx->gen_dev, S, gen.step, A.attn, ctx->dattn, ctx->H, ctx->Hkv, ctx->dh, scale, ctx->gen_rows));
        else
        CTX_RC(attn_decode<AT>(st, A.qkv, ctx->dqkv, kc, vc, ctx->gen_dev, S, gen.step, A.attn, ctx->dattn, ctx->H, ctx->Hkv, ctx->dh, scale, ctx->gen_rows));
        prof_end(ctx, st, slot, PROF_ATTN, 1, 4.0 * ctx->cur_sumsq_len * ctx->H * ctx->dh);   // q . K^T + P . V over the cached keys (cur_sumsq_len = their count)
      } else if (gen.mode == 3) {
        const int slot = prof_begin(ctx, st, ctx->prof_hbm);
        CTX_RC(attn_extend<AT>(st, A.qkv, ctx->dqkv, kc, vc, ctx->cand_dev, ctx->cand_n_ext, T, A.attn, ctx->dattn, ctx->H, ctx->Hkv, ctx->dh, scale, ctx->gen_rows));
        prof_end(ctx, st, slot, PROF_ATTN, 1, 4.0 * ctx->cur_sumsq_len * ctx->H * ctx->dh);
      }
    }
    if (gen.mode < 2) {
      const int slot = prof_begin(ctx, st, ctx->prof_hbm);
      if (whatif() & 2) {
      } else if constexpr (sizeof(AT) == 2)
        CTX_RC(attn_fwd(st, A.qkv, ctx->dqkv, ctx->d_cu, ctx->cur_S, ctx->cur_maxlen, A.attn, ctx->dattn, A.lse, T, ctx->H, ctx->Hkv, ctx->dh, scale,
                        rope_in ? ctx->cosT : nullptr, rope_in ? ctx->sinT : nullptr, attn_order_on() ? ctx->d_order : nullptr));
      else
      CTX_RC(attn_fwd(st, A.qkv, ctx->dqkv, ctx->d_cu, ctx->cur_S, ctx->cur_maxlen, A.attn, ctx->dattn, A.lse, T, ctx->H, ctx->Hkv, ctx->dh, scale));
      prof_end(ctx, st, slot, PROF_ATTN, 1, 2.0 * ctx->cur_sumsq_len * ctx->H * ctx->dh);   // causal QK^T + PV: 4 * S^2/2 * dh per head
    }
    if (l == ctx->L - 1 && ctx->lc_used) {
      // last layer: everything behind the attention is row-wise and only the head's rows are read (head_forward gathers exactly these): o projection and
      // MLP on the R gathered rows
      CTX_RC(gather_rows<AT>(st, A.attn, ctx->d_lab_idx, ctx->lc_attn, ctx->cur_R, ctx->dattn, 0));
      CTX_RC(gather_rows<AT>(st, x_in, ctx->d_lab_idx, ctx->lc_xin, ctx->cur_R, d, 0));
      CTX_RC(tail_fwd<AT>(ctx, W, compact_rows(ctx), compact_tail(ctx)));
    } else {
      CTX_RC(tail_fwd<AT>(ctx, W, rows, token_tail(ctx, A, x_in, x_out)));
    }
  }
  return TST_OK;
}

template <typename AT>
AT* final_hidden(CtxT<AT>* ctx, bool stash) {
  if (stash) return ctx->x_last;
  return (ctx->L & 1) ? ctx->x_last : ctx->layers[0].x_in;
}

// final norm + LM head on the selected rows only: logits fp32 [R, V]
template <typename AT>
int head_forward(CtxT<AT>* ctx, bool stash) {
  const int R = ctx->cur_R, d = ctx->d;
  CTX_RC(opt_join(ctx));   // the head (last in the optimizer's order): from here on the stream is behind the whole step
  if (R <= 0) return TST_OK;
  hipStream_t st = ctx->stream;
  if (!ctx->lc_used) CTX_RC(gather_rows<AT>(st, final_hidden(ctx, stash), ctx->d_lab_idx, ctx->xg, R, d, 0));   // (compacted last layer: forward wrote xg itself)
  CTX_RC(norm_fwd<AT>(ctx, ctx->xg, ctx->final_norm, ctx->final_norm_b, ctx->xf, ctx->rstd_f, R));
  GemmParamsT<AT> p = gp<AT>(ctx->xf, d, ctx->lm_head, d, ctx->logits, ctx->Vp, R, ctx->Vp, d);
  p.out_f32 = 1;
  return run_gemm(ctx, p);
}

// data-parallel full fine-tune: the gradient regions [dp_next, upto) are final on the main stream -> all-reduce them in place on the
// communication stream while backward goes on
template <typename AT>
int region_done(CtxT<AT>* ctx, size_t upto) {
  while (ctx->dp_next < upto && ctx->dp_next < ctx->dp_regions.size()) {
    const auto& rg = ctx->dp_regions[ctx->dp_next++];
    CTX_HIP(hipEventRecord(ctx->dp_ev, ctx->stream));
    CTX_HIP(hipStreamWaitEvent(ctx->dp_stream, ctx->dp_ev, 0));
    if (ctx->dp_bf16 && ctx->dp_stage && rg.second <= ctx->dp_stage_elems) {
      // DDP on a bf16 model reduces bf16 gradients (the parameter dtype); here the fp32 gradient is rounded once for the wire and the sum is
      // widened back: every rank ends with the same fp32 values (bf16-representable), the optimizer state stays fp32
      CTX_RC(cast_from_f32<bf16_t>(ctx->dp_stream, ctx->tg + rg.first, ctx->dp_stage, rg.second, 1.0f));
      ctx->dp_n_coll += 1;
      ctx->dp_n_elems += rg.second;
      if (ncclAllReduce(ctx->dp_stage, ctx->dp_stage, (size_t)rg.second, ncclBfloat16, ncclSum, ctx->dp_comm, ctx->dp_stream) != ncclSuccess)
        return fail(ctx, TST_EHIP, "ncclAllReduce (bf16 transport) failed");
      CTX_RC(cast_to_f32<bf16_t>(ctx->dp_stream, ctx->dp_stage, ctx->tg + rg.first, rg.second));
    } else {
      CTX_RC(dp_allreduce(ctx, ctx->tg + rg.first, (size_t)rg.second, ctx->dp_stream));
    }
  }
  return TST_OK;
}
// all regions handed over: the main stream waits for the communication stream
template <typename AT>
int regions_join(CtxT<AT>* ctx) {
  CTX_RC(region_done(ctx, ctx->dp_regions.size()));
  CTX_HIP(hipEventRecord(ctx->dp_done, ctx->dp_stream));
  CTX_HIP(hipStreamWaitEvent(ctx->stream, ctx->dp_done, 0));
  return TST_OK;
}

// the collected adapter-gradient contractions of one layer, as one grouped launch (bf16 path only: tn_pending stays empty otherwise); rows: what they contract over
template <typename AT>
int flush_tn(CtxT<AT>* ctx, const Rows& rows) {
  if (ctx->tn_pending.empty() && ctx->tns_pending.empty()) return TST_OK;
  if (whatif() & 16) { ctx->tn_pending.clear(); ctx->tns_pending.clear(); ctx->tn_pending_flop = 0; return TST_OK; }
  int rc = TST_OK;
  if constexpr (sizeof(AT) == 2) {
    hipStream_t st = ctx->stream;
    const int slot = prof_begin(ctx, st, ctx->prof);
    for (size_t i = 0; i < ctx->tns_pending.size() && rc == TST_OK; i += TST_MAX_GROUPED) {
      const size_t n = ctx->tns_pending.size() - i < TST_MAX_GROUPED ? ctx->tns_pending.size() - i : TST_MAX_GROUPED;
      rc = gemm_tns_grouped(st, ctx->tns_pending.data() + i, (int)n, ctx->ns, *rows.ends);
    }
    for (size_t i = 0; i < ctx->tn_pending.size() && rc == TST_OK; i += TST_MAX_GROUPED) {
      const size_t n = ctx->tn_pending.size() - i < TST_MAX_GROUPED ? ctx->tn_pending.size() - i : TST_MAX_GROUPED;
      rc = gemm_tn_grouped(st, ctx->tn_pending.data() + i, (int)n, ctx->slab, ctx->slab_bytes);
    }
    prof_end(ctx, st, slot, 3, 1, ctx->tn_pending_flop);
  }
  ctx->tn_pending.clear();
  ctx->tns_pending.clear();
  ctx->tn_pending_flop = 0;
  if (rc != TST_OK && ctx->err.empty()) ctx->err = "gemm_tn_grouped / gemm_tns_grouped rc=" + std::to_string(rc);
  return rc;
}

// full fine-tune: the gradient of weight tensor w lives at tg + (w - wb) (the flat buffers share one layout); nullptr otherwise
template <typename AT>
float* grad_of(CtxT<AT>* ctx, const AT* w) { return (ctx->full && w) ? ctx->tg + (w - ctx->wb) : nullptr; }

// backward of tail_fwd: down projection, SwiGLU / GELU, gate|up projection, MLP norm (+ the residual), o projection; leaves dH and the attention output's gradient
template <typename AT>
int tail_bwd(CtxT<AT>* ctx, LayerT<AT>& W, const Rows& rows, const TailBufsT<AT>& B) {
  hipStream_t st = ctx->stream;
  const int n = rows.n, d = ctx->d;
  // compact rows are LoRA only (backward(): lc = lc_used && !full): no bias column sums, no dW, no ndw_wait, no norm_bwd_dw
  const bool full = ctx->full && !rows.compact;
  auto gof = [&](const AT* w) -> float* { return full ? grad_of(ctx, w) : nullptr; };
  // MLP block: out = hmid + down(act)
  if (full && W.bd) CTX_RC(colsum<AT>(st, B.dout, d, gof(W.bd), n, d, ctx->colred_ws));
  CTX_RC(linear_bwd<AT>(ctx, B.dout, B.act, W.proj[P_D], B.us_d, B.dact, rows, gof(W.proj[P_D].W), 0));
  bool du_done = false;
  if (ctx->gpt2) CTX_RC(gelu_bwd<AT>(st, B.dact, B.gu, B.dgu, (long)n * ctx->F));
  else {
    const int slot = prof_begin(ctx, st, ctx->prof_hbm && !rows.compact);   // compact rows: no bracket (as in tail_fwd)
    SwiRank sr;
    if (swr_setup<AT>(ctx, W.g_gu, true, rows, du_target(ctx, W.g_gu, 1), sr)) {   // dgu AND the gate|up projection's du = dgu . Bg in one pass
      if constexpr (sizeof(AT) == 2) CTX_RC(swiglu_rank_bwd(st, B.dact, B.gu, B.dgu, n, ctx->F, sr));
      du_done = true;
    } else if (!(whatif() & 4)) CTX_RC(swiglu_bwd<AT>(st, B.dact, B.gu, B.dgu, n, ctx->F));
    prof_end(ctx, st, slot, PROF_SWIGLU, 1, 5.0 * n * ctx->F * sizeof(AT));   // read dact, gate, up; write dgate, dup
  }
  if (full && W.bgu) CTX_RC(colsum<AT>(st, B.dgu, ctx->Fgu, gof(W.bgu), n, ctx->Fgu, ctx->colred_ws));
  if (full) CTX_RC(ndw_wait(ctx, 1));   // (the previous layer's attention-norm reduction on the side stream reads dxn, which the contraction below overwrites)
  CTX_RC(linear_bwd<AT>(ctx, B.dgu, B.xn2, W.proj[P_GU], B.us_gu, B.dxn, rows, gof(W.proj[P_GU].W), 1, true, du_done));
  {
    int frc = TST_OK;
    if (!norm_bwd_dw<AT>(ctx, B.dxn, B.hmid, B.rstd2, W.mlp_norm, B.dout, B.dH, gof(W.mlp_norm), n, &frc)) {
      if (full) CTX_RC(norm_dw<AT>(ctx, B.dxn, B.hmid, B.rstd2, gof(W.mlp_norm), gof(W.mlp_norm_b), n, 0));
      CTX_RC(norm_bwd<AT>(ctx, B.dxn, B.hmid, B.rstd2, W.mlp_norm, B.dout, B.dH, n));
    }
    CTX_RC(frc);
  }
  // attention block: hmid = x_in + o(attn)
  if (full && W.bo) CTX_RC(colsum<AT>(st, B.dH, d, gof(W.bo), n, d, ctx->colred_ws));
  return linear_bwd<AT>(ctx, B.dH, B.attn, W.proj[P_O], B.us_o, B.dattn, rows, gof(W.proj[P_O].W), 2);
}

// the seed of an attribution's backward pass, and the row statistics its log s(x) is read from: attr_seed over the labelled rows of the current batch
template <typename AT>
int attr_seed_rows(CtxT<AT>* ctx) {
  const int* kinds = (const int*)ctx->attr_dev + ctx->Rmax;
  return attr_seed<AT>(ctx->stream, ctx->logits, ctx->Vp, ctx->d_targets, ctx->attr_dev, kinds, kinds + ctx->Rmax, ctx->attr_nopt, ctx->cur_R, ctx->V, ctx->Vp, ctx->stats,
                       ctx->dlogits, ctx->Vp);
}

// num_items: what the loss is normalised by (one slot); slot_items: per-slot counts of a stacked context (nullptr: every slot by its own labelled rows in this
// batch). reduce_regions: a data-parallel full fine-tune's step -- the gradient regions are all-reduced on the communication stream as backward finishes them
template <typename AT>
int backward(CtxT<AT>* ctx, int num_items, const int32_t* slot_items = nullptr, bool reduce_regions = false, AttrPass ap = {}) {
  const int T = ctx->cur_T, d = ctx->d, R = ctx->cur_R;
  hipStream_t st = ctx->stream;
  const float scale = 1.0f / sqrtf((float)ctx->dh);
  const float inv_items = 1.0f / (float)num_items;
  const bool full = ctx->full;
  // An attribution (attr_forward_backward) is this pass with two differences: the seed is d (sum_i log s(x_i)) / d logits instead of the loss gradient, and the
  // gradient of layer 0's input is formed in LoRA contexts too. The weight- and adapter-gradient contractions stay in: the flat gradient is unspecified afterwards.
  const bool attr = ap.backward;
  CTX_RC(opt_join(ctx));     // (a no-op behind head_forward: backward overwrites the gradient a pending optimizer step reads)
  ctx->dw_side_open = false;
  ctx->ndw_open[0] = ctx->ndw_open[1] = false;
  ctx->in_backward = true;
  struct Leave { tst_ctx* c; ~Leave() { c->in_backward = false; } } leave{ctx};
  ctx->tn_pending.clear();   // (a previous backward that failed half-way may have left entries)
  ctx->tns_pending.clear();
  ctx->tn_pending_flop = 0;
  auto gof = [&](const AT* w) -> float* { return grad_of(ctx, w); };
  const Rows rows = token_rows(ctx);
  if (full) {
    ctx->gn_fused = ctx->gn_partial != nullptr && !reduce_regions;
    ctx->gn_used = 0;
    if (ctx->gn_fused) CTX_HIP(hipMemsetAsync(ctx->gn_partial, 0, (size_t)ctx->gn_cap * sizeof(float), st));
    // regions that are accumulated with atomics start from zero: embedding rows and the norm vectors
    // (GPT-2: the token-embedding gradient starts as the tied head's dW, written below, so only wpe is cleared)
    // (an attribution reads dX itself and forms no embedding gradient: nothing to clear)
    if (attr) {
    } else if (ctx->gpt2) CTX_HIP(hipMemsetAsync(gof(ctx->wpe), 0, (size_t)ctx->npos * d * sizeof(float), st));
    else CTX_HIP(hipMemsetAsync(gof(ctx->embed), 0, (size_t)ctx->Vp * d * sizeof(float), st));
    CTX_HIP(hipMemsetAsync(ctx->tg + ctx->n_decay, 0, (size_t)(ctx->n_train - ctx->n_decay) * sizeof(float), st));
  }
  if (attr) {
    CTX_RC(attr_seed_rows(ctx));
  } else if (ctx->ns == 1) {
    CTX_RC(logit_rows<AT>(st, ctx->logits, ctx->Vp, ctx->d_targets, R, ctx->V, ctx->stats, ctx->dlogits, ctx->Vp, inv_items, nullptr, 0, nullptr));
    CTX_RC(loss_reduce(st, ctx->stats, R, inv_items, ctx->d_loss));
  } else {
    // every stacked fold has its own loss: mean over ITS labelled rows (the rows of a slot are contiguous)
    CTX_HIP(hipMemsetAsync(ctx->d_loss, 0, sizeof(float) * TST_MAX_STACK, st));
    for (int sl = 0; sl < ctx->ns; ++sl) {
      const int r0 = ctx->slot_r0[sl], Rs = ctx->slot_r0[sl + 1] - r0;
      if (Rs <= 0) continue;
      const float inv = 1.0f / (float)(slot_items ? slot_items[sl] : Rs);   // (checked > 0 by the caller)
      CTX_RC(logit_rows<AT>(st, ctx->logits + (long)r0 * ctx->Vp, ctx->Vp, ctx->d_targets + r0, Rs, ctx->V, ctx->stats + 4L * r0, ctx->dlogits + (long)r0 * ctx->Vp,
                        ctx->Vp, inv, nullptr, 0, nullptr));
      CTX_RC(loss_reduce(st, ctx->stats + 4L * r0, Rs, inv, ctx->d_loss + sl));
    }
  }
  // d lm_head[V,d] = dlogits^T . xf   (contraction over the labelled rows)
  if (full) CTX_RC(run_gemm_tn<AT>(ctx, ctx->dlogits, ctx->Vp, ctx->xf, d, gof(ctx->lm_head), d, ctx->Vp, d, R, 1.0f));
  const bool regions = full && reduce_regions && !ctx->dp_regions.empty();
  const size_t r_head = (regions && !ctx->gpt2) ? 1 : 0;   // region 0 = lm_head (a tied head goes with the embedding, at the end)
  if (regions) { ctx->dp_next = 0; CTX_RC(region_done(ctx, r_head)); }
  // d xf = dlogits . lm_head
  bool dxf_done = false;
  if constexpr (sizeof(AT) == 2) {
    if (!ctx->lm_headT) {   // (ctx->kmajor bit 0) the NN member on the stored head [Vp][d]; few rows and a long K: split over K to cover the CUs
      GemmParams q = gp<AT>(ctx->dlogits, ctx->Vp, ctx->lm_head, d, ctx->dxf, d, R, d, ctx->Vp);
      q.tb = 1; q.no_tail = 1;
      const int tiles = tst_ceil_div(R, 256) * tst_ceil_div(d, 256);
      int sk = 256 / tiles;
      sk = sk < 1 ? 1 : (sk > 16 ? 16 : sk);
      CTX_RC(run_gemm_kmajor(ctx, q, false, sk, 2.0 * R * d * (double)ctx->Vp, "NN, head"));
      dxf_done = true;
    }
  }
  if (!dxf_done) CTX_RC(run_gemm(ctx, gp<AT>(ctx->dlogits, ctx->Vp, ctx->lm_headT, ctx->Vp, ctx->dxf, d, R, d, ctx->Vp)));
  {
    int frc = TST_OK;
    if (!norm_bwd_dw<AT>(ctx, ctx->dxf, ctx->xg, ctx->rstd_f, ctx->final_norm, nullptr, ctx->dxg, gof(ctx->final_norm), R, &frc)) {
      if (full) CTX_RC(norm_dw<AT>(ctx, ctx->dxf, ctx->xg, ctx->rstd_f, gof(ctx->final_norm), gof(ctx->final_norm_b), R));
      CTX_RC(norm_bwd<AT>(ctx, ctx->dxf, ctx->xg, ctx->rstd_f, ctx->final_norm, nullptr, ctx->dxg, R));
    }
    CTX_RC(frc);
  }
  const bool lc = ctx->lc_used && !full;
  if (!lc) {
    CTX_HIP(hipMemsetAsync(ctx->dX, 0, (size_t)T * d * sizeof(AT), st));
    CTX_RC(gather_rows<AT>(st, ctx->dxg, ctx->d_lab_idx, ctx->dX, R, d, 1));
  }
  for (int l = ctx->L - 1; l >= 0; --l) {
    LayerT<AT>& W = ctx->layers[l];
    if (lc && l == ctx->L - 1) {
      // the compacted last layer (forward): MLP and o projection backward on its R rows, then the rows go back to their token positions in front of the
      // attention backward (zeros elsewhere: no other row of this layer's output is read)
      const TailBufsT<AT> B = compact_tail(ctx);
      CTX_RC(tail_bwd<AT>(ctx, W, compact_rows(ctx), B));
      CTX_RC(flush_tn(ctx, compact_rows(ctx)));   // these three groups contract over the compact rows: their own launch, with the rows' slot boundaries
      CTX_HIP(hipMemsetAsync(ctx->dattn_b, 0, (size_t)T * ctx->dattn * sizeof(AT), st));
      CTX_RC(gather_rows<AT>(st, B.dattn, ctx->d_lab_idx, ctx->dattn_b, R, ctx->dattn, 1));
      CTX_HIP(hipMemsetAsync(ctx->dH, 0, (size_t)T * d * sizeof(AT), st));
      CTX_RC(gather_rows<AT>(st, B.dH, ctx->d_lab_idx, ctx->dH, R, d, 1));
    } else {
      CTX_RC(tail_bwd<AT>(ctx, W, rows, token_tail(ctx, W)));
    }
    const bool rope_in = !ctx->gpt2 && rope_fused(ctx);   // (the same answer as in this step's forward: same batch, process-wide switches)
    const bool attn_order = attn_order_on();
    if (whatif() & 2) {
    } else if constexpr (sizeof(AT) == 2)
      CTX_RC(attn_bwd(st, W.qkv, ctx->dqkv, W.attn, ctx->dattn, ctx->dattn_b, ctx->dattn, W.lse, ctx->delta, ctx->d_cu, ctx->cur_S, ctx->cur_maxlen,
                      ctx->dqkv_b, T, ctx->H, ctx->Hkv, ctx->dh, scale, rope_in ? ctx->cosT : nullptr, rope_in ? ctx->sinT : nullptr, attn_order ? ctx->d_order : nullptr));
    else
    CTX_RC(attn_bwd(st, W.qkv, ctx->dqkv, W.attn, ctx->dattn, ctx->dattn_b, ctx->dattn, W.lse, ctx->delta, ctx->d_cu, ctx->cur_S, ctx->cur_maxlen,
                    ctx->dqkv_b, T, ctx->H, ctx->Hkv, ctx->dh, scale));
    if (ctx->qk_norm) {
      // Qwen3: (un-rotate,) head-norm backward in place on dq|dk; a full fine-tune takes the two weight gradients in the same pass
      const int slot = prof_begin(ctx, st, ctx->prof_hbm);
      CTX_RC(head_norm_bwd<AT>(st, ctx->dqkv_b, ctx->dqkv, W.q_norm, W.k_norm, W.rstd_qk, W.qk_raw, T, ctx->H, ctx->Hkv, rope_in ? nullptr : ctx->d_pos, ctx->cosT,
                               ctx->sinT, full ? gof(W.q_norm) : nullptr, full ? gof(W.k_norm) : nullptr, ctx->hn_ws));
      prof_end(ctx, st, slot, PROF_NORM, 1, 3.0 * T * (ctx->dq + ctx->dkv) * sizeof(AT));
    } else
    if (!ctx->gpt2 && !rope_in) CTX_RC(rope_apply<AT>(st, ctx->dqkv_b, ctx->d_pos, ctx->cosT, ctx->sinT, T, ctx->H + ctx->Hkv, ctx->dh, ctx->dqkv, 1));
    if (full && W.bqkv) CTX_RC(colsum<AT>(st, ctx->dqkv_b, ctx->dqkv, gof(W.bqkv), T, ctx->dqkv, ctx->colred_ws));
    // LoRA: the embedding is frozen, so the gradient of layer 0's INPUT has no reader: its q|k|v projection's dX contraction and the norm backward behind it are skipped
    // (an attribution is after exactly that gradient)
    const bool input_grad = full || l > 0 || attr;
    AT* dxq = ctx->dxn;
    CTX_RC(ndw_wait(ctx, 0));   // (this layer's MLP-norm reduction on the side stream reads dxn)
    CTX_RC(linear_bwd<AT>(ctx, ctx->dqkv_b, W.xn1, W.proj[P_QKV], W.us_qkv, dxq, rows, gof(W.proj[P_QKV].W), 3, input_grad));
    CTX_RC(flush_tn(ctx, rows));
    // (this layer's dy buffers (dX, dgu, dH, dqkv_b) and du4 are still intact here)
    if (!full && ctx->side && gemm_big_tile_level(-1) == 3) {
      // join: the side stream still reads this layer's dy buffers (dX, dgu, dH, dqkv_b) and du4; dX is overwritten next, the
      // others and du4 by the next layer
      CTX_HIP(hipEventRecord(ctx->ev_join, ctx->side));
      CTX_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
    }
    if (ctx->dw_side_open) {
      // the side stream still reads this layer's dy buffers (dX, dgu, dH, dqkv_b) for the weight gradients: dX is overwritten next, the others by the next layer
      CTX_HIP(hipEventRecord(ctx->ev_join, ctx->side));
      CTX_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
      ctx->dw_side_open = false;
    }
    {
      int frc = TST_OK;
      if (!(input_grad && norm_bwd_dw<AT>(ctx, dxq, W.x_in, W.rstd1, W.attn_norm, ctx->dH, ctx->dX, gof(W.attn_norm), T, &frc))) {
        if (full) CTX_RC(norm_dw<AT>(ctx, dxq, W.x_in, W.rstd1, gof(W.attn_norm), gof(W.attn_norm_b), T, 1));
        if (input_grad) CTX_RC(norm_bwd<AT>(ctx, dxq, W.x_in, W.rstd1, W.attn_norm, ctx->dH, ctx->dX, T));
      }
      CTX_RC(frc);
    }
    if (regions) CTX_RC(region_done(ctx, r_head + (size_t)(ctx->L - l)));   // this layer's four weight gradients are final
  }
  if (ctx->ndw_open[0] || ctx->ndw_open[1]) {   // the norm-weight gradients still in flight on the side stream: final before anything reads the gradient vector
    CTX_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    CTX_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
    ctx->ndw_open[0] = ctx->ndw_open[1] = false;
  }
  if (full && !attr) CTX_RC(embed_bwd<AT>(st, ctx->d_ids, ctx->dX, gof(ctx->embed), T, d, ctx->V));
  if (full && !attr && ctx->gpt2) CTX_RC(embed_bwd<AT>(st, ctx->d_pos, ctx->dX, gof(ctx->wpe), T, d, ctx->npos));
  if (regions) CTX_RC(regions_join(ctx));   // embedding side and the norm / bias tail, then the main stream waits for the reduction
  CTX_RC(lora_unpack_grad<AT>(st, ctx->descs_dev, (int)ctx->descs.size(), ctx->tg, ctx->pack_max_elems));
  return TST_OK;
}

// W^T copies for the dX contractions (after tst_set_weight / after every optimizer step of a full fine-tune)
template <typename AT>
int refresh_transposes(CtxT<AT>* ctx) {
  hipStream_t st = ctx->stream;
  const int d = ctx->d;
  if (!ctx->lm_headT) return TST_OK;   // (ctx->kmajor bit 0: a full fine-tune that contracts dX against the stored weights keeps no W^T copies)
  CTX_RC(transpose_mat<AT>(st, ctx->lm_head, d, ctx->lm_headT, ctx->Vp, ctx->Vp, d, ctx->Vp));
  for (auto& W : ctx->layers)
    for (const ProjT<AT>& P : W.proj) CTX_RC(transpose_mat<AT>(st, P.W, P.din, P.WT, P.dout, P.dout, P.din, P.dout));
  return TST_OK;
}

// HF state_dict name -> its entry in the context's table (nullptr: the family has no such tensor)
template <typename AT>
const typename CtxT<AT>::Named* find_weight(const CtxT<AT>* ctx, const char* name) {
  for (const auto& t : ctx->named)
    if (t.name == name) return &t;
  return nullptr;
}

// The table's builders, one per naming scheme; every pointer is assigned by now. mat: [rows, cols] as stored; vec: [n] as 1 x n; optional tensors appear where they exist.
// Llama / Qwen2 / Qwen3 (modeling_llama.py; q|k|v and gate|up are fused on the device: the HF tensors are row slices)
template <typename AT>
void name_tensors_llama(CtxT<AT>* ctx) {
  const int d = ctx->d, F = ctx->F, dq = ctx->dq, dkv = ctx->dkv;
  auto add = [&](const std::string& n, AT* p, int64_t rows, int64_t cols) { if (p) ctx->named.push_back({n, p, rows, cols, false, false}); };
  add("model.embed_tokens.weight", ctx->embed, ctx->V, d);
  add("lm_head.weight", ctx->lm_head, ctx->V, d);
  add("model.norm.weight", ctx->final_norm, 1, d);
  for (int l = 0; l < ctx->L; ++l) {
    const LayerT<AT>& W = ctx->layers[l];
    const std::string pre = "model.layers." + std::to_string(l) + ".";
    AT *Wqkv = W.proj[P_QKV].W, *Wgu = W.proj[P_GU].W;
    add(pre + "input_layernorm.weight", W.attn_norm, 1, d);
    add(pre + "post_attention_layernorm.weight", W.mlp_norm, 1, d);
    add(pre + "self_attn.q_proj.weight", Wqkv, dq, d);
    add(pre + "self_attn.k_proj.weight", Wqkv + (int64_t)dq * d, dkv, d);
    add(pre + "self_attn.v_proj.weight", Wqkv + (int64_t)(dq + dkv) * d, dkv, d);
    add(pre + "self_attn.o_proj.weight", W.proj[P_O].W, d, ctx->dattn);
    add(pre + "mlp.gate_proj.weight", Wgu, F, d);
    add(pre + "mlp.up_proj.weight", Wgu + (int64_t)F * d, F, d);
    add(pre + "mlp.down_proj.weight", W.proj[P_D].W, d, F);
    if (W.bqkv) {   // Qwen2
      add(pre + "self_attn.q_proj.bias", W.bqkv, 1, dq);
      add(pre + "self_attn.k_proj.bias", W.bqkv + dq, 1, dkv);
      add(pre + "self_attn.v_proj.bias", W.bqkv + dq + dkv, 1, dkv);
    }
    add(pre + "self_attn.q_norm.weight", W.q_norm, 1, ctx->dh);   // Qwen3
    add(pre + "self_attn.k_norm.weight", W.k_norm, 1, ctx->dh);
  }
}
// GPT-2 (modeling_gpt2.py:486-497, 637-646): Conv1D weights are [in, out] in HF and [out, in] on the device; the head is tied to wte (:638)
template <typename AT>
void name_tensors_gpt2(CtxT<AT>* ctx) {
  const int d = ctx->d;
  auto add = [&](const std::string& n, AT* p, int64_t rows, int64_t cols, bool conv1d = false, bool alias = false) { ctx->named.push_back({n, p, rows, cols, conv1d, alias}); };
  add("transformer.wte.weight", ctx->embed, ctx->V, d);
  add("lm_head.weight", ctx->embed, ctx->V, d, false, true);
  add("transformer.wpe.weight", ctx->wpe, ctx->npos, d);
  add("transformer.ln_f.weight", ctx->final_norm, 1, d);
  add("transformer.ln_f.bias", ctx->final_norm_b, 1, d);
  static const char* const mod[4] = {"attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"};   // P_QKV .. P_D
  for (int l = 0; l < ctx->L; ++l) {
    const LayerT<AT>& W = ctx->layers[l];
    const std::string pre = "transformer.h." + std::to_string(l) + ".";
    AT* const bias[4] = {W.bqkv, W.bo, W.bgu, W.bd};
    add(pre + "ln_1.weight", W.attn_norm, 1, d);
    add(pre + "ln_1.bias", W.attn_norm_b, 1, d);
    add(pre + "ln_2.weight", W.mlp_norm, 1, d);
    add(pre + "ln_2.bias", W.mlp_norm_b, 1, d);
    for (int p = 0; p < 4; ++p) {
      add(pre + mod[p] + ".weight", W.proj[p].W, W.proj[p].dout, W.proj[p].din, true);
      add(pre + mod[p] + ".bias", bias[p], 1, W.proj[p].dout);
    }
  }
}

// ---- construction. build_ctx (below) is the list of these stages; their order is the order of the device allocations, and addresses follow it.
#define ALLOC(dst, type, count) \
  do { dst = palloc<type>(ctx, (int64_t)(count)); if (!dst) return fail(ctx, TST_ENOMEM, "hipMalloc failed: " #dst); } while (0)

inline int head_rows(const tst_ctx* ctx) { return roundup(ctx->Rmax, 64); }   // whole 64-row k-steps are readable (lm_head dW contracts over the labelled rows)
template <typename AT>
int rank_pad_max(const CtxT<AT>* ctx) {   // widest padded rank block of any module group (groups are padded to multiples of 64, at most 3 * 64)
  int rp = 64;
  for (auto& g : ctx->descs) if (g.RP > rp) rp = g.RP;
  return rp;
}
// LoRA: the adapter-gradient contractions get a side stream unless TST_NO_SIDE_STREAM; a full fine-tune's weight gradients always run beside the dX chain
inline bool wants_side_stream(const tst_ctx* ctx) {
  if (ctx->full) return true;
  static const bool no_side = env_flag("TST_NO_SIDE_STREAM", false);
  return !no_side;
}
// dimensions, stated once: host_logic.h model_dims and (full fine-tune) full_layout; the configuration has passed check_cfg
template <typename AT>
int set_dims(CtxT<AT>* ctx) {
  const tst_model_cfg& c = ctx->cfg;
  const tsthost::ModelDims m = ctx->md = tsthost::model_dims(c);
  ctx->d = m.d; ctx->L = m.L; ctx->F = m.F; ctx->Fgu = m.Fgu; ctx->Vp = m.V; ctx->npos = m.npos; ctx->dh = m.dh; ctx->gpt2 = m.gpt2; ctx->qk_norm = m.qk_norm;
  ctx->dq = m.dq; ctx->dkv = m.dkv; ctx->dqkv = m.dqkv; ctx->dattn = m.dattn; ctx->H = c.num_heads; ctx->Hkv = c.num_kv_heads; ctx->V = c.vocab_size;
  ctx->Tmax = c.max_tokens; ctx->Smax = c.max_seqs; ctx->Rmax = c.max_labelled;
  // every [tokens, .] buffer has Tpad_max rows: the TN contractions read whole 64-row k-steps (rows >= n_tokens are
  // masked in-kernel but must be readable and finite, hence the pool's zero fill)
  ctx->Tpad_max = roundup(ctx->Tmax, 64);
  tsthost::proj_dims(m, ctx->proj_dout, ctx->proj_din);
  ctx->full = (c.train_mode == TST_TRAIN_FULL);
  if constexpr (sizeof(AT) == 2) {
    // K-major members for the full fine-tune's backward (tst_ctx::kmajor). Every contraction axis they meet (d_qkv, d, F or 2F, the padded vocabulary) is a
    // multiple of 64 and every free axis a multiple of 8 by check_cfg. TST_KMAJOR = 0 / 1 / 2 / 3 (default 3) is the A/B switch; bit 0 decides what
    // is ALLOCATED (no W^T copies), so it is fixed here
    static const int km_env = env_int("TST_KMAJOR", 3);
    ctx->kmajor = ctx->full ? (km_env & 3) : 0;
  }
  ctx->ns = c.n_stack > 1 ? c.n_stack : 1;
  ctx->zero_on = c.zero_ranks >= 1;
  ctx->zero = ctx->zero_on ? c.zero_ranks : 1;
  ctx->zero_rank = ctx->zero_on ? c.zero_rank : 0;
  if (!ctx->full) return TST_OK;
  const tsthost::FullLayout fl = tsthost::full_layout(m);
  ctx->n_decay = fl.n_decay; ctx->n_train = fl.n_train; ctx->per_layer = fl.per_layer;
  ctx->n_pad = ctx->n_train; ctx->z_lo = 0; ctx->z_hi = ctx->n_train; ctx->z_shard = ctx->n_train;
  if (ctx->zero_on) {
    const tsthost::ZeroShard z = tsthost::zero_shard(ctx->n_train, ctx->zero, ctx->zero_rank);   // (host_logic.h)
    ctx->n_pad = z.n_pad; ctx->z_shard = z.shard; ctx->z_lo = z.lo; ctx->z_hi = z.hi;
  }
  return TST_OK;
}
// Weight storage, one of three. Full fine-tune: one flat buffer in the master's order [embed | per layer Wqkv, Wo, Wgu, Wd | lm_head | norms], every tensor a
// slice of it. Fork: the frozen weights are the parent's (one copy in HBM for all folds). Root: one allocation per tensor. A layer's OWN allocations
// (layer_weights) are made layer by layer, between the previous layer's stash and this layer's module groups.
template <typename AT>
int weight_storage(CtxT<AT>* ctx) {
  const int d = ctx->d, V = ctx->Vp, Fgu = ctx->Fgu;
  const bool gpt2 = ctx->gpt2, qk_norm = ctx->qk_norm, qkv_bias = ctx->md.qkv_bias;
  ctx->layers.resize(ctx->L);
  for (auto& W : ctx->layers) {
    const LoraGroupT<AT>* const groups[4] = {&W.g_qkv, &W.g_o, &W.g_gu, &W.g_d};
    for (int p = 0; p < 4; ++p) { W.proj[p].dout = ctx->proj_dout[p]; W.proj[p].din = ctx->proj_din[p]; W.proj[p].g = groups[p]; }
  }
  if (const CtxT<AT>* sh = ctx->parent) {
    ctx->embed = sh->embed; ctx->lm_head = sh->lm_head; ctx->lm_headT = sh->lm_headT; ctx->final_norm = sh->final_norm; ctx->wpe = sh->wpe; ctx->final_norm_b = sh->final_norm_b;
    for (int l = 0; l < ctx->L; ++l) {
      LayerT<AT>& W = ctx->layers[l];
      const LayerT<AT>& S = sh->layers[l];
      W.attn_norm = S.attn_norm; W.mlp_norm = S.mlp_norm; W.bqkv = S.bqkv; W.q_norm = S.q_norm; W.k_norm = S.k_norm;
      W.attn_norm_b = S.attn_norm_b; W.mlp_norm_b = S.mlp_norm_b; W.bo = S.bo; W.bgu = S.bgu; W.bd = S.bd;
      for (int p = 0; p < 4; ++p) { W.proj[p].W = S.proj[p].W; W.proj[p].WT = S.proj[p].WT; }
    }
    return TST_OK;
  }
  if (!ctx->full) {
    ALLOC(ctx->embed, AT, (int64_t)V * d);
    if (gpt2) { ctx->lm_head = ctx->embed; ALLOC(ctx->wpe, AT, (int64_t)ctx->npos * d); ALLOC(ctx->final_norm_b, AT, d); }   // tied head
    else ALLOC(ctx->lm_head, AT, (int64_t)V * d);
    ALLOC(ctx->lm_headT, AT, (int64_t)V * d);
    ALLOC(ctx->final_norm, AT, d);
    return TST_OK;
  }
  ALLOC(ctx->wb, AT, ctx->n_pad);     // (all-gather target: zero_ranks equal shards)
  ALLOC(ctx->wb0, AT, ctx->n_train);
  int64_t wofs = 0;
  auto take = [&](int64_t n) { AT* p = ctx->wb + wofs; wofs += n; return p; };
  ctx->embed = take((int64_t)V * d);
  if (gpt2) ctx->wpe = take((int64_t)ctx->npos * d);
  for (auto& W : ctx->layers)
    for (auto& P : W.proj) P.W = take(P.numel());
  if (gpt2) ctx->lm_head = ctx->embed;  // tied head: one parameter, its gradient is the sum of both uses
  else ctx->lm_head = take((int64_t)V * d);
  // the no-decay tail, layer by layer: norm vectors and biases (GPT-2: 2 LayerNorms with bias and 4 Conv1D biases, + ln_f)
  for (auto& W : ctx->layers) {
    if (gpt2) {
      W.attn_norm = take(d); W.attn_norm_b = take(d); W.mlp_norm = take(d); W.mlp_norm_b = take(d);
      W.bqkv = take(ctx->dqkv); W.bo = take(d); W.bgu = take(Fgu); W.bd = take(d);
      continue;
    }
    W.attn_norm = take(d); W.mlp_norm = take(d);
    if (qkv_bias) W.bqkv = take(ctx->dqkv);
    // Qwen3 head-norm vectors: with the other norm vectors in the no-decay tail (HF's Trainer excludes every "_norm" parameter from decay)
    if (qk_norm) { W.q_norm = take(ctx->dh); W.k_norm = take(ctx->dh); }
  }
  ctx->final_norm = take(d);
  if (gpt2) ctx->final_norm_b = take(d);
  if (wofs != ctx->n_train) return fail(ctx, TST_ESTATE, "internal: full fine-tune weight layout mismatch");
  // the order of the slices above IS the flat layout; host_logic.h states the same layout as arithmetic (the CPU tests and the region table use it)
  const tsthost::FullLayout fl = tsthost::full_layout(ctx->md);
  if (fl.embed != ctx->embed - ctx->wb || fl.layer0 != ctx->layers[0].proj[P_QKV].W - ctx->wb || fl.lm_head != ctx->lm_head - ctx->wb ||
      (gpt2 && fl.wpe != ctx->wpe - ctx->wb) || fl.tail != ctx->layers[0].attn_norm - ctx->wb)
    return fail(ctx, TST_ESTATE, "internal: full fine-tune layout disagrees with host_logic.h full_layout");
  if (!(ctx->kmajor & 1)) ALLOC(ctx->lm_headT, AT, (int64_t)V * d);
  return TST_OK;
}
template <typename AT>
int layer_weights(CtxT<AT>* ctx, LayerT<AT>& W) {
  const int d = ctx->d;
  if (ctx->parent) return TST_OK;
  if (ctx->full) {
    if (!(ctx->kmajor & 1))   // (else dX = dY . W on the NN member: one copy of every weight)
      for (auto& P : W.proj) ALLOC(P.WT, AT, P.numel());
    return TST_OK;
  }
  ALLOC(W.attn_norm, AT, d); ALLOC(W.mlp_norm, AT, d);
  if (ctx->md.qkv_bias) ALLOC(W.bqkv, AT, ctx->dqkv);
  if (ctx->qk_norm) { ALLOC(W.q_norm, AT, ctx->dh); ALLOC(W.k_norm, AT, ctx->dh); }
  if (ctx->gpt2) {
    ALLOC(W.attn_norm_b, AT, d); ALLOC(W.mlp_norm_b, AT, d);
    ALLOC(W.bo, AT, d); ALLOC(W.bgu, AT, ctx->Fgu); ALLOC(W.bd, AT, d);
  }
  for (auto& P : W.proj) { ALLOC(P.W, AT, P.numel()); ALLOC(P.WT, AT, P.numel()); }
  return TST_OK;
}
// the device side of one module group: its enabled modules and slot 0's offsets come from host_logic.h lora_layout, the other slots' follow once n1 is known (trainables)
template <typename AT>
int add_group(CtxT<AT>* ctx, LoraGroupT<AT>& g, const ProjT<AT>& P, const tsthost::LoraGroupLayout& lay) {
  const int r = ctx->cfg.lora_r, din = P.din, dout = P.dout;
  if (lay.nseg == 0) { g.on = false; return TST_OK; }
  LoraGroupDescT<AT> dsc;
  memset(&dsc, 0, sizeof(dsc));
  for (int m = 0; m < lay.nseg; ++m) { dsc.seg_row0[m] = lay.row0[m]; dsc.seg_row1[m] = lay.row1[m]; dsc.a_off[m] = lay.a_off[m]; dsc.b_off[m] = lay.b_off[m]; }
  dsc.din = din; dsc.dout = dout; dsc.r = r; dsc.nmod = lay.nseg; dsc.nslot = ctx->ns; dsc.nseg = lay.nseg * ctx->ns;
  dsc.RP = roundup(dsc.nseg * r, 64);
  dsc.scale = ctx->cfg.lora_alpha / (float)r;
  ALLOC(dsc.Ag, AT, (int64_t)dsc.RP * din); ALLOC(dsc.AgT, AT, (int64_t)din * dsc.RP);
  ALLOC(dsc.Bg, AT, (int64_t)dout * dsc.RP); ALLOC(dsc.BgT, AT, (int64_t)dsc.RP * dout);
  ALLOC(dsc.dAg, float, (int64_t)dsc.RP * din); ALLOC(dsc.dBg, float, (int64_t)dout * dsc.RP);
  g.on = true; g.d = dsc; g.index = (int)ctx->descs.size();
  ctx->descs.push_back(dsc);
  const long elems = (long)dsc.RP * din + (long)dout * dsc.RP;
  if (elems > ctx->pack_max_elems) ctx->pack_max_elems = elems;
  if (din > ctx->pack_max_long) ctx->pack_max_long = din;
  if (dout > ctx->pack_max_long) ctx->pack_max_long = dout;
  return TST_OK;
}
// per layer: its own weight allocations, its four module groups (LoRA; a full fine-tune has none), its stash
template <typename AT>
int build_layers(CtxT<AT>* ctx) {
  const int d = ctx->d, F = ctx->F, Fgu = ctx->Fgu, T = ctx->Tpad_max;
  tsthost::LoraLayout lay;
  if (!ctx->full) {
    lay = tsthost::lora_layout(ctx->md, ctx->cfg.lora_r, ctx->cfg.lora_targets, ctx->ns);
    ctx->tinfo = lay.entries;
    ctx->n_train = lay.n1;
  }
  for (int l = 0; l < ctx->L; ++l) {
    LayerT<AT>& W = ctx->layers[l];
    LoraGroupT<AT>* const groups[4] = {&W.g_qkv, &W.g_o, &W.g_gu, &W.g_d};
    AT** const us[4] = {&W.us_qkv, &W.us_o, &W.us_gu, &W.us_d};
    CTX_RC(layer_weights(ctx, W));
    if (!ctx->full)
      for (int p = 0; p < 4; ++p) CTX_RC(add_group(ctx, *groups[p], W.proj[p], lay.group[(size_t)4 * l + p]));
    // stash
    ALLOC(W.x_in, AT, (int64_t)T * d); ALLOC(W.xn1, AT, (int64_t)T * d); ALLOC(W.qkv, AT, (int64_t)T * ctx->dqkv);
    ALLOC(W.attn, AT, (int64_t)T * ctx->dattn); ALLOC(W.hmid, AT, (int64_t)T * d); ALLOC(W.xn2, AT, (int64_t)T * d);
    ALLOC(W.gu, AT, (int64_t)T * Fgu); ALLOC(W.act, AT, (int64_t)T * F);
    ALLOC(W.rstd1, float, 2 * T); ALLOC(W.rstd2, float, 2 * T); ALLOC(W.lse, float, (int64_t)ctx->H * T);  // LayerNorm keeps {mean, rstd}
    if (ctx->qk_norm) { ALLOC(W.qk_raw, AT, (int64_t)T * (ctx->dq + ctx->dkv)); ALLOC(W.rstd_qk, float, (int64_t)T * (ctx->H + ctx->Hkv)); }
    for (int p = 0; p < 4; ++p) {
      *us[p] = nullptr;
      if (groups[p]->on) ALLOC(*us[p], AT, (int64_t)T * groups[p]->d.RP);
    }
  }
  ALLOC(ctx->x_last, AT, (int64_t)T * d);
  return TST_OK;
}
// the flat trainable vector (ns slots of n1 elements) and its optimizer state
template <typename AT>
int trainables(CtxT<AT>* ctx) {
  ctx->n1 = ctx->n_train;
  ctx->n_train = ctx->n1 * ctx->ns;
  for (auto& g : ctx->descs)   // slot s keeps the layout of slot 0, shifted by s * n1
    for (int sl = 1; sl < ctx->ns; ++sl)
      for (int m = 0; m < g.nmod; ++m) {
        g.a_off[sl * g.nmod + m] = g.a_off[m] + sl * ctx->n1;
        g.b_off[sl * g.nmod + m] = g.b_off[m] + sl * ctx->n1;
      }
  if (ctx->zero_on) {   // this rank's shard of the optimizer state; the gradient stays full length (reduce-scatter input), padded
    ALLOC(ctx->tp, float, ctx->z_shard); ALLOC(ctx->tm, float, ctx->z_shard); ALLOC(ctx->tv, float, ctx->z_shard);
    ALLOC(ctx->tg, float, ctx->n_pad);
    ALLOC(ctx->z_sumsq, float, 4);
  } else {
    // the per-slot losses sit right behind the flat gradient: the stacked data-parallel step reduces both with ONE ncclAllReduce
    ALLOC(ctx->tp, float, ctx->n_train); ALLOC(ctx->tg, float, ctx->n_train + TST_MAX_STACK); ALLOC(ctx->tm, float, ctx->n_train); ALLOC(ctx->tv, float, ctx->n_train);
    ctx->d_loss = ctx->tg + ctx->n_train;
  }
  ALLOC(ctx->descs_dev, LoraGroupDescT<AT>, ctx->descs.size());
  ALLOC(ctx->clip_out, float, 2 * TST_MAX_STACK); ALLOC(ctx->clip_partial, float, 4096);
  if (!ctx->d_loss) ALLOC(ctx->d_loss, float, TST_MAX_STACK);
  return TST_OK;
}
// RoPE tables: inv_freq = theta^(-2i/dh) (modeling_llama.py:108), cos/sin cast to bf16 (:127); a fork reads its parent's
template <typename AT>
int rope_tables(CtxT<AT>* ctx) {
  const tst_model_cfg& c = ctx->cfg;
  if (ctx->parent) { ctx->cosT = ctx->parent->cosT; ctx->sinT = ctx->parent->sinT; return TST_OK; }
  if (ctx->gpt2) return TST_OK;
  const int half = ctx->dh / 2, P = c.max_position;
  std::vector<float> hc((size_t)P * half), hs((size_t)P * half);
  for (int i = 0; i < half; ++i) {
    const float inv_freq = rope_inv_freq(c, i, ctx->dh);
    for (int p = 0; p < P; ++p) {
      const float ang = (float)p * inv_freq;
      hc[(size_t)p * half + i] = sizeof(AT) == 2 ? host_bf2f(host_f2bf(cosf(ang))) : cosf(ang);
      hs[(size_t)p * half + i] = sizeof(AT) == 2 ? host_bf2f(host_f2bf(sinf(ang))) : sinf(ang);
    }
  }
  ALLOC(ctx->cosT, float, (int64_t)P * half); ALLOC(ctx->sinT, float, (int64_t)P * half);
  CTX_HIP(hipMemcpy(ctx->cosT, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
  CTX_HIP(hipMemcpy(ctx->sinT, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
  return TST_OK;
}
// the batch on the device (one int array, host_logic.h stage_ints) and the pinned buffers of the asynchronous entry points
inline int batch_staging(tst_ctx* ctx) {
  const size_t stage_ints = tsthost::stage_ints(batch_limits(ctx));   // layout of upload_batch's staging buffer
  ALLOC(ctx->d_ids, int, stage_ints + 64);
  ctx->d_pos = ctx->d_ids + ctx->Tmax; ctx->d_cu = ctx->d_pos + ctx->Tmax; ctx->d_lab_idx = ctx->d_cu + (ctx->Smax + 1); ctx->d_targets = ctx->d_lab_idx + ctx->Rmax; ctx->d_order = ctx->d_targets + ctx->Rmax;
  ALLOC(ctx->d_opt_ids, int, 256);
  ALLOC(ctx->d_idflag, int, 4);
  CTX_HIP(hipHostMalloc((void**)&ctx->h_idflag, 4 * sizeof(int), hipHostMallocDefault));
  ctx->h_idflag[0] = 0;
  for (int i = 0; i < 2; ++i) {
    CTX_HIP(hipHostMalloc((void**)&ctx->h_stage[i], stage_ints * sizeof(int), hipHostMallocDefault));
    CTX_HIP(hipEventCreateWithFlags(&ctx->stage_evt[i], hipEventDisableTiming));
  }
  CTX_HIP(hipHostMalloc((void**)&ctx->h_score, (size_t)ctx->Rmax * 260 * sizeof(float), hipHostMallocDefault));
  CTX_HIP(hipEventCreateWithFlags(&ctx->score_evt, hipEventDisableTiming));
  CTX_HIP(hipHostMalloc((void**)&ctx->h_opt_ids, 256 * sizeof(int), hipHostMallocDefault));
  CTX_HIP(hipHostMalloc((void**)&ctx->h_metrics, 4 * TST_MAX_STACK * sizeof(float), hipHostMallocDefault));   // [loss of slot s (8) | {grad norm, clip coef} of slot s (16) | tst_fetch_loss (8)]
  memset(ctx->h_metrics, 0, 4 * TST_MAX_STACK * sizeof(float));
  return TST_OK;
}

template <typename AT>
int head_workspace(CtxT<AT>* ctx) {
  const int d = ctx->d, V = ctx->Vp, R = head_rows(ctx);
  ALLOC(ctx->xg, AT, (int64_t)R * d); ALLOC(ctx->xf, AT, (int64_t)R * d); ALLOC(ctx->dxf, AT, (int64_t)R * d); ALLOC(ctx->dxg, AT, (int64_t)R * d);
  ALLOC(ctx->dlogits, AT, (int64_t)R * V); ALLOC(ctx->rstd_f, float, 2 * R); ALLOC(ctx->logits, float, (int64_t)R * V);
  ALLOC(ctx->stats, float, (int64_t)R * 4); ALLOC(ctx->optl, float, (int64_t)R * 256);
  return TST_OK;
}
// backward scratch. LoRA: the last layer's compact stash and one du buffer per module group for the side stream; full fine-tune: the gradient-norm slots,
// the column-reduction workspaces and (without kmajor bit 1) the transposed activations of the weight-gradient contractions
template <typename AT>
int backward_scratch(CtxT<AT>* ctx) {
  const int d = ctx->d, F = ctx->F, Fgu = ctx->Fgu, T = ctx->Tpad_max, R = head_rows(ctx), rp = rank_pad_max(ctx);
  ALLOC(ctx->dX, AT, (int64_t)T * d); ALLOC(ctx->dH, AT, (int64_t)T * d); ALLOC(ctx->dxn, AT, (int64_t)T * d);
  ALLOC(ctx->dattn_b, AT, (int64_t)T * ctx->dattn); ALLOC(ctx->dqkv_b, AT, (int64_t)T * ctx->dqkv);
  ALLOC(ctx->dact, AT, (int64_t)T * F); ALLOC(ctx->dgu, AT, (int64_t)T * Fgu);
  ALLOC(ctx->du, AT, (int64_t)T * rp);
  if (!ctx->full) {
    static const bool lc_env = env_flag("TST_LAST_COMPACT", true);
    if (lc_env) {   // R = roundup64(Rmax) rows each: a few MB
      ALLOC(ctx->lc_attn, AT, (int64_t)R * ctx->dattn); ALLOC(ctx->lc_xin, AT, (int64_t)R * d); ALLOC(ctx->lc_hmid, AT, (int64_t)R * d);
      ALLOC(ctx->lc_xn2, AT, (int64_t)R * d); ALLOC(ctx->lc_gu, AT, (int64_t)R * Fgu); ALLOC(ctx->lc_act, AT, (int64_t)R * F);
      ALLOC(ctx->lc_us_o, AT, (int64_t)R * rp); ALLOC(ctx->lc_us_gu, AT, (int64_t)R * rp); ALLOC(ctx->lc_us_d, AT, (int64_t)R * rp);
      ALLOC(ctx->lc_dact, AT, (int64_t)R * F); ALLOC(ctx->lc_dgu, AT, (int64_t)R * Fgu); ALLOC(ctx->lc_dxn, AT, (int64_t)R * d);
      ALLOC(ctx->lc_dH, AT, (int64_t)R * d); ALLOC(ctx->lc_dattn, AT, (int64_t)R * ctx->dattn); ALLOC(ctx->lc_rstd2, float, 2 * (int64_t)R);
      ctx->lc_have = ctx->lc_on = true;
    }
    if (wants_side_stream(ctx))
      for (int g = 0; g < 4; ++g) ALLOC(ctx->du4[g], AT, (int64_t)T * rp);
  } else {
    // gradient regions in the order backward finishes them: lm_head (untied), layers L-1 .. 0, embedding side, norm / bias tail (host_logic.h)
    ctx->gn_regions = tsthost::full_layout(ctx->md).regions;
    for (int p = 0; p < 4; ++p) ctx->gn_cap += ctx->L * gn_slots(ctx->proj_dout[p], ctx->proj_din[p]);
    ctx->gn_cap += 3 * 1024;   // embedding side, head, norm / bias tail: summed at the optimizer step
    ALLOC(ctx->gn_partial, float, ctx->gn_cap);
    const int dout_max = (Fgu > ctx->dqkv) ? Fgu : ctx->dqkv, din_max = (F > d) ? F : d;
    ALLOC(ctx->colred_ws, float, 2 * colred_ws_floats(T, dout_max > d ? dout_max : d));
    ALLOC(ctx->colred_ws_side, float, 2 * colred_ws_floats(T, d));
    if (ctx->qk_norm) ALLOC(ctx->hn_ws, float, HEAD_NORM_WS_FLOATS);
    if (!(ctx->kmajor & 2)) {   // transposed activations for the weight-gradient contractions (else dW = dy^T . x on the TN member: no transposed copies)
      ALLOC(ctx->dyT, AT, (int64_t)dout_max * T);
      ALLOC(ctx->xT, AT, (int64_t)din_max * T);
    }
  }
  ALLOC(ctx->delta, float, (int64_t)ctx->H * T);
  return TST_OK;
}
// The streams beside the context's own. side: LoRA's adapter-gradient contractions, a full fine-tune's weight-gradient contractions (linear_bwd).
// opt_stream: the optimizer of an unsharded full fine-tune (see tst_ctx::opt_stream).
inline int make_streams(tst_ctx* ctx) {
  int cus = 0;   // a CU mask is laid out for the 256 CUs of the unpartitioned device (another partition mode: no mask)
  hipDeviceProp_t prop;
  if (ctx->full && hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) cus = prop.multiProcessorCount;
  if (wants_side_stream(ctx)) {
    // TST_DW_CUS=n (A/B switch, full fine-tune): the weight gradients' stream confined to n CUs, as the optimizer's below -- the dX chain and the small kernels
    // between its contractions then always find free CUs
    int dw_cus = 0;
    if (ctx->full) { static const int dw_cus_env = env_int("TST_DW_CUS", 0); dw_cus = dw_cus_env; }
    if (dw_cus > 0 && dw_cus < 256 && cus == 256) {
      ctx->side = masked_stream(ctx->device, dw_cus);
      if (!ctx->side) return fail(ctx, TST_EHIP, "hipExtStreamCreateWithCUMask failed");
      ctx->side_shared = true;
    } else {
      CTX_HIP(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    }
    CTX_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    CTX_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  if (ctx->full)
    for (auto& e : ctx->ev_ndw) CTX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!ctx->full || ctx->zero_on) return TST_OK;
  // The optimizer's stream is confined to 160 of the 256 CUs (TST_OPT_CUS = n; 0 = a plain stream), the same share of every XCD (the driver deals the
  // mask's bits round-robin over the XCDs, then over an XCD's shader engines): a 256-VGPR, 128 KB-LDS projection tile needs an EMPTY CU, and AdamW blocks
  // streaming over all CUs keep the next forward's tiles waiting for one. A CU streams at most ~37 GB/s, so AdamW needs most of the chip for the HBM rate.
  // 160 measured best (profiles/r05_full_opt_cus_ab.txt: 23.74 QA-pairs/s against 22.94 / 23.47 / 23.30 / 22.82 / 22.52 at 128 / 152 / 168 / 192 / 208;
  // DESIGN.md section 8). Round 4 had settled on 192 (profiles/r04_full_overlap_ab.txt block 8; docs/DESIGN_HISTORY.md).
  static const int opt_cus = env_int("TST_OPT_CUS", 160);
  if (opt_cus > 0 && opt_cus < 256 && cus == 256) {
    ctx->opt_stream = masked_stream(ctx->device, opt_cus);
    if (!ctx->opt_stream) return fail(ctx, TST_EHIP, "hipExtStreamCreateWithCUMask failed");
    ctx->opt_stream_shared = true;
  } else {
    // TST_OPT_PRIO=1: the optimizer's queue at the device's LOWEST priority -- the forward's workgroups are dispatched first, AdamW takes what is left
    static const bool low = env_flag("TST_OPT_PRIO", false);
    int lo = 0, hi = 0;
    if (low && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) CTX_HIP(hipStreamCreateWithPriority(&ctx->opt_stream, hipStreamNonBlocking, lo));
    else CTX_HIP(hipStreamCreateWithFlags(&ctx->opt_stream, hipStreamNonBlocking));
  }
  CTX_HIP(hipEventCreateWithFlags(&ctx->opt_go, hipEventDisableTiming));
  ctx->opt_ev.resize((size_t)ctx->L + 2);
  for (auto& e : ctx->opt_ev) CTX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return TST_OK;
}
// split-K slabs: sized for the largest planned split of any shape this engine issues
template <typename AT>
int splitk_slabs(CtxT<AT>* ctx) {
  const int d = ctx->d, F = ctx->F, Fgu = ctx->Fgu, V = ctx->Vp, T = ctx->Tpad_max, R = head_rows(ctx), rp = rank_pad_max(ctx);
  size_t need = 64u << 20;
  auto consider = [&](int M, int N, int K, int K2) {
    int v, sk;
    gemm_plan(M, N, K, K2, &v, &sk);
    const size_t b = gemm_slab_bytes(M, N, sk);
    if (b > need) need = b;
    const size_t b2 = (long)tst_ceil_div(M, 256) * tst_ceil_div(N, 256) <= 128 ? gemm_slab_bytes(M, N, 4) : 0;   // tile policy 3 may be switched on later
    if (b2 > need) need = b2;
  };
  consider(T, ctx->dqkv, d, rp); consider(T, d, ctx->dattn, rp); consider(T, Fgu, d, rp); consider(T, d, F, rp);
  consider(T, d, ctx->dqkv, rp); consider(T, ctx->dattn, d, rp); consider(T, d, Fgu, rp); consider(T, F, d, rp);
  consider(T, rp, d, 0); consider(T, rp, F, 0); consider(T, rp, Fgu, 0); consider(T, rp, ctx->dqkv, 0);
  consider(Fgu, rp, T, 0); consider(ctx->dqkv, rp, T, 0); consider(d, rp, T, 0);
  consider(rp, d, T, 0); consider(rp, F, T, 0);
  consider(R, V, d, 0); consider(R, d, V, 0);
  ctx->slab_bytes = need;
  ctx->slab = (float*)ctx->pool.alloc((int64_t)need);
  if (!ctx->slab) return fail(ctx, TST_ENOMEM, "hipMalloc failed: slab");
  if (ctx->side) {   // the side stream's split-K contractions (LoRA: token axis, <= 64 columns on one side; full fine-tune: the weight gradients' tail slices) need their own slabs
    ctx->side_slab_bytes = ctx->full ? need : (64u << 20);
    ctx->side_slab = (float*)ctx->pool.alloc((int64_t)ctx->side_slab_bytes);
    if (!ctx->side_slab) return fail(ctx, TST_ENOMEM, "hipMalloc failed: side slab");
  }
  return TST_OK;
}
// the state_dict name table; the trainables of a full fine-tune are its entries inside the flat buffer, in its order (a LoRA context's are the module groups')
template <typename AT>
int name_tables(CtxT<AT>* ctx) {
  if (ctx->gpt2) name_tensors_gpt2(ctx);
  else name_tensors_llama(ctx);
  if (!ctx->full) return TST_OK;
  for (const auto& t : ctx->named)
    if (!t.alias && t.ptr >= ctx->wb && t.ptr < ctx->wb + ctx->n_train) ctx->tinfo.push_back({t.name, (int64_t)(t.ptr - ctx->wb), t.rows, t.cols});
  std::sort(ctx->tinfo.begin(), ctx->tinfo.end(), [](const TrainableInfo& a, const TrainableInfo& b) { return a.offset < b.offset; });
  return TST_OK;
}
#undef ALLOC

template <typename AT>
int build_ctx(CtxT<AT>* ctx) {
  // (no configuration check here: tst_create and fork_impl, the two callers, have run host_logic.h check_cfg before they allocated the context)
  CTX_RC(set_dims(ctx));
  CTX_RC(weight_storage(ctx));
  CTX_RC(build_layers(ctx));
  CTX_RC(trainables(ctx));
  CTX_RC(rope_tables(ctx));
  CTX_RC(batch_staging(ctx));
  CTX_RC(head_workspace(ctx));
  CTX_RC(backward_scratch(ctx));
  CTX_RC(make_streams(ctx));
  CTX_RC(splitk_slabs(ctx));
  CTX_RC(name_tables(ctx));
  CTX_HIP(hipMemcpy(ctx->descs_dev, ctx->descs.data(), ctx->descs.size() * sizeof(LoraGroupDescT<AT>), hipMemcpyHostToDevice));
  CTX_HIP(hipDeviceSynchronize());  // the ctx stream is non-blocking: setup copies/memsets must have landed before it is used
  return TST_OK;
}

template <typename AT>
int repack(CtxT<AT>* ctx) { return lora_pack<AT>(ctx->stream, ctx->descs_dev, (int)ctx->descs.size(), ctx->tp, ctx->pack_max_long); }


// ---- typed halves of the C-ABI entry points (dispatched on ctx->strict below)
template <typename AT>
int fork_impl(CtxT<AT>* parent, tst_ctx** out) {
  if (parent->parent) return fail(parent, TST_EINVAL, "fork from the root context, not from a fork");
  if (!parent->finalized) return fail(parent, TST_ESTATE, "finalise the parent's weights before forking");
  if (const int rc = tsthost::check_cfg(parent->cfg, true, parent->err)) return rc;   // (a full fine-tune cannot be forked)
  if (hipSetDevice(parent->device) != hipSuccess) return fail(parent, TST_EHIP, "hipSetDevice failed");
  CtxT<AT>* ctx = new CtxT<AT>();
  ctx->cfg = parent->cfg;
  ctx->strict = parent->strict;
  ctx->device = parent->device;
  ctx->parent = parent;
  ctx->has_parent = true;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return fail(parent, TST_EHIP, "hipStreamCreate failed");
  }
  ctx->own_stream = ctx->stream;
  int rc = build_ctx(ctx);
  if (rc == TST_OK) rc = repack(ctx);
  if (rc == TST_OK && hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  if (rc != TST_OK) {
    parent->err = ctx->err;
    tst_destroy(ctx);
    return rc;
  }
  ctx->finalized = true;
  *out = ctx;
  return TST_OK;
}

// host fp32 / bf16 -> device element type (GPT-2 Conv1D weights are transposed on the way: HF [in, out] -> device [out, in],
// pytorch_utils.py:110-120: y = x @ W + b)
template <typename AT>
int set_weight_impl(CtxT<AT>* ctx, const char* name, const void* host, int dtype, int64_t numel) {
  if (ctx->parent) return fail(ctx, TST_ESTATE, "a forked context borrows its parent's weights");
  const auto* t = find_weight(ctx, name);
  if (!t) return fail(ctx, TST_ENOTFOUND, std::string("unknown weight: ") + name);
  if (t->rows * t->cols != numel) return fail(ctx, TST_EINVAL, std::string("numel mismatch for ") + name);
  const int64_t conv_in = t->conv1d ? t->cols : 0, conv_out = t->conv1d ? t->rows : 0;   // Conv1D: the HF tensor is [in, out], the device tensor [out, in]
  ctx->finalized = false;
  if (dtype != TST_DTYPE_BF16 && dtype != TST_DTYPE_F32) return fail(ctx, TST_EINVAL, "dtype must be TST_DTYPE_F32 or TST_DTYPE_BF16");
  const float* f = (const float*)host;
  const uint16_t* h = (const uint16_t*)host;
  const bool same = (sizeof(AT) == 2) == (dtype == TST_DTYPE_BF16);
  std::vector<AT> tmp;
  const void* src = host;
  if (!same || conv_in) {
    tmp.resize((size_t)numel);
    auto conv = [&](int64_t sidx) -> AT {
      if (sizeof(AT) == 2) return (AT)(dtype == TST_DTYPE_F32 ? host_f2bf(f[sidx]) : h[sidx]);
      const float v = dtype == TST_DTYPE_F32 ? f[sidx] : host_bf2f(h[sidx]);
      AT o;
      memcpy(&o, &v, sizeof(AT) < sizeof(v) ? sizeof(AT) : sizeof(v));
      return o;
    };
    if (conv_in) {
      for (int64_t i = 0; i < conv_in; ++i)
        for (int64_t o = 0; o < conv_out; ++o) tmp[(size_t)(o * conv_in + i)] = conv(i * conv_out + o);
    } else {
      for (int64_t i = 0; i < numel; ++i) tmp[(size_t)i] = conv(i);
    }
    src = tmp.data();
  }
  CTX_HIP(hipMemcpy(t->ptr, src, (size_t)numel * sizeof(AT), hipMemcpyHostToDevice));
  if (ctx->qk_norm)
    for (auto& W : ctx->layers) {
      if (t->ptr == W.q_norm) W.q_norm_set = true;
      if (t->ptr == W.k_norm) W.k_norm_set = true;
    }
  return TST_OK;
}

template <typename AT>
int get_weight_impl(CtxT<AT>* ctx, const char* name, float* host_out, int64_t numel) {
  const auto* t = find_weight(ctx, name);
  if (!t) return fail(ctx, TST_ENOTFOUND, std::string("unknown weight: ") + name);
  if (t->rows * t->cols != numel) return fail(ctx, TST_EINVAL, std::string("numel mismatch for ") + name);
  const int64_t conv_in = t->conv1d ? t->cols : 0, conv_out = t->conv1d ? t->rows : 0;   // Conv1D: the HF tensor is [in, out], the device tensor [out, in]
  std::vector<AT> tmp((size_t)numel);
  CTX_RC(ctx_sync(ctx));
  CTX_HIP(hipMemcpy(tmp.data(), t->ptr, (size_t)numel * sizeof(AT), hipMemcpyDeviceToHost));
  auto val = [&](int64_t i) -> float {
    if (sizeof(AT) == 2) { uint16_t b; memcpy(&b, &tmp[(size_t)i], 2); return host_bf2f(b); }
    float v; memcpy(&v, &tmp[(size_t)i], sizeof(AT) < 4 ? sizeof(AT) : 4); return v;
  };
  if (conv_in) {  // back to the HF Conv1D layout [in, out]
    for (int64_t o = 0; o < conv_out; ++o)
      for (int64_t i = 0; i < conv_in; ++i) host_out[i * conv_out + o] = val(o * conv_in + i);
    return TST_OK;
  }
  for (int64_t i = 0; i < numel; ++i) host_out[i] = val(i);
  return TST_OK;
}

template <typename AT>
int finalize_weights_impl(CtxT<AT>* ctx) {
  if (ctx->parent) return fail(ctx, TST_ESTATE, "a forked context borrows its parent's weights");
  if (ctx->qk_norm)
    for (size_t l = 0; l < ctx->layers.size(); ++l)
      if (!ctx->layers[l].q_norm_set || !ctx->layers[l].k_norm_set)
        return fail(ctx, TST_ESTATE, "Qwen3: model.layers." + std::to_string(l) + ".self_attn.q_norm.weight / k_norm.weight were not set");
  CTX_HIP(hipDeviceSynchronize());  // tst_set_weight copies (default stream) must have landed
  hipStream_t st = ctx->stream;
  CTX_RC(refresh_transposes(ctx));
  if (ctx->full) {
    // the fp32 master starts as the exact bf16 value of every weight; wb0 is the fold-start snapshot that
    // tst_reset_trainable restores
    CTX_RC(cast_to_f32<AT>(st, ctx->wb + ctx->z_lo, ctx->tp, ctx->z_hi - ctx->z_lo));   // (the whole vector unless the optimizer state is sharded)
    CTX_HIP(hipMemcpyAsync(ctx->wb0, ctx->wb, (size_t)ctx->n_train * sizeof(AT), hipMemcpyDeviceToDevice, st));
  }
  CTX_RC(repack(ctx));
  CTX_HIP(hipStreamSynchronize(st));
  ctx->finalized = true;
  return TST_OK;
}

template <typename AT>
int init_random_impl(CtxT<AT>* ctx, uint64_t seed, float stdv) {
  if (ctx->parent) return fail(ctx, TST_ESTATE, "a forked context borrows its parent's weights");
  hipStream_t st = ctx->stream;
  const int d = ctx->d;
  unsigned s = (unsigned)(seed * 2654435761ULL + 12345ULL);
  CTX_RC(randn_fill<AT>(st, ctx->embed, (long)ctx->V * d, s += 101, stdv));  // rows V..Vp-1 stay zero
  if (ctx->gpt2) {
    CTX_RC(randn_fill<AT>(st, ctx->wpe, (long)ctx->npos * d, s += 101, stdv));
    CTX_RC(fill_const<AT>(st, ctx->final_norm_b, d, 0.0f));
  } else {
    CTX_RC(randn_fill<AT>(st, ctx->lm_head, (long)ctx->V * d, s += 101, stdv));
  }
  CTX_RC(fill_const<AT>(st, ctx->final_norm, d, 1.0f));
  for (auto& W : ctx->layers) {
    CTX_RC(fill_const<AT>(st, W.attn_norm, d, 1.0f));
    CTX_RC(fill_const<AT>(st, W.mlp_norm, d, 1.0f));
    if (W.bqkv) CTX_RC(fill_const<AT>(st, W.bqkv, ctx->dqkv, 0.0f));
    if (ctx->qk_norm) {
      CTX_RC(fill_const<AT>(st, W.q_norm, ctx->dh, 1.0f)); CTX_RC(fill_const<AT>(st, W.k_norm, ctx->dh, 1.0f));
      W.q_norm_set = W.k_norm_set = true;
    }
    if (ctx->gpt2) {
      CTX_RC(fill_const<AT>(st, W.attn_norm_b, d, 0.0f)); CTX_RC(fill_const<AT>(st, W.mlp_norm_b, d, 0.0f));
      CTX_RC(fill_const<AT>(st, W.bo, d, 0.0f)); CTX_RC(fill_const<AT>(st, W.bgu, ctx->Fgu, 0.0f)); CTX_RC(fill_const<AT>(st, W.bd, d, 0.0f));
    }
    for (const ProjT<AT>& P : W.proj) CTX_RC(randn_fill<AT>(st, P.W, (long)P.numel(), s += 101, stdv));
  }
  ctx->finalized = false;
  return finalize_weights_impl(ctx);
}

template <typename AT>
int set_trainable_impl(CtxT<AT>* ctx, const float* host) {
  CTX_RC(ctx_sync(ctx));
  if (ctx->zero_on) {   // sharded optimizer state: the gradient buffer stages the full vector; the master keeps this rank's shard
    CTX_HIP(hipMemcpy(ctx->tg, host, (size_t)ctx->n_train * 4, hipMemcpyHostToDevice));
    CTX_HIP(hipDeviceSynchronize());
    CTX_RC(cast_from_f32<AT>(ctx->stream, ctx->tg, ctx->wb, ctx->n_train, 1.0f));
    CTX_HIP(hipMemcpyAsync(ctx->tp, ctx->tg + ctx->z_lo, (size_t)(ctx->z_hi - ctx->z_lo) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CTX_HIP(hipMemsetAsync(ctx->tg, 0, (size_t)ctx->n_pad * 4, ctx->stream));
    CTX_RC(refresh_transposes(ctx));
    CTX_RC(ctx_sync(ctx));
    return TST_OK;
  }
  CTX_HIP(hipMemcpy(ctx->tp + ctx->sel_slot * ctx->n1, host, (size_t)ctx->n1 * 4, hipMemcpyHostToDevice));
  CTX_HIP(hipDeviceSynchronize());
  if (ctx->full) {
    CTX_RC(cast_from_f32<AT>(ctx->stream, ctx->tp, ctx->wb, ctx->n_train, 1.0f));
    CTX_RC(refresh_transposes(ctx));
  }
  CTX_RC(repack(ctx));
  CTX_RC(ctx_sync(ctx));
  return TST_OK;
}

template <typename AT>
int reset_trainable_impl(CtxT<AT>* ctx, uint64_t seed) {
  ctx->acc_active = false;   // an accumulation window left open belongs to the fold that ends here: it must not reach the fresh trainables
  if (ctx->full) {
    // a new fold starts from the base model: restore the snapshot taken by tst_finalize_weights
    if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
    hipStream_t st = ctx->stream;
    CTX_RC(opt_join(ctx));   // a pending optimizer step still writes the weights this restores
    CTX_HIP(hipMemcpyAsync(ctx->wb, ctx->wb0, (size_t)ctx->n_train * sizeof(AT), hipMemcpyDeviceToDevice, st));
    const int64_t nsh = ctx->z_hi - ctx->z_lo;   // = n_train unless the optimizer state is sharded
    CTX_RC(cast_to_f32<AT>(st, ctx->wb + ctx->z_lo, ctx->tp, nsh));
    CTX_HIP(hipMemsetAsync(ctx->tm, 0, (size_t)nsh * 4, st));
    CTX_HIP(hipMemsetAsync(ctx->tv, 0, (size_t)nsh * 4, st));
    CTX_HIP(hipMemsetAsync(ctx->tg, 0, (size_t)ctx->n_pad * 4, st));
    ctx->opt_steps[0] = 0;
    CTX_RC(refresh_transposes(ctx));
    CTX_HIP(hipStreamSynchronize(st));
    return TST_OK;
  }
  // LoRA: the selected slot's adapters (one slot unless folds are stacked)
  const int64_t so = ctx->sel_slot * ctx->n1;
  // everything on the context's stream, nothing the host waits for: lora_B, both moments and the gradient are zeros, every lora_A is drawn on the
  // device (one splitmix64 stream per (seed, tensor); peft: kaiming_uniform_(A, a=sqrt(5)) => U(-1/sqrt(fan_in), 1/sqrt(fan_in))), then the packed
  // operands are rebuilt
  hipStream_t st = ctx->stream;
  CTX_HIP(hipMemsetAsync(ctx->tp + so, 0, (size_t)ctx->n1 * 4, st));
  CTX_HIP(hipMemsetAsync(ctx->tm + so, 0, (size_t)ctx->n1 * 4, st));
  CTX_HIP(hipMemsetAsync(ctx->tv + so, 0, (size_t)ctx->n1 * 4, st));
  CTX_HIP(hipMemsetAsync(ctx->tg + so, 0, (size_t)ctx->n1 * 4, st));
  for (size_t t = 0; t < ctx->tinfo.size(); ++t) {
    const TrainableInfo& ti = ctx->tinfo[t];
    if (!(ti.name.size() > 6 && ti.name.compare(ti.name.size() - 6, 6, "lora_A") == 0)) continue;
    const uint64_t state0 = seed * 0x9e3779b97f4a7c15ULL + (uint64_t)t * 0xd1b54a32d192ed03ULL + 1;
    CTX_RC(lora_a_init(st, ctx->tp + so + ti.offset, (long)(ti.rows * ti.cols), state0, 1.0f / sqrtf((float)ti.cols)));
  }
  ctx->opt_steps[ctx->sel_slot] = 0;
  return repack(ctx);
}

// slot_items: per-slot labelled-token counts of the whole accumulated / global batch (nullptr: every slot is normalised by its own count in b)
template <typename AT>
int fwd_bwd_enqueue(CtxT<AT>* ctx, const tst_batch* b, int32_t num_items, const int32_t* slot_items = nullptr) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised: call tst_finalize_weights / tst_init_random first");
  ctx->err.clear();
  CTX_RC(upload_batch(ctx, b, true, nullptr, 0));
  if (ctx->cur_R <= 0) return fail(ctx, TST_EINVAL, "batch has no labelled tokens");
  if (ctx->ns > 1 && num_items > 0) return fail(ctx, TST_EINVAL, "stacked folds: num_items must be 0 (every slot is normalised by its own labelled-token count, or by slot_items)");
  for (int sl = 0; sl < ctx->ns; ++sl) ctx->slot_steps[sl] = ctx->ns == 1 ? true : (ctx->slot_r0[sl + 1] - ctx->slot_r0[sl] > 0);
  if (slot_items) {
    for (int sl = 0; sl < ctx->ns; ++sl) {
      const int rows = ctx->ns == 1 ? ctx->cur_R : ctx->slot_r0[sl + 1] - ctx->slot_r0[sl];
      if (rows > 0 && slot_items[sl] < rows) return fail(ctx, TST_EINVAL, "num_items of a slot is smaller than its labelled tokens in this batch");
    }
    if (ctx->ns == 1) num_items = slot_items[0];
  }
  const int items = num_items > 0 ? num_items : ctx->cur_R;
  ctx->cur_items = items;
  ctx->grad_stale = false;
  CTX_RC(forward(ctx, true));
  CTX_RC(head_forward(ctx, true));
  return backward(ctx, items, slot_items);
}

// workgroups (= partial sums, fixed assignment: reproducible) of the gradient-norm pass: 256 pulled the 168 MB of one Llama-3-8B adapter set at 1.1 TB/s
inline int clip_parts(int64_t n) { return n > (64L << 20) ? 4096 : (n > (4L << 20) ? 1024 : 256); }

// the optimizer steps take the gradient they apply as `tg`: the context's flat gradient, or the running sum of an accumulation window (tacc)
template <typename AT>
int opt_enqueue_stacked(CtxT<AT>* ctx, const float* lrs, float* tg) {
  const tst_model_cfg& c = ctx->cfg;
  hipStream_t st = ctx->stream;
  for (int sl = 0; sl < ctx->ns; ++sl) {
    if (!ctx->slot_steps[sl]) continue;   // no labelled token in this (accumulated / global) batch: the slot takes no step
    ctx->opt_steps[sl] += 1;
    const double bc1 = 1.0 - pow((double)c.adam_beta1, (double)ctx->opt_steps[sl]);
    const double bc2 = 1.0 - pow((double)c.adam_beta2, (double)ctx->opt_steps[sl]);
    const int64_t o = sl * ctx->n1;
    CTX_RC(grad_clip_coef(st, tg + o, ctx->n1, c.max_grad_norm, ctx->clip_partial, clip_parts(ctx->n1), ctx->clip_out + 2 * sl));
    const int slot = prof_begin(ctx, st, ctx->prof_hbm);
    CTX_RC(adamw_step<AT>(st, ctx->tp + o, tg + o, ctx->tm + o, ctx->tv + o, ctx->n1, ctx->clip_out + 2 * sl, lrs[sl], c.adam_beta1, c.adam_beta2, c.adam_eps,
                      c.weight_decay, (float)bc1, (float)sqrt(bc2), nullptr));
    prof_end(ctx, st, slot, PROF_ADAMW, 1, 28.0 * ctx->n1);   // read p, g, m, v; write p, m, v (fp32)
  }
  CTX_RC(repack(ctx));
  return TST_OK;
}

// sharded optimizer state: the full trainable vector = this rank's fp32 master on [z_lo, z_hi), the compute copy (rounded) elsewhere
template <typename AT>
int get_trainable_sharded(CtxT<AT>* ctx, float* host_out) {
  std::vector<AT> tmp((size_t)ctx->n_train);
  CTX_HIP(hipMemcpy(tmp.data(), ctx->wb, (size_t)ctx->n_train * sizeof(AT), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < ctx->n_train; ++i) {
    if (sizeof(AT) == 2) { uint16_t b; memcpy(&b, &tmp[(size_t)i], 2); host_out[i] = host_bf2f(b); }
    else memcpy(&host_out[i], &tmp[(size_t)i], 4);
  }
  CTX_HIP(hipMemcpy(host_out + ctx->z_lo, ctx->tp, (size_t)(ctx->z_hi - ctx->z_lo) * 4, hipMemcpyDeviceToHost));
  return TST_OK;
}

// ZeRO stage 1 step (cfg.zero_ranks > 1): reduce-scatter the gradient, clip by the GROUP's norm, AdamW on this rank's shard, all-gather the
// compute copy. Without a communicator (one-GPU shard tests) the collectives are skipped: the local gradient is the group sum, the norm is
// taken over all of it, only this rank's shard of the weights moves.
template <typename AT>
int opt_enqueue_zero(CtxT<AT>* ctx, float lr, float* tg) {
  const tst_model_cfg& c = ctx->cfg;
  hipStream_t st = ctx->stream;
  ctx->opt_steps[0] += 1;
  const double bc1 = 1.0 - pow((double)c.adam_beta1, (double)ctx->opt_steps[0]);
  const double bc2 = 1.0 - pow((double)c.adam_beta2, (double)ctx->opt_steps[0]);
  const int64_t lo = ctx->z_lo, hi = ctx->z_hi, nsh = hi - lo;
  ctx->gn_fused = false;
  if (ctx->dp_comm) {
    if (ctx->dp_ranks != ctx->zero) return fail(ctx, TST_ESTATE, "the data-parallel group must have zero_ranks ranks");
    ctx->dp_n_coll += 1; ctx->dp_n_elems += ctx->n_pad;
    if (ncclReduceScatter(tg, tg + (int64_t)ctx->zero_rank * ctx->z_shard, (size_t)ctx->z_shard, ncclFloat, ncclSum, ctx->dp_comm, st) != ncclSuccess)
      return fail(ctx, TST_EHIP, "ncclReduceScatter failed");
    CTX_RC(sumsq_partial(st, tg + lo, nsh > 0 ? nsh : 1, ctx->clip_partial, 256));
    CTX_RC(sum_partials(st, ctx->clip_partial, 256, ctx->z_sumsq));
    CTX_RC(dp_allreduce(ctx, ctx->z_sumsq, 1, st));
    CTX_RC(clip_from_sumsq(st, ctx->z_sumsq, c.max_grad_norm, ctx->clip_out));
  } else {
    CTX_RC(grad_clip_coef(st, tg, ctx->n_train, c.max_grad_norm, ctx->clip_partial, clip_parts(ctx->n_train), ctx->clip_out));
  }
  // HF's two parameter groups (trainer.py:1181-1196): decay on [0, n_decay), none on the norm / bias tail; the shard may straddle the border
  const float b1 = (float)bc1, b2s = (float)sqrt(bc2);
  const int slot = prof_begin(ctx, st, ctx->prof_hbm);
  const tsthost::DecaySplit ds = tsthost::decay_split(lo, hi, ctx->n_decay);
  const int64_t d_hi = ds.d_hi;
  if (d_hi > lo)
    CTX_RC(adamw_step<AT>(st, ctx->tp, tg + lo, ctx->tm, ctx->tv, d_hi - lo, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2, c.adam_eps, c.weight_decay, b1, b2s, ctx->wb + lo));
  const int64_t n_lo = ds.n_lo;
  if (hi > n_lo)
    CTX_RC(adamw_step<AT>(st, ctx->tp + (n_lo - lo), tg + n_lo, ctx->tm + (n_lo - lo), ctx->tv + (n_lo - lo), hi - n_lo, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2,
                          c.adam_eps, 0.0f, b1, b2s, ctx->wb + n_lo));
  prof_end(ctx, st, slot, PROF_ADAMW, 1, (28.0 + sizeof(AT)) * nsh);
  if (ctx->dp_comm) {
    ctx->dp_n_coll += 1; ctx->dp_n_elems += ctx->n_pad;
    if (ncclAllGather(ctx->wb + (int64_t)ctx->zero_rank * ctx->z_shard, ctx->wb, (size_t)ctx->z_shard, sizeof(AT) == 2 ? ncclBfloat16 : ncclFloat, ctx->dp_comm, st) != ncclSuccess)
      return fail(ctx, TST_EHIP, "ncclAllGather failed");
  }
  return refresh_transposes(ctx);   // the dX contractions' W^T operands, from the gathered compute copy
}

template <typename AT>
int opt_enqueue(CtxT<AT>* ctx, float lr, float* tg) {
  if (ctx->zero_on) return opt_enqueue_zero(ctx, lr, tg);
  const tst_model_cfg& c = ctx->cfg;
  hipStream_t st = ctx->stream;
  // a pending overlapped step still reads clip_out and the gradient-norm partials that this call rewrites on the context's stream (two optimizer steps with no
  // backward between them): join it first. A no-op behind a backward, which joins itself
  CTX_RC(opt_join(ctx));
  if (ctx->ns > 1) {
    float lrs[TST_MAX_STACK];
    for (int i = 0; i < TST_MAX_STACK; ++i) lrs[i] = lr;
    return opt_enqueue_stacked(ctx, lrs, tg);
  }
  ctx->opt_steps[0] += 1;
  // adam.py:406-414: bias corrections in host double precision, as python floats
  const double bc1 = 1.0 - pow((double)c.adam_beta1, (double)ctx->opt_steps[0]);
  const double bc2 = 1.0 - pow((double)c.adam_beta2, (double)ctx->opt_steps[0]);
  if (ctx->full && ctx->gn_fused && ctx->gn_used + 3 * 1024 <= ctx->gn_cap) {
    // the layer matrices' sums of squares are in their slots; what is left: everything outside the per-layer regions
    const int64_t first = ctx->layers[0].proj[P_QKV].W - ctx->wb;
    const int64_t after = first + ctx->L * ctx->per_layer;
    float* rest = ctx->gn_partial + ctx->gn_used;
    // (1024 / 2048 workgroups: 256 pulled the 2.1 GB of the embedding gradient at 2.3 TB/s)
    CTX_RC(sumsq_partial(st, tg, first, rest, 1024));                                  // embedding side
    CTX_RC(sumsq_partial(st, tg + after, ctx->n_train - after, rest + 1024, 2048));    // head (untied) + norm / bias tail
    CTX_RC(clip_finalize(st, ctx->gn_partial, (int)(ctx->gn_used + 3 * 1024), c.max_grad_norm, ctx->clip_out));
    ctx->gn_fused = false;
  } else {
    CTX_RC(grad_clip_coef(st, tg, ctx->n_train, c.max_grad_norm, ctx->clip_partial, clip_parts(ctx->n_train), ctx->clip_out));
  }
  if (ctx->full) {
    // two parameter groups as HF builds them (trainer.py:1181-1196): weight decay on the matrices, none on the norm vectors;
    // the kernel also rounds the updated master into the bf16 compute copy, then the W^T copies are rebuilt
    const int64_t nd = ctx->n_decay, nn = ctx->n_train - ctx->n_decay;
    const float b1 = (float)bc1, b2s = (float)sqrt(bc2);
    // Overlapped form (default): the launches go to the optimizer stream behind the clip coefficient, in the order the next forward needs the
    // weights, one event per stage (tst_ctx::opt_stream); the serial form issues the same launches in the same order on the context's stream.
    const bool ov = ctx->opt_overlap && ctx->opt_stream != nullptr;
    hipStream_t os = ov ? ctx->opt_stream : st;
    if (ov) {
      CTX_HIP(hipEventRecord(ctx->opt_go, st));   // backward is through with every weight and gradient, the clip coefficient is final
      CTX_HIP(hipStreamWaitEvent(os, ctx->opt_go, 0));
    }
    size_t stage = 0;
    auto stage_done = [&]() -> int {
      if (ov) CTX_HIP(hipEventRecord(ctx->opt_ev[stage], os));
      ++stage;
      return TST_OK;
    };
    // decay group: every matrix that has a transposed copy is updated tile-wise, writing W (bf16) and W^T together; the rest
    // (token embedding of an untied model, learned positions) goes through the flat kernel
    auto flat = [&](const AT* from, const AT* to, float wd) {
      const int64_t o = from - ctx->wb, n = to - from;
      return n <= 0 ? TST_OK : adamw_step<AT>(os, ctx->tp + o, tg + o, ctx->tm + o, ctx->tv + o, n, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2, c.adam_eps, wd,
                                          b1, b2s, ctx->wb + o);
    };
    auto matrix = [&](AT* W, AT* WT, int rows, int cols) {
      if (!WT) return flat(W, W + (int64_t)rows * cols, c.weight_decay);   // (ctx->kmajor bit 0: no transposed copy to keep in step -- 30 B / param)
      const int64_t o = W - ctx->wb;
      return adamw_step_matrix<AT>(os, ctx->tp + o, tg + o, ctx->tm + o, ctx->tv + o, rows, cols, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2, c.adam_eps,
                               c.weight_decay, b1, b2s, W, WT);
    };
    const int d = ctx->d;
    const int slot_full = prof_begin(ctx, os, ctx->prof_hbm);
    // no-decay group first: norm vectors and biases of EVERY layer (a quarter of a million floats; layer 0's forward reads its share)
    CTX_RC(adamw_step<AT>(os, ctx->tp + nd, tg + nd, ctx->tm + nd, ctx->tv + nd, nn, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2, c.adam_eps, 0.0f, b1, b2s,
                      ctx->wb + nd));
    if (ctx->gpt2) {   // wte is also the head: [Vp, d] with its transpose; wpe flat
      CTX_RC(matrix(ctx->embed, ctx->lm_headT, ctx->Vp, d));
      CTX_RC(flat(ctx->wpe, ctx->layers[0].proj[P_QKV].W, c.weight_decay));
    } else {
      CTX_RC(flat(ctx->embed, ctx->layers[0].proj[P_QKV].W, c.weight_decay));
    }
    CTX_RC(stage_done());
    for (auto& W : ctx->layers) {
      for (const ProjT<AT>& P : W.proj) CTX_RC(matrix(P.W, P.WT, P.dout, P.din));
      CTX_RC(stage_done());
    }
    if (!ctx->gpt2) CTX_RC(matrix(ctx->lm_head, ctx->lm_headT, ctx->Vp, d));
    CTX_RC(stage_done());
    // fp32 p, g, m, v read + p, m, v written = 28 B, + the compute copy (and, for the matrices, its transpose where one is kept)
    prof_end(ctx, os, slot_full, PROF_ADAMW, 1, (28.0 + ((ctx->kmajor & 1) ? 1.0 : 2.0) * sizeof(AT)) * ctx->n_train);
    if (ov) { ctx->opt_pending = true; ctx->opt_joined = 0; }
    return TST_OK;
  }
  const int slot = prof_begin(ctx, st, ctx->prof_hbm);
  CTX_RC(adamw_step<AT>(st, ctx->tp, tg, ctx->tm, ctx->tv, ctx->n_train, ctx->clip_out, lr, c.adam_beta1, c.adam_beta2, c.adam_eps, c.weight_decay,
                    (float)bc1, (float)sqrt(bc2), nullptr));
  prof_end(ctx, st, slot, PROF_ADAMW, 1, 28.0 * ctx->n_train);
  CTX_RC(repack(ctx));
  return TST_OK;
}

template <typename AT>
int train_step_dp_body(CtxT<AT>* ctx, const tst_batch* b, float lr, int32_t num_items_global);
template <typename AT>
int train_step_dp_async_impl(CtxT<AT>* ctx, const tst_batch* b, float lr, int32_t num_items_global) {
  if (!ctx->dp_comm) return fail(ctx, TST_ESTATE, "tst_dp_init has not been called on this context (or its group was aborted after a failed step)");
  const int rc = train_step_dp_body(ctx, b, lr, num_items_global);
  if (rc != TST_OK) dp_abort(ctx, "this rank's step failed before or between its collectives");   // the peers must not wait for them
  return rc;
}
template <typename AT>
int train_step_dp_body(CtxT<AT>* ctx, const tst_batch* b, float lr, int32_t num_items_global) {
  if (!ctx->dp_comm) return fail(ctx, TST_ESTATE, "tst_dp_init has not been called on this context");
  if (ctx->ns > 1) return fail(ctx, TST_EINVAL, "a stacked context shares its folds through tst_train_step_stacked_dp_async (per-slot counts and learning rates)");
  if (num_items_global <= 0) return fail(ctx, TST_EINVAL, "num_items_global must be the labelled-token count of the whole micro-batch");
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised: call tst_finalize_weights / tst_init_random first");
  hipStream_t st = ctx->stream;
  ctx->err.clear();
  bool have_rows = false;
  if (b && b->n_tokens > 0) {
    CTX_RC(upload_batch(ctx, b, true, nullptr, 0));
    have_rows = ctx->cur_R > 0;
  }
  if (have_rows) {
    ctx->cur_items = num_items_global;
    CTX_RC(forward(ctx, true));
    CTX_RC(head_forward(ctx, true));
    CTX_RC(backward(ctx, num_items_global, nullptr, true));   // (the gradient regions are reduced as backward finishes them)
  } else {
    // this rank's shard carries no loss term: it contributes a zero gradient and still joins the collectives
    CTX_RC(opt_join(ctx));   // (no forward ran: the previous step's optimizer may still read the gradient)
    CTX_HIP(hipMemsetAsync(ctx->tg, 0, (size_t)ctx->n_train * sizeof(float), st));
    CTX_HIP(hipMemsetAsync(ctx->d_loss, 0, sizeof(float), st));
  }
  // every rank normalised by the global count, so the SUM over the group is the full-batch gradient / loss
  if (!ctx->dp_regions.empty()) {
    if (!have_rows) {   // same collectives in the same order as the ranks that ran backward
      ctx->dp_next = 0;
      CTX_RC(regions_join(ctx));
    }   // else: backward() reduced every region on the communication stream and joined it
  } else if (!ctx->zero_on) {
    CTX_RC(dp_allreduce(ctx, ctx->tg, (size_t)ctx->n_train, st));
  }   // (sharded optimizer state: the gradient is reduce-scattered inside the optimizer step)
  CTX_RC(dp_allreduce(ctx, ctx->d_loss, 1, st));
  CTX_RC(opt_enqueue(ctx, lr, ctx->tg));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], ctx->d_loss, 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[TST_MAX_STACK], ctx->clip_out, 8, hipMemcpyDeviceToHost, st));
  return TST_OK;
}

// ---- gradient accumulation (HF/trainer.py:1740-1758, 2141-2175): micro-batch i of an accumulation window. The flat gradient of the
// micro-batch (normalised by the window's labelled-token count) is added to tacc, its loss to d_loss_acc; the optimizer then steps on the sums.
template <typename AT>
int accumulate_async_impl(CtxT<AT>* ctx, const tst_batch* b, const int32_t* num_items, int first) {
  if (!b || !num_items) return TST_EINVAL;
  if (ctx->dp_comm) return fail(ctx, TST_ESTATE, "gradient accumulation on a data-parallel context is not supported: accumulate by enlarging the group's micro-batch");
  if (!first && !ctx->acc_active) return fail(ctx, TST_ESTATE, "tst_accumulate_async(first = 0) without an open accumulation window");
  hipStream_t st = ctx->stream;
  const int64_t n = ctx->zero_on ? ctx->n_pad : ctx->n_train;
  if (!ctx->tacc) {   // the one allocation outside tst_create: a context that never accumulates does not pay for the buffer
    ctx->tacc = (float*)ctx->pool.alloc((n + TST_MAX_STACK) * (int64_t)sizeof(float));
    if (!ctx->tacc) return fail(ctx, TST_ENOMEM, "hipMalloc failed: gradient accumulation buffer");
    ctx->d_loss_acc = ctx->tacc + n;
  }
  bool steps[TST_MAX_STACK];
  for (int sl = 0; sl < TST_MAX_STACK; ++sl) steps[sl] = first ? false : ctx->slot_steps[sl];
  for (int sl = 0; sl < ctx->ns; ++sl)
    if (num_items[sl] < 0) return fail(ctx, TST_EINVAL, "num_items must be >= 0");
  const int rc = fwd_bwd_enqueue(ctx, b, 0, num_items);
  if (rc != TST_OK) { ctx->acc_active = false; return rc; }
  for (int sl = 0; sl < ctx->ns; ++sl) ctx->slot_steps[sl] = ctx->slot_steps[sl] || steps[sl];
  ctx->gn_fused = false;   // the contraction epilogues' sums of squares describe this micro-batch only
  CTX_RC(grad_accumulate(st, ctx->tacc, ctx->tg, n, first));
  CTX_RC(grad_accumulate(st, ctx->d_loss_acc, ctx->d_loss, TST_MAX_STACK, first));
  ctx->acc_active = true;
  return TST_OK;
}

// optimizer step on the accumulated gradient (or, without an open window, on the gradient of the last tst_forward_backward); lr[stack size]
template <typename AT>
int optimizer_step_async_impl(CtxT<AT>* ctx, const float* lr) {
  const bool acc = ctx->acc_active;
  if (!acc && ctx->grad_stale) return fail(ctx, TST_ESTATE, "an attribution has overwritten the gradient of the last tst_forward_backward: run it again before the optimizer step");
  float* tg = acc ? ctx->tacc : ctx->tg;
  ctx->acc_active = false;
  if (ctx->ns > 1) CTX_RC(opt_enqueue_stacked(ctx, lr, tg));
  else CTX_RC(opt_enqueue(ctx, lr[0], tg));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], acc ? ctx->d_loss_acc : ctx->d_loss, 4 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[TST_MAX_STACK], ctx->clip_out, 8 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  return TST_OK;
}

// ---- stacked folds x data parallelism (the "dp-stacked" layout: every GPU hosts all k folds in the one-GPU layout, the ranks take
// disjoint micro-batches of each fold; HF DDP semantics, TORCH/nn/parallel/distributed.py:828-834). One lockstep step of the context's
// slots on this rank's part of the GLOBAL batch, every slot normalised by its labelled tokens over all ranks, then ONE ncclAllReduce
// over [flat gradient of all slots | per-slot losses], then each slot's own clip + AdamW: every rank ends the step with the same adapters.
template <typename AT>
int train_step_stacked_dp_body(CtxT<AT>* ctx, const tst_batch* b, const float* lrs, const int32_t* items_global) {
  if (ctx->full) return fail(ctx, TST_EINVAL, "tst_train_step_stacked_dp_async is the LoRA layout (a full fine-tune shares a fold through tst_train_step_dp_async)");
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised: call tst_finalize_weights / tst_init_random first");
  if (ctx->acc_active) return fail(ctx, TST_ESTATE, "an accumulation window is open on this context");
  hipStream_t st = ctx->stream;
  ctx->err.clear();
  for (int sl = 0; sl < ctx->ns; ++sl)
    if (items_global[sl] < 0) return fail(ctx, TST_EINVAL, "num_items_global must be >= 0");
  bool have_rows = false;
  if (b && b->n_tokens > 0) {
    // (fwd_bwd_enqueue refuses a batch without labelled tokens; a rank whose part carries none contributes zeros below)
    bool any = false;
    if (b->labels)
      for (int t = 0; t < b->n_tokens && !any; ++t) any = b->labels[t] != -100;
    if (any) {
      CTX_RC(fwd_bwd_enqueue(ctx, b, 0, items_global));
      have_rows = true;
    }
  }
  if (!have_rows) CTX_HIP(hipMemsetAsync(ctx->tg, 0, (size_t)(ctx->n_train + TST_MAX_STACK) * sizeof(float), st));   // gradient and losses
  CTX_RC(dp_allreduce(ctx, ctx->tg, (size_t)ctx->n_train + TST_MAX_STACK, st));
  for (int sl = 0; sl < ctx->ns; ++sl) ctx->slot_steps[sl] = items_global[sl] > 0;   // the same decision on every rank
  if (ctx->ns > 1) CTX_RC(opt_enqueue_stacked(ctx, lrs, ctx->tg));
  else if (ctx->slot_steps[0]) CTX_RC(opt_enqueue(ctx, lrs[0], ctx->tg));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], ctx->d_loss, 4 * TST_MAX_STACK, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[TST_MAX_STACK], ctx->clip_out, 8 * TST_MAX_STACK, hipMemcpyDeviceToHost, st));
  return TST_OK;
}
template <typename AT>
int train_step_stacked_dp_impl(CtxT<AT>* ctx, const tst_batch* b, const float* lrs, const int32_t* items_global) {
  if (!ctx->dp_comm) return fail(ctx, TST_ESTATE, "tst_dp_init has not been called on this context (or its group was aborted after a failed step)");
  const int rc = train_step_stacked_dp_body(ctx, b, lrs, items_global);
  if (rc != TST_OK) dp_abort(ctx, "this rank's step failed before or between its collectives");   // the peers must not wait for them
  return rc;
}

template <typename AT>
int score_async_impl(CtxT<AT>* ctx, const tst_batch* b, const int32_t* option_ids, int32_t n_opt) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  if (n_opt < 0 || n_opt > 256 || (n_opt > 0 && !option_ids)) return fail(ctx, TST_EINVAL, "bad option ids");
  for (int j = 0; j < n_opt; ++j)
    if (option_ids[j] < 0 || option_ids[j] >= ctx->V) return fail(ctx, TST_EINVAL, "option id out of vocabulary");
  ctx->err.clear();
  ctx->score_R = -1;
  CTX_RC(upload_batch(ctx, b, true, nullptr, 0));
  const int R = ctx->cur_R;
  ctx->score_nopt = n_opt;
  ctx->score_row_seq = ctx->row_seq;
  const int* h_tgt = ctx->cur_stage + 2 * ctx->Tmax + (ctx->Smax + 1) + ctx->Rmax;
  ctx->score_tgt.assign(h_tgt, h_tgt + R);
  if (R > 0) {
    if (n_opt > 0) {
      memcpy(ctx->h_opt_ids, option_ids, sizeof(int) * n_opt);
      CTX_HIP(hipMemcpyAsync(ctx->d_opt_ids, ctx->h_opt_ids, sizeof(int) * n_opt, hipMemcpyHostToDevice, ctx->stream));
    }
    CTX_RC(forward(ctx, false));
    CTX_RC(head_forward(ctx, false));
    CTX_RC(logit_rows<AT>(ctx->stream, ctx->logits, ctx->Vp, ctx->d_targets, R, ctx->V, ctx->stats, nullptr, 0, 0.f, n_opt > 0 ? ctx->d_opt_ids : nullptr, n_opt,
                      ctx->optl));
    CTX_HIP(hipMemcpyAsync(ctx->h_score, ctx->stats, (size_t)R * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (n_opt > 0) CTX_HIP(hipMemcpyAsync(ctx->h_score + (size_t)ctx->Rmax * 4, ctx->optl, (size_t)R * n_opt * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  CTX_HIP(hipEventRecord(ctx->score_evt, ctx->stream));
  ctx->score_R = R;
  return TST_OK;
}

// ---- greedy generation: prefill + max_new - 1 decode steps, all enqueued at once (include/tst_hip.h tst_generate_async)
int gen_reserve(tst_ctx* ctx, int max_new) {
  if (ctx->gen_kv && max_new <= ctx->gen_cap_new) return TST_OK;
  const tsthost::BatchLimits lim = batch_limits(ctx);
  if (ctx->gen_kv) {   // a larger max_new: nothing of the old buffers may be in flight
    CTX_RC(ctx_sync(ctx));
    ctx->pool.free_one(ctx->gen_kv, ctx->gen_kv_bytes);
    ctx->pool.free_one(ctx->gen_dev, ctx->gen_dev_bytes);
    ctx->pool.free_one(ctx->gen_tok, ctx->gen_out_bytes);
    if (ctx->h_gen) (void)hipHostFree(ctx->h_gen);
    ctx->gen_kv = nullptr; ctx->gen_dev = nullptr; ctx->gen_tok = nullptr; ctx->gen_logp = nullptr; ctx->h_gen = nullptr;
    ctx->gen_cap_new = 0; ctx->gen_S = -1;
  }
  const long rows = tsthost::gen_cache_rows(lim, max_new);
  const size_t esz = ctx->strict ? 4 : 2;
  ctx->gen_kv_bytes = (int64_t)ctx->L * 2 * rows * ctx->Hkv * ctx->dh * (int64_t)esz;
  ctx->gen_dev_bytes = (int64_t)tsthost::gen_dev_ints(lim, max_new) * 4;
  ctx->gen_out_bytes = (int64_t)ctx->Smax * max_new * 8;
  ctx->gen_kv = ctx->pool.alloc(ctx->gen_kv_bytes);
  ctx->gen_dev = (int*)ctx->pool.alloc(ctx->gen_dev_bytes);
  ctx->gen_tok = (int*)ctx->pool.alloc(ctx->gen_out_bytes);
  if (!ctx->gen_kv || !ctx->gen_dev || !ctx->gen_tok) {
    if (ctx->gen_kv) ctx->pool.free_one(ctx->gen_kv, ctx->gen_kv_bytes);
    if (ctx->gen_dev) ctx->pool.free_one(ctx->gen_dev, ctx->gen_dev_bytes);
    if (ctx->gen_tok) ctx->pool.free_one(ctx->gen_tok, ctx->gen_out_bytes);
    ctx->gen_kv = nullptr; ctx->gen_dev = nullptr; ctx->gen_tok = nullptr;
    return fail(ctx, TST_ENOMEM, "hipMalloc failed: KV cache of the generation");
  }
  ctx->gen_logp = (float*)(ctx->gen_tok + (size_t)ctx->Smax * max_new);
  CTX_HIP(hipStreamSynchronize(nullptr));   // the pool zero-fills on the null stream: it must not land behind this generation's first cache writes
  CTX_HIP(hipHostMalloc((void**)&ctx->h_gen, (size_t)(ctx->gen_dev_bytes + ctx->gen_out_bytes), hipHostMallocDefault));
  if (!ctx->gen_evt) CTX_HIP(hipEventCreateWithFlags(&ctx->gen_evt, hipEventDisableTiming));
  CTX_HIP(hipEventRecord(ctx->gen_evt, ctx->stream));
  ctx->gen_rows = rows;
  ctx->gen_cap_new = max_new;
  return TST_OK;
}

template <typename AT>
int generate_async_impl(CtxT<AT>* ctx, const tst_batch* b, int32_t max_new, const int32_t* eos_ids, int32_t n_eos) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  ctx->err.clear();
  // what a generation adds to a batch's checks is refused here, before an allocation or a launch (plan_generate walks cu_seqlens and seq_slot itself to build
  // the row map, so it repeats plan_batch's checks of those two)
  const tsthost::BatchLimits lim = batch_limits(ctx);
  tsthost::GenPlan plan;
  {
    std::string perr;
    if (tsthost::plan_generate(b, lim, max_new, eos_ids, n_eos, plan, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
  }
  if (ctx->H % ctx->Hkv || ctx->H / ctx->Hkv > 8 || (ctx->dh != 64 && ctx->dh != 128))
    return fail(ctx, TST_EINVAL, "generation needs head_dim 64 or 128 and at most 8 query heads per kv head");
  hipStream_t st = ctx->stream;
  const int S = plan.S;
  // the prompts as a batch whose head rows are the last token of each: upload_batch refuses what plan_batch finds (ids outside the vocabulary) on the host,
  // before its own copies -- and before the cache is allocated or grown, so a refused generation leaves the context's memory as it was
  CTX_RC(upload_batch(ctx, b, false, plan.last_rows.data(), S));
  ctx->gen_S = -1;
  CTX_RC(gen_reserve(ctx, max_new));
  CTX_RC(ctx_event_sync(ctx, ctx->gen_evt));   // the staging image may still feed the previous generation's copy
  {
    int* h = ctx->h_gen;
    const size_t o_pre = (size_t)3 + 2 * (size_t)ctx->Smax, o_dec = o_pre + (size_t)ctx->Tmax;
    memcpy(h, plan.meta.data(), plan.meta.size() * sizeof(int));
    memcpy(h + o_pre, plan.prefill_rows.data(), plan.prefill_rows.size() * sizeof(int));
    if (!plan.decode_rows.empty()) memcpy(h + o_dec, plan.decode_rows.data(), plan.decode_rows.size() * sizeof(int));
    CTX_HIP(hipMemcpyAsync(ctx->gen_dev, h, (o_dec + plan.decode_rows.size()) * sizeof(int), hipMemcpyHostToDevice, st));
  }
  auto step_tail = [&](int j) -> int {
    CTX_RC(head_forward(ctx, false));
    CTX_RC(logit_rows<AT>(st, ctx->logits, ctx->Vp, ctx->d_targets, S, ctx->V, ctx->stats, nullptr, 0, 0.f, nullptr, 0, ctx->optl));
    return next_token(st, ctx->stats, ctx->gen_dev, S, j, ctx->gen_tok, ctx->gen_logp, ctx->d_ids, ctx->d_pos, ctx->d_lab_idx);
  };
  CTX_RC(forward(ctx, false, GenPass{1, 0}));   // prefill
  CTX_RC(step_tail(0));
  if (max_new > 1) {
    // decode steps: the same forward() over one row per sequence. "Tokens" are sequences now: the slot boundaries are sequence counts, the head reads every row
    ctx->cur_T = ctx->cur_S = ctx->cur_R = S;
    ctx->cur_maxlen = 1;
    for (int q = 0; q < TST_MAX_STACK; ++q) ctx->slot_ends.t_end[q] = ctx->row_ends.t_end[q] = plan.slot_s_end[q];
    double keys = (double)plan.T;
    for (int j = 1; j < max_new; ++j) {
      keys += S;
      ctx->cur_sumsq_len = keys;
      CTX_RC(forward(ctx, false, GenPass{2, j}));
      CTX_RC(step_tail(j));
    }
  }
  float* h_out = (float*)(ctx->h_gen + ctx->gen_dev_bytes / 4);
  CTX_HIP(hipMemcpyAsync(h_out, ctx->gen_tok, (size_t)S * max_new * 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipMemcpyAsync(h_out + (size_t)ctx->Smax * ctx->gen_cap_new, ctx->gen_logp, (size_t)S * max_new * 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipEventRecord(ctx->gen_evt, st));
  ctx->gen_eos.assign(eos_ids, eos_ids + n_eos);
  ctx->gen_S = S;
  ctx->gen_new = max_new;
  ctx->gen_samples = 0;
  ctx->gen_cand = 0;
  return TST_OK;
}

// ---- sampled generation: ONE prefill over the S prompts, then n_samples draws of each as S n_samples decode rows that share the prompt's cache rows
// (include/tst_hip.h tst_sample_async; kernels in decode.hip, row map in host_logic.h plan_sample). The cache, the device image, the output block and the pending
// slot are the greedy generation's.
// the seeds of a sampled generation: 8 bytes per max_seqs on the device and pinned, allocated by the first tst_sample_async of a context and counted in
// tst_device_bytes (the generation's own image has no room for them: geo | prefill rows | decode rows fill it exactly)
int sample_reserve(tst_ctx* ctx) {
  if (!ctx->smp_seeds) {
    ctx->smp_seeds = (int*)ctx->pool.alloc(8 * (int64_t)ctx->Smax);
    if (!ctx->smp_seeds) return fail(ctx, TST_ENOMEM, "hipMalloc failed: seeds of the sampled generation");
    CTX_HIP(hipStreamSynchronize(nullptr));   // (the pool's zero fill, as in gen_reserve)
  }
  if (!ctx->h_smp_seeds) CTX_HIP(hipHostMalloc((void**)&ctx->h_smp_seeds, 8 * (size_t)ctx->Smax, hipHostMallocDefault));
  return TST_OK;
}

template <typename AT>
int sample_async_impl(CtxT<AT>* ctx, const tst_batch* b, int32_t max_new, int32_t n_samples, float temperature, const uint64_t* seq_seeds, const int32_t* eos_ids,
                      int32_t n_eos) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  ctx->err.clear();
  const tsthost::BatchLimits lim = batch_limits(ctx);
  tsthost::SamplePlan plan;
  {
    std::string perr;
    if (tsthost::plan_sample(b, lim, max_new, n_samples, temperature, seq_seeds, eos_ids, n_eos, plan, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
  }
  if (ctx->H % ctx->Hkv || ctx->H / ctx->Hkv > 8 || (ctx->dh != 64 && ctx->dh != 128))
    return fail(ctx, TST_EINVAL, "generation needs head_dim 64 or 128 and at most 8 query heads per kv head");
  hipStream_t st = ctx->stream;
  const int S = plan.S, R = plan.R;
  CTX_RC(upload_batch(ctx, b, false, plan.last_rows.data(), S));   // (refuses a host id outside the vocabulary before the cache is allocated or grown)
  ctx->gen_S = -1;
  CTX_RC(gen_reserve(ctx, max_new));
  CTX_RC(sample_reserve(ctx));
  CTX_RC(ctx_event_sync(ctx, ctx->gen_evt));   // the staging images may still feed the previous generation's copies
  const size_t o_pre = tsthost::sample_off_prefill(lim), o_dec = tsthost::sample_off_decode(lim);
  {
    int* h = ctx->h_gen;
    memcpy(h, plan.geo.data(), plan.geo.size() * sizeof(int));
    memcpy(ctx->h_smp_seeds, plan.seeds.data(), plan.seeds.size() * sizeof(int));
    CTX_HIP(hipMemcpyAsync(ctx->smp_seeds, ctx->h_smp_seeds, plan.seeds.size() * sizeof(int), hipMemcpyHostToDevice, st));
    memcpy(h + o_pre, plan.prefill_rows.data(), plan.prefill_rows.size() * sizeof(int));
    if (!plan.decode_rows.empty()) memcpy(h + o_dec, plan.decode_rows.data(), plan.decode_rows.size() * sizeof(int));
    CTX_HIP(hipMemcpyAsync(ctx->gen_dev, h, (o_dec + plan.decode_rows.size()) * sizeof(int), hipMemcpyHostToDevice, st));
  }
  const float inv_temp = 1.0f / temperature;
  auto step_tail = [&](int j) -> int {
    CTX_RC(head_forward(ctx, false));   // step 0: the S last rows of the prompts; afterwards the R decode rows
    return sample_rows(st, ctx->logits, ctx->Vp, ctx->V, ctx->gen_dev, ctx->smp_seeds, R, j, inv_temp, ctx->gen_tok, ctx->gen_logp, ctx->d_ids, ctx->d_pos,
                       ctx->d_lab_idx);
  };
  CTX_RC(forward(ctx, false, GenPass{1, 0, true}));   // prefill
  CTX_RC(step_tail(0));
  if (max_new > 1) {
    // decode steps: forward() over one row per draw; the slot boundaries are decode-row counts (rows are s-major: a stacked context's slot order is kept)
    ctx->cur_T = ctx->cur_S = ctx->cur_R = R;
    ctx->cur_maxlen = 1;
    for (int q = 0; q < TST_MAX_STACK; ++q) ctx->slot_ends.t_end[q] = ctx->row_ends.t_end[q] = plan.slot_r_end[q];
    double keys = (double)plan.T * n_samples;
    for (int j = 1; j < max_new; ++j) {
      keys += R;
      ctx->cur_sumsq_len = keys;
      CTX_RC(forward(ctx, false, GenPass{2, j, true}));
      CTX_RC(step_tail(j));
    }
  }
  float* h_out = (float*)(ctx->h_gen + ctx->gen_dev_bytes / 4);
  CTX_HIP(hipMemcpyAsync(h_out, ctx->gen_tok, (size_t)R * max_new * 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipMemcpyAsync(h_out + (size_t)ctx->Smax * ctx->gen_cap_new, ctx->gen_logp, (size_t)R * max_new * 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipEventRecord(ctx->gen_evt, st));
  ctx->gen_eos.assign(eos_ids, eos_ids + n_eos);
  ctx->gen_S = R;
  ctx->gen_new = max_new;
  ctx->gen_samples = n_samples;
  ctx->gen_cand = 0;
  return TST_OK;
}

// ---- candidate scoring: ONE prefill over the S prompts, then ONE forward pass over the R_e extend rows "candidate c, position p" (include/tst_hip.h
// tst_score_candidates_async; kernels in decode.hip, row map in host_logic.h plan_candidates). The cache and the pending slot are the generation's (a one-token
// generation's cache holds T + R_e rows); the geometry image and the output block are the call's own.
int cand_reserve(tst_ctx* ctx) {
  const tsthost::BatchLimits lim = batch_limits(ctx);
  const size_t ints = tsthost::cand_dev_ints(lim);
  if (!ctx->cand_dev) {
    ctx->cand_dev = (int*)ctx->pool.alloc((int64_t)(ints + (size_t)ctx->Rmax) * 4);
    if (!ctx->cand_dev) return fail(ctx, TST_ENOMEM, "hipMalloc failed: buffers of the candidate scoring");
    CTX_HIP(hipStreamSynchronize(nullptr));   // (the pool's zero fill, as in gen_reserve)
  }
  if (!ctx->h_cand) CTX_HIP(hipHostMalloc((void**)&ctx->h_cand, (ints + 4 * (size_t)tsthost::cand_ext_cap(lim) + (size_t)ctx->Rmax) * 4, hipHostMallocDefault));
  return TST_OK;
}

template <typename AT>
int score_candidates_async_impl(CtxT<AT>* ctx, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int32_t n_cands) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  ctx->err.clear();
  const tsthost::BatchLimits lim = batch_limits(ctx);
  tsthost::CandPlan plan;
  {
    std::string perr;
    if (tsthost::plan_candidates(b, lim, cand_ids, cu_cand, cand_seq, n_cands, plan, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
  }
  if (ctx->H % ctx->Hkv || ctx->H / ctx->Hkv > 8 || (ctx->dh != 64 && ctx->dh != 128))
    return fail(ctx, TST_EINVAL, "generation needs head_dim 64 or 128 and at most 8 query heads per kv head");
  hipStream_t st = ctx->stream;
  const int S = plan.S, R = plan.R_e, N = plan.n_tok;
  CTX_RC(upload_batch(ctx, b, false, plan.last_rows.data(), S));   // (refuses a host id outside the vocabulary before anything is allocated or grown)
  ctx->gen_S = -1;
  CTX_RC(gen_reserve(ctx, 1));
  CTX_RC(cand_reserve(ctx));
  CTX_RC(ctx_event_sync(ctx, ctx->gen_evt));   // the staging images may still feed the previous call's copies
  const size_t o_pre = tsthost::sample_off_prefill(lim), o_rows = tsthost::cand_off_rows(lim), o_src = tsthost::cand_off_src(lim), ints = tsthost::cand_dev_ints(lim);
  const size_t cap_e = (size_t)tsthost::cand_ext_cap(lim);
  int* h = ctx->h_cand;
  int* h_ext = h + ints;                               // ids | pos | lab_idx | targets of the extend rows
  float* h_out = (float*)(h_ext + 4 * cap_e);
  float* d_out = (float*)(ctx->cand_dev + ints);
  {
    memcpy(ctx->h_gen + o_pre, plan.prefill_rows.data(), plan.prefill_rows.size() * sizeof(int));
    CTX_HIP(hipMemcpyAsync(ctx->gen_dev + o_pre, ctx->h_gen + o_pre, plan.prefill_rows.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!plan.geo.empty()) memcpy(h, plan.geo.data(), plan.geo.size() * sizeof(int));
    if (R > 0) memcpy(h + o_rows, plan.ext_rows.data(), (size_t)R * sizeof(int));
    memcpy(h + o_src, plan.src.data(), plan.src.size() * sizeof(int));
    CTX_HIP(hipMemcpyAsync(ctx->cand_dev, h, (o_src + plan.src.size()) * sizeof(int), hipMemcpyHostToDevice, st));
    for (int r = 0; r < R; ++r) {
      h_ext[r] = plan.ext_ids[(size_t)r];
      h_ext[cap_e + r] = plan.ext_pos[(size_t)r];
      h_ext[2 * cap_e + r] = r;   // the head reads every row of the extend pass
      h_ext[3 * cap_e + r] = plan.ext_tgt[(size_t)r];
    }
  }
  const int* d_src = ctx->cand_dev + o_src;
  CTX_RC(forward(ctx, false, GenPass{1, 0, true}));   // prefill: the sampled generation's, prompts at cache rows 0 .. T
  CTX_RC(head_forward(ctx, false));
  CTX_RC(logit_rows<AT>(st, ctx->logits, ctx->Vp, ctx->d_targets, S, ctx->V, ctx->stats, nullptr, 0, 0.f, nullptr, 0, ctx->optl));   // (for its lse)
  // first tokens: from prompt s's one logits row, before the extend pass overwrites logits and stats
  CTX_RC(cand_logp(st, ctx->logits, ctx->Vp, ctx->V, ctx->stats, S, d_src, N, 0, d_out));
  if (R > 0) {
    // the extend pass: forward() over one row per (candidate, position); ids, positions, head rows and targets were laid out on the host
    const size_t rb = (size_t)R * sizeof(int);
    CTX_HIP(hipMemcpyAsync(ctx->d_ids, h_ext, rb, hipMemcpyHostToDevice, st));
    CTX_HIP(hipMemcpyAsync(ctx->d_pos, h_ext + cap_e, rb, hipMemcpyHostToDevice, st));
    CTX_HIP(hipMemcpyAsync(ctx->d_lab_idx, h_ext + 2 * cap_e, rb, hipMemcpyHostToDevice, st));
    CTX_HIP(hipMemcpyAsync(ctx->d_targets, h_ext + 3 * cap_e, rb, hipMemcpyHostToDevice, st));
    ctx->cur_T = ctx->cur_S = ctx->cur_R = R;
    ctx->cur_maxlen = 1;
    ctx->cand_n_ext = plan.n_ext;
    for (int q = 0; q < TST_MAX_STACK; ++q) ctx->slot_ends.t_end[q] = ctx->row_ends.t_end[q] = plan.slot_r_end[q];
    double keys = 0;
    for (int r = 0; r < R; ++r) keys += (double)plan.ext_pos[(size_t)r] + 1.0;
    ctx->cur_sumsq_len = keys;
    CTX_RC(forward(ctx, false, GenPass{3, 0, true}));
    CTX_RC(head_forward(ctx, false));
    CTX_RC(logit_rows<AT>(st, ctx->logits, ctx->Vp, ctx->d_targets, R, ctx->V, ctx->stats, nullptr, 0, 0.f, nullptr, 0, ctx->optl));
    CTX_RC(cand_logp(st, ctx->logits, ctx->Vp, ctx->V, ctx->stats, R, d_src, N, 1, d_out));
  }
  CTX_HIP(hipMemcpyAsync(h_out, d_out, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  CTX_HIP(hipEventRecord(ctx->gen_evt, st));
  ctx->cand_cu.assign(cu_cand, cu_cand + n_cands + 1);
  ctx->gen_S = N;
  ctx->gen_new = 0;
  ctx->gen_samples = 0;
  ctx->gen_cand = n_cands;
  return TST_OK;
}

// ---- token attribution (include/tst_hip.h tst_attribute_async): forward with the stash, head, the backward pass seeded with d (sum_i log s(x_i)) / d logits
// down to the gradient of layer 0's input, then one reduction per token
int attr_reserve(tst_ctx* ctx) {
  if (ctx->attr_dev) return TST_OK;
  const int64_t words = 2 * (int64_t)ctx->Rmax + tsthost::kAttrMaxOpt + 2 * (int64_t)ctx->Tmax;
  float* dev = (float*)ctx->pool.alloc(words * 4);
  if (!dev) return fail(ctx, TST_ENOMEM, "hipMalloc failed: attribution buffers");
  CTX_HIP(hipStreamSynchronize(nullptr));   // the pool zero-fills on the null stream: it must not land behind this attribution's first writes
  if (!ctx->h_attr) CTX_HIP(hipHostMalloc((void**)&ctx->h_attr, (size_t)(words + 4 * (int64_t)ctx->Rmax) * 4, hipHostMallocDefault));
  if (!ctx->attr_evt) CTX_HIP(hipEventCreateWithFlags(&ctx->attr_evt, hipEventDisableTiming));
  CTX_HIP(hipEventRecord(ctx->attr_evt, ctx->stream));
  ctx->attr_dev = dev;
  return TST_OK;
}

// integrated gradients add the device baseline ids and the per-token sum to those (layout at tst_ctx::ig_dev)
int ig_reserve(tst_ctx* ctx) {
  const int64_t words = 2 * (int64_t)ctx->Tmax;
  if (!ctx->ig_dev) {   // (kept at once: a failure further down must not leave the block to be allocated, and counted, a second time)
    ctx->ig_dev = (float*)ctx->pool.alloc(words * 4);
    if (!ctx->ig_dev) return fail(ctx, TST_ENOMEM, "hipMalloc failed: integrated-gradients buffers");
    CTX_HIP(hipStreamSynchronize(nullptr));   // (the pool's zero fill, as in attr_reserve)
  }
  if (!ctx->h_ig) CTX_HIP(hipHostMalloc((void**)&ctx->h_ig, (size_t)(words + 8 * (int64_t)ctx->Rmax) * 4, hipHostMallocDefault));
  return TST_OK;
}

// forward with the stash, head, and the backward pass of an attribution down to dX, the gradient of layer 0's input (backward joins its side streams)
template <typename AT>
int attr_forward_backward(CtxT<AT>* ctx, bool interp = false, float alpha = 1.0f) {
  CTX_RC(forward(ctx, true, {}, AttrPass{false, interp, alpha}));
  CTX_RC(head_forward(ctx, true));
  return backward(ctx, ctx->cur_R, nullptr, false, AttrPass{true});
}

// The passes of an integrated-gradients call, behind the uploads of attribute_async_impl. Everything is enqueued at once -- a forward + head pass at the baseline
// (alpha = 0) and one at the real prompt (alpha = 1) for the two log s, then n_steps times embed_interp(alpha_k) -> forward -> head -> backward -> token_ig -- with
// no host wait in between; the caller records one event behind the result copies.
template <typename AT>
int ig_enqueue(CtxT<AT>* ctx, const int32_t* baseline_ids, int n_steps) {
  hipStream_t st = ctx->stream;
  const int R = ctx->cur_R, S = ctx->cur_S, T = ctx->cur_T, Rmax = ctx->Rmax, Tmax = ctx->Tmax;
  // the baseline ids follow the input ids onto the device: the tokens upload_batch kept, in its order
  if (tsthost::trim_tokens_i32(baseline_ids, ctx->attr_cu_dev.data(), ctx->attr_cu_src.data(), S, (int32_t*)ctx->h_ig) != TST_OK)
    return fail(ctx, TST_EINVAL, "internal: trim map");
  int* d_bids = (int*)ctx->ig_dev;
  float* d_acc = ctx->ig_dev + Tmax;
  CTX_HIP(hipMemcpyAsync(d_bids, ctx->h_ig, (size_t)T * 4, hipMemcpyHostToDevice, st));
  float* h_res = ctx->h_ig + Tmax;
  for (int end = 0; end < 2; ++end) {   // log s at the baseline, then at the real prompt: attr_seed for the row statistics it leaves, no backward
    CTX_RC(forward(ctx, true, {}, AttrPass{false, true, (float)end}));
    CTX_RC(head_forward(ctx, true));
    CTX_RC(attr_seed_rows(ctx));
    CTX_HIP(hipMemcpyAsync(h_res + Tmax + (size_t)end * 4 * Rmax, ctx->stats, (size_t)R * 16, hipMemcpyDeviceToHost, st));
  }
  const float w = 1.0f / (float)n_steps;
  for (int k = 1; k <= n_steps; ++k) {
    CTX_RC(attr_forward_backward(ctx, true, tsthost::ig_alpha(k, n_steps)));
    // (dX is the gradient at x_k; the step's term is taken against e - b from the table, not against x_k)
    CTX_RC(token_ig<AT>(st, ctx->dX, ctx->embed, ctx->d_ids, d_bids, T, ctx->d, ctx->V, w, k == 1, d_acc));
  }
  CTX_HIP(hipMemcpyAsync(h_res, d_acc, (size_t)T * 4, hipMemcpyDeviceToHost, st));
  return TST_OK;
}

// ig = false: the plain attribution (one forward + head + backward, token_attr). ig = true: integrated gradients from baseline_ids over n_steps midpoints.
template <typename AT>
int attribute_async_impl(CtxT<AT>* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, const int32_t* baseline_ids = nullptr,
                         int32_t n_steps = 0, bool ig = false) {
  if (!b) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  if (ctx->acc_active) return fail(ctx, TST_ESTATE, "an accumulation window is open on this context: an attribution would overwrite the micro-batch gradient path");
  if (ctx->dp_comm) return fail(ctx, TST_ESTATE, "attribution on a context that has joined a data-parallel group is not supported");
  ctx->err.clear();
  tsthost::AttrPlan plan;
  {
    std::string perr;
    if (tsthost::plan_attribute(b, batch_limits(ctx), seq_kind, option_ids, n_opt, plan, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
    if (ig && tsthost::plan_ig(b, batch_limits(ctx), baseline_ids, n_steps, perr) != TST_OK) return fail(ctx, TST_EINVAL, perr);
  }
  CTX_RC(upload_batch(ctx, b, true, nullptr, 0));   // (the batch's own checks: nothing is copied or allocated for a refused batch)
  if (ctx->cur_R != plan.R) return fail(ctx, TST_EINVAL, "internal: labelled rows of plan_batch and plan_attribute differ");
  ctx->attr_S = -1;
  CTX_RC(attr_reserve(ctx));
  if (ig) CTX_RC(ig_reserve(ctx));
  CTX_RC(ctx_event_sync(ctx, ctx->attr_evt));   // the staging image may still feed the previous attribution's copies
  hipStream_t st = ctx->stream;
  const int R = plan.R, S = ctx->cur_S, T = ctx->cur_T, Rmax = ctx->Rmax, Tmax = ctx->Tmax;
  const size_t head_words = 2 * (size_t)Rmax + tsthost::kAttrMaxOpt;
  {
    float* h = ctx->h_attr;
    memcpy(h, plan.row_w.data(), sizeof(float) * (size_t)R);
    memcpy(h + Rmax, plan.row_kind.data(), sizeof(int) * (size_t)R);
    if (n_opt > 0) memcpy(h + 2 * (size_t)Rmax, option_ids, sizeof(int) * (size_t)n_opt);
    CTX_HIP(hipMemcpyAsync(ctx->attr_dev, h, head_words * 4, hipMemcpyHostToDevice, st));
  }
  ctx->attr_nopt = n_opt;
  const int* h_cu = ctx->cur_stage + 2 * Tmax;
  ctx->attr_cu_dev.assign(h_cu, h_cu + S + 1);
  ctx->attr_cu_src.assign(b->cu_seqlens, b->cu_seqlens + S + 1);
  ctx->grad_stale = true;
  if (ig) {
    CTX_RC(ig_enqueue(ctx, baseline_ids, n_steps));
  } else {
    CTX_RC(attr_forward_backward(ctx));
    // (dX is the gradient of layer 0's stashed input, the embedding-layer output -- for GPT-2 wte + wpe)
    float* gxi = ctx->attr_dev + head_words;
    CTX_RC(token_attr<AT>(st, ctx->dX, ctx->layers[0].x_in, T, ctx->d, gxi, gxi + Tmax));
    float* h_res = ctx->h_attr + head_words;
    CTX_HIP(hipMemcpyAsync(h_res, gxi, (size_t)T * 4, hipMemcpyDeviceToHost, st));
    CTX_HIP(hipMemcpyAsync(h_res + Tmax, gxi + Tmax, (size_t)T * 4, hipMemcpyDeviceToHost, st));
    CTX_HIP(hipMemcpyAsync(h_res + 2 * (size_t)Tmax, ctx->stats, (size_t)R * 16, hipMemcpyDeviceToHost, st));
  }
  CTX_HIP(hipEventRecord(ctx->attr_evt, st));
  ctx->attr_plan = std::move(plan);
  ctx->attr_ig = ig;
  ctx->attr_S = S;
  return TST_OK;
}

template <typename AT>
int forward_logits_impl(CtxT<AT>* ctx, const tst_batch* b, const int32_t* rows, int32_t n_rows, float* logits_out) {
  if (!b || !rows || !logits_out || n_rows <= 0) return TST_EINVAL;
  if (!ctx->finalized) return fail(ctx, TST_ESTATE, "weights not finalised");
  ctx->err.clear();
  CTX_RC(upload_batch(ctx, b, false, rows, n_rows));
  CTX_RC(forward(ctx, false));
  CTX_RC(head_forward(ctx, false));
  CTX_RC(ctx_sync(ctx));
  CTX_HIP(hipMemcpy2D(logits_out, (size_t)ctx->V * 4, ctx->logits, (size_t)ctx->Vp * 4, (size_t)ctx->V * 4, (size_t)n_rows, hipMemcpyDeviceToHost));
  return TST_OK;
}

// ---- shader-clock probe (measurement hook tst_clock_probe): one wave stamps the shader-clock counter (s_memtime) and the constant 100 MHz counter
// (s_memrealtime) around a spin of `spin_ticks` real-time ticks: held clock = d(s_memtime) / d(s_memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS
// give-back item 6). The stamps go to a buffer of their own; nothing else reads them. Bounded: the spin ends after spin_ticks real-time ticks.
__global__ void clock_probe_kernel(unsigned long long* out, unsigned long long spin_ticks) {
  if (threadIdx.x != 0) return;
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < spin_ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  out[0] = c1 - c0;
  out[1] = r1 - r0;
}
struct ClockProbe {
  std::mutex mu;
  hipStream_t st[16] = {};
  unsigned long long* host[16] = {};
};
ClockProbe g_clock;

// precision dispatch: a tst_ctx is a CtxT<float> (strict) or a CtxT<bf16_t>
template <typename F>
int typed(tst_ctx* c, F&& f) {
  return c->strict ? f(static_cast<CtxT<float>*>(c)) : f(static_cast<CtxT<bf16_t>*>(c));
}
}  // namespace

extern "C" {

int tst_set_tile_policy(int level) { return gemm_big_tile_level(level); }
int tst_set_option(tst_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return TST_EINVAL;
  if (!strcmp(name, "last_compact")) {
    if (!ctx->lc_have) return TST_EINVAL;
    if (value >= 0) ctx->lc_on = value != 0;
    return ctx->lc_on ? 1 : 0;
  }
  if (!strcmp(name, "dw_side")) {
    if (!ctx->full || !ctx->side) return TST_EINVAL;
    if (value >= 0) ctx->dw_side = value != 0;
    return ctx->dw_side ? 1 : 0;
  }
  if (!strcmp(name, "kmajor")) {   // read-only view of both bits (fixed at creation: without bit 0 the transposed weight copy is allocated, without bit 1 the transposed scratch)
    return ctx->kmajor;
  }
  if (!strcmp(name, "ndw_side")) {
    if (!ctx->full || !ctx->side) return TST_EINVAL;
    if (value >= 0) ctx->ndw_side = value != 0;
    return ctx->ndw_side ? 1 : 0;
  }
  if (!strcmp(name, "opt_overlap")) {
    if (!ctx->opt_stream) return TST_EINVAL;
    if (value >= 0) ctx->opt_overlap = value != 0;
    return ctx->opt_overlap ? 1 : 0;
  }
  if (!strcmp(name, "norm_bwd_dw")) {
    if (!ctx->full) return TST_EINVAL;
    if (value >= 0) ctx->nbdw = value & 1;
    return ctx->nbdw;
  }
  if (!strcmp(name, "norm_rank")) {
    if (value >= 0) ctx->nrk = value & 1;
    return ctx->nrk;
  }
  if (!strcmp(name, "swiglu_rank")) {
    if (value >= 0) ctx->swr = value & 3;
    return ctx->swr;
  }
  if (!strcmp(name, "trim_last_token")) {
    if (value >= 0) ctx->trim_last = value != 0;
    return ctx->trim_last ? 1 : 0;
  }
  return TST_EINVAL;
}

int tst_abi_struct_sizes(int32_t* model_cfg_bytes, int32_t* batch_bytes) {
  if (model_cfg_bytes) *model_cfg_bytes = (int32_t)sizeof(tst_model_cfg);
  if (batch_bytes) *batch_bytes = (int32_t)sizeof(tst_batch);
  return TST_OK;
}

int tst_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tst_create(const tst_model_cfg* cfg, int device, tst_ctx** out) {
  if (!cfg || !out) { g_create_err = "null argument"; return TST_EINVAL; }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    g_create_err = "no HIP device visible: libtst_hip has no CPU fallback";
    return TST_EHIP;
  }
  if (device < 0 || device >= n) { g_create_err = "device index out of range"; return TST_EINVAL; }
  if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return TST_EHIP; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_err = "hipGetDeviceProperties failed"; return TST_EHIP; }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_err = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only";
    return TST_EHIP;
  }
  if (const int rc = tsthost::check_cfg(*cfg, false, g_create_err)) return rc;   // (before anything is allocated; the precision decides the context's type)
  const bool strict = cfg->precision == TST_PRECISION_STRICT;
  tst_ctx* ctx = strict ? static_cast<tst_ctx*>(new CtxT<float>()) : static_cast<tst_ctx*>(new CtxT<bf16_t>());
  ctx->cfg = *cfg;
  ctx->strict = strict;
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_err = "hipStreamCreate failed";
    delete ctx;
    return TST_EHIP;
  }
  ctx->own_stream = ctx->stream;
  int rc = typed(ctx, [&](auto* c) { return build_ctx(c); });
  if (rc != TST_OK) {
    g_create_err = ctx->err;
    tst_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return TST_OK;
}

int tst_fork(tst_ctx* parent, tst_ctx** out) {
  if (!parent || !out) return TST_EINVAL;
  *out = nullptr;
  return typed(parent, [&](auto* c) { return fork_impl(c, out); });
}

int tst_destroy(tst_ctx* ctx) {
  if (!ctx) return TST_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->dp_comm && ctx->stream) (void)dp_wait(ctx, ctx->stream);   // bounded: a dead peer ends in ncclCommAbort, after which the kernels exit
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->dp_stream) (void)hipStreamSynchronize(ctx->dp_stream);
  if (ctx->dp_comm) (void)ncclCommDestroy(ctx->dp_comm);
  if (ctx->dp_stream) (void)hipStreamDestroy(ctx->dp_stream);
  if (ctx->dp_ev) (void)hipEventDestroy(ctx->dp_ev);
  if (ctx->dp_done) (void)hipEventDestroy(ctx->dp_done);
  if (ctx->opt_stream) (void)hipStreamSynchronize(ctx->opt_stream);
  if (ctx->opt_stream && !ctx->opt_stream_shared) (void)hipStreamDestroy(ctx->opt_stream);
  if (ctx->opt_go) (void)hipEventDestroy(ctx->opt_go);
  for (auto& e : ctx->opt_ev) if (e) (void)hipEventDestroy(e);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); if (!ctx->side_shared) (void)hipStreamDestroy(ctx->side); }
  for (auto& e : ctx->ev_ndw) if (e) (void)hipEventDestroy(e);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  for (auto& e : ctx->prof_events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (ctx->prof_ref) (void)hipEventDestroy(ctx->prof_ref);
  ctx->pool.release();
  for (int i = 0; i < 2; ++i) {
    if (ctx->h_stage[i]) (void)hipHostFree(ctx->h_stage[i]);
    if (ctx->stage_evt[i]) (void)hipEventDestroy(ctx->stage_evt[i]);
  }
  if (ctx->h_metrics) (void)hipHostFree(ctx->h_metrics);
  if (ctx->h_score) (void)hipHostFree(ctx->h_score);
  if (ctx->h_gen) (void)hipHostFree(ctx->h_gen);
  if (ctx->h_attr) (void)hipHostFree(ctx->h_attr);
  if (ctx->h_smp_seeds) (void)hipHostFree(ctx->h_smp_seeds);
  if (ctx->h_cand) (void)hipHostFree(ctx->h_cand);
  if (ctx->h_ig) (void)hipHostFree(ctx->h_ig);
  if (ctx->attr_evt) (void)hipEventDestroy(ctx->attr_evt);
  if (ctx->gen_evt) (void)hipEventDestroy(ctx->gen_evt);
  if (ctx->score_evt) (void)hipEventDestroy(ctx->score_evt);
  if (ctx->h_opt_ids) (void)hipHostFree(ctx->h_opt_ids);
  if (ctx->h_idflag) (void)hipHostFree(ctx->h_idflag);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return TST_OK;
}

const char* tst_last_error(tst_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int tst_sync(tst_ctx* ctx) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  return TST_OK;
}

int tst_dp_stats(tst_ctx* ctx, int64_t* collectives_out, int64_t* elements_out) {
  if (!ctx) return TST_EINVAL;
  if (collectives_out) *collectives_out = ctx->dp_n_coll;
  if (elements_out) *elements_out = ctx->dp_n_elems;
  return TST_OK;
}

int tst_set_stream(tst_ctx* ctx, void* hip_stream, int stream_is_set) {
  if (!ctx) return TST_EINVAL;
  CTX_HIP(hipSetDevice(ctx->device));
  CTX_RC(ctx_sync(ctx));   // nothing of this context is left in flight on the stream it leaves
  ctx->stream = stream_is_set ? (hipStream_t)hip_stream : ctx->own_stream;
  return TST_OK;
}

int64_t tst_device_bytes(tst_ctx* ctx) { return ctx ? ctx->pool.bytes : 0; }

int tst_set_weight(tst_ctx* ctx, const char* name, const void* host, int dtype, int64_t numel) {
  if (!ctx || !name || !host) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return set_weight_impl(c, name, host, dtype, numel); });
}

int tst_get_weight(tst_ctx* ctx, const char* name, float* host_out, int64_t numel) {
  if (!ctx || !name || !host_out) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return get_weight_impl(c, name, host_out, numel); });
}

int tst_init_random(tst_ctx* ctx, uint64_t seed, float stdv) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return init_random_impl(c, seed, stdv); });
}

int tst_finalize_weights(tst_ctx* ctx) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return finalize_weights_impl(c); });
}

int64_t tst_trainable_numel(tst_ctx* ctx) { return ctx ? ctx->n1 : 0; }
int tst_stack_size(tst_ctx* ctx) { return ctx ? ctx->ns : 0; }
int tst_select_slot(tst_ctx* ctx, int slot) {
  if (!ctx) return TST_EINVAL;
  if (slot < 0 || slot >= ctx->ns) return fail(ctx, TST_EINVAL, "slot out of range");
  ctx->sel_slot = slot;
  return TST_OK;
}
int tst_trainable_count(tst_ctx* ctx) { return ctx ? (int)ctx->tinfo.size() : 0; }

int tst_trainable_info(tst_ctx* ctx, int index, char* name_out, int name_cap, int64_t* offset, int64_t* rows, int64_t* cols) {
  if (!ctx || index < 0 || index >= (int)ctx->tinfo.size()) return TST_EINVAL;
  const TrainableInfo& t = ctx->tinfo[index];
  if (name_out && name_cap > 0) {
    strncpy(name_out, t.name.c_str(), (size_t)name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  if (offset) *offset = t.offset;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return TST_OK;
}

int tst_get_trainable(tst_ctx* ctx, float* host_out) {
  if (!ctx || !host_out) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  if (ctx->zero_on) return typed(ctx, [&](auto* c) { return get_trainable_sharded(c, host_out); });
  CTX_HIP(hipMemcpy(host_out, ctx->tp + ctx->sel_slot * ctx->n1, (size_t)ctx->n1 * 4, hipMemcpyDeviceToHost));
  return TST_OK;
}

int tst_set_trainable(tst_ctx* ctx, const float* host) {
  if (!ctx || !host) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return set_trainable_impl(c, host); });
}

int tst_get_grads(tst_ctx* ctx, float* host_out) {
  if (!ctx || !host_out) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  // inside an accumulation window "the gradient" is the running sum the optimizer will step on, not the last micro-batch's
  const float* g = (ctx->acc_active && ctx->tacc) ? ctx->tacc : ctx->tg;
  CTX_HIP(hipMemcpy(host_out, g + ctx->sel_slot * ctx->n1, (size_t)ctx->n1 * 4, hipMemcpyDeviceToHost));
  return TST_OK;
}

int tst_get_opt_state(tst_ctx* ctx, float* m_out, float* v_out, int32_t* step_out) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  const int64_t o = ctx->sel_slot * ctx->n1;
  if (ctx->zero_on) {   // sharded: this rank's elements [z_lo, z_hi) of the full-length vectors, zeros elsewhere
    const int64_t n = ctx->z_hi - ctx->z_lo;
    if (m_out) { memset(m_out, 0, (size_t)ctx->n1 * 4); CTX_HIP(hipMemcpy(m_out + ctx->z_lo, ctx->tm, (size_t)n * 4, hipMemcpyDeviceToHost)); }
    if (v_out) { memset(v_out, 0, (size_t)ctx->n1 * 4); CTX_HIP(hipMemcpy(v_out + ctx->z_lo, ctx->tv, (size_t)n * 4, hipMemcpyDeviceToHost)); }
    if (step_out) *step_out = ctx->opt_steps[0];
    return TST_OK;
  }
  if (m_out) CTX_HIP(hipMemcpy(m_out, ctx->tm + o, (size_t)ctx->n1 * 4, hipMemcpyDeviceToHost));
  if (v_out) CTX_HIP(hipMemcpy(v_out, ctx->tv + o, (size_t)ctx->n1 * 4, hipMemcpyDeviceToHost));
  if (step_out) *step_out = ctx->opt_steps[ctx->sel_slot];
  return TST_OK;
}

int tst_set_opt_state(tst_ctx* ctx, const float* m, const float* v, int32_t step) {
  if (!ctx || !m || !v || step < 0) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  const int64_t o = ctx->sel_slot * ctx->n1;
  if (ctx->zero_on) {   // full-length vectors in, this rank's shard kept
    const int64_t n = ctx->z_hi - ctx->z_lo;
    CTX_HIP(hipMemcpy(ctx->tm, m + ctx->z_lo, (size_t)n * 4, hipMemcpyHostToDevice));
    CTX_HIP(hipMemcpy(ctx->tv, v + ctx->z_lo, (size_t)n * 4, hipMemcpyHostToDevice));
    CTX_HIP(hipDeviceSynchronize());
    ctx->opt_steps[0] = step;
    return TST_OK;
  }
  CTX_HIP(hipMemcpy(ctx->tm + o, m, (size_t)ctx->n1 * 4, hipMemcpyHostToDevice));
  CTX_HIP(hipMemcpy(ctx->tv + o, v, (size_t)ctx->n1 * 4, hipMemcpyHostToDevice));
  CTX_HIP(hipDeviceSynchronize());
  ctx->opt_steps[ctx->sel_slot] = step;
  return TST_OK;
}

int tst_grad_buffer(tst_ctx* ctx, void** dptr_out, int64_t* numel_out) {
  if (!ctx || !dptr_out || !numel_out) return TST_EINVAL;
  *dptr_out = (ctx->acc_active && ctx->tacc) ? ctx->tacc : ctx->tg;   // (an open accumulation window: the running sum, which is what tst_optimizer_step applies)
  *numel_out = ctx->n_train;
  ctx->gn_fused = false;   // the caller may change the gradient (its own collective): the norm is taken over the buffer at the optimizer step
  return TST_OK;
}

int tst_reset_optimizer(tst_ctx* ctx) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  const int64_t o = ctx->zero_on ? 0 : ctx->sel_slot * ctx->n1;
  const int64_t n = ctx->zero_on ? ctx->z_hi - ctx->z_lo : ctx->n1;
  CTX_HIP(hipMemset(ctx->tm + o, 0, (size_t)n * 4));
  CTX_HIP(hipMemset(ctx->tv + o, 0, (size_t)n * 4));
  CTX_HIP(hipMemset(ctx->tg + o, 0, (size_t)(ctx->zero_on ? ctx->n_pad : ctx->n1) * 4));
  CTX_HIP(hipDeviceSynchronize());
  ctx->opt_steps[ctx->sel_slot] = 0;
  return TST_OK;
}

int tst_reset_trainable(tst_ctx* ctx, uint64_t seed) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return reset_trainable_impl(c, seed); });
}

static int fwd_bwd_enqueue(tst_ctx* ctx, const tst_batch* b, int32_t num_items) {
  if (!ctx || !b) return TST_EINVAL;
  ctx->acc_active = false;   // a plain forward / backward overwrites the gradient: an open accumulation window is dropped
  return typed(ctx, [&](auto* c) { return fwd_bwd_enqueue(c, b, num_items); });
}

// stacked folds: one clip + AdamW per slot that had labelled tokens in this batch (its own step count, learning rate and norm)
static int opt_enqueue_stacked(tst_ctx* ctx, const float* lrs) {
  return typed(ctx, [&](auto* c) { return opt_enqueue_stacked(c, lrs, c->tg); });
}

static int opt_enqueue(tst_ctx* ctx, float lr) {
  return typed(ctx, [&](auto* c) { return opt_enqueue(c, lr, c->tg); });
}

int tst_forward_backward(tst_ctx* ctx, const tst_batch* b, int32_t num_items, float* loss_out) {
  int rc = fwd_bwd_enqueue(ctx, b, num_items);
  if (rc != TST_OK) return rc;
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], ctx->d_loss, 4 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  CTX_RC(ctx_sync(ctx));
  if (loss_out) *loss_out = ctx->h_metrics[ctx->sel_slot];
  return TST_OK;
}

int tst_optimizer_step(tst_ctx* ctx, float lr, float* grad_norm_out) {
  if (!ctx) return TST_EINVAL;
  float lrs[TST_MAX_STACK];
  for (int i = 0; i < TST_MAX_STACK; ++i) lrs[i] = lr;
  CTX_RC(tst_optimizer_step_async(ctx, lrs));   // steps on the accumulated gradient when an accumulation window is open
  CTX_RC(ctx_sync(ctx));
  if (grad_norm_out) *grad_norm_out = ctx->h_metrics[TST_MAX_STACK + 2 * ctx->sel_slot];
  return TST_OK;
}

int tst_train_step_async(tst_ctx* ctx, const tst_batch* b, float lr) {
  int rc = fwd_bwd_enqueue(ctx, b, 0);
  if (rc != TST_OK) return rc;
  CTX_RC(opt_enqueue(ctx, lr));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], ctx->d_loss, 4 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[TST_MAX_STACK], ctx->clip_out, 8 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  return TST_OK;
}

int tst_train_step_stacked_async(tst_ctx* ctx, const tst_batch* b, const float* lr) {
  if (!ctx || !lr) return TST_EINVAL;
  int rc = fwd_bwd_enqueue(ctx, b, 0);
  if (rc != TST_OK) return rc;
  if (ctx->ns > 1) CTX_RC(opt_enqueue_stacked(ctx, lr));
  else CTX_RC(opt_enqueue(ctx, lr[0]));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[0], ctx->d_loss, 4 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  CTX_HIP(hipMemcpyAsync(&ctx->h_metrics[TST_MAX_STACK], ctx->clip_out, 8 * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  return TST_OK;
}

int tst_fetch_metrics_stacked(tst_ctx* ctx, float* loss_out, float* grad_norm_out) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  for (int sl = 0; sl < ctx->ns; ++sl) {
    if (loss_out) loss_out[sl] = ctx->h_metrics[sl];
    if (grad_norm_out) grad_norm_out[sl] = ctx->h_metrics[TST_MAX_STACK + 2 * sl];
  }
  return TST_OK;
}

// ---- intra-fold data parallelism (BASELINE.json config 4) ----
int tst_dp_unique_id(void* id_out, int64_t cap) {
  if (!id_out || cap < (int64_t)sizeof(ncclUniqueId)) return TST_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return TST_EHIP;
  memcpy(id_out, &id, sizeof(id));
  return TST_OK;
}

int tst_dp_init(tst_ctx* ctx, const void* id, int64_t id_bytes, int nranks, int rank) {
  if (!ctx || !id || id_bytes < (int64_t)sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks) return TST_EINVAL;
  if (ctx->dp_comm) return fail(ctx, TST_ESTATE, "data-parallel group already initialised");
  // everything that can be refused locally is refused BEFORE the collective ncclCommInitRank (a rank bailing out later would leave its peers inside it)
  if (ctx->zero_on && (nranks != ctx->zero || rank != ctx->zero_rank))
    return fail(ctx, TST_EINVAL, "optimizer-state sharding: the group must have cfg.zero_ranks ranks and this context's rank must be cfg.zero_rank");
  if (ctx->acc_active) return fail(ctx, TST_ESTATE, "an accumulation window is open on this context");
  CTX_HIP(hipSetDevice(ctx->device));
  hipStream_t dps = nullptr;
  hipEvent_t e1 = nullptr, e2 = nullptr;
  if (ctx->full && !ctx->zero_on) {   // communication stream + events of the region-wise overlapped reduction
    if (hipStreamCreateWithFlags(&dps, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e2, hipEventDisableTiming) != hipSuccess) {
      if (dps) (void)hipStreamDestroy(dps);
      if (e1) (void)hipEventDestroy(e1);
      return fail(ctx, TST_EHIP, "could not create the communication stream / events");
    }
  }
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = ncclCommInitRank(&ctx->dp_comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    ctx->dp_comm = nullptr;
    if (dps) { (void)hipStreamDestroy(dps); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2); }
    return fail(ctx, TST_EHIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  ctx->dp_ranks = nranks;
  ctx->dp_n_coll = ctx->dp_n_elems = 0;
  if (dps) {
    ctx->dp_stream = dps; ctx->dp_ev = e1; ctx->dp_done = e2;
    ctx->dp_regions = ctx->gn_regions;
  }
  return TST_OK;
}

int tst_dp_set_transport(tst_ctx* ctx, int dtype) {
  if (!ctx) return TST_EINVAL;
  if (dtype != TST_DTYPE_F32 && dtype != TST_DTYPE_BF16) return fail(ctx, TST_EINVAL, "transport must be TST_DTYPE_F32 or TST_DTYPE_BF16");
  if (dtype == TST_DTYPE_BF16) {
    if (!ctx->full || ctx->zero_on || ctx->dp_regions.empty())
      return fail(ctx, TST_ESTATE, "bf16 transport belongs to the region-wise gradient reduction of a full fine-tune: call tst_dp_init first (LoRA gradients are 0.2 % of that volume and stay fp32)");
    if (!ctx->dp_stage) {
      int64_t mx = 0;
      for (const auto& rg : ctx->dp_regions) mx = rg.second > mx ? rg.second : mx;
      CTX_RC(ctx_sync(ctx));
      ctx->dp_stage = (unsigned short*)ctx->pool.alloc(mx * 2);
      if (!ctx->dp_stage) return fail(ctx, TST_ENOMEM, "hipMalloc failed: bf16 transport staging buffer");
      ctx->dp_stage_elems = mx;
    }
  }
  ctx->dp_bf16 = dtype == TST_DTYPE_BF16;
  return TST_OK;
}

int tst_train_step_dp_async(tst_ctx* ctx, const tst_batch* b, float lr, int32_t num_items_global) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return train_step_dp_async_impl(c, b, lr, num_items_global); });
}

int tst_train_step_stacked_dp_async(tst_ctx* ctx, const tst_batch* b, const float* lr, const int32_t* num_items_global) {
  if (!ctx || !lr || !num_items_global) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return train_step_stacked_dp_impl(c, b, lr, num_items_global); });
}

int tst_accumulate_async(tst_ctx* ctx, const tst_batch* b, const int32_t* num_items, int first) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return accumulate_async_impl(c, b, num_items, first); });
}

int tst_fetch_loss(tst_ctx* ctx, float* loss_out) {
  if (!ctx || !loss_out) return TST_EINVAL;
  // into a pinned slot: a copy into pageable memory would block inside the call, past the bounded wait of a data-parallel context
  float* slot = ctx->h_metrics + 3 * TST_MAX_STACK;
  CTX_HIP(hipMemcpyAsync(slot, ctx->d_loss, sizeof(float) * TST_MAX_STACK, hipMemcpyDeviceToHost, ctx->stream));
  CTX_RC(ctx_sync(ctx));
  for (int sl = 0; sl < ctx->ns; ++sl) loss_out[sl] = slot[sl];
  return TST_OK;
}

int tst_optimizer_step_async(tst_ctx* ctx, const float* lr) {
  if (!ctx || !lr) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return optimizer_step_async_impl(c, lr); });
}

int tst_fetch_metrics(tst_ctx* ctx, float* loss_out, float* grad_norm_out) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  if (loss_out) *loss_out = ctx->h_metrics[ctx->sel_slot];
  if (grad_norm_out) *grad_norm_out = ctx->h_metrics[TST_MAX_STACK + 2 * ctx->sel_slot];
  return TST_OK;
}

int tst_train_step(tst_ctx* ctx, const tst_batch* b, float lr, float* loss_out, float* grad_norm_out) {
  int rc = tst_train_step_async(ctx, b, lr);
  if (rc != TST_OK) return rc;
  return tst_fetch_metrics(ctx, loss_out, grad_norm_out);
}

int tst_score_async(tst_ctx* ctx, const tst_batch* b, const int32_t* option_ids, int32_t n_opt) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return score_async_impl(c, b, option_ids, n_opt); });
}

// the opening of every *_fetch: nothing pending (count < 0) -> TST_ESTATE with `none`; else wait for the event recorded behind the pass's result copies (work
// enqueued after the pass, such as the next train steps, keeps running), hand the count out and clear it
int take_pending(tst_ctx* ctx, int& pending, hipEvent_t evt, const char* none, int& n) {
  if (pending < 0) return fail(ctx, TST_ESTATE, none);
  CTX_RC(ctx_event_sync(ctx, evt));
  n = pending;
  pending = -1;
  return TST_OK;
}

int tst_score_fetch(tst_ctx* ctx, float* logp_out, int32_t* correct_out, float* opt_logit_out, int32_t* row_seq_out, int32_t* n_rows_out) {
  int R;
  if (!ctx) return TST_EINVAL;
  CTX_RC(take_pending(ctx, ctx->score_R, ctx->score_evt, "tst_score_fetch without a pending tst_score_async", R));
  if (n_rows_out) *n_rows_out = R;
  const float* st = ctx->h_score;
  for (int r = 0; r < R; ++r) {
    if (logp_out) logp_out[r] = st[(size_t)r * 4 + 1] - st[(size_t)r * 4 + 0];
    int am;
    memcpy(&am, &st[(size_t)r * 4 + 2], 4);
    if (correct_out) correct_out[r] = (am == ctx->score_tgt[(size_t)r]) ? 1 : 0;
    if (row_seq_out) row_seq_out[r] = ctx->score_row_seq[(size_t)r];
  }
  if (opt_logit_out && ctx->score_nopt > 0) memcpy(opt_logit_out, ctx->h_score + (size_t)ctx->Rmax * 4, (size_t)R * ctx->score_nopt * 4);
  return TST_OK;
}

int tst_score(tst_ctx* ctx, const tst_batch* b, const int32_t* option_ids, int32_t n_opt, float* logp_out, int32_t* correct_out, float* opt_logit_out,
              int32_t* row_seq_out, int32_t* n_rows_out) {
  int rc = tst_score_async(ctx, b, option_ids, n_opt);
  if (rc != TST_OK) return rc;
  return tst_score_fetch(ctx, logp_out, correct_out, opt_logit_out, row_seq_out, n_rows_out);
}

int tst_attribute_async(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return attribute_async_impl(c, b, seq_kind, option_ids, n_opt); });
}

int tst_attribute_fetch(tst_ctx* ctx, float* gxi_out, float* gnorm_out, float* logs_out) {
  int S;
  if (!ctx) return TST_EINVAL;
  if (ctx->attr_S >= 0 && ctx->attr_ig) return fail(ctx, TST_ESTATE, "the pending attribution is a tst_attribute_ig_async: fetch it with tst_attribute_ig_fetch");
  CTX_RC(take_pending(ctx, ctx->attr_S, ctx->attr_evt, "tst_attribute_fetch without a pending tst_attribute_async", S));
  const float* h_res = ctx->h_attr + 2 * (size_t)ctx->Rmax + tsthost::kAttrMaxOpt;
  // the caller's token order: a token trim_last_token kept off the device gets 0 (nothing reads it under the causal mask: its gradient is exactly 0)
  if (gxi_out && tsthost::untrim_tokens(h_res, ctx->attr_cu_dev.data(), ctx->attr_cu_src.data(), S, gxi_out) != TST_OK) return fail(ctx, TST_EINVAL, "internal: un-trim map");
  if (gnorm_out && tsthost::untrim_tokens(h_res + ctx->Tmax, ctx->attr_cu_dev.data(), ctx->attr_cu_src.data(), S, gnorm_out) != TST_OK)
    return fail(ctx, TST_EINVAL, "internal: un-trim map");
  if (logs_out) tsthost::attr_logs(h_res + 2 * (size_t)ctx->Tmax, ctx->attr_plan, S, logs_out);
  return TST_OK;
}

int tst_attribute(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, float* gxi_out, float* gnorm_out,
                  float* logs_out) {
  int rc = tst_attribute_async(ctx, b, seq_kind, option_ids, n_opt);
  if (rc != TST_OK) return rc;
  return tst_attribute_fetch(ctx, gxi_out, gnorm_out, logs_out);
}

int tst_attribute_ig_async(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, const int32_t* baseline_ids,
                           int32_t n_steps) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return attribute_async_impl(c, b, seq_kind, option_ids, n_opt, baseline_ids, n_steps, true); });
}

int tst_attribute_ig_fetch(tst_ctx* ctx, float* ig_out, float* logs_out, float* logs_base_out) {
  int S;
  if (!ctx) return TST_EINVAL;
  if (ctx->attr_S >= 0 && !ctx->attr_ig) return fail(ctx, TST_ESTATE, "the pending attribution is a tst_attribute_async: fetch it with tst_attribute_fetch");
  CTX_RC(take_pending(ctx, ctx->attr_S, ctx->attr_evt, "tst_attribute_ig_fetch without a pending tst_attribute_ig_async", S));
  ctx->attr_ig = false;
  const float* h_res = ctx->h_ig + ctx->Tmax;
  if (ig_out && tsthost::untrim_tokens(h_res, ctx->attr_cu_dev.data(), ctx->attr_cu_src.data(), S, ig_out) != TST_OK) return fail(ctx, TST_EINVAL, "internal: un-trim map");
  const float* h_stats = h_res + ctx->Tmax;
  if (logs_base_out) tsthost::attr_logs(h_stats, ctx->attr_plan, S, logs_base_out);
  if (logs_out) tsthost::attr_logs(h_stats + 4 * (size_t)ctx->Rmax, ctx->attr_plan, S, logs_out);
  return TST_OK;
}

int tst_attribute_ig(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, const int32_t* baseline_ids, int32_t n_steps,
                     float* ig_out, float* logs_out, float* logs_base_out) {
  int rc = tst_attribute_ig_async(ctx, b, seq_kind, option_ids, n_opt, baseline_ids, n_steps);
  if (rc != TST_OK) return rc;
  return tst_attribute_ig_fetch(ctx, ig_out, logs_out, logs_base_out);
}

int tst_generate_async(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, const int32_t* eos_ids, int32_t n_eos) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return generate_async_impl(c, b, max_new_tokens, eos_ids, n_eos); });
}

// the fetch side of both kinds of generation: S rows of the pinned output block, each cut behind its first eos token
static int gen_fetch_rows(tst_ctx* ctx, const char* what, int32_t* tokens_out, float* logp_out, int32_t* n_new_out) {
  int S;
  CTX_RC(take_pending(ctx, ctx->gen_S, ctx->gen_evt, what, S));
  const int n = ctx->gen_new;
  const int32_t* h_tok = (const int32_t*)(ctx->h_gen + ctx->gen_dev_bytes / 4);
  const float* h_lp = (const float*)h_tok + (size_t)ctx->Smax * ctx->gen_cap_new;
  std::vector<int32_t> tok(h_tok, h_tok + (size_t)S * n);
  std::vector<float> lp(h_lp, h_lp + (size_t)S * n);
  std::vector<int32_t> nn((size_t)S);
  tsthost::cut_at_eos(tok.data(), lp.data(), nn.data(), S, n, ctx->gen_eos.data(), (int)ctx->gen_eos.size());
  if (tokens_out) memcpy(tokens_out, tok.data(), tok.size() * 4);
  if (logp_out) memcpy(logp_out, lp.data(), lp.size() * 4);
  if (n_new_out) memcpy(n_new_out, nn.data(), nn.size() * 4);
  return TST_OK;
}

int tst_generate_fetch(tst_ctx* ctx, int32_t* tokens_out, float* logp_out, int32_t* n_new_out) {
  if (!ctx) return TST_EINVAL;
  if (ctx->gen_S >= 0 && ctx->gen_cand > 0) return fail(ctx, TST_ESTATE, "the pending call is a tst_score_candidates_async: fetch it with tst_score_candidates_fetch");
  if (ctx->gen_S >= 0 && ctx->gen_samples > 0) return fail(ctx, TST_ESTATE, "the pending generation is a tst_sample_async: fetch it with tst_sample_fetch");
  return gen_fetch_rows(ctx, "tst_generate_fetch without a pending tst_generate_async", tokens_out, logp_out, n_new_out);
}

int tst_sample_async(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, int32_t n_samples, float temperature, const uint64_t* seq_seeds,
                     const int32_t* eos_ids, int32_t n_eos) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return sample_async_impl(c, b, max_new_tokens, n_samples, temperature, seq_seeds, eos_ids, n_eos); });
}

int tst_sample_fetch(tst_ctx* ctx, int32_t* tokens_out, float* logp_out, int32_t* n_new_out) {
  if (!ctx) return TST_EINVAL;
  if (ctx->gen_S >= 0 && ctx->gen_cand > 0) return fail(ctx, TST_ESTATE, "the pending call is a tst_score_candidates_async: fetch it with tst_score_candidates_fetch");
  if (ctx->gen_S >= 0 && ctx->gen_samples == 0) return fail(ctx, TST_ESTATE, "the pending generation is a tst_generate_async: fetch it with tst_generate_fetch");
  return gen_fetch_rows(ctx, "tst_sample_fetch without a pending tst_sample_async", tokens_out, logp_out, n_new_out);
}

int tst_sample(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, int32_t n_samples, float temperature, const uint64_t* seq_seeds, const int32_t* eos_ids,
               int32_t n_eos, int32_t* tokens_out, float* logp_out, int32_t* n_new_out) {
  int rc = tst_sample_async(ctx, b, max_new_tokens, n_samples, temperature, seq_seeds, eos_ids, n_eos);
  if (rc != TST_OK) return rc;
  return tst_sample_fetch(ctx, tokens_out, logp_out, n_new_out);
}

int tst_score_candidates_async(tst_ctx* ctx, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int32_t n_cands) {
  if (!ctx || !b) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return score_candidates_async_impl(c, b, cand_ids, cu_cand, cand_seq, n_cands); });
}

int tst_score_candidates_fetch(tst_ctx* ctx, float* logp_tok_out, float* logp_cand_out) {
  if (!ctx) return TST_EINVAL;
  if (ctx->gen_S >= 0 && ctx->gen_cand == 0)
    return fail(ctx, TST_ESTATE, ctx->gen_samples > 0 ? "the pending generation is a tst_sample_async: fetch it with tst_sample_fetch"
                                                      : "the pending generation is a tst_generate_async: fetch it with tst_generate_fetch");
  int N;
  CTX_RC(take_pending(ctx, ctx->gen_S, ctx->gen_evt, "tst_score_candidates_fetch without a pending tst_score_candidates_async", N));
  const tsthost::BatchLimits lim = batch_limits(ctx);
  const float* h_out = (const float*)(ctx->h_cand + tsthost::cand_dev_ints(lim) + 4 * (size_t)tsthost::cand_ext_cap(lim));
  if (logp_tok_out) memcpy(logp_tok_out, h_out, (size_t)N * 4);
  if (logp_cand_out)
    for (int c = 0; c < ctx->gen_cand; ++c) {
      double acc = 0.0;   // in token order, rounded once
      for (int t = ctx->cand_cu[(size_t)c]; t < ctx->cand_cu[(size_t)c + 1]; ++t) acc += (double)h_out[t];
      logp_cand_out[c] = (float)acc;
    }
  ctx->gen_cand = 0;
  return TST_OK;
}

int tst_score_candidates(tst_ctx* ctx, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int32_t n_cands,
                         float* logp_tok_out, float* logp_cand_out) {
  int rc = tst_score_candidates_async(ctx, b, cand_ids, cu_cand, cand_seq, n_cands);
  if (rc != TST_OK) return rc;
  return tst_score_candidates_fetch(ctx, logp_tok_out, logp_cand_out);
}

int tst_generate(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, const int32_t* eos_ids, int32_t n_eos, int32_t* tokens_out, float* logp_out,
                 int32_t* n_new_out) {
  int rc = tst_generate_async(ctx, b, max_new_tokens, eos_ids, n_eos);
  if (rc != TST_OK) return rc;
  return tst_generate_fetch(ctx, tokens_out, logp_out, n_new_out);
}

int tst_forward_logits(tst_ctx* ctx, const tst_batch* b, const int32_t* rows, int32_t n_rows, float* logits_out) {
  if (!ctx) return TST_EINVAL;
  return typed(ctx, [&](auto* c) { return forward_logits_impl(c, b, rows, n_rows, logits_out); });
}

int tst_clock_probe(int device, int spin_us, float* mhz_out) {
  if (!mhz_out || device < 0 || device >= 16 || spin_us < 1 || spin_us > 100000) return TST_EINVAL;
  std::lock_guard<std::mutex> lk(g_clock.mu);
  if (hipSetDevice(device) != hipSuccess) return TST_EHIP;
  if (!g_clock.st[device]) {
    if (hipStreamCreateWithFlags(&g_clock.st[device], hipStreamNonBlocking) != hipSuccess) return TST_EHIP;
    if (hipHostMalloc((void**)&g_clock.host[device], 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) return TST_EHIP;
  }
  unsigned long long* h = g_clock.host[device];
  h[0] = h[1] = 0;
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, g_clock.st[device], h, (unsigned long long)spin_us * 100ull);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(g_clock.st[device]) != hipSuccess) return TST_EHIP;
  if (h[1] == 0) return TST_EHIP;
  *mhz_out = 100.0f * (float)((double)h[0] / (double)h[1]);
  return TST_OK;
}

int tst_profile_enable(tst_ctx* ctx, int on) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  ctx->prof = (on & 1) != 0;
  ctx->prof_hbm = (on & 2) != 0;
  ctx->prof_used = 0;
  if (on) {
    if (!ctx->prof_ref) CTX_HIP(hipEventCreate(&ctx->prof_ref));
    CTX_HIP(hipEventRecord(ctx->prof_ref, ctx->stream));
    CTX_HIP(hipEventSynchronize(ctx->prof_ref));
  }
  return TST_OK;
}

// start/end (ms after ref_ctx's profile_enable) and FLOP of every logged launch of one tile variant: lets the caller
// compute the time the kernel actually occupied the GPU when several folds' streams overlap (union of intervals)
int tst_profile_intervals(tst_ctx* ctx, tst_ctx* ref_ctx, int variant, int unsplit_only, double* start_ms, double* end_ms, double* flop, int64_t cap,
                          int64_t* n_out) {
  if (!ctx || !ref_ctx || !ref_ctx->prof_ref || !n_out) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  int64_t n = 0;
  for (size_t i = 0; i < ctx->prof_used && n < cap; ++i) {
    const tst_ctx::ProfMeta& pm = ctx->prof_meta[i];
    if (variant >= 0 ? pm.variant != variant : pm.variant >= 100) continue;
    if (unsplit_only && pm.splitk != 1) continue;
    float a = 0, b = 0;
    CTX_HIP(hipEventElapsedTime(&a, ref_ctx->prof_ref, ctx->prof_events[i].first));
    CTX_HIP(hipEventElapsedTime(&b, ref_ctx->prof_ref, ctx->prof_events[i].second));
    if (start_ms) start_ms[n] = a;
    if (end_ms) end_ms[n] = b;
    if (flop) flop[n] = pm.flop;
    ++n;
  }
  *n_out = n;
  return TST_OK;
}

int tst_profile_read(tst_ctx* ctx, int variant, int unsplit_only, double* gemm_ms, double* gemm_flop, int64_t* gemm_launches, int reset) {
  if (!ctx) return TST_EINVAL;
  CTX_RC(ctx_sync(ctx));
  double ms = 0, flop = 0;
  int64_t n = 0;
  for (size_t i = 0; i < ctx->prof_used; ++i) {
    const tst_ctx::ProfMeta& pm = ctx->prof_meta[i];
    if (variant >= 0 ? pm.variant != variant : pm.variant >= 100) continue;   // variant < 0: every CONTRACTION (ids < 100)
    if (unsplit_only && pm.splitk != 1) continue;
    float t = 0;
    CTX_HIP(hipEventElapsedTime(&t, ctx->prof_events[i].first, ctx->prof_events[i].second));
    ms += t;
    flop += pm.flop;
    ++n;
  }
  if (gemm_ms) *gemm_ms = ms;
  if (gemm_flop) *gemm_flop = flop;
  if (gemm_launches) *gemm_launches = n;
  if (reset) ctx->prof_used = 0;
  return TST_OK;
}

}  // extern "C"
