/*
 * libtst_hip -- C-ABI of the MI355X-native TsT-LLM hot path (k-fold text-only fine-tune + held-out scoring).
 *
 * Upstream interface this replaces: NONE EXISTS. vision-x-nyu/test-set-training ships no code
 * (/root/reference/README.md:38-39 "Code -- Coming soon!"), so there is no reference FFI to bind.
 * The entry points below are therefore shaped after the only de-facto reference API of this path, the
 * HuggingFace objects BASELINE.json config 1 names; each function cites the HF/torch
 * line whose role it takes:
 *
 *   tst_create / tst_set_weight      <- LlamaForCausalLM.__init__ / load_state_dict (modeling_llama.py:421-437)
 *   tst_forward_backward             <- Trainer.training_step: model(**inputs) + loss.backward()
 *                                       (trainer.py:1892-1963; modeling_llama.py:438-492; loss_utils.py:49-71)
 *   tst_optimizer_step               <- clip_grad_norm_ + AdamW.step + zero_grad
 *                                       (trainer.py:1781-1796; clip_grad.py:50-183; adam.py:215,347-547)
 *   tst_train_step                   <- one iteration of Trainer._inner_training_loop (trainer.py:1722-1796)
 *   tst_score                        <- Trainer.prediction_step (trainer.py:2921-3010) + restricted softmax s(x)
 *   tst_forward_logits               <- model(**inputs).logits under no_grad (trainer.py:2975)
 *
 * Conventions: plain pointers and sizes only (no torch types). All *host* buffers are owned by the caller;
 * the ctx owns every device allocation (weights, adapters, optimizer state, workspace) and allocates
 * nothing inside step calls. One ctx = one device = one HIP stream; a ctx is not thread-safe, distinct
 * ctxs are independent (one per fold-worker process). Every function returns 0 or a negative TST_E* code;
 * tst_last_error() gives the message. There is NO CPU fallback: without a gfx950 device tst_create fails.
 *
 * Token layout: sequences are PACKED (pad tokens removed): input_ids/labels are [n_tokens], cu_seqlens is
 * [n_seqs+1] with cu_seqlens[0]=0. labels follow the HF convention (aligned with input_ids, -100 = ignore;
 * the one-token shift happens inside, loss_utils.py:59-63).
 */
#ifndef TST_HIP_H
#define TST_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The libraries are built with -fvisibility=hidden: the declarations between this push and its pop are the ONLY dynamic symbols they export. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define TST_OK 0
#define TST_EINVAL (-1)    /* bad argument / unsupported shape */
#define TST_EHIP (-2)      /* HIP runtime error (message in tst_last_error) */
#define TST_ENOMEM (-3)
#define TST_ESTATE (-4)    /* call order violated (e.g. step before weights finalised) */
#define TST_ENOTFOUND (-5) /* unknown tensor name */

#define TST_ARCH_LLAMA 0   /* RMSNorm, RoPE (half-split), GQA, SwiGLU, untied head: Llama-3 */
#define TST_ARCH_QWEN2 1   /* the same + bias on the q/k/v projections (modeling_qwen2.py:189-191): Qwen2.5 */
/* GPT-2 family (modeling_gpt2.py:246-311, 486-710; BASELINE.json config 1): LayerNorm with bias (eps in rms_norm_eps),
 * learned positions (wpe has max_position rows), fused c_attn, biased Conv1D linears, gelu_new MLP, head_dim 64 or 128,
 * num_kv_heads == num_heads, head tied to wte, dropout 0. Weight names are those of GPT2LMHeadModel.state_dict()
 * ("transformer.h.0.attn.c_attn.weight", ...; "lm_head.weight" is an alias of "transformer.wte.weight").
 * tst_set_weight / tst_get_weight take and return Conv1D weights in the HF layout [in, out]; on the device they are
 * [out, in], and that is the layout tst_trainable_info (rows = out, cols = in) and the flat trainable / gradient vectors
 * use in full fine-tune. LoRA targets: Q|K|V -> attn.c_attn, O -> attn.c_proj, GATE|UP -> mlp.c_fc, DOWN -> mlp.c_proj.
 * The vocabulary need not be a multiple of 64 (50257): it is padded internally, logits_out stays [n_rows, vocab]. */
#define TST_ARCH_GPT2 2
/* Qwen3 (dense): the Llama layer without q/k/v bias plus an RMSNorm over head_dim on every query head and every key head, behind the projection and before
 * RoPE (modeling_qwen3.py:237-238 q_norm / k_norm = Qwen3RMSNorm(head_dim), :252-253 q_norm(q_proj(x).view(.., head_dim)), k_norm(...)); eps = rms_norm_eps.
 * Two more weights per layer, "model.layers.N.self_attn.q_norm.weight" and "...k_norm.weight" ([head_dim] each, shared by all query resp. key heads):
 * tst_finalize_weights fails with TST_ESTATE while one is missing; a full fine-tune trains them in the no-decay group (trainer.py:1313 excludes "_norm").
 * head_dim 128; num_heads * head_dim need not equal hidden_size. Not built: sliding-window layers, attention_bias, the MoE variant. */
#define TST_ARCH_QWEN3 3

#define TST_TRAIN_LORA 0
#define TST_TRAIN_FULL 1   /* every weight trainable (BASELINE config 3): fp32 master/grad/moments for all parameters */

#define TST_LORA_Q 1u
#define TST_LORA_K 2u
#define TST_LORA_V 4u
#define TST_LORA_O 8u
#define TST_LORA_GATE 16u
#define TST_LORA_UP 32u
#define TST_LORA_DOWN 64u
#define TST_LORA_ALL 127u

#define TST_DTYPE_F32 0
#define TST_DTYPE_BF16 1

/* Precision mode of a context (tst_model_cfg.precision).
 * BF16 (default, the product path): weights, activations and MFMA operands bf16; accumulators, statistics, logits, loss, trainable
 *   masters, gradients and Adam moments fp32.
 * STRICT (parity mode; SURVEY.md §4 T1/T3 "fp32 strict mode"): every tensor fp32, contractions on v_mfma_f32_16x16x4_f32 (exact fp32
 *   fma chains), attention probabilities kept in fp32, RoPE tables unrounded -- the arithmetic of the reference's fp32 run
 *   (HF model.float()), which is what "s(x) within 1e-3 of the reference" is checked against. Same entry points, same layouts on the
 *   host side; ~16x slower contractions, 2x the weight memory. One fold per context (no stacked folds); forks, LoRA, full fine-tune,
 *   all three model families and intra-fold data parallelism work as in BF16 mode. tst_set_weight(TST_DTYPE_F32) keeps all 24 bits. */
#define TST_ROPE_DEFAULT 0
#define TST_ROPE_LINEAR 1
#define TST_ROPE_LLAMA3 2
#define TST_PRECISION_BF16 0
#define TST_PRECISION_STRICT 1

typedef struct tst_ctx tst_ctx;

typedef struct tst_model_cfg {
  int32_t arch;
  int32_t vocab_size, hidden_size, num_layers, num_heads, num_kv_heads, head_dim, intermediate_size;
  float rope_theta, rms_norm_eps;
  int32_t max_position;  /* rows of the RoPE table (GPT-2: of wpe) = longest sequence accepted */
  int32_t max_tokens;    /* workspace: packed tokens per step */
  int32_t max_seqs;      /* workspace: sequences per step */
  int32_t max_labelled;  /* workspace: labelled (answer) token rows per step */
  int32_t train_mode;    /* TST_TRAIN_* */
  int32_t lora_r;
  float lora_alpha;
  uint32_t lora_targets; /* TST_LORA_* mask */
  float adam_beta1, adam_beta2, adam_eps, weight_decay; /* torch/optim/adamw.py:24-27 defaults 0.9, 0.999, 1e-8, HF wd 0 */
  float max_grad_norm;   /* HF training_args.py:856 default 1.0; <= 0 disables clipping */
  int32_t n_stack;       /* 0 / 1: one fold per context. 2..8 (LoRA only): that many folds STACKED in this context, see below */
  int32_t precision;     /* TST_PRECISION_* */
  /* Optimizer-state sharding over the fold's data-parallel group (ZeRO stage 1; full fine-tune only; SURVEY.md §8 f4: bases whose fp32
   * Adam state does not fit 288 GB next to the weights). zero_ranks > 1: this context keeps the fp32 master, m and v of shard zero_rank
   * only -- the flat trainable vector, padded to a multiple of 64 * zero_ranks, is cut into zero_ranks equal contiguous shards -- i.e.
   * 12 B / param / zero_ranks instead of 12 B / param. A step is then: forward / backward on the rank's micro-batch shard ->
   * ncclReduceScatter of the flat fp32 gradient (every rank receives the group sum of ITS shard) -> sum of squares of the shard,
   * all-reduced (one float) for the global clip norm -> AdamW on the shard, writing its part of the compute copy of the weights ->
   * ncclAllGather of the compute copy. tst_dp_init must be given nranks == zero_ranks, rank == zero_rank.
   * 0 = off (every rank holds the whole optimizer state and all-reduces the gradient, region by region under the backward).
   * 1 = the sharded step with ONE shard: reduce-scatter / all-gather with a 1-rank group, no fused gradient norm, no region-overlapped
   *     all-reduce -- a bring-up / test configuration (full fine-tunes only, like every value >= 1; a LoRA context refuses it).
   * Without a communicator a sharded context updates its own shard only (one-GPU shard tests). STATUS as for tst_dp_*: the collectives
   * have run with 1-rank communicators only; shard arithmetic is tested per shard on one GPU (tests/test_zero_gpu.py). */
  int32_t zero_ranks, zero_rank;
  /* RoPE frequency scaling of the checkpoint (HF config.json "rope_scaling" / "rope_parameters"; transformers/modeling_rope_utils.py):
   * TST_ROPE_DEFAULT  inv_freq_i = theta^(-2i/dh)                                   (_compute_default_rope_parameters)
   * TST_ROPE_LINEAR   inv_freq_i / rope_factor                                      (_compute_linear_scaling_rope_parameters)
   * TST_ROPE_LLAMA3   Llama-3.1 / 3.2: wavelengths above rope_original_max_position / rope_low_freq_factor are divided by rope_factor,
   *                   those between that and rope_original_max_position / rope_high_freq_factor interpolated (_compute_llama3_parameters)
   * The attention scale is unchanged by all three. Other types (dynamic, yarn, longrope) are refused by tst_create. */
  int32_t rope_scaling;  /* TST_ROPE_* */
  float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
  int32_t rope_original_max_position;
} tst_model_cfg;

typedef struct tst_batch {
  const int32_t* input_ids;  /* [n_tokens] */
  const int32_t* labels;     /* [n_tokens], -100 = ignore; may be NULL for tst_forward_logits */
  const int32_t* cu_seqlens; /* [n_seqs+1] */
  int32_t n_seqs, n_tokens;
  const int32_t* seq_slot;   /* stacked folds: [n_seqs] slot (fold) of each sequence, non-decreasing; NULL = all slot 0 */
  int32_t flags;             /* TST_BATCH_*; 0 = every pointer above is host memory */
} tst_batch;

/* input_ids is a DEVICE pointer (int32 [n_tokens], e.g. torch.Tensor.data_ptr() of an int32 CUDA tensor): the ids are copied
 * device-to-device on the context's stream, nothing crosses PCIe for them. labels / cu_seqlens / seq_slot stay host memory (the
 * labelled-row map is built on the host). Ids outside the vocabulary cannot be rejected on the host in this form: one device pass checks
 * them (the embedding kernels clamp, so nothing faults) and the NEXT host wait of the context -- tst_sync, tst_fetch_metrics[_stacked],
 * tst_score_fetch, tst_forward_backward, tst_forward_logits, ... -- returns TST_EINVAL ("input id out of vocabulary"): the results of
 * the steps enqueued since the previous wait are then invalid (a fold loop should stop). Order the producer of the ids before the step with tst_set_stream (same stream) or by
 * synchronising the producer's stream first. */
#define TST_BATCH_DEVICE_IDS 1

/* ---- lifecycle ---- */
int tst_device_count(void);
/* sizeof(tst_model_cfg), sizeof(tst_batch) as this library was built: a binding checks its own struct definitions against them */
int tst_abi_struct_sizes(int32_t* model_cfg_bytes, int32_t* batch_bytes);
/* process-wide contraction tile policy: 0 = 128x128 tiles; 1 = projections on the 256x256 ping-pong tile (>= 2 resident
 * folds per GPU: the folds' kernels fill each other's tile-grid holes); 2 = as 1 but only projections with N >= 6144;
 * 3 = ONE stream per GPU (one fold, or one stacked context): the 256x256 tile with split-K for the projections whose tile grid
 *     is under half a wave, K-sliced tail tiles beyond the last full wave of 256 workgroups, and the adapter-gradient
 *     contractions on a side stream beside the dX chain;
 * level < 0 queries. Returns the level in force. Default: env TST_BIG_TILE or 0. */
int tst_set_tile_policy(int level);
/* Per-context switches for work whose results nobody reads (both default ON; value 0 / 1 sets, value < 0 queries; returns the setting in force or a
 * negative code for an unknown name / a context the option does not apply to). The results are the same with either setting:
 *  "last_compact"    LoRA contexts: the last decoder layer behind its attention (o projection, MLP, their backward) runs on the rows the head reads
 *                    only -- the labelled rows of a training batch, the option rows of a scoring batch -- because nothing else of that layer's
 *                    output is ever read (HF computes all rows: modeling_llama.py LlamaDecoderLayer.forward; the logits of unlabelled positions
 *                    do not enter ForCausalLMLoss). Not available on a full fine-tune or when created under TST_LAST_COMPACT=0.
 *  "trim_last_token" batches with labels: the LAST token of every sequence is not run through the model. Position p predicts labels[p + 1]
 *                    (loss_utils.py:59-63), so the last position predicts nothing, and under the causal mask no other position attends to it. Host
 *                    and TST_BATCH_DEVICE_IDS batches alike (the latter are gathered on the device); kept for caller-chosen rows (tst_forward_logits).
 *  "opt_overlap"     full fine-tunes (not with zero_ranks): clip + AdamW (trainer.py:1781-1796, adam.py:347-547: global-norm clip, then the step) run on
 *                    a second HIP stream behind the clip coefficient, matrix by matrix in the order the NEXT forward reads the weights (embedding side,
 *                    layers 0 .. L-1, head); a forward -- training or scoring -- waits per layer for that layer's update only, so the 44 ms of AdamW
 *                    traffic of an 8B model (30 B / parameter, streamed non-temporally) run under the next forward's contractions. 0 = the same launches on the context's stream. Results are
 *                    bit-identical either way (env TST_OPT_OVERLAP=0 starts with it off; TST_OPT_CUS=n confines the optimizer stream to n CUs, default 160).
 *                    The CU-confined optimizer queue is ONE per (device, n) for the whole process: full fine-tune contexts of one device share it, so their
 *                    optimizer steps serialise on it, and tst_destroy waits for whatever is queued on it (its own step is complete by then). It is never
 *                    destroyed by a context (on this runtime destroying a CU-masked stream while other streams are alive makes a later hipStreamDestroy
 *                    hang) but by an exit handler, before the HIP runtime shuts down (csrc/engine.hip masked_stream; probes under tools/probes/).
 *  "dw_side"         full fine-tunes: the weight-gradient contractions dW = dY^T.X (with their sums of squares) run on a side stream beside the
 *                    dX chain and are joined once per layer; 0 = everything on the context's stream. Bit-identical either way (env TST_FULL_DW_SIDE).
 *  "kmajor"          full fine-tunes, read-only after creation (env TST_KMAJOR, default 3): bit 0 = dX = dY.W from the one stored W (no transposed weight
 *                    copy is allocated), bit 1 = dW = dY^T.X straight from the row-major activations (no transposes); the K-major members of the 256x256 tile.
 *  "norm_bwd_dw"     full fine-tunes: the RMSNorm backward and the norm-weight gradient in one pass (slice sums + ordered finish); 0 = the separate column
 *                    reduction. "ndw_side": that reduction on the side stream (only with norm_bwd_dw = 0). Bit-identical in every combination.
 *  "norm_rank"       bf16 LoRA contexts: RMSNorm and the rank-axis contraction us = s.xn.Ag^T of the projection that reads the normalised rows (QKV, gate|up) run as
 *                    ONE kernel (env TST_NRK, default 1); xn within one bf16 ulp on <= 5e-6 of its elements (another summation order of the row statistic).
 *  "swiglu_rank"     bf16 LoRA contexts: SwiGLU and the rank-axis contraction that reads its result run as ONE kernel -- bit 0 (value 1) the forward (act and the down
 *                    projection's us), bit 1 (value 2) the backward (d gate|up and the gate|up projection's du); default 3, 0 = separate kernels (env TST_SWR).
 *                    act / d gate|up are bit-identical either way; us / du sum the same products in another order (fp32). Returns the mask in force. */
int tst_set_option(tst_ctx* ctx, const char* name, int value);
int tst_create(const tst_model_cfg* cfg, int device, tst_ctx** out);
/* A second fold on the same GPU: the new context BORROWS the parent's frozen weights (one copy in HBM) and owns its
 * adapters, optimizer state, activation workspace and HIP stream. Several forks may run steps concurrently from one
 * host thread (the async entry points only enqueue): the hardware interleaves the folds' kernels, which fills the
 * tile-quantisation holes a single micro-batch leaves on 256 CUs. The parent must outlive its forks. */
int tst_fork(tst_ctx* parent, tst_ctx** out);
int tst_destroy(tst_ctx* ctx);
const char* tst_last_error(tst_ctx* ctx); /* ctx may be NULL: last error of a failed tst_create */
int tst_sync(tst_ctx* ctx);
/* Run this context's work on the CALLER's HIP stream (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream; 0 = the legacy
 * default stream) instead of the stream the context created: steps are then ordered with the caller's own kernels on that stream
 * without any synchronisation. stream_is_set = 0 returns to the context's own stream. The context synchronises the stream it leaves.
 * The library can be loaded into a process whose torch.cuda is already initialised (it then runs on the HIP runtime torch loaded). */
int tst_set_stream(tst_ctx* ctx, void* hip_stream, int stream_is_set);
int64_t tst_device_bytes(tst_ctx* ctx);   /* device memory owned by the ctx */

/* ---- base weights (HF state_dict names, e.g. "model.layers.3.self_attn.q_proj.weight", "lm_head.weight") ---- */
int tst_set_weight(tst_ctx* ctx, const char* name, const void* host, int dtype, int64_t numel);
int tst_get_weight(tst_ctx* ctx, const char* name, float* host_out, int64_t numel);
int tst_init_random(tst_ctx* ctx, uint64_t seed, float std); /* device-side N(0,std^2) (modeling_utils.py:2381-2395), norms = 1 */
int tst_finalize_weights(tst_ctx* ctx); /* LoRA: builds the transposed weight copies used by the dX contractions; a full fine-tune contracts with W as stored */

/* ---- trainable parameters (flat fp32 vector; LoRA: per layer, per target, A[r,in] then B[out,r]) ---- */
int64_t tst_trainable_numel(tst_ctx* ctx);
int tst_trainable_count(tst_ctx* ctx);
int tst_trainable_info(tst_ctx* ctx, int index, char* name_out, int name_cap, int64_t* offset, int64_t* rows, int64_t* cols);
int tst_get_trainable(tst_ctx* ctx, float* host_out);
int tst_set_trainable(tst_ctx* ctx, const float* host);
int tst_get_grads(tst_ctx* ctx, float* host_out);
int tst_get_opt_state(tst_ctx* ctx, float* m_out, float* v_out, int32_t* step_out);
/* mid-fold resume (optimizer.load_state_dict, adam.py:60-110): Adam moments in the layout of tst_get_opt_state and the step
 * count. Together with tst_set_trainable it restores a fold exactly: the continued trajectory is bit-identical. */
int tst_set_opt_state(tst_ctx* ctx, const float* m, const float* v, int32_t step);
/* Intra-fold data parallelism (BASELINE.json config 4: "intra-fold DDP (RCCL/xGMI) 2 GPUs x 4 concurrent folds"; the
 * role of torch DDP, TORCH/nn/parallel/distributed.py:828-834). The `dp` ranks that share a fold form one RCCL
 * communicator (disjoint 2-rank groups each ride their own point-to-point xGMI link). Rank 0 of the group calls
 * tst_dp_unique_id and hands the 128-byte id to the others over any host channel (tst/ddp.py: a gloo broadcast); every
 * rank calls tst_dp_init. tst_train_step_dp_async then runs forward/backward on this rank's SHARD of the micro-batch
 * with the loss normalised by num_items_global (labelled tokens of the WHOLE micro-batch, trainer.py:2141-2175), sums
 * the flat fp32 gradient and the loss over the group IN PLACE on the ctx's own stream (one ncclAllReduce per step: LoRA
 * 168 MB ~ 1 ms on a 153 GB/s link), and applies the optimizer step: all ranks hold identical trainables afterwards.
 * b may be NULL / empty for a rank whose shard has no labelled token. Results: tst_fetch_metrics (global loss).
 * Full fine-tune: the 30 GB flat gradient is NOT reduced in one piece after backward; it is reduced region by region (lm_head,
 * then layer L-1 .. 0 -- 0.87 GB of fp32 per Llama-3-8B layer --, then the embedding side and the norm / bias tail) on a second
 * HIP stream as soon as backward has finished a region, so the xGMI transfers run under the remaining layers' contractions
 * (the role of DDP's bucketed all-reduce hooks, distributed.py:828-834); the optimizer waits for the last region. */
int tst_dp_unique_id(void* id_out, int64_t cap);  /* cap >= 128 */
int tst_dp_init(tst_ctx* ctx, const void* id, int64_t id_bytes, int nranks, int rank);
int tst_train_step_dp_async(tst_ctx* ctx, const tst_batch* b, float lr, int32_t num_items_global);
/* Failure handling: when a rank's tst_train_step_dp_async fails (bad batch, HIP error, ...), its communicator is aborted
 * (ncclCommAbort) before the call returns, so no peer is left waiting inside the step's collectives for a contribution that never
 * comes; tst_last_error says so and further DP steps on the context return TST_ESTATE. On the waiting side tst_sync and
 * tst_fetch_metrics of a DP context poll the stream instead of blocking: an RCCL asynchronous error, or no completion within
 * TST_DP_TIMEOUT_S seconds (environment, default 600), aborts the communicator and returns TST_EHIP. A caller that gets an error from
 * any of them should exit non-zero (tst.cli does; torch.distributed.run then ends the whole job).
 * STATUS: the 2-rank exchange has run on CPU stand-ins (gloo) and with 1-rank communicators on one MI355X only; no multi-GPU box was
 * available to the build -- treat --dp > 1 as unverified on hardware.
 * tst_dp_stats: collectives enqueued and fp32 elements reduced since tst_dp_init (a rank with an empty shard must show the same
 * numbers as its peers after every step). */
int tst_dp_stats(tst_ctx* ctx, int64_t* collectives_out, int64_t* elements_out);
/* Wire format of the region-wise gradient reduction of a full fine-tune (after tst_dp_init): TST_DTYPE_F32 (default: the flat fp32 gradient is
 * summed as it is, 30 GB per step for Llama-3-8B = ~200 ms on one 153 GB/s xGMI link against a ~120 ms step) or TST_DTYPE_BF16: every
 * region is rounded to bf16 into a staging buffer (allocated here: the largest region, 1 GB for the 128 k head), all-reduced as ncclBfloat16
 * on the communication stream and widened back into the fp32 gradient -- half the bytes, the precision torch DDP reduces a bf16 model's
 * gradients in (the gradient dtype is the parameter dtype there). Optimizer state and clipping stay fp32. LoRA contexts refuse it. */
int tst_dp_set_transport(tst_ctx* ctx, int dtype);
/* DEVICE address and length of the flat fp32 gradient (valid between tst_forward_backward and tst_optimizer_step), for a
 * caller that brings its own collective and shares this library's HIP runtime. Synchronise with tst_sync first. While an accumulation
 * window is open (tst_accumulate_async) this and tst_get_grads address the RUNNING SUM of the window -- the buffer tst_optimizer_step
 * applies --, not the last micro-batch's gradient. tst_reset_trainable drops an open window. */
int tst_grad_buffer(tst_ctx* ctx, void** dptr_out, int64_t* numel_out);
/* new fold: adapters A ~ U(-1/sqrt(in), 1/sqrt(in)) (peft kaiming_uniform a=sqrt(5)), B = 0; Adam moments and step = 0. LoRA contexts: enqueued on
 * the context's stream like a step (the values are drawn on the device; every later call on the context is ordered behind it, tst_get_trainable
 * included); element i of tensor t is draw i of the splitmix64 stream keyed by (seed, t): reproducible across runs and builds. */
int tst_reset_trainable(tst_ctx* ctx, uint64_t seed);
int tst_reset_optimizer(tst_ctx* ctx); /* Adam moments and step count = 0, adapters untouched (optimizer re-creation) */

/* ---- the hot path ---- */
/* num_items <= 0: use the number of labelled tokens of this batch (trainer.py:2141-2175) */
int tst_forward_backward(tst_ctx* ctx, const tst_batch* b, int32_t num_items, float* loss_out);
int tst_optimizer_step(tst_ctx* ctx, float lr, float* grad_norm_out);
int tst_train_step(tst_ctx* ctx, const tst_batch* b, float lr, float* loss_out, float* grad_norm_out);
/* Gradient accumulation (HF gradient_accumulation_steps: trainer.py:1740-1758 runs the micro-batches of one optimizer update under ONE
 * num_items_in_batch, trainer.py:2141-2175; backward adds into .grad; clip / AdamW / zero_grad follow once, :1781-1796).
 *   tst_accumulate_async(ctx, b, num_items, first)  forward + backward of one micro-batch with the loss normalised by num_items = the
 *       labelled tokens of the WHOLE accumulated batch -- num_items[stack size], one count per slot (a plain context: num_items[0]);
 *       first != 0 opens the window (the sum starts from this micro-batch), first == 0 adds to it.
 *   tst_optimizer_step_async(ctx, lr)               lr[stack size]; clip + AdamW on the accumulated gradient (a slot steps when any of
 *       the window's micro-batches held a labelled token of it), closes the window; without an open window it steps on the gradient of
 *       the last tst_forward_backward. Results: tst_fetch_metrics[_stacked] (loss = sum of the micro-batches' losses = CE sum / num_items).
 * tst_optimizer_step does the same synchronously. The first tst_accumulate_async of a context allocates its accumulation buffer (one
 * fp32 vector of the trainables: LoRA 168 MB per slot at Llama-3-8B r = 16; full fine-tune 4 B / parameter) -- the only device
 * allocation outside tst_create / tst_fork. Not available on a context that has joined a data-parallel group. */
int tst_accumulate_async(tst_ctx* ctx, const tst_batch* b, const int32_t* num_items, int first);
/* loss_out[stack size]: the loss of the LAST forward / backward pass alone (the micro-batch under the normalisation it was given) -- what
 * HF's model(**inputs).loss returns inside an accumulation window; waits for the context's stream. */
int tst_fetch_loss(tst_ctx* ctx, float* loss_out);
int tst_optimizer_step_async(tst_ctx* ctx, const float* lr);
/* asynchronous variant: enqueues the step; loss / grad-norm of step i are fetched later with tst_fetch_metrics */
int tst_train_step_async(tst_ctx* ctx, const tst_batch* b, float lr);
int tst_fetch_metrics(tst_ctx* ctx, float* loss_out, float* grad_norm_out);

/* ---- stacked folds (cfg.n_stack = S > 1) ----
 * The k folds of a TsT run fine-tune the SAME frozen base on different subsets; only the adapters differ. A stacked context
 * holds S adapter sets ("slots") with their own AdamW state and runs the folds in lockstep: one step takes the S folds'
 * micro-batches concatenated (sequences grouped by slot, tst_batch.seq_slot), so every frozen projection is ONE contraction
 * over M = sum of the folds' tokens instead of S short ones -- the 256x256 tile grid of a 16-QA micro-batch of an 8B model
 * covers a third of the 256 CUs, three stacked folds fill it. The adapters stay separate: the rank axis of each module group
 * carries one block per slot and a token keeps its own slot's block only, so slot s computes exactly what a context of its
 * own would (same loss normalisation by ITS labelled tokens, its own clip norm, step count and learning rate).
 * Stacked contexts can be forked like any other: F resident stacks x S slots.
 *   tst_select_slot            the slot addressed by tst_get/set_trainable, tst_get_grads, tst_get/set_opt_state,
 *                              tst_reset_trainable, tst_reset_optimizer, tst_fetch_metrics, tst_forward_backward's loss
 *                              (default 0; tst_trainable_numel / tst_trainable_info describe ONE slot)
 *   tst_train_step_stacked_async  lr[S]; a slot without labelled tokens in this batch takes no optimizer step
 *   tst_fetch_metrics_stacked  loss_out[S], grad_norm_out[S] of the last step (slots that did not step keep old values)
 * tst_train_step[_async] on a stacked context uses one lr for all slots; tst_score_async accepts seq_slot as well. */
/* Stacked folds x data parallelism -- the "dp-stacked" layout of a k-fold sweep on N GPUs (bench.py --layout dp-stacked, tst/ddp.py):
 * every GPU hosts ALL k folds in the measured best one-GPU layout (stacked contexts on two streams), the N ranks take disjoint
 * micro-batches of every fold (HF DDP semantics: global batch = N x per-device batch, TORCH/nn/parallel/distributed.py:828-834), so a
 * GPU's contractions keep their full M whatever N is. Context j of every rank joins communicator j (tst_dp_init). One step:
 *   forward / backward of this rank's part of the global batch, slot s normalised by num_items_global[s] = labelled tokens of slot s over
 *   ALL ranks (trainer.py:2141-2175) -> ONE ncclAllReduce(sum) over [flat fp32 gradient of all slots | per-slot losses] on the context's
 *   stream (Llama-3-8B r = 16, 3 slots: 504 MB) -> per slot its own clip + AdamW with lr[s]; a slot with num_items_global[s] == 0 takes
 *   no step (on any rank). All ranks hold identical adapters afterwards. b may be NULL / without labelled tokens: the rank contributes zeros.
 * Failure handling and STATUS as tst_train_step_dp_async: 1-rank communicators on one MI355X and gloo stand-ins only. */
int tst_train_step_stacked_dp_async(tst_ctx* ctx, const tst_batch* b, const float* lr, const int32_t* num_items_global);
int tst_stack_size(tst_ctx* ctx);
int tst_select_slot(tst_ctx* ctx, int slot);
int tst_train_step_stacked_async(tst_ctx* ctx, const tst_batch* b, const float* lr);
int tst_fetch_metrics_stacked(tst_ctx* ctx, float* loss_out, float* grad_norm_out);

/* Held-out scoring. For every labelled row r (token predicting an answer token, in packed order):
 *   logp[r]    = log softmax(logits[r])[target]      correct[r] = (argmax(logits[r]) == target)
 *   opt_logit[r*n_opt + j] = logits[r][option_ids[j]]   (n_opt may be 0)
 * row_seq[r] = index of the sequence the row belongs to. Returns the number of rows in *n_rows_out. */
int tst_score(tst_ctx* ctx, const tst_batch* b, const int32_t* option_ids, int32_t n_opt, float* logp_out, int32_t* correct_out,
              float* opt_logit_out, int32_t* row_seq_out, int32_t* n_rows_out);
/* the same in two halves: enqueue (returns at once) / wait + read the results of the last enqueue. The fetch waits only for
 * the scoring pass itself: steps enqueued on the context after tst_score_async keep running (a fold loop fetches the scores of
 * batch i after it has enqueued the work of batch i+1, so the stream never drains). One scoring pass may be pending per ctx. */
int tst_score_async(tst_ctx* ctx, const tst_batch* b, const int32_t* option_ids, int32_t n_opt);
int tst_score_fetch(tst_ctx* ctx, float* logp_out, int32_t* correct_out, float* opt_logit_out, int32_t* row_seq_out, int32_t* n_rows_out);
/* fp32 logits of selected packed token rows: logits_out[n_rows, vocab] */
int tst_forward_logits(tst_ctx* ctx, const tst_batch* b, const int32_t* rows, int32_t n_rows, float* logits_out);

/* ---- greedy generation ----
 * Arg-max continuation of the packed prompts of b (labels ignored; seq_slot as for tst_score_async: every sequence is continued under its own slot's
 * adapters) by max_new_tokens tokens each, with a per-context KV cache; available on every context that can score. tst_generate_async enqueues the prefill
 * (one forward over the prompts, the head on the last token of each) and max_new_tokens - 1 decode steps (one token per sequence against its cached keys) and
 * returns: the chosen token feeds the next step on the device, no host wait sits between steps. Sequences are not compacted when they finish, so a
 * sequence's tokens do not depend on where its neighbours stop. tst_generate_fetch waits for the generation only (like tst_score_fetch) and cuts row s behind
 * its first token that is in eos_ids: n_new_out[s] counts that token, the entries behind it are -1 in tokens_out and 0 in logp_out; without a hit
 * n_new_out[s] = max_new_tokens. logp_out[s, j] = log softmax(logits)[token]. One generation may be pending per context.
 * The cache (all layers, activation dtype, (max_tokens + max_seqs * max_new_tokens) rows of 2 * num_kv_heads * head_dim elements per layer; row of (sequence s,
 * position p) = cu_seqlens[s] + s * max_new_tokens + p) is allocated by the first tst_generate_async of a context -- the second device allocation outside
 * tst_create / tst_fork, counted in tst_device_bytes -- and re-allocated, behind a stream synchronisation, when a later call asks for more new tokens. Forks
 * own theirs; a context that never generates allocates nothing.
 * TST_EINVAL before anything is allocated or launched (the batch's own checks, e.g. a host id outside the vocabulary, included): max_new_tokens outside 1 .. TST_GEN_MAX_NEW, n_seqs > max_labelled (the head runs on n_seqs rows), a prompt with
 * length + max_new_tokens > max_position, an eos id outside the vocabulary, n_eos > 16. tst_generate_fetch without a pending generation: TST_ESTATE.
 * TST_BATCH_DEVICE_IDS prompts are accepted (the device-side id check applies). A generation reads the weights and adapters only: trainables, gradients,
 * optimizer state, an open accumulation window and a pending scoring pass are left as they are. */
#define TST_GEN_MAX_NEW 256
int tst_generate_async(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, const int32_t* eos_ids, int32_t n_eos);
int tst_generate_fetch(tst_ctx* ctx, int32_t* tokens_out /* [n_seqs, max_new_tokens] */, float* logp_out /* [n_seqs, max_new_tokens] */,
                       int32_t* n_new_out /* [n_seqs] */);
int tst_generate(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, const int32_t* eos_ids, int32_t n_eos, int32_t* tokens_out, float* logp_out,
                 int32_t* n_new_out);

/* ---- sampled generation: n draws per prompt at one prefill ----
 * n_samples continuations of every packed prompt of b, each drawn token by token from softmax(logits / temperature) -- the model's own distribution at that
 * temperature, nothing truncated (no top-k / top-p). Available wherever tst_generate_async is; seq_slot as there. tst_sample_async enqueues ONE prefill over the
 * n_seqs prompts, the first draw of every (sequence s, sample i) from the prompt's last-row logits, and max_new_tokens - 1 decode steps over the
 * n_seqs * n_samples decode rows r = s * n_samples + i: a row attends to its prompt's cache rows, which the n samples share, and then to its own tokens. The
 * draw is Gumbel-max on the device: token = first index of max_v (logit_v / temperature + g_v), g = -log(-log u), u = ((x >> 9) + 0.5) * 2^-23 from the
 * Philox4x32-10 word x = word (v & 3) of counter (v >> 2, step, i, 0) under the key (low, high 32 bits of seq_seeds[s]). A sequence's draws are thus a function
 * of its logits, its seed, the step and the sample index only: not of the batch it is in, its place there, or the slot layout. Bit-reproducible.
 * tst_sample_fetch: tokens_out / logp_out [n_seqs, n_samples, max_new_tokens], n_new_out [n_seqs, n_samples], every (s, i) row cut behind its first eos token as
 * in tst_generate_fetch; logp_out = log softmax(logits / temperature)[token]. Rows are not compacted when they end: a row does not depend on its neighbours.
 * The call uses the generation's cache, buffers and pending slot (prompts at cache rows 0 .. n_tokens, the tail of row r at n_tokens + r * max_new_tokens; the
 * same allocation rule for max_new_tokens): ONE generation of either kind may be pending per context, and a fetch of the other kind returns TST_ESTATE, as does
 * a fetch without a pending call.
 * Beside them the first tst_sample_async of a context allocates 8 bytes per max_seqs for the seeds (device, counted in tst_device_bytes, and pinned); a
 * context that only generates greedily allocates what it did before.
 * TST_EINVAL before anything is allocated or launched: everything tst_generate_async refuses; n_samples outside 1 .. 64; n_seqs * n_samples > min(max_seqs,
 * max_labelled) (every draw is a decode row and a head row); n_seqs * n_samples > max_tokens (a decode step is a forward pass over that many token rows --
 * possible where max_seqs exceeds max_tokens and the prompts are shorter than n_samples tokens); temperature not finite or outside [0.01, 100]; seq_seeds NULL.
 * Like a greedy generation it reads weights and adapters only. */
int tst_sample_async(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, int32_t n_samples, float temperature, const uint64_t* seq_seeds /* [n_seqs] */,
                     const int32_t* eos_ids, int32_t n_eos);
int tst_sample_fetch(tst_ctx* ctx, int32_t* tokens_out /* [n_seqs, n_samples, max_new_tokens] */, float* logp_out /* same */,
                     int32_t* n_new_out /* [n_seqs, n_samples] */);
int tst_sample(tst_ctx* ctx, const tst_batch* b, int32_t max_new_tokens, int32_t n_samples, float temperature, const uint64_t* seq_seeds, const int32_t* eos_ids,
               int32_t n_eos, int32_t* tokens_out, float* logp_out, int32_t* n_new_out);

/* ---- candidate scoring: exact log p(candidate | prompt) for given continuations, at one prefill ----
 * Candidate c = the tokens cand_ids[cu_cand[c] .. cu_cand[c + 1]) (1 .. TST_CAND_MAX_LEN of them, host memory) continues prompt cand_seq[c] of the packed
 * prompts of b (labels ignored; seq_slot and TST_BATCH_DEVICE_IDS as for tst_score_async); cand_seq is non-decreasing, a prompt without candidates is prefilled
 * and nothing more. For candidate c = c_0 .. c_{L-1} behind a prompt of len tokens
 *   logp_tok_out[cu_cand[c] + p] = log softmax(logits(prompt, c_0 .. c_{p-1}))[c_p]       (teacher-forced, temperature 1)
 *   logp_cand_out[c]             = their sum, formed on the host in double in token order and rounded once.
 * tst_score_candidates_async enqueues, without a host wait in between: ONE prefill over the prompts (cache rows 0 .. n_tokens; the head on the n_seqs last
 * rows -- every candidate's first token is read from its prompt's one logits row), then ONE forward pass over the R_e = sum_c (L_c - 1) "extend rows"
 * (candidate c, position p), p = 0 .. L_c - 2, c-major: row (c, p) is fed c_p at position len + p, its k | v join the cache at row n_tokens + (cu_cand[c] - c) + p
 * (the tails packed behind the prompts), attention is ONE launch per layer over all positions of all candidates (csrc/decode.hip attn_extend, bit-identical per
 * position to the decode step of a sampled generation), and the head runs on all R_e rows with targets c_{p+1}.
 * Available wherever tst_generate_async is; it reads weights and adapters only: trainables, gradients, optimizer state, an open accumulation window, a pending
 * scoring pass and a pending attribution are left as they are. It uses the generation's cache and pending slot: ONE of tst_generate_async, tst_sample_async and
 * tst_score_candidates_async may be pending per context; a fetch of another kind, or without a pending call, returns TST_ESTATE, and a mismatched fetch leaves
 * the pending call pending.
 * Memory: the cache of a one-token generation (max_tokens + max_seqs rows; a larger one a generation left is used as it is) under the generation's allocation
 * rule, and on the first call a device image / output block of its own (4 bytes x (6 min(max_tokens, max_seqs, max_labelled) + 3 max_labelled)), counted in
 * tst_device_bytes and freed with the context; forks own theirs. A context that never calls it allocates what it did before.
 * TST_EINVAL before anything is allocated or launched (tst_last_error names the reason; tst_device_bytes is unchanged): the batch's own checks as for
 * tst_generate_async; n_cands < 1; cu_cand not strictly increasing from 0; a candidate longer than TST_CAND_MAX_LEN; a candidate id outside the vocabulary;
 * cand_seq outside 0 .. n_seqs - 1 or decreasing; len + L_c - 1 > max_position; more candidate tokens than max_labelled; R_e > min(max_tokens, max_seqs,
 * max_labelled) (the extend pass is a forward over R_e one-token rows, as a sampled decode step is over its draws); n_seqs > max_labelled; the head_dim /
 * heads-per-kv-head restriction of generation. */
#define TST_CAND_MAX_LEN 16
int tst_score_candidates_async(tst_ctx* ctx, const tst_batch* b, const int32_t* cand_ids /* [n_cand_tokens] */, const int32_t* cu_cand /* [n_cands + 1] */,
                               const int32_t* cand_seq /* [n_cands] */, int32_t n_cands);
int tst_score_candidates_fetch(tst_ctx* ctx, float* logp_tok_out /* [n_cand_tokens] */, float* logp_cand_out /* [n_cands] */);
int tst_score_candidates(tst_ctx* ctx, const tst_batch* b, const int32_t* cand_ids, const int32_t* cu_cand, const int32_t* cand_seq, int32_t n_cands,
                         float* logp_tok_out, float* logp_cand_out);

/* ---- token attribution: input-gradient saliency of s(x) ----
 * Which tokens of a sequence carry its score. Position p predicts labels[p + 1]; rows(i) = the labelled rows of sequence i, n_i their number, z_r the fp32
 * logits of row r. Per sequence (seq_kind[i]; NULL = all 0):
 *   0, open form    J_i = (1 / n_i) sum_{r in rows(i)} log softmax(z_r)[target_r]              (log of the numeric / open s(x))
 *   1, option form  J_i = z_r[target_r] - logsumexp_j z_r[option_ids[j]]                      (log of the multiple-choice s(x); exactly one labelled row,
 *                                                                                               whose target is one of option_ids)
 * With e[t, :] the embedding-layer output of token t (embed_tokens[id]; GPT-2: wte[id] + wpe[pos]) and g = d (sum_i J_i) / d e -- sequences of a packed batch do
 * not interact, so one backward pass yields every sequence's own gradient -- the call returns, accumulated in fp32,
 *   gxi_out[t]   = sum_d g[t, d] e[t, d]     (gradient x input, signed)
 *   gnorm_out[t] = sqrt(sum_d g[t, d]^2)
 * in the caller's token order (a token the model does not run, "trim_last_token", gets 0: nothing reads it under the causal mask) and logs_out[i] = J_i.
 * Under bf16 gradient x input cancels and is the noisier of the two; gnorm is the robust output.
 * Available on every context that can score (LoRA plain, forked, stacked with seq_slot as for tst_score_async; full fine-tune; bf16 and strict).
 * tst_attribute_async enqueues a forward, the backward pass seeded with d (sum_i J_i) / d logits down to the embedding output, and the per-token reduction;
 * tst_attribute_fetch waits for the attribution only (like tst_score_fetch). One attribution may be pending per context.
 * The call reads weights and adapters only: trainables, optimizer state and step counts, the KV cache, a pending scoring pass and a pending generation are
 * left as they are. The flat gradient (tst_get_grads, tst_grad_buffer) and the last-loss metrics (tst_fetch_loss, tst_fetch_metrics) are UNSPECIFIED afterwards:
 * a tst_optimizer_step[_async] that would apply a gradient overwritten by an attribution returns TST_ESTATE (run tst_forward_backward again).
 * Its small buffers (row weights, per-token results, pinned staging: 8 bytes per max_tokens + 8 per max_labelled + 1 KB on the device) are allocated by the
 * first tst_attribute_async of a context -- like the KV cache of a generation -- and counted in tst_device_bytes.
 * TST_ESTATE before anything is launched: weights not finalised, an open accumulation window, a context that has joined a data-parallel group;
 * tst_attribute_fetch without a pending attribution. TST_EINVAL before anything is allocated or launched: the batch's own checks, no labelled token, n_opt
 * outside 0 .. 256, an option id outside the vocabulary, a seq_kind other than 0 / 1, a kind-1 sequence whose labelled-row count is not 1 or whose target is not
 * in option_ids, a kind-1 sequence with n_opt == 0. */
int tst_attribute_async(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind /* [n_seqs] or NULL */, const int32_t* option_ids, int32_t n_opt);
int tst_attribute_fetch(tst_ctx* ctx, float* gxi_out /* [n_tokens] */, float* gnorm_out /* [n_tokens] */, float* logs_out /* [n_seqs] */);
int tst_attribute(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, float* gxi_out, float* gnorm_out,
                  float* logs_out);

/* ---- token attribution: integrated gradients of log s(x) along a baseline path ----
 * J_i, seq_kind, option_ids and the embedding-layer output e[t, :] are those of tst_attribute_async. baseline_ids[n_tokens] (HOST memory, like labels, also for a
 * TST_BATCH_DEVICE_IDS batch; one id per token of the caller's batch) names the baseline prompt: b[t, :] = embed_tokens[baseline_ids[t]] (GPT-2:
 * wte[baseline_ids[t]] + wpe[pos], so the position term cancels in e - b). There is no zero-vector baseline: on RMSNorm models the first norm is scale-invariant down
 * to eps and the integrand is singular at the origin. A token with baseline_ids[t] == input_ids[t] is not interpolated; its result is exactly 0.
 * For n_steps = m the path is sampled by the midpoint rule, alpha_k = (k - 1/2) / m, x_k = b + alpha_k (e - b) -- evaluated in fp32 as written and
 * rounded once to the activation type -- and with g_k = d (sum_i J_i) / d x at x_k the call returns
 *   ig_out[t]        = (1 / m) sum_{k = 1 .. m} sum_d g_k[t, d] (e - b)[t, d]      (signed; fp32 accumulation, k ascending: bit-reproducible)
 *   logs_out[i]      = J_i(e)     (what tst_attribute returns as logs_out)
 *   logs_base_out[i] = J_i(b)
 * in the caller's token order (a token "trim_last_token" keeps off the device gets 0). Completeness is the contract a reader can use: the ig of the tokens of
 * sequence i sum to logs_out[i] - logs_base_out[i] as m grows; at a fixed m the sum is a quantity of its own and the gap is the quadrature error.
 * tst_attribute_ig_async enqueues everything at once -- a forward + head pass at the baseline, one at the real prompt, then m times interpolation, forward, head,
 * backward to the embedding output and the per-token reduction -- without a host wait in between; tst_attribute_ig_fetch waits for that work only.
 * Availability, side effects (the flat gradient is UNSPECIFIED afterwards; an optimizer step on it returns TST_ESTATE) and the TST_ESTATE cases are those of
 * tst_attribute_async. ONE attribution of either kind may be pending per context; a fetch of the other kind returns TST_ESTATE and leaves the pending one pending.
 * Its buffers (8 bytes per max_tokens on the device, besides tst_attribute_async's own; pinned staging) are allocated by the first call and counted in
 * tst_device_bytes. TST_EINVAL before anything is allocated or launched: the cases of tst_attribute_async, baseline_ids == NULL, a baseline id outside the vocabulary,
 * n_steps outside 1 .. TST_IG_MAX_STEPS. */
#define TST_IG_MAX_STEPS 256
int tst_attribute_ig_async(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind /* [n_seqs] or NULL */, const int32_t* option_ids, int32_t n_opt,
                           const int32_t* baseline_ids /* [n_tokens], host */, int32_t n_steps);
int tst_attribute_ig_fetch(tst_ctx* ctx, float* ig_out /* [n_tokens] */, float* logs_out /* [n_seqs] */, float* logs_base_out /* [n_seqs] */);
int tst_attribute_ig(tst_ctx* ctx, const tst_batch* b, const int32_t* seq_kind, const int32_t* option_ids, int32_t n_opt, const int32_t* baseline_ids, int32_t n_steps,
                     float* ig_out, float* logs_out, float* logs_base_out);

/* ---- measurement hooks (bench.py): HIP events on the ctx stream around the dominant kernel class ---- */
/* on: bit 0 = bracket every dense contraction launch with HIP events on its stream; bit 1 = also bracket the HBM-bound kernel classes
 * (variant ids 101 AdamW, 102 SwiGLU, 103 RMSNorm / LayerNorm, 104 attention); 0 = off */
int tst_profile_enable(tst_ctx* ctx, int on);
/* totals since enable over the launches of one tile variant (0: 128x128, 1: 128x64, 2: 64x128, 3: TN, 4 / 5: 256x256 tiles, 30 / 31:
 * fp32 strict; < 0: every contraction), optionally only launches without split-K (one kernel per bracket); reset != 0 clears the
 * log. For the class ids >= 100, *gemm_flop receives the algorithmic BYTES of the launches (FLOPs for 104). */
int tst_profile_read(tst_ctx* ctx, int variant, int unsplit_only, double* gemm_ms, double* gemm_flop, int64_t* gemm_launches, int reset);

/* Shader clock the device holds RIGHT NOW, in MHz: one wave on a stream of its own stamps the shader-clock counter and the constant 100 MHz counter
 * around a bounded spin of spin_us microseconds (1 .. 100000) -- clock = d(s_memtime) / d(s_memrealtime) x 100 MHz. Context-free and thread-safe: bench.py
 * samples it from a side thread while the timed sweep runs, so that `roofline.frac` can be restated against the clock the chip held under the dense
 * MFMA load (2.5 PFLOP/s assumes 2.4 GHz). The call waits for its own wave only; the wave needs one free wave slot on any CU. */
int tst_clock_probe(int device, int spin_us, float* mhz_out);

/* start / end (ms after ref_ctx's tst_profile_enable(1)) and FLOP of every logged launch of one variant; with several
 * folds per GPU the union of these intervals is the time the kernel really occupied the device */
int tst_profile_intervals(tst_ctx* ctx, tst_ctx* ref_ctx, int variant, int unsplit_only, double* start_ms, double* end_ms, double* flop, int64_t cap,
                          int64_t* n_out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
