// Internal launcher interface between the engine (engine.cpp) and the HIP kernels. All launchers are
// asynchronous on the given stream, allocate nothing and return TST_OK / TST_E*.
#pragma once
#include "common.h"

#define TST_MAX_STACK 8
#define TST_MAX_GROUPED 8   // contractions per grouped launch (gemm_tn_grouped)
// stacked folds: rows (tokens) [t_end[s-1], t_end[s]) belong to slot s and keep only that slot's rank columns [s*width, (s+1)*width)
struct SlotEnds { int t_end[TST_MAX_STACK]; };

// AT = element type of the operands: bf16_t (product path, the hand-scheduled MFMA tiles of gemm*.hip) or float (fp32 "strict"
// parity mode, gemm_f32.hip: every tensor fp32, v_mfma_f32_16x16x4_f32, no split-K; out_f32 is implied)
template <typename AT>
struct GemmParamsT {
  const AT* A;  const AT* B;             // A[M,K] (lda), B[N,K] (ldb): both K-contiguous
  const AT* A2; const AT* B2;            // optional second K segment (K2 columns), may be null when K2 == 0
  void* C;                               // AT or f32 [M,N] (ldc)
  const AT* R;                           // optional residual added before rounding (AT output only)
  const AT* bias;                        // optional bias[N] added before rounding (AT output only; Qwen2 q/k/v)
  float* slab;                           // set by gemm_nt
  long lda, ldb, lda2, ldb2, ldc, ldr;
  int M, N, K, K2;
  int kvalid;                            // TN forms only: real rows of the contraction axis (K = kvalid rounded up to 64)
  int ta, tb;                            // 256x256 ping-pong tile only (gemm_pp_kmajor): the operand is stored K-major -- ta: A is [K][M] (lda), tb: B is [K][N] (ldb).
                                         // ta = tb = 1 is the TN form (dW = dy^T . x straight from the row-major activations; rows >= kvalid read as zeros),
                                         // ta = 0, tb = 1 the NN form (dX = dY . W from the one stored W[K = d_out][N = d_in]); no second K segment
  int out_f32;
  int splitk;                            // set by gemm_nt
  float alpha;
  int mtiles, ntiles;                    // set by gemm_nt
  int gm;                                // gemm_pp: tile rows per group of its XCD-aware tile order (set by gemm_pp)
  int tail_s, tail_full, tail_n;         // gemm_pp tail split (set by gemm_pp): K slices per tail tile, first tail block, tail tiles
  int no_splitk;                         // caller's veto of the tile policy's split-K on the 256x256 tile (same reason as no_tail)
  int no_tail;                           // caller's veto of the tail split: the stream does not have the GPU to itself (full fine-tune: weight gradients / AdamW run beside it)
  size_t slab_cap;                       // bytes behind slab (set by gemm_nt)
  float* sumsq;                          // optional, fp32 output on the 256x256 ping-pong tile without split-K: per-workgroup sums of squares of the
                                         // stored values, slots [0, mtiles*ntiles) (+ 16 per tail tile behind the full waves); unused slots are not written
  int mask_width, mask_nslot;            // stacked folds: bf16 output rows keep their slot's column block only (0 = off)
  SlotEnds mask_ends;
  int k2_w;                              // stacked folds, second K segment: row t of A2 is zero outside the column block [s*k2_w, (s+1)*k2_w) of its slot s (slots from
                                         // mask_nslot / mask_ends, which may be set with mask_width == 0). The 256x256 ping-pong tile then runs only the K2 k-tiles that
                                         // overlap the blocks of its rows' slots (the others add exact zeros); every other tile family ignores it. 0 = all of K2
};
typedef GemmParamsT<bf16_t> GemmParams;
typedef GemmParamsT<float> GemmParamsF;

// used (optional, int[2]) receives the tile variant and split-K factor that were launched
int gemm_nt(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int force_variant, int force_splitk, int* used);
// C[M,N] = alpha * sum_{t<kvalid} A[t,M] * B[t,N] (p.A/p.B = [rows t][cols], p.kvalid set; p.K is derived)
int gemm_tn(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int* used);
// up to TST_MAX_GROUPED TN contractions (fp32 outputs) in one launch, no split-K (gemm.hip)
int gemm_tn_grouped(hipStream_t st, const GemmParams* ps, int n, float* slab_ws, size_t slab_ws_bytes);
// Adapter gradients restricted to what is not zero (gemm_tns.hip): one problem = one module group's dAg (kind 0: C[rank row, wide col], ldc = wn) or
// dBg (kind 1: C[wide row, rank col], ldc = rp). rk = the rank-side operand [tokens, rp] (du or us: per token only its slot's block of w columns
// is non-zero), wd = the wide operand [tokens, wn] (x or dy). Slot s owns rank columns [s w, (s + 1) w) and the tokens [t_end[s-1], t_end[s]).
struct TnsProblem {
  const bf16_t* rk; long ldr; int rp;
  const bf16_t* wd; long ldw; int wn;
  float* c; long ldc;
  int w;           // rank columns per slot (nmod * r, a multiple of 8)
  float alpha;
  int kind;        // 0: dAg layout, 1: dBg layout
  int rows_pad;    // readable token rows of both operands (roundup64 of the workspace's token capacity)
};
bool gemm_tns_supported(const TnsProblem& p);
int gemm_tns_grouped(hipStream_t st, const TnsProblem* ps, int n, int nslot, const SlotEnds& ends);
// fp32 strict mode (gemm_f32.hip): the same contracts on fp32 operands; one tile family, no split-K (the workspace arguments are unused)
int gemm_nt(hipStream_t st, GemmParamsF p, float* slab_ws, size_t slab_ws_bytes, int force_variant, int force_splitk, int* used);
int gemm_tn(hipStream_t st, GemmParamsF p, float* slab_ws, size_t slab_ws_bytes, int* used);
// 256x256 software-pipelined tile (gemm_big.hip), variant id 4
int gemm_big(hipStream_t st, GemmParams p);
int gemm_big_tile_level(int level);
// 256x256 ping-pong tile (gemm_pp.hip), variant id 5: two wave groups alternate between memory and MFMA phases
int gemm_pp(hipStream_t st, GemmParams p);   // falls back to gemm_big when an operand exceeds 32-bit buffer offsets
bool gemm_pp_supported(const GemmParams& p);
// the same tile with K-major operands (p.ta / p.tb): C[M,N] = alpha * A.B^T with A given as [K][M] and / or B as [K][N]; any M, N (multiples of 8), K a multiple
// of 64 (TN: p.kvalid real rows); optional split-K through slab_ws (+ the reduce launch). used[2] as gemm_nt
int gemm_pp_kmajor(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int force_splitk, int* used);
bool gemm_pp_kmajor_supported(const GemmParams& p);
inline bool gemm_pp_supported(const GemmParamsF&) { return false; }
// rank-axis contraction (gemm_rank.hip), variant id 8: bf16 C[M, N <= 512] = alpha A.B^T, K split over the 8 waves of a workgroup, slot mask in the epilogue
int gemm_rank(hipStream_t st, GemmParams p, int form = 0);   // form 1 (variant 9): the register-loading kernel instead of the LDS-staged one
bool gemm_rank_supported(const GemmParams& p);
int gemm_pp_splitk(int M, int N, int Ktot);   // split factor the tile policy uses for this shape
void gemm_pp_set_stamps(unsigned long long* dev);  // diagnostic build with in-kernel s_memtime stamps while non-null
void gemm_plan(int M, int N, int K, int K2, int* variant, int* splitk);
size_t gemm_slab_bytes(int M, int N, int splitk);
int gemm_ref(hipStream_t st, const bf16_t* A, long sam, long sak, const bf16_t* B, long sbn, long sbk, float* C, long ldc, int M, int N, int K);
template <typename AT> int transpose_mat(hipStream_t st, const AT* in, long ldi, AT* out, long ldo, int R, int C, int R_pad);

// elementwise.hip: every launcher exists for AT = bf16_t and AT = float (explicitly instantiated there)
template <typename AT> int embed_fwd(hipStream_t st, const int* ids, const AT* E, AT* out, int T, int d, int vocab);
template <typename AT> int gather_rows(hipStream_t st, const AT* in, const int* idx, AT* out, int n, int d, int scatter);
template <typename AT> int rmsnorm_fwd(hipStream_t st, const AT* x, const AT* w, AT* y, float* rstd, int T, int d, float eps);
template <typename AT> int rmsnorm_bwd(hipStream_t st, const AT* dy, const AT* x, const float* rstd, const AT* w, const AT* dres, AT* dx, int T, int d);
// column reductions of the full fine-tune: two launches, no atomics (bit-reproducible); ws = colred_ws_floats(T, n) floats of scratch (layernorm_dwdb: twice that)
long colred_ws_floats(int T, int n);
template <typename AT> int rmsnorm_dw(hipStream_t st, const AT* dy, const AT* x, const float* rstd, float* dw, int T, int d, float* ws);   // dw +=
// GPT-2 family: LayerNorm (stats[2*row] = mean, stats[2*row+1] = rstd), gelu_new, token + learned-position embedding
template <typename AT> int layernorm_fwd(hipStream_t st, const AT* x, const AT* w, const AT* b, AT* y, float* stats, int T, int d, float eps);
template <typename AT> int layernorm_bwd(hipStream_t st, const AT* dy, const AT* x, const float* stats, const AT* w, const AT* dres, AT* dx, int T, int d);
template <typename AT> int layernorm_dwdb(hipStream_t st, const AT* dy, const AT* x, const float* stats, float* dw, float* db, int T, int d, float* ws);  // +=
template <typename AT> int gelu_fwd(hipStream_t st, const AT* x, AT* y, long n);
template <typename AT> int gelu_bwd(hipStream_t st, const AT* dy, const AT* x, AT* dx, long n);
template <typename AT> int embed_pos_fwd(hipStream_t st, const int* ids, const int* pos, const AT* E, const AT* P, AT* out, int T, int d, int vocab, int npos);
template <typename AT> int rope_apply(hipStream_t st, AT* qkv, const int* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, long ld, int backward);
// head_norm.hip -- Qwen3 per-head q/k RMSNorm, in place on the first (H + Hkv) 128 columns of qkv / dqkv [T, ld]: the H query heads take wq [128], the Hkv key
// heads wk [128]; v is not touched. rstd fp32 [T, H + Hkv]. stash (forward: optional, backward: required) = the raw rows [T, H + Hkv, 128] the backward re-forms
// x_hat from. pos != nullptr: the half-split rotation of rope_apply in the same pass (forward: norm, round, rotate; backward: un-rotate, round, norm backward),
// bit-identical to the two passes. dwq != nullptr (with dwk and ws = HEAD_NORM_WS_FLOATS floats): dwq[j] += sum_{t, h < H} dy x_hat, dwk[j] += the key heads' sum
// (per-workgroup partial sums + an ordered finish, no atomics)
#define HEAD_NORM_WS_FLOATS (1024 * 256)
template <typename AT> int head_norm_fwd(hipStream_t st, AT* qkv, long ld, const AT* wq, const AT* wk, float* rstd, AT* stash, int T, int H, int Hkv, float eps,
                                         const int* pos, const float* cosT, const float* sinT);
template <typename AT> int head_norm_bwd(hipStream_t st, AT* dqkv, long ld, const AT* wq, const AT* wk, const float* rstd, const AT* stash, int T, int H, int Hkv,
                                         const int* pos, const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws);
// gu = [gate F | up F]
template <typename AT> int swiglu_fwd(hipStream_t st, const AT* gu, AT* act, int T, int F);
template <typename AT> int swiglu_bwd(hipStream_t st, const AT* dact, const AT* gu, AT* dgu, int T, int F);
// SwiGLU fused with the rank-axis contraction that reads its result (swiglu_rank.hip; bf16): C[T, N] = alpha * (act | dgu) . B^T, bf16, each row
// keeping its slot's block of mask_width columns only (stacked folds; 0 = all N <= 64 columns). forward: B = Ag [N][F]; backward: B = BgT [N][2F]
struct SwiRank {
  const bf16_t* B; long ldb;
  bf16_t* C; int N;
  float alpha;
  int mask_width, mask_nslot;
  SlotEnds mask_ends;
  int block_diag;   // backward: the rank block of a slot is [gate module | up module] (equal halves) and BgT is zero where a module's rows meet the other one's columns
};
// RMSNorm forward fused with the rank-axis contraction that reads its result (norm_rank.hip; bf16, d in {256, 512, 1024, 2048, 3072, 3584, 4096}):
// y = w . bf16(x . rstd) and C[T, N] = alpha * y . B^T (B = Ag [N][d]), each row keeping its slot's block of mask_width columns only. r == nullptr (or r->B == nullptr):
// the plain norm by the same code (y and rstd bit-identical to the fused form)
struct NormRank {
  const bf16_t* B; long ldb;
  bf16_t* C; int N;
  float alpha;
  int mask_width, mask_nslot;
  SlotEnds mask_ends;
};
bool rmsnorm_rank_width_ok(int d);
bool rmsnorm_rank_supported(int T, int d, const NormRank* r);
int rmsnorm_rank_fwd(hipStream_t st, const bf16_t* x, const bf16_t* w, bf16_t* y, float* rstd, int T, int d, float eps, const NormRank* r);
// RMSNorm backward with the norm-weight gradient in the same pass (norm_rank.hip; bf16, the widths of rmsnorm_rank_width_ok): dx as rmsnorm_bwd; dw != null:
// dw[c] += sum_t dy[t, c] bf16(x[t, c] rstd[t]) through slice sums in ws (colred_ws_floats(T, d) floats) and an ordered finish -- no atomics
int rmsnorm_bwd_dw(hipStream_t st, const bf16_t* dy, const bf16_t* x, const float* rstd, const bf16_t* w, const bf16_t* dres, bf16_t* dx, float* dw, int T, int d, float* ws);
bool swiglu_rank_supported(int T, int F, const SwiRank& r);
int swiglu_rank_fwd(hipStream_t st, const bf16_t* gu, bf16_t* act, int T, int F, const SwiRank& r);
int swiglu_rank_bwd(hipStream_t st, const bf16_t* dact, const bf16_t* gu, bf16_t* dgu, int T, int F, const SwiRank& r);
template <typename AT> int logit_rows(hipStream_t st, const float* logits, long ld, const int* target, int n_rows, int V, float* stats, AT* dlogits, long ldd,
                                      float inv_items, const int* opt_ids, int n_opt, float* optl);
int loss_reduce(hipStream_t st, const float* stats, int n, float inv_items, float* loss_out);
// attribute.hip -- token attribution (backward seeded with J = sum_i log s(x_i) instead of the training loss).
// attr_seed: dlogits[r, 0 .. Vp) = d J / d logits of labelled row r (padding exactly 0): row_w[r] (onehot(target) - softmax(z_r)) for row_kind[r] == 0, the same over
// the option ids only (0 at every other column) for row_kind[r] == 1; stats[r] = {lse, logit[target], option logsumexp, max}. One 256-thread workgroup per row.
template <typename AT> int attr_seed(hipStream_t st, const float* logits, long ld, const int* target, const float* row_w, const int* row_kind, const int* opt_ids,
                                     int n_opt, int n_rows, int V, int Vp, float* stats, AT* dlogits, long ldd);
// token_attr: gxi[t] = sum_c g[t, c] e[t, c], gnorm[t] = sqrt(sum_c g[t, c]^2) for T rows of d columns (a multiple of 8, at most 8192); one wave per token, fp32
template <typename AT> int token_attr(hipStream_t st, const AT* g, const AT* e, int T, int d, float* gxi, float* gnorm);
// integrated gradients (tst_attribute_ig_async). embed_interp: out[t, :] = E[bids[t]] + alpha (E[ids[t]] - E[bids[t]]) (+ P[pos[t]] when P != nullptr: GPT-2) in fp32,
// ONE rounding; alpha == 1 writes what embed_fwd / embed_pos_fwd write, bit for bit, and a token with bids[t] == ids[t] gets its table row at every alpha.
// token_ig: acc[t] = (first ? 0 : acc[t]) + w sum_c g[t, c] (E[ids[t], c] - E[bids[t], c]). One wave per token; d a multiple of 8; ids clamped into [0, vocab).
template <typename AT> int embed_interp(hipStream_t st, const int* ids, const int* bids, const int* pos, const AT* E, const AT* P, AT* out, int T, int d, int vocab,
                                        int npos, float alpha);
template <typename AT> int token_ig(hipStream_t st, const AT* g, const AT* E, const int* ids, const int* bids, int T, int d, int vocab, float w, bool first, float* acc);
int ids_gather(hipStream_t st, const int* src, int* ids, int n, int n_src);    // ids[i] = src[ids[i]] (device-side batch of a trimmed TST_BATCH_DEVICE_IDS call)
int ids_check(hipStream_t st, const int* ids, int T, int vocab, int* flag);   // *flag = 1 when an id lies outside [0, vocab)
template <typename AT> int cast_from_f32(hipStream_t st, const float* in, AT* out, long n, float scale);
int lora_a_init(hipStream_t st, float* out, long n, unsigned long long state0, float bound);   // U(-bound, bound): draw i of the splitmix64 stream from state0
template <typename AT> int randn_fill(hipStream_t st, AT* out, long n, unsigned seed, float stdv);   // N(0, stdv^2) rounded to bf16 precision in both modes
template <typename AT> int fill_const(hipStream_t st, AT* out, long n, float v);

// cosT / sinT != nullptr: RoPE inside the kernels (q, k of qkv UN-rotated; dq, dk of dqkv come back un-rotated too) -- only where
// attn_rope_fusable(max_len, dh) says so (sequences <= 128 tokens, head_dim 128); tables fp32 [max_position][64]
bool attn_rope_fusable(int max_len, int dh);
int attn_fwd(hipStream_t st, const bf16_t* qkv, long ld, const int* cu, int n_seqs, int max_len, bf16_t* out, long ldo, float* lse, int T, int H, int Hkv,
             int dh, float scale, const float* cosT = nullptr, const float* sinT = nullptr, const int* order = nullptr);   // order: as for attn_bwd
int attn_bwd(hipStream_t st, const bf16_t* qkv, long ld, const bf16_t* out, long ldo, const bf16_t* dO, long lddo, const float* lse, float* delta,
             const int* cu, int n_seqs, int max_len, bf16_t* dqkv, int T, int H, int Hkv, int dh, float scale, const float* cosT = nullptr,
             const float* sinT = nullptr, const int* order = nullptr);   // order: sequence indices longest first (launch order of the single backward kernel)
// the single backward kernel for sequences of at most 128 tokens: 1 / 0 force it on / off, -1 = environment TST_ATTN_FUSED_BWD; returns the previous setting
int attn_fused_bwd(int on);
// fp32 strict mode (attn_f32.hip): the same contract on fp32 tensors (v_mfma_f32_16x16x4_f32, fp32 P and dS)
int attn_fwd(hipStream_t st, const float* qkv, long ld, const int* cu, int n_seqs, int max_len, float* out, long ldo, float* lse, int T, int H, int Hkv,
             int dh, float scale);
int attn_bwd(hipStream_t st, const float* qkv, long ld, const float* out, long ldo, const float* dO, long lddo, const float* lse, float* delta,
             const int* cu, int n_seqs, int max_len, float* dqkv, int T, int H, int Hkv, int dh, float scale);
int tr_probe(hipStream_t st, unsigned short* out_dev, int d0);
// decode.hip -- greedy generation. meta = device ints S | max_new | cu[0 .. S] | len[0 .. S) (host_logic.h plan_generate); the cache row of (sequence s,
// position p) is cu[s] + s max_new + p; cap_rows = rows behind kcache / vcache (a row outside it is skipped, never touched).
// kv_append: the k | v columns qkv[t, k_off .. k_off + 2 Hkv dh) -> kcache / vcache [cap_rows, Hkv dh] row rows[t], 16-byte vectors, bit-exact.
template <typename AT> int kv_append(hipStream_t st, const AT* qkv, long ld, int k_off, const int* rows, AT* kcache, AT* vcache, int T, int Hkv, int dh, long cap_rows);
// attn_decode: out[s, h dh ..] = softmax(scale q[s, h] . K_s^T) V_s over the keys 0 .. len[s] + step - 1 of sequence s; q [n_seqs, ldq] holds the (rotated) query
// heads, H / Hkv <= 8, dh 64 or 128. fp32 online softmax, no atomics, bit-reproducible.
template <typename AT> int attn_decode(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* meta, int n_seqs, int step, AT* out,
                                       long ldo, int H, int Hkv, int dh, float scale, long cap_rows);
// next_token: from the rows logit_rows left in stats: tok[s, j] = argmax, logp[s, j] = max - lse, d_ids[s] = argmax, d_pos[s] = len[s] + j, lab_idx[s] = s
int next_token(hipStream_t st, const float* stats, const int* meta, int n_seqs, int j, int* tok, float* logp, int* d_ids, int* d_pos, int* lab_idx);
// decode.hip -- sampled generation. geo = device ints rows R | max_new | n_samples | {pre_row0, len, tail_row0} per decode row r = s n_samples + i
// (host_logic.h plan_sample): the prompt of sequence s lies at cache rows [pre_row0, pre_row0 + len), shared by its n samples; row r's own tokens at
// [tail_row0, tail_row0 + step). seeds = device ints {low, high 32 bits of seq_seeds[s]} per sequence.
// attn_decode_shared: attn_decode with key k of row r at cache row k < len ? pre_row0 + k : tail_row0 + k - len; the same code path, the same bits for the same keys.
template <typename AT> int attn_decode_shared(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* geo, int n_rows, int step,
                                              AT* out, long ldo, int H, int Hkv, int dh, float scale, long cap_rows);
// sample_rows: step j of a sampled generation, one pass over logits row (j == 0 ? s : r) [V of ld fp32]: tok[r, j] = first index of max_v fmaf(logit_v, inv_temp,
// g_v) with g the Gumbel noise of Philox4x32-10 (key seeds[s], counter (v >> 2, j, i, 0), word v & 3), logp[r, j] = logit[tok] inv_temp - logsumexp(logit inv_temp),
// d_ids[r] = tok, d_pos[r] = len + j, lab_idx[r] = r. ld a multiple of 4 and >= V rounded up to 4; the columns >= V are never candidates. Bit-reproducible.
int sample_rows(hipStream_t st, const float* logits, long ld, int V, const int* geo, const int* seeds, int n_rows, int j, float inv_temp, int* tok, float* logp,
                int* d_ids, int* d_pos, int* lab_idx);
// decode.hip -- candidate scoring. geo = device ints {pre_row0, len, tail_row0, q_row0, n_pos} per candidate with at least two tokens (host_logic.h
// plan_candidates). attn_extend: out[q_row0 + p, h dh ..] = attention of query row q_row0 + p over the keys 0 .. len + p (the prompt's rows, then the candidate's
// own rows 0 .. p), p = 0 .. n_pos - 1, all candidates in one launch; per (p, h) bit-identical to attn_decode_shared at step = p + 1. n_rows = rows of q / out.
template <typename AT> int attn_extend(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* geo, int n_cands, int n_rows, AT* out,
                                       long ldo, int H, int Hkv, int dh, float scale, long cap_rows);
// cand_logp: out[t] for the n candidate tokens, src = {row, tok} each. phase 0 writes the entries with tok >= 0 (a first token): logits[row, tok] - stats[row].lse;
// phase 1 those with tok < 0: stats[row].logit[target] - stats[row].lse. stats = the {lse, logit[target], argmax, max} rows of logit_rows; n_rows = its rows.
int cand_logp(hipStream_t st, const float* logits, long ld, int V, const float* stats, int n_rows, const int* src, int n, int phase, float* out);

// One LoRA "module group" = adapters of linears that share an input (q,k,v | o | gate,up | down).
template <typename AT>
struct LoraGroupDescT {
  int din, dout, r, nseg, RP;     // RP = padded group rank (multiple of 64) = K2 of the fused GEMM segment
  int nmod, nslot;                // nseg = nslot * nmod: segment s = slot * nmod + m (stacked folds: one adapter set per slot)
  int seg_row0[4], seg_row1[4];   // output rows [row0,row1) of the fused projection owned by module m
  long a_off[4 * TST_MAX_STACK], b_off[4 * TST_MAX_STACK];  // offsets of A_seg [r,din] / B_seg [rows,r] in the flat fp32 master/grad buffers
  float scale;                    // alpha / r
  AT *Ag, *AgT, *Bg, *BgT;        // packed MFMA operands (see optim.hip): bf16, or fp32 in strict mode
  float *dAg, *dBg;               // padded fp32 gradients [RP,din], [dout,RP]
};
typedef LoraGroupDescT<bf16_t> LoraGroupDesc;
template <typename AT> int lora_pack(hipStream_t st, const LoraGroupDescT<AT>* descs_dev, int ngroups, const float* master, long max_elems);
template <typename AT> int lora_unpack_grad(hipStream_t st, const LoraGroupDescT<AT>* descs_dev, int ngroups, float* grad, long max_elems);
// (SlotEnds: see above GemmParams)
int rank_mask(hipStream_t st, bf16_t* u, int ld, int T, int width, int nslot, SlotEnds ends);

int grad_accumulate(hipStream_t st, float* acc, const float* g, long n, int first);   // acc = first ? g : acc + g
// grad_clip_coef / sumsq_partial read g in 16-byte pieces without a scalar form: g must be 16-byte aligned (TST_EINVAL otherwise, nothing is launched). Every
// range the engine hands over is: ZeRO shards, stacked slots and layer regions start at multiples of 64 floats (host_logic.h zero_shard pads to 64 * ranks).
int grad_clip_coef(hipStream_t st, const float* g, long n, float max_norm, float* partial_ws, int nparts, float* out2);
int sumsq_partial(hipStream_t st, const float* g, long n, float* partial, int nparts);       // stage 1 alone: partial[0..nparts)
int clip_finalize(hipStream_t st, const float* partial, int nparts, float max_norm, float* out2);  // stage 2 alone
int sum_partials(hipStream_t st, const float* partial, int nparts, float* out1);                    // out1[0] = sum(partial)
int clip_from_sumsq(hipStream_t st, const float* sumsq1, float max_norm, float* out2);             // {norm, coef} from a (group-summed) sum of squares
template <typename AT>
int adamw_step(hipStream_t st, float* p, const float* g, float* m, float* v, long n, const float* clip, float lr, float beta1, float beta2, float eps,
               float wd, float bc1, float bc2_sqrt, AT* shadow);
// the same update on one [rows, cols] weight matrix (multiples of 64), writing the bf16 compute copy and its transpose [cols, rows]
template <typename AT>
int adamw_step_matrix(hipStream_t st, float* p, const float* g, float* m, float* v, int rows, int cols, const float* clip, float lr, float beta1,
                      float beta2, float eps, float wd, float bc1, float bc2_sqrt, AT* shadow, AT* shadowT);
template <typename AT> int embed_bwd(hipStream_t st, const int* ids, const AT* dx, float* dE, int T, int d, int vocab);
template <typename AT> int cast_to_f32(hipStream_t st, const AT* in, float* out, long n);
template <typename AT> int colsum(hipStream_t st, const AT* x, long ld, float* out, int T, int n, float* ws);  // out[c] += sum_t x[t,c]
