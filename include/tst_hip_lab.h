/*
 * libtst_hip_lab -- test / measurement entry points of the MI355X-native TsT-LLM hot path: raw device helpers and one hook per
 * hand-written kernel (device pointers as void*), so the GPU parity tests drive every kernel on its own through a C-ABI. A maintainer
 * binding the product binds include/tst_hip.h / libtst_hip.so only; this library (the same objects + csrc/lab_hooks.hip) also exports every
 * product entry point, so a test process needs to load just one of the two. (The stream-K and four-wave tile families that lived here in
 * rounds 1-2 were measured, rejected and removed in round 3: profiles/r01_gemm_sweep_*, r01_o_gemm_four_wave_experiment.txt keep their numbers.)
 * No reference counterpart exists for anything in this file (the upstream repository ships no code).
 */
#ifndef TST_HIP_LAB_H
#define TST_HIP_LAB_H
#include "tst_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The libraries are built with -fvisibility=hidden: the declarations between this push and its pop are the ONLY dynamic symbols they export. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- raw device helpers + per-kernel entry points (GPU parity tests; device pointers as void*) ---- */
int tst_dev_alloc(void** dptr, int64_t bytes);
int tst_dev_free(void* dptr);
int tst_dev_h2d(void* dptr, const void* host, int64_t bytes);
int tst_dev_d2h(void* host, const void* dptr, int64_t bytes);
int tst_dev_memset(void* dptr, int value, int64_t bytes);
int tst_dev_sync(void);
/* attention backward of sequences of at most 128 tokens: 1 = the single fused kernel (dQ, dK, dV, delta), 0 = the dQ + dK/dV kernel pair,
 * -1 = what the environment says (TST_ATTN_FUSED_BWD). Returns the previous setting. */
int tst_dev_attn_fused_bwd(int on);

/* C[M,N] = alpha*(A[M,K].B[N,K]^T + A2[M,K2].B2[N,K2]^T) (+R); bf16 in, bf16 or f32 out; variant/splitk < 0: heuristic */
int tst_k_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C,
                  int64_t ldc, const void* R, int64_t ldr, int M, int N, int K, int K2, float alpha, int out_f32, int variant, int splitk);
/* bf16 C[M,N] = alpha * A[M,K].B[N,K]^T with the stacked folds' slot mask (row m of slot s keeps columns [s*mask_width, (s+1)*mask_width) only;
 * t_end[s] = first row after slot s; mask_width 0 = no mask). variant 8 = the rank-axis kernel (csrc/gemm_rank.hip), 0 / 1 = the tiled families. */
int tst_k_gemm_k2slots(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C, int64_t ldc, int M, int N,
                       int K, int K2, int k2_w, int nslot, const int32_t* t_end, int variant);
int tst_k_gemm_masked(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K, float alpha, int mask_width,
                      int mask_nslot, const int32_t* t_end, int variant, int splitk);
/* C[M,N] = alpha * sum_{t<kvalid} P[t,M] * Q[t,N]  (contraction over the ROW axis of both operands: adapter gradients
 * dB = dY^T u, dA = du^T x). P and Q must be readable up to kvalid rounded up to 64 rows.
 * variant 3 = tile-per-workgroup + split-K (the product path's form). */
int tst_k_gemm_tn(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int M, int N, int kvalid, float alpha, int out_f32,
                  int variant);
/* K-major members of the 256x256 ping-pong tile (csrc/gemm_pp.hip, TA / TB): ta = tb = 1 -> C[M,N] = alpha * sum_{t<kvalid} A[t,M] B[t,N] (rows >= kvalid of
 * both operands are never used: they may hold anything, NaNs included); ta = 0, tb = 1 -> C[M,N] = alpha * A[M,K] . B[K,N], K = kvalid (multiple of 64).
 * iters > 0 times it (ms_out = milliseconds per call); sumsq_out (optional; fp32 output, no split) = sum of squares of C from the tile epilogues. */
int tst_k_gemm_pp_kmajor(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int kvalid, float alpha, int out_f32, int ta,
                         int tb, int splitk, int iters, float* ms_out, float* sumsq_out);
/* slot-restricted token-axis contraction (csrc/gemm_tns.hip; the adapter gradients of stacked folds): rk [tokens, rp] holds, per token, only its slot's
 * block of w rank columns; wd [tokens, wn] is the wide operand. kind 0: c[(s w + r) * ldc + n] = alpha * sum_{t in slot s} rk[t, s w + r] wd[t, n];
 * kind 1: c[n * ldc + s w + r] = the same sum. Blocks of other slots in c are not touched. Both operands readable up to rows_pad (a multiple of 64) rows. */
int tst_k_gemm_tns(const void* rk, int64_t ldr, int rp, const void* wd, int64_t ldw, int wn, float* c, int64_t ldc, int w, float alpha, int kind, int rows_pad,
                   int nslot, const int32_t* t_end);
int tst_k_gemm_ref(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbn, int64_t sbk, float* C, int64_t ldc, int M, int N, int K);
int tst_k_transpose(const void* in, int64_t ldi, void* out, int64_t ldo, int R, int C, int R_pad);
int tst_k_embed(const int32_t* ids, const void* E, void* out, int T, int d, int vocab);
int tst_k_embed_bwd(const int32_t* ids, const void* dx, float* dE, int T, int d, int vocab, int iters, float* ms_out);   /* dE[ids[t], :] += dx[t, :], token order */
int tst_k_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps);
/* RMSNorm forward fused with the rank-axis contraction that reads its result (csrc/norm_rank.hip): y as tst_k_rmsnorm_fwd, C[T, N] = alpha * y . B^T with
 * B = [N][d] (ldb); stacked folds: mask_nslot slots of mask_width columns, t_end[s] = first row after slot s. B == NULL: the plain norm through the same kernel. */
/* RMSNorm backward with the norm-weight gradient in the same pass (csrc/norm_rank.hip): dx as tst_k_rmsnorm_bwd; dw_inout (device fp32 [d], may be NULL) +=
 * sum_t dy[t, c] bf16(x[t, c] rstd[t]) */
int tst_k_rmsnorm_bwd_dw(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, float* dw_inout, int T, int d);
int tst_k_rmsnorm_rank_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps, const void* B, int64_t ldb, void* C, int N, float alpha,
                           int mask_width, int mask_nslot, const int32_t* t_end);
int tst_k_rmsnorm_bwd(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, int T, int d);
int tst_k_rope(void* qkv, const int32_t* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, int64_t ld, int backward);
/* Qwen3 per-head q/k RMSNorm (csrc/head_norm.hip), in place on the first (H + Hkv) * 128 columns of qkv / dqkv [T, ld]: the H query heads take wq [128], the Hkv
 * key heads wk [128]; the v columns are not touched. rstd: fp32 [T, H + Hkv]. stash [T, H + Hkv, 128]: the raw rows (forward: written when non-NULL; backward:
 * required). pos / cosT / sinT non-NULL: the rotation of tst_k_rope in the same pass (forward: norm then rotate; backward: un-rotate then norm backward),
 * bit-identical to the two passes. dwq / dwk (device fp32 [128], both or neither) += the weight gradients (partial sums + ordered finish, no atomics); they need
 * ws, a caller-owned device scratch of TST_HEAD_NORM_WS_FLOATS floats (NULL otherwise). */
#define TST_HEAD_NORM_WS_FLOATS (1024 * 256)
int tst_k_head_norm_fwd(void* qkv, int64_t ld, const void* wq, const void* wk, float* rstd, void* stash, int T, int H, int Hkv, float eps, const int32_t* pos,
                        const float* cosT, const float* sinT);
int tst_k_head_norm_bwd(void* dqkv, int64_t ld, const void* wq, const void* wk, const float* rstd, const void* stash, int T, int H, int Hkv, const int32_t* pos,
                        const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws);
int tst_k_swiglu_fwd(const void* gu, void* act, int T, int F);
int tst_k_swiglu_bwd(const void* dact, const void* gu, void* dgu, int T, int F);
/* SwiGLU fused with the rank-axis contraction that reads its result (csrc/swiglu_rank.hip): act / dgu as above AND us[T,N] = alpha act . Ag^T (Ag [N][F]) resp.
   du[T,N] = alpha dgu . BgT^T (BgT [N][2F]); width > 0: stacked folds -- row t keeps the block [s width, (s+1) width) of its slot s only, ends = the first
   nslot - 1 slot boundaries (host int32) */
int tst_k_swiglu_rank_fwd(const void* gu, void* act, int T, int F, const void* Ag, int64_t ldb, void* us, int N, float alpha, int width, int nslot, const int32_t* ends);
int tst_k_swiglu_rank_bwd(const void* dact, const void* gu, void* dgu, int T, int F, const void* BgT, int64_t ldb, void* du, int N, float alpha, int width, int nslot,
                          const int32_t* ends, int block_diag);   /* block_diag: BgT rows of the first half of a rank block are zero on the up columns, of the second half on the gate columns */
/* GPT-2 family kernels: LayerNorm (stats[2*row] = mean, stats[2*row+1] = rstd; dw/db accumulate into fp32), gelu_new, wte + wpe */
int tst_k_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* stats, int T, int d, float eps);
int tst_k_layernorm_bwd(const void* dy, const void* x, const float* stats, const void* w, const void* dres, void* dx, float* dw, float* db, int T, int d);
int tst_k_gelu_fwd(const void* x, void* y, int64_t n);
int tst_k_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n);
int tst_k_embed_pos(const int32_t* ids, const int32_t* pos, const void* E, const void* P, void* out, int T, int d, int vocab, int npos);
int tst_k_logit_rows(const float* logits, int64_t ld, const int32_t* target, int n_rows, int V, float* stats, void* dlogits, int64_t ldd,
                     float inv_items, const int32_t* opt_ids, int n_opt, float* optl);
/* token attribution kernels (csrc/attribute.hip); every pointer is a device pointer, the _f32 forms are the strict-mode instances.
 * attr_seed: dlogits[r, 0 .. Vp) (bf16 / fp32, padding columns exactly 0) = row_w[r] (onehot(target[r]) - softmax(logits[r, 0 .. V))) for row_kind[r] == 0; for
 * row_kind[r] == 1 the softmax runs over the n_opt <= 256 columns opt_ids only and every other column is 0. stats[r] = {lse, logit[target], option logsumexp, max}.
 * Needs Vp >= V, Vp % 4 == 0, ld and ldd >= Vp and multiples of 4; targets and option ids inside [0, V) are the caller's to guarantee.
 * token_attr: gxi[t] = sum_c g[t, c] e[t, c], gnorm[t] = sqrt(sum_c g[t, c]^2), rows of d elements (d % 8 == 0, d <= 8192), fp32 accumulation, bit-reproducible. */
int tst_k_attr_seed(const float* logits, int64_t ld, const int32_t* target, const float* row_w, const int32_t* row_kind, const int32_t* opt_ids, int n_opt, int n_rows,
                    int V, int Vp, float* stats, void* dlogits, int64_t ldd);
int tst_k_attr_seed_f32(const float* logits, int64_t ld, const int32_t* target, const float* row_w, const int32_t* row_kind, const int32_t* opt_ids, int n_opt,
                        int n_rows, int V, int Vp, float* stats, float* dlogits, int64_t ldd);
int tst_k_token_attr(const void* g, const void* e, int T, int d, float* gxi, float* gnorm);
int tst_k_token_attr_f32(const float* g, const float* e, int T, int d, float* gxi, float* gnorm);
/* integrated-gradients kernels (csrc/attribute.hip). embed_interp: out[t, 0 .. d) = b + alpha (e - b), e = E[ids[t]], b = E[bids[t]] (+ P[pos[t]] when P != NULL; pos and npos
 * are ignored otherwise), the difference, the product and each sum rounded to fp32, ONE rounding to the element type; 0 <= alpha <= 1, d % 8 == 0, ids clamped into [0, vocab).
 * alpha == 1 copies E[ids[t]] (what tst_k_embed writes; with P, what tst_k_embed_pos writes), alpha == 0 copies E[bids[t]], and a token with bids[t] == ids[t] gets
 * its table row at every alpha, all bit for bit.
 * token_ig: acc[t] = (first ? 0 : acc[t]) + w sum_c g[t, c] (E[ids[t], c] - E[bids[t], c]), the difference in fp32; exactly (first ? 0 : acc[t]) + 0 for a token
 * with bids[t] == ids[t]. fp32 accumulation in token_attr's order, bit-reproducible. */
int tst_k_embed_interp(const int32_t* ids, const int32_t* bids, const int32_t* pos, const void* E, const void* P, void* out, int T, int d, int vocab, int npos,
                       float alpha);
int tst_k_embed_interp_f32(const int32_t* ids, const int32_t* bids, const int32_t* pos, const float* E, const float* P, float* out, int T, int d, int vocab, int npos,
                           float alpha);
int tst_k_token_ig(const void* g, const void* E, const int32_t* ids, const int32_t* bids, int T, int d, int vocab, float w, int first, float* acc);
int tst_k_token_ig_f32(const float* g, const float* E, const int32_t* ids, const int32_t* bids, int T, int d, int vocab, float w, int first, float* acc);
int tst_k_attn_fwd(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H,
                   int Hkv, int dh, float scale);
int tst_k_attn_bwd(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta,
                   const int32_t* cu, int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale);
/* the same with RoPE applied INSIDE the kernels: qkv holds un-rotated q and k, cosT / sinT are fp32 [max_position][64] tables; dq and dk of
 * dqkv come back through the inverse rotation. Sequences of at most 128 tokens, head_dim 128 (TST_EINVAL otherwise). */
int tst_k_attn_fwd_rope(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H, int Hkv,
                        int dh, float scale, const float* cosT, const float* sinT);
int tst_k_attn_bwd_rope(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta,
                        const int32_t* cu, int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale, const float* cosT,
                        const float* sinT);
/* greedy generation kernels (csrc/decode.hip). meta = device int32 {n_seqs, max_new, cu[0 .. n_seqs], len[0 .. n_seqs)}; the cache row of (sequence s,
 * position p) is cu[s] + s * max_new + p; kcache / vcache are [cap_rows, Hkv * dh].
 * kv_append: the k | v columns qkv[t, k_off .. k_off + 2 Hkv dh) of the T rows go to cache row rows[t] (device int32 [T]), bit-exact.
 * attn_decode: out[s, ldo] = attention of the ONE query token q[s, ldq] (H heads, rotated) over the cached keys 0 .. len[s] + step - 1 of sequence s;
 * H / Hkv <= 8, dh 64 or 128. Rows of the cache outside a sequence's keys are never read. */
int tst_k_kv_append(const void* qkv, int64_t ld, int k_off, const int32_t* rows, void* kcache, void* vcache, int T, int Hkv, int dh, int64_t cap_rows);
int tst_k_attn_decode(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* meta, int n_seqs, int step, void* out, int64_t ldo, int H,
                      int Hkv, int dh, float scale, int64_t cap_rows);
/* sampled generation kernels (csrc/decode.hip). geo = device int32 {rows R, max_new, n_samples, {pre_row0, len, tail_row0} per decode row r = s n_samples + i};
 * seeds = device int32 {low, high 32 bits of the seed} per sequence.
 * attn_decode_shared: attn_decode with key k of row r at cache row k < len ? pre_row0 + k : tail_row0 + k - len (len + step keys).
 * sample_rows: step j over the fp32 logits row (j == 0 ? s : r) [V of ld]: tok[r, j], logp[r, j] ([R, max_new]), d_ids[r], d_pos[r] = len + j, lab_idx[r] = r. */
int tst_k_attn_decode_shared(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_rows, int step, void* out, int64_t ldo,
                             int H, int Hkv, int dh, float scale, int64_t cap_rows);
int tst_k_attn_decode_shared_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_rows, int step, void* out,
                                 int64_t ldo, int H, int Hkv, int dh, float scale, int64_t cap_rows);
int tst_k_sample_rows(const float* logits, int64_t ld, int V, const int32_t* geo, const int32_t* seeds, int n_rows, int j, float inv_temp, int32_t* tok, float* logp,
                      int32_t* d_ids, int32_t* d_pos, int32_t* lab_idx);
/* candidate-scoring kernels (csrc/decode.hip). geo = device int32 {pre_row0, len, tail_row0, q_row0, n_pos} per candidate with at least two tokens.
 * attn_extend: rows q_row0 .. q_row0 + n_pos - 1 of out (n_rows rows, as q) = attention of the query in the same row of q over the keys 0 .. len + p, key k at
 * cache row k < len ? pre_row0 + k : tail_row0 + k - len; per (position, head) bit-identical to attn_decode_shared at step = p + 1.
 * cand_logp: out[t], t < n, from src = {row, tok} per candidate token: phase 0 writes logits[row, tok] - stats[row, 0] where tok >= 0, phase 1 writes
 * stats[row, 1] - stats[row, 0] where tok < 0; stats = fp32 [n_rows, 4] as logit_rows leaves it. */
int tst_k_attn_extend(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_cands, int n_rows, void* out, int64_t ldo, int H,
                      int Hkv, int dh, float scale, int64_t cap_rows);
int tst_k_attn_extend_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_cands, int n_rows, void* out, int64_t ldo,
                          int H, int Hkv, int dh, float scale, int64_t cap_rows);
int tst_k_cand_logp(const float* logits, int64_t ld, int V, const float* stats, int n_rows, const int32_t* src, int n, int phase, float* out);
int tst_k_adamw(float* p, const float* g, float* m, float* v, int64_t n, float max_norm, float lr, float beta1, float beta2, float eps, float wd,
                int step, float* norm_coef_out /* device [2] */, float* partial_ws /* device [256] */);
/* the optimizer kernels of csrc/optim.hip one by one; every pointer is a device pointer unless stated, every hook synchronises.
 * clip_coef = sumsq_partial + clip_finalize as the engine chains them: out2 = {||g||, min(1, max_norm / (||g|| + 1e-6))} (coefficient 1 for max_norm <= 0),
 * 1 <= nparts <= 4096 partials in partial_ws (clamped to the work). g must be 16-byte aligned in clip_coef and sumsq_partial (TST_EINVAL, nothing launched).
 * sumsq_partial: partial[0 .. nparts) = the workgroups' sums of squares (an idle workgroup writes 0). clip_finalize: out2 from nparts partials.
 * sum_partials: out1[0] = their sum; clip_from_sumsq: out2 from a sum of squares. */
int tst_k_clip_coef(const float* g, int64_t n, float max_norm, float* partial_ws, int nparts, float* out2);
int tst_k_sumsq_partial(const float* g, int64_t n, float* partial, int nparts);
int tst_k_clip_finalize(const float* partial, int nparts, float max_norm, float* out2);
int tst_k_sum_partials(const float* partial, int nparts, float* out1);
int tst_k_clip_from_sumsq(const float* sumsq1, float max_norm, float* out2);
/* one AdamW step on flat buffers, no clip pass of its own: clip = device {norm, coef} (the gradient is scaled by coef) or NULL; bias corrections from `step` in
 * host double precision as tst_k_adamw; shadow (may be NULL) also receives the new parameters, rounded to bf16 (f32 = 0) or as fp32 (f32 = 1).
 * adamw_matrix: the same on a row-major [rows, cols] matrix (multiples of 64), shadow [rows, cols] and shadowT [cols, rows] both required. */
int tst_k_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* clip, float lr, float beta1, float beta2, float eps, float wd, int step,
                     void* shadow, int f32);
int tst_k_adamw_matrix(float* p, const float* g, float* m, float* v, int rows, int cols, const float* clip, float lr, float beta1, float beta2, float eps, float wd,
                       int step, void* shadow, void* shadowT, int f32);
int tst_k_grad_accumulate(float* acc, const float* g, int64_t n, int first);   /* acc = first ? g : acc + g */
/* LoRA pack / unpack of ngroups <= 16 module groups in ONE launch (layout: csrc/optim.hip above lora_pack_tiled_kernel). Host arrays describe group i:
 * dims[5 i ..] = {din, dout, r, nmod, nslot} (din, dout multiples of 64; r <= 64; nmod <= 4 enabled modules; nslot <= 8), seg_row0 / seg_row1[4 i + m] = output rows
 * [row0, row1) of enabled module m, a_off / b_off[32 i + slot nmod + m] = float offsets of A [r, din] / B [rows, r] in master resp. grad (multiples of 4),
 * scale[i], bufs[6 i ..] = device {Ag [RP, din], AgT [din, RP], Bg [dout, RP], BgT [RP, dout], dAg [RP, din] fp32, dBg [dout, RP] fp32}, RP = nslot nmod r rounded
 * up to 64; the first four hold bf16 (f32 = 0) or fp32 (f32 = 1). pack reads master and writes Ag .. BgT; unpack reads dAg, dBg and writes the groups' ranges of grad. */
int tst_k_lora_pack(int ngroups, const int32_t* dims, const int32_t* seg_row0, const int32_t* seg_row1, const int64_t* a_off, const int64_t* b_off,
                    const float* scale, void* const* bufs, const float* master, int f32);
int tst_k_lora_unpack_grad(int ngroups, const int32_t* dims, const int32_t* seg_row0, const int32_t* seg_row1, const int64_t* a_off, const int64_t* b_off,
                           const float* scale, void* const* bufs, float* grad, int f32);
int tst_k_tr_probe(void* out_u16_64x8, int d0);
/* diagnostic: while a device buffer of 2 x 256 uint64 is set, the ping-pong contraction (variant 5) runs a build that
 * stamps s_memtime after each main-loop barrier of workgroup 0 (waves 0 and 4) into it; NULL restores the plain kernel */
int tst_k_gemm_pp_stamps(void* dev_u64_2x1024);
/* times `iters` back-to-back launches of one contraction (after 3 warm-up launches) with HIP events; *ms_out = mean ms per launch */
int tst_k_gemm_bench(const void* A, const void* B, void* C, int M, int N, int K, int out_f32, int variant, int splitk, int iters, float* ms_out);
/* the same with the stacked folds' slot mask (nslot equal runs of rows; slot s keeps columns [s * mask_width, (s + 1) * mask_width)): the rank-axis contractions as the bench issues them */
int tst_k_gemm_bench_masked(const void* A, const void* B, void* C, int M, int N, int K, int out_f32, int variant, int splitk, int iters, int mask_width, int nslot,
                            float* ms_out);

/* ---- fp32 "strict" kernels (csrc/gemm_f32.hip, csrc/attn_f32.hip): the same contracts on fp32 tensors ---- */
/* C[M,N] (fp32) = alpha*(A[M,K].B[N,K]^T + A2[M,K2].B2[N,K2]^T) (+R) (+bias[N]); every operand fp32 */
int tst_k_gemm_f32_nt(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C,
                      int64_t ldc, const void* R, int64_t ldr, const void* bias, int M, int N, int K, int K2, float alpha);
/* C[M,N] (fp32) = alpha * sum_{t<kvalid} P[t,M] * Q[t,N] */
int tst_k_gemm_f32_tn(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int M, int N, int kvalid, float alpha);
int tst_k_attn_fwd_f32(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H,
                       int Hkv, int dh, float scale);
int tst_k_attn_bwd_f32(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta,
                       const int32_t* cu, int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale);
/* elementwise kernels in fp32 (the bf16 hooks above with every bf16 tensor replaced by fp32) */
int tst_k_rmsnorm_fwd_f32(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps);
int tst_k_rmsnorm_bwd_f32(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, int T, int d);
int tst_k_rope_f32(void* qkv, const int32_t* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, int64_t ld, int backward);
int tst_k_head_norm_fwd_f32(void* qkv, int64_t ld, const void* wq, const void* wk, float* rstd, void* stash, int T, int H, int Hkv, float eps, const int32_t* pos,
                            const float* cosT, const float* sinT);
int tst_k_head_norm_bwd_f32(void* dqkv, int64_t ld, const void* wq, const void* wk, const float* rstd, const void* stash, int T, int H, int Hkv, const int32_t* pos,
                            const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws);
int tst_k_kv_append_f32(const void* qkv, int64_t ld, int k_off, const int32_t* rows, void* kcache, void* vcache, int T, int Hkv, int dh, int64_t cap_rows);
int tst_k_attn_decode_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* meta, int n_seqs, int step, void* out, int64_t ldo,
                          int H, int Hkv, int dh, float scale, int64_t cap_rows);
int tst_k_swiglu_fwd_f32(const void* gu, void* act, int T, int F);
int tst_k_swiglu_bwd_f32(const void* dact, const void* gu, void* dgu, int T, int F);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
