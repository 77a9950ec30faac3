// Lab / test entry points (include/tst_hip_lab.h): raw device helpers and one hook per hand-written kernel, so the GPU parity tests can
// drive every kernel on its own through the C-ABI. Built only into libtst_hip_lab.so (-DTST_BUILD_LAB); the product library
// libtst_hip.so exports none of this.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tst_hip_lab.h"
#include "common.h"
#include "kernels.h"

namespace {
// tst_k_lora_pack (master != NULL) / tst_k_lora_unpack_grad (grad != NULL): the descriptors as engine.hip add_group / build_ctx fill them (nseg = nslot * nmod,
// RP = nseg * r rounded up to 64), uploaded, one launch with the engine's grid bounds (longest axis resp. most padded elements of a group), synchronised, freed.
// What the kernels rely on is checked here: 64-wide tiles along din / dout, 16-byte reads of the A master always and of the B master on the r % 8 == 0 path.
template <typename AT>
int lora_lab(int ngroups, const int32_t* dims, const int32_t* seg_row0, const int32_t* seg_row1, const int64_t* a_off, const int64_t* b_off, const float* scale,
             void* const* bufs, const float* master, float* grad) {
  if (ngroups < 1 || ngroups > 16 || !dims || !seg_row0 || !seg_row1 || !a_off || !b_off || !scale || !bufs || (!master && !grad)) return TST_EINVAL;
  if (master && (((unsigned long long)master) & 15ull)) return TST_EINVAL;
  std::vector<LoraGroupDescT<AT>> descs((size_t)ngroups);
  long max_long = 0, max_elems = 0;
  for (int i = 0; i < ngroups; ++i) {
    LoraGroupDescT<AT>& d = descs[(size_t)i];
    memset(&d, 0, sizeof(d));
    d.din = dims[5 * i]; d.dout = dims[5 * i + 1]; d.r = dims[5 * i + 2]; d.nmod = dims[5 * i + 3]; d.nslot = dims[5 * i + 4];
    if (d.din < 64 || (d.din & 63) || d.dout < 64 || (d.dout & 63) || d.r < 1 || d.r > 64 || d.nmod < 1 || d.nmod > 4 || d.nslot < 1 || d.nslot > TST_MAX_STACK)
      return TST_EINVAL;
    d.nseg = d.nslot * d.nmod;
    d.RP = (d.nseg * d.r + 63) / 64 * 64;
    d.scale = scale[i];
    for (int m = 0; m < d.nmod; ++m) {
      d.seg_row0[m] = seg_row0[4 * i + m]; d.seg_row1[m] = seg_row1[4 * i + m];
      if (d.seg_row0[m] < 0 || d.seg_row1[m] <= d.seg_row0[m] || d.seg_row1[m] > d.dout) return TST_EINVAL;
    }
    for (int s = 0; s < d.nseg; ++s) {
      d.a_off[s] = (long)a_off[32 * i + s]; d.b_off[s] = (long)b_off[32 * i + s];
      if (d.a_off[s] < 0 || d.b_off[s] < 0 || (d.a_off[s] & 3) || (d.b_off[s] & 3)) return TST_EINVAL;
    }
    for (int b = 0; b < 6; ++b)
      if (!bufs[6 * i + b]) return TST_EINVAL;
    d.Ag = (AT*)bufs[6 * i]; d.AgT = (AT*)bufs[6 * i + 1]; d.Bg = (AT*)bufs[6 * i + 2]; d.BgT = (AT*)bufs[6 * i + 3];
    d.dAg = (float*)bufs[6 * i + 4]; d.dBg = (float*)bufs[6 * i + 5];
    max_long = std::max(max_long, (long)std::max(d.din, d.dout));
    max_elems = std::max(max_elems, (long)d.RP * d.din + (long)d.dout * d.RP);
  }
  LoraGroupDescT<AT>* dev = nullptr;
  const size_t bytes = descs.size() * sizeof(LoraGroupDescT<AT>);
  if (hipMalloc((void**)&dev, bytes) != hipSuccess) return TST_ENOMEM;
  int rc = hipMemcpy(dev, descs.data(), bytes, hipMemcpyHostToDevice) == hipSuccess ? TST_OK : TST_EHIP;
  if (rc == TST_OK) rc = master ? lora_pack<AT>(nullptr, dev, ngroups, master, max_long) : lora_unpack_grad<AT>(nullptr, dev, ngroups, grad, max_elems);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  (void)hipFree(dev);
  return rc;
}
}  // namespace

extern "C" {

int tst_dev_alloc(void** dptr, int64_t bytes) { return (dptr && hipMalloc(dptr, (size_t)(bytes > 0 ? bytes : 16)) == hipSuccess) ? TST_OK : TST_ENOMEM; }
int tst_dev_free(void* dptr) { return hipFree(dptr) == hipSuccess ? TST_OK : TST_EHIP; }
int tst_dev_h2d(void* dptr, const void* host, int64_t bytes) { return hipMemcpy(dptr, host, (size_t)bytes, hipMemcpyHostToDevice) == hipSuccess ? TST_OK : TST_EHIP; }
int tst_dev_d2h(void* host, const void* dptr, int64_t bytes) {
  if (hipDeviceSynchronize() != hipSuccess) return TST_EHIP;
  return hipMemcpy(host, dptr, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? TST_OK : TST_EHIP;
}
int tst_dev_memset(void* dptr, int value, int64_t bytes) { return hipMemset(dptr, value, (size_t)bytes) == hipSuccess ? TST_OK : TST_EHIP; }
int tst_dev_sync(void) { return hipDeviceSynchronize() == hipSuccess ? TST_OK : TST_EHIP; }
int tst_dev_attn_fused_bwd(int on) { return attn_fused_bwd(on); }

int tst_k_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C, int64_t ldc,
                  const void* R, int64_t ldr, int M, int N, int K, int K2, float alpha, int out_f32, int variant, int splitk) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = lda; p.B = (const bf16_t*)B; p.ldb = ldb;
  p.A2 = (const bf16_t*)A2; p.lda2 = lda2; p.B2 = (const bf16_t*)B2; p.ldb2 = ldb2;
  p.C = C; p.ldc = ldc; p.R = (const bf16_t*)R; p.ldr = ldr; p.M = M; p.N = N; p.K = K; p.K2 = K2; p.alpha = alpha; p.out_f32 = out_f32;
  int v, sk;
  gemm_plan(M, N, K, K2, &v, &sk);
  if (splitk > 0) sk = splitk;
  float* slab = nullptr;
  size_t sb = gemm_slab_bytes(M, N, sk);
  if (sb < (64u << 20)) sb = 64u << 20;   // as in a context: the 256x256 tile's tail split needs a workspace even when K is not split
  if (hipMalloc((void**)&slab, sb) != hipSuccess) return TST_ENOMEM;
  int rc = gemm_nt(nullptr, p, slab, sb, variant, sk, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  if (slab) (void)hipFree(slab);
  return rc;
}
// rank-axis contraction with the stacked folds' slot mask: variant 8 = gemm_rank.hip, 0 / 1 = the tiled families (mask in their epilogue / split-K reduce)
int tst_k_gemm_masked(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K, float alpha, int mask_width,
                      int mask_nslot, const int32_t* t_end, int variant, int splitk) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = lda; p.B = (const bf16_t*)B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.alpha = alpha;
  p.mask_width = mask_width; p.mask_nslot = mask_nslot;
  for (int q = 0; q < TST_MAX_STACK; ++q) p.mask_ends.t_end[q] = (t_end && q < mask_nslot) ? t_end[q] : M;
  float* slab = nullptr;
  const size_t sb = 256u << 20;
  if (hipMalloc((void**)&slab, sb) != hipSuccess) return TST_ENOMEM;
  int rc = gemm_nt(nullptr, p, slab, sb, variant, splitk, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  (void)hipFree(slab);
  return rc;
}
// projection with a second K segment whose A2 rows are zero outside their slot's column block (k2_w > 0: the ping-pong tile skips the other slots' K2 k-tiles)
int tst_k_gemm_k2slots(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C, int64_t ldc, int M, int N,
                       int K, int K2, int k2_w, int nslot, const int32_t* t_end, int variant) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = lda; p.B = (const bf16_t*)B; p.ldb = ldb; p.A2 = (const bf16_t*)A2; p.lda2 = lda2; p.B2 = (const bf16_t*)B2; p.ldb2 = ldb2;
  p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.K2 = K2; p.alpha = 1.0f;
  p.k2_w = k2_w; p.mask_nslot = nslot;
  for (int q = 0; q < TST_MAX_STACK; ++q) p.mask_ends.t_end[q] = (t_end && q < nslot) ? t_end[q] : M;
  int rc = gemm_nt(nullptr, p, nullptr, 0, variant, 1, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  return rc;
}
int tst_k_gemm_tn(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int M, int N, int kvalid, float alpha, int out_f32,
                  int variant) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)P; p.lda = ldp; p.B = (const bf16_t*)Q; p.ldb = ldq; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = (kvalid + 63) / 64 * 64; p.kvalid = kvalid; p.alpha = alpha; p.out_f32 = out_f32;
  int rc;
  (void)variant;   // (3 = tile-per-workgroup + split-K: the only form left)
  float* slab = nullptr;
  const size_t sb = (size_t)32 * M * N * sizeof(float);
  if (hipMalloc((void**)&slab, sb) != hipSuccess) return TST_ENOMEM;
  rc = gemm_tn(nullptr, p, slab, sb, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  (void)hipFree(slab);
  return rc;
}
// K-major members of the 256x256 ping-pong tile: ta = tb = 1 (TN): C[M,N] = alpha * sum_{t<kvalid} A[t,M] B[t,N]; ta = 0, tb = 1 (NN): C[M,N] = alpha * A[M,K] . B[K,N]
// (K = kvalid, a multiple of 64). iters > 0: timed repeats, ms_out = milliseconds per call (random operands are the caller's business); sumsq_out (optional,
// fp32 output without split-K): the sum of the per-workgroup sums of squares
int tst_k_gemm_pp_kmajor(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int kvalid, float alpha, int out_f32, int ta,
                         int tb, int splitk, int iters, float* ms_out, float* sumsq_out) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = lda; p.B = (const bf16_t*)B; p.ldb = ldb; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = (kvalid + 63) / 64 * 64; p.kvalid = (ta && tb) ? kvalid : 0; p.alpha = alpha; p.out_f32 = out_f32; p.ta = ta; p.tb = tb;
  float *slab = nullptr, *ssq = nullptr;
  const size_t sb = std::max(gemm_slab_bytes(M, N, splitk > 1 ? splitk : 1), (size_t)64 << 20);
  if (hipMalloc((void**)&slab, sb) != hipSuccess) return TST_ENOMEM;
  const int nslots = ((M + 255) / 256) * ((N + 255) / 256) + 2048;
  if (sumsq_out) {
    if (hipMalloc((void**)&ssq, (size_t)nslots * sizeof(float)) != hipSuccess) { (void)hipFree(slab); return TST_ENOMEM; }
    (void)hipMemset(ssq, 0, (size_t)nslots * sizeof(float));
    p.sumsq = ssq;
  }
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return TST_EHIP;
  int rc = gemm_pp_kmajor(nullptr, p, slab, sb, splitk > 0 ? splitk : 1, nullptr);
  if (iters > 0) {
    for (int i = 0; i < 2 && rc == TST_OK; ++i) rc = gemm_pp_kmajor(nullptr, p, slab, sb, splitk > 0 ? splitk : 1, nullptr);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && rc == TST_OK; ++i) rc = gemm_pp_kmajor(nullptr, p, slab, sb, splitk > 0 ? splitk : 1, nullptr);
    (void)hipEventRecord(e1, nullptr);
  }
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  if (iters > 0 && ms_out) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / (float)iters;
  }
  if (sumsq_out && rc == TST_OK) {
    std::vector<float> h((size_t)nslots);
    if (hipMemcpy(h.data(), ssq, (size_t)nslots * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = TST_EHIP;
    double t = 0;
    for (float v : h) t += v;
    *sumsq_out = (float)t;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ssq) (void)hipFree(ssq);
  (void)hipFree(slab);
  return rc;
}
// slot-restricted adapter-gradient contraction (gemm_tns.hip): one problem; t_end[nslot] = slot boundaries
int tst_k_gemm_tns(const void* rk, int64_t ldr, int rp, const void* wd, int64_t ldw, int wn, float* c, int64_t ldc, int w, float alpha, int kind, int rows_pad,
                   int nslot, const int32_t* t_end) {
  TnsProblem p;
  memset(&p, 0, sizeof(p));
  p.rk = (const bf16_t*)rk; p.ldr = ldr; p.rp = rp; p.wd = (const bf16_t*)wd; p.ldw = ldw; p.wn = wn; p.c = c; p.ldc = ldc; p.w = w; p.alpha = alpha; p.kind = kind;
  p.rows_pad = rows_pad;
  SlotEnds ends;
  for (int q = 0; q < TST_MAX_STACK; ++q) ends.t_end[q] = t_end[q < nslot ? q : nslot - 1];
  int rc = gemm_tns_grouped(nullptr, &p, 1, nslot, ends);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  return rc;
}
int tst_k_gemm_ref(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbn, int64_t sbk, float* C, int64_t ldc, int M, int N, int K) {
  return gemm_ref(nullptr, (const bf16_t*)A, sam, sak, (const bf16_t*)B, sbn, sbk, C, ldc, M, N, K);
}
int tst_k_transpose(const void* in, int64_t ldi, void* out, int64_t ldo, int R, int C, int R_pad) {
  return transpose_mat<bf16_t>(nullptr, (const bf16_t*)in, ldi, (bf16_t*)out, ldo, R, C, R_pad);
}
int tst_k_embed(const int32_t* ids, const void* E, void* out, int T, int d, int vocab) { return embed_fwd(nullptr, ids, (const bf16_t*)E, (bf16_t*)out, T, d, vocab); }
// dE[ids[t], :] += dx[t, :] (fp32 dE, bf16 dx); iters > 0 and ms_out: average milliseconds of a launch (HIP events), dE keeps the sum of all launches
int tst_k_embed_bwd(const int32_t* ids, const void* dx, float* dE, int T, int d, int vocab, int iters, float* ms_out) {
  if (iters <= 0 || !ms_out) return embed_bwd(nullptr, ids, (const bf16_t*)dx, dE, T, d, vocab);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return TST_EHIP;
  (void)hipEventRecord(e0, nullptr);
  int rc = TST_OK;
  for (int i = 0; i < iters && rc == TST_OK; ++i) rc = embed_bwd(nullptr, ids, (const bf16_t*)dx, dE, T, d, vocab);
  (void)hipEventRecord(e1, nullptr);
  float ms = 0.f;
  if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = TST_EHIP;
  *ms_out = ms / iters;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return rc;
}
int tst_k_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps) {
  return rmsnorm_fwd(nullptr, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rstd, T, d, eps);
}
// RMSNorm forward fused with the rank-axis contraction (norm_rank.hip); B == NULL: the plain norm through the same kernel
int tst_k_rmsnorm_rank_fwd(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps, const void* B, int64_t ldb, void* C, int N, float alpha,
                           int mask_width, int mask_nslot, const int32_t* t_end) {
  NormRank r;
  memset(&r, 0, sizeof(r));
  r.B = (const bf16_t*)B; r.ldb = ldb; r.C = (bf16_t*)C; r.N = N; r.alpha = alpha; r.mask_width = mask_width; r.mask_nslot = mask_nslot;
  for (int q = 0; q < TST_MAX_STACK; ++q) r.mask_ends.t_end[q] = (t_end && q < mask_nslot) ? t_end[q] : T;
  return rmsnorm_rank_fwd(nullptr, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rstd, T, d, eps, B ? &r : nullptr);
}
// RMSNorm backward + norm-weight gradient in one pass (norm_rank.hip): dw_inout += the gradient (device fp32 [d]); dw_inout == NULL: dx only
int tst_k_rmsnorm_bwd_dw(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, float* dw_inout, int T, int d) {
  float* ws = nullptr;
  if (dw_inout && hipMalloc((void**)&ws, (size_t)colred_ws_floats(T, d) * sizeof(float)) != hipSuccess) return TST_ENOMEM;
  int rc = rmsnorm_bwd_dw(nullptr, (const bf16_t*)dy, (const bf16_t*)x, rstd, (const bf16_t*)w, (const bf16_t*)dres, (bf16_t*)dx, dw_inout, T, d, ws);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  if (ws) (void)hipFree(ws);
  return rc;
}
int tst_k_rmsnorm_bwd(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, int T, int d) {
  return rmsnorm_bwd(nullptr, (const bf16_t*)dy, (const bf16_t*)x, rstd, (const bf16_t*)w, (const bf16_t*)dres, (bf16_t*)dx, T, d);
}
int tst_k_rope(void* qkv, const int32_t* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, int64_t ld, int backward) {
  return rope_apply(nullptr, (bf16_t*)qkv, pos, cosT, sinT, T, nheads_rot, dh, ld, backward);
}
int tst_k_swiglu_fwd(const void* gu, void* act, int T, int F) { return swiglu_fwd(nullptr, (const bf16_t*)gu, (bf16_t*)act, T, F); }
int tst_k_swiglu_bwd(const void* dact, const void* gu, void* dgu, int T, int F) { return swiglu_bwd(nullptr, (const bf16_t*)dact, (const bf16_t*)gu, (bf16_t*)dgu, T, F); }
// SwiGLU + rank-axis contraction in one pass (swiglu_rank.hip): ends = the first nslot - 1 slot boundaries (token rows), width = rank columns per slot (0: unstacked)
static SwiRank swi_rank(const void* B, int64_t ldb, void* C, int N, float alpha, int width, int nslot, const int32_t* ends) {
  SwiRank r;
  memset(&r, 0, sizeof(r));
  r.B = (const bf16_t*)B; r.ldb = ldb; r.C = (bf16_t*)C; r.N = N; r.alpha = alpha; r.mask_width = width; r.mask_nslot = nslot;
  for (int q = 0; ends && q < nslot - 1 && q < TST_MAX_STACK; ++q) r.mask_ends.t_end[q] = ends[q];
  return r;
}
int tst_k_swiglu_rank_fwd(const void* gu, void* act, int T, int F, const void* Ag, int64_t ldb, void* us, int N, float alpha, int width, int nslot, const int32_t* ends) {
  return swiglu_rank_fwd(nullptr, (const bf16_t*)gu, (bf16_t*)act, T, F, swi_rank(Ag, ldb, us, N, alpha, width, nslot, ends));
}
int tst_k_swiglu_rank_bwd(const void* dact, const void* gu, void* dgu, int T, int F, const void* BgT, int64_t ldb, void* du, int N, float alpha, int width, int nslot,
                          const int32_t* ends, int block_diag) {
  SwiRank r = swi_rank(BgT, ldb, du, N, alpha, width, nslot, ends);
  r.block_diag = block_diag;
  return swiglu_rank_bwd(nullptr, (const bf16_t*)dact, (const bf16_t*)gu, (bf16_t*)dgu, T, F, r);
}
int tst_k_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* stats, int T, int d, float eps) {
  return layernorm_fwd(nullptr, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, stats, T, d, eps);
}
int tst_k_layernorm_bwd(const void* dy, const void* x, const float* stats, const void* w, const void* dres, void* dx, float* dw, float* db, int T, int d) {
  if (dw && db) {
    float* ws = nullptr;
    if (hipMalloc(&ws, (size_t)(2 * colred_ws_floats(T, d) + 4) * sizeof(float)) != hipSuccess) return TST_ENOMEM;
    int rc = layernorm_dwdb(nullptr, (const bf16_t*)dy, (const bf16_t*)x, stats, dw, db, T, d, ws);
    (void)hipDeviceSynchronize();
    (void)hipFree(ws);
    if (rc != TST_OK) return rc;
  }
  return layernorm_bwd(nullptr, (const bf16_t*)dy, (const bf16_t*)x, stats, (const bf16_t*)w, (const bf16_t*)dres, (bf16_t*)dx, T, d);
}
int tst_k_gelu_fwd(const void* x, void* y, int64_t n) { return gelu_fwd(nullptr, (const bf16_t*)x, (bf16_t*)y, (long)n); }
int tst_k_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n) { return gelu_bwd(nullptr, (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx, (long)n); }
int tst_k_embed_pos(const int32_t* ids, const int32_t* pos, const void* E, const void* P, void* out, int T, int d, int vocab, int npos) {
  return embed_pos_fwd(nullptr, ids, pos, (const bf16_t*)E, (const bf16_t*)P, (bf16_t*)out, T, d, vocab, npos);
}
int tst_k_logit_rows(const float* logits, int64_t ld, const int32_t* target, int n_rows, int V, float* stats, void* dlogits, int64_t ldd, float inv_items,
                     const int32_t* opt_ids, int n_opt, float* optl) {
  return logit_rows(nullptr, logits, ld, target, n_rows, V, stats, (bf16_t*)dlogits, ldd, inv_items, opt_ids, n_opt, optl);
}
// token attribution (csrc/attribute.hip): every pointer is a device pointer; the _f32 forms are the strict-mode instances
int tst_k_attr_seed(const float* logits, int64_t ld, const int32_t* target, const float* row_w, const int32_t* row_kind, const int32_t* opt_ids, int n_opt, int n_rows,
                    int V, int Vp, float* stats, void* dlogits, int64_t ldd) {
  return attr_seed<bf16_t>(nullptr, logits, ld, target, row_w, row_kind, opt_ids, n_opt, n_rows, V, Vp, stats, (bf16_t*)dlogits, ldd);
}
int tst_k_attr_seed_f32(const float* logits, int64_t ld, const int32_t* target, const float* row_w, const int32_t* row_kind, const int32_t* opt_ids, int n_opt,
                        int n_rows, int V, int Vp, float* stats, float* dlogits, int64_t ldd) {
  return attr_seed<float>(nullptr, logits, ld, target, row_w, row_kind, opt_ids, n_opt, n_rows, V, Vp, stats, dlogits, ldd);
}
int tst_k_token_attr(const void* g, const void* e, int T, int d, float* gxi, float* gnorm) {
  return token_attr<bf16_t>(nullptr, (const bf16_t*)g, (const bf16_t*)e, T, d, gxi, gnorm);
}
int tst_k_token_attr_f32(const float* g, const float* e, int T, int d, float* gxi, float* gnorm) { return token_attr<float>(nullptr, g, e, T, d, gxi, gnorm); }
int tst_k_embed_interp(const int32_t* ids, const int32_t* bids, const int32_t* pos, const void* E, const void* P, void* out, int T, int d, int vocab, int npos,
                       float alpha) {
  return embed_interp<bf16_t>(nullptr, ids, bids, pos, (const bf16_t*)E, (const bf16_t*)P, (bf16_t*)out, T, d, vocab, npos, alpha);
}
int tst_k_embed_interp_f32(const int32_t* ids, const int32_t* bids, const int32_t* pos, const float* E, const float* P, float* out, int T, int d, int vocab, int npos,
                           float alpha) {
  return embed_interp<float>(nullptr, ids, bids, pos, E, P, out, T, d, vocab, npos, alpha);
}
int tst_k_token_ig(const void* g, const void* E, const int32_t* ids, const int32_t* bids, int T, int d, int vocab, float w, int first, float* acc) {
  return token_ig<bf16_t>(nullptr, (const bf16_t*)g, (const bf16_t*)E, ids, bids, T, d, vocab, w, first != 0, acc);
}
int tst_k_token_ig_f32(const float* g, const float* E, const int32_t* ids, const int32_t* bids, int T, int d, int vocab, float w, int first, float* acc) {
  return token_ig<float>(nullptr, g, E, ids, bids, T, d, vocab, w, first != 0, acc);
}
int tst_k_attn_fwd(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H, int Hkv, int dh,
                   float scale) {
  return attn_fwd(nullptr, (const bf16_t*)qkv, ld, cu, n_seqs, max_len, (bf16_t*)out, ldo, lse, T, H, Hkv, dh, scale);
}
int tst_k_attn_bwd(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta, const int32_t* cu,
                   int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale) {
  return attn_bwd(nullptr, (const bf16_t*)qkv, ld, (const bf16_t*)out, ldo, (const bf16_t*)dO, lddo, lse, delta, cu, n_seqs, max_len, (bf16_t*)dqkv, T, H, Hkv,
                  dh, scale);
}
// attention with RoPE inside the kernels (qkv un-rotated, tables fp32 [max_position][64]); TST_EINVAL where the fused path does not apply
int tst_k_attn_fwd_rope(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H, int Hkv, int dh,
                        float scale, const float* cosT, const float* sinT) {
  if (!attn_rope_fusable(max_len, dh)) return TST_EINVAL;
  return attn_fwd(nullptr, (const bf16_t*)qkv, ld, cu, n_seqs, max_len, (bf16_t*)out, ldo, lse, T, H, Hkv, dh, scale, cosT, sinT);
}
int tst_k_attn_bwd_rope(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta, const int32_t* cu,
                        int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale, const float* cosT, const float* sinT) {
  if (!attn_rope_fusable(max_len, dh)) return TST_EINVAL;
  return attn_bwd(nullptr, (const bf16_t*)qkv, ld, (const bf16_t*)out, ldo, (const bf16_t*)dO, lddo, lse, delta, cu, n_seqs, max_len, (bf16_t*)dqkv, T, H, Hkv,
                  dh, scale, cosT, sinT);
}
int tst_k_adamw(float* p, const float* g, float* m, float* v, int64_t n, float max_norm, float lr, float beta1, float beta2, float eps, float wd, int step,
                float* norm_coef_out, float* partial_ws) {
  int rc = grad_clip_coef(nullptr, g, n, max_norm, partial_ws, 256, norm_coef_out);
  if (rc != TST_OK) return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  return adamw_step<bf16_t>(nullptr, p, g, m, v, n, norm_coef_out, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), nullptr);
}
// ---- the optimizer kernels one by one (optim.hip); a hook launches, synchronises and returns the library's status
static int synced(int rc) { return hipDeviceSynchronize() == hipSuccess ? rc : TST_EHIP; }
int tst_k_clip_coef(const float* g, int64_t n, float max_norm, float* partial_ws, int nparts, float* out2) {
  return synced(grad_clip_coef(nullptr, g, (long)n, max_norm, partial_ws, nparts, out2));
}
int tst_k_sumsq_partial(const float* g, int64_t n, float* partial, int nparts) { return synced(sumsq_partial(nullptr, g, (long)n, partial, nparts)); }
int tst_k_clip_finalize(const float* partial, int nparts, float max_norm, float* out2) { return synced(clip_finalize(nullptr, partial, nparts, max_norm, out2)); }
int tst_k_sum_partials(const float* partial, int nparts, float* out1) { return synced(sum_partials(nullptr, partial, nparts, out1)); }
int tst_k_clip_from_sumsq(const float* sumsq1, float max_norm, float* out2) { return synced(clip_from_sumsq(nullptr, sumsq1, max_norm, out2)); }
int tst_k_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* clip, float lr, float beta1, float beta2, float eps, float wd, int step,
                     void* shadow, int f32) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  return synced(f32 ? adamw_step<float>(nullptr, p, g, m, v, (long)n, clip, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), (float*)shadow)
                    : adamw_step<bf16_t>(nullptr, p, g, m, v, (long)n, clip, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), (bf16_t*)shadow));
}
int tst_k_adamw_matrix(float* p, const float* g, float* m, float* v, int rows, int cols, const float* clip, float lr, float beta1, float beta2, float eps, float wd,
                       int step, void* shadow, void* shadowT, int f32) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  return synced(f32 ? adamw_step_matrix<float>(nullptr, p, g, m, v, rows, cols, clip, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), (float*)shadow,
                                               (float*)shadowT)
                    : adamw_step_matrix<bf16_t>(nullptr, p, g, m, v, rows, cols, clip, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), (bf16_t*)shadow,
                                                (bf16_t*)shadowT));
}
int tst_k_grad_accumulate(float* acc, const float* g, int64_t n, int first) { return synced(grad_accumulate(nullptr, acc, g, (long)n, first)); }
int tst_k_lora_pack(int ngroups, const int32_t* dims, const int32_t* seg_row0, const int32_t* seg_row1, const int64_t* a_off, const int64_t* b_off,
                    const float* scale, void* const* bufs, const float* master, int f32) {
  return f32 ? lora_lab<float>(ngroups, dims, seg_row0, seg_row1, a_off, b_off, scale, bufs, master, nullptr)
             : lora_lab<bf16_t>(ngroups, dims, seg_row0, seg_row1, a_off, b_off, scale, bufs, master, nullptr);
}
int tst_k_lora_unpack_grad(int ngroups, const int32_t* dims, const int32_t* seg_row0, const int32_t* seg_row1, const int64_t* a_off, const int64_t* b_off,
                           const float* scale, void* const* bufs, float* grad, int f32) {
  return f32 ? lora_lab<float>(ngroups, dims, seg_row0, seg_row1, a_off, b_off, scale, bufs, nullptr, grad)
             : lora_lab<bf16_t>(ngroups, dims, seg_row0, seg_row1, a_off, b_off, scale, bufs, nullptr, grad);
}
int tst_k_tr_probe(void* out_u16_64x8, int d0) { return tr_probe(nullptr, (unsigned short*)out_u16_64x8, d0); }
int tst_k_gemm_pp_stamps(void* dev_u64_2x1024) { gemm_pp_set_stamps((unsigned long long*)dev_u64_2x1024); return TST_OK; }

int tst_k_gemm_bench_masked(const void* A, const void* B, void* C, int M, int N, int K, int out_f32, int variant, int splitk, int iters, int mask_width, int nslot,
                            float* ms_out);
int tst_k_gemm_bench(const void* A, const void* B, void* C, int M, int N, int K, int out_f32, int variant, int splitk, int iters, float* ms_out) {
  return tst_k_gemm_bench_masked(A, B, C, M, N, K, out_f32, variant, splitk, iters, 0, 0, ms_out);
}
// the same with the stacked folds' slot mask: nslot equal runs of rows, slot s keeps columns [s * mask_width, (s + 1) * mask_width)
int tst_k_gemm_bench_masked(const void* A, const void* B, void* C, int M, int N, int K, int out_f32, int variant, int splitk, int iters, int mask_width, int nslot,
                            float* ms_out) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16_t*)A; p.lda = K; p.B = (const bf16_t*)B; p.ldb = K; p.C = C; p.ldc = N; p.M = M; p.N = N; p.K = K; p.alpha = 1.0f; p.out_f32 = out_f32;
  if (mask_width > 0 && nslot > 0) {
    p.mask_width = mask_width; p.mask_nslot = nslot;
    for (int q = 0; q < TST_MAX_STACK; ++q) p.mask_ends.t_end[q] = q < nslot - 1 ? (int)((long)M * (q + 1) / nslot) : M;
  }
  int v, sk;
  gemm_plan(M, N, K, 0, &v, &sk);
  if (splitk > 0) sk = splitk;
  float* slab = nullptr;
  size_t sb = gemm_slab_bytes(M, N, sk);
  if (sb < (64u << 20)) sb = 64u << 20;   // as in a context (tail split of the 256x256 tile)
  if (hipMalloc((void**)&slab, sb) != hipSuccess) return TST_ENOMEM;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return TST_EHIP;
  int rc = TST_OK;
  for (int i = 0; i < 3 && rc == TST_OK; ++i) rc = gemm_nt(nullptr, p, slab, sb, variant, sk, nullptr);
  (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters && rc == TST_OK; ++i) rc = gemm_nt(nullptr, p, slab, sb, variant, sk, nullptr);
  (void)hipEventRecord(e1, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (ms_out) *ms_out = ms / (float)(iters > 0 ? iters : 1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (slab) (void)hipFree(slab);
  return rc;
}

// ---- fp32 "strict" kernels
int tst_k_gemm_f32_nt(const void* A, int64_t lda, const void* B, int64_t ldb, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, void* C, int64_t ldc,
                      const void* R, int64_t ldr, const void* bias, int M, int N, int K, int K2, float alpha) {
  GemmParamsF p;
  memset(&p, 0, sizeof(p));
  p.A = (const float*)A; p.lda = lda; p.B = (const float*)B; p.ldb = ldb;
  p.A2 = (const float*)A2; p.lda2 = lda2; p.B2 = (const float*)B2; p.ldb2 = ldb2;
  p.C = C; p.ldc = ldc; p.R = (const float*)R; p.ldr = ldr; p.bias = (const float*)bias; p.M = M; p.N = N; p.K = K; p.K2 = K2; p.alpha = alpha; p.out_f32 = 1;
  int rc = gemm_nt(nullptr, p, nullptr, 0, -1, -1, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  return rc;
}
int tst_k_gemm_f32_tn(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int M, int N, int kvalid, float alpha) {
  GemmParamsF p;
  memset(&p, 0, sizeof(p));
  p.A = (const float*)P; p.lda = ldp; p.B = (const float*)Q; p.ldb = ldq; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.kvalid = kvalid; p.alpha = alpha; p.out_f32 = 1;
  int rc = gemm_tn(nullptr, p, nullptr, 0, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) rc = TST_EHIP;
  return rc;
}
int tst_k_attn_fwd_f32(const void* qkv, int64_t ld, const int32_t* cu, int n_seqs, int max_len, void* out, int64_t ldo, float* lse, int T, int H, int Hkv, int dh,
                       float scale) {
  return attn_fwd(nullptr, (const float*)qkv, ld, cu, n_seqs, max_len, (float*)out, ldo, lse, T, H, Hkv, dh, scale);
}
int tst_k_attn_bwd_f32(const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dO, int64_t lddo, const float* lse, float* delta, const int32_t* cu,
                       int n_seqs, int max_len, void* dqkv, int T, int H, int Hkv, int dh, float scale) {
  return attn_bwd(nullptr, (const float*)qkv, ld, (const float*)out, ldo, (const float*)dO, lddo, lse, delta, cu, n_seqs, max_len, (float*)dqkv, T, H, Hkv, dh,
                  scale);
}
int tst_k_rmsnorm_fwd_f32(const void* x, const void* w, void* y, float* rstd, int T, int d, float eps) {
  return rmsnorm_fwd<float>(nullptr, (const float*)x, (const float*)w, (float*)y, rstd, T, d, eps);
}
int tst_k_rmsnorm_bwd_f32(const void* dy, const void* x, const float* rstd, const void* w, const void* dres, void* dx, int T, int d) {
  return rmsnorm_bwd<float>(nullptr, (const float*)dy, (const float*)x, rstd, (const float*)w, (const float*)dres, (float*)dx, T, d);
}
int tst_k_rope_f32(void* qkv, const int32_t* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, int64_t ld, int backward) {
  return rope_apply<float>(nullptr, (float*)qkv, pos, cosT, sinT, T, nheads_rot, dh, ld, backward);
}
// Qwen3 per-head q/k RMSNorm (head_norm.hip)
int tst_k_head_norm_fwd(void* qkv, int64_t ld, const void* wq, const void* wk, float* rstd, void* stash, int T, int H, int Hkv, float eps, const int32_t* pos,
                        const float* cosT, const float* sinT) {
  return head_norm_fwd<bf16_t>(nullptr, (bf16_t*)qkv, (long)ld, (const bf16_t*)wq, (const bf16_t*)wk, rstd, (bf16_t*)stash, T, H, Hkv, eps, pos, cosT, sinT);
}
int tst_k_head_norm_bwd(void* dqkv, int64_t ld, const void* wq, const void* wk, const float* rstd, const void* stash, int T, int H, int Hkv, const int32_t* pos,
                        const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws) {
  return head_norm_bwd<bf16_t>(nullptr, (bf16_t*)dqkv, (long)ld, (const bf16_t*)wq, (const bf16_t*)wk, rstd, (const bf16_t*)stash, T, H, Hkv, pos, cosT, sinT, dwq, dwk, ws);
}
int tst_k_head_norm_fwd_f32(void* qkv, int64_t ld, const void* wq, const void* wk, float* rstd, void* stash, int T, int H, int Hkv, float eps, const int32_t* pos,
                            const float* cosT, const float* sinT) {
  return head_norm_fwd<float>(nullptr, (float*)qkv, (long)ld, (const float*)wq, (const float*)wk, rstd, (float*)stash, T, H, Hkv, eps, pos, cosT, sinT);
}
int tst_k_head_norm_bwd_f32(void* dqkv, int64_t ld, const void* wq, const void* wk, const float* rstd, const void* stash, int T, int H, int Hkv, const int32_t* pos,
                            const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws) {
  return head_norm_bwd<float>(nullptr, (float*)dqkv, (long)ld, (const float*)wq, (const float*)wk, rstd, (const float*)stash, T, H, Hkv, pos, cosT, sinT, dwq, dwk, ws);
}
int tst_k_kv_append(const void* qkv, int64_t ld, int k_off, const int32_t* rows, void* kcache, void* vcache, int T, int Hkv, int dh, int64_t cap_rows) {
  return kv_append<bf16_t>(nullptr, (const bf16_t*)qkv, (long)ld, k_off, rows, (bf16_t*)kcache, (bf16_t*)vcache, T, Hkv, dh, (long)cap_rows);
}
int tst_k_kv_append_f32(const void* qkv, int64_t ld, int k_off, const int32_t* rows, void* kcache, void* vcache, int T, int Hkv, int dh, int64_t cap_rows) {
  return kv_append<float>(nullptr, (const float*)qkv, (long)ld, k_off, rows, (float*)kcache, (float*)vcache, T, Hkv, dh, (long)cap_rows);
}
int tst_k_attn_decode(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* meta, int n_seqs, int step, void* out, int64_t ldo, int H,
                      int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_decode<bf16_t>(nullptr, (const bf16_t*)q, (long)ldq, (const bf16_t*)kcache, (const bf16_t*)vcache, meta, n_seqs, step, (bf16_t*)out, (long)ldo, H, Hkv,
                             dh, scale, (long)cap_rows);
}
int tst_k_attn_decode_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* meta, int n_seqs, int step, void* out, int64_t ldo,
                          int H, int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_decode<float>(nullptr, (const float*)q, (long)ldq, (const float*)kcache, (const float*)vcache, meta, n_seqs, step, (float*)out, (long)ldo, H, Hkv, dh,
                            scale, (long)cap_rows);
}
int tst_k_attn_decode_shared(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_rows, int step, void* out, int64_t ldo,
                             int H, int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_decode_shared<bf16_t>(nullptr, (const bf16_t*)q, (long)ldq, (const bf16_t*)kcache, (const bf16_t*)vcache, geo, n_rows, step, (bf16_t*)out, (long)ldo, H,
                                    Hkv, dh, scale, (long)cap_rows);
}
int tst_k_attn_decode_shared_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_rows, int step, void* out,
                                 int64_t ldo, int H, int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_decode_shared<float>(nullptr, (const float*)q, (long)ldq, (const float*)kcache, (const float*)vcache, geo, n_rows, step, (float*)out, (long)ldo, H, Hkv,
                                   dh, scale, (long)cap_rows);
}
int tst_k_sample_rows(const float* logits, int64_t ld, int V, const int32_t* geo, const int32_t* seeds, int n_rows, int j, float inv_temp, int32_t* tok, float* logp,
                      int32_t* d_ids, int32_t* d_pos, int32_t* lab_idx) {
  return sample_rows(nullptr, logits, (long)ld, V, geo, seeds, n_rows, j, inv_temp, tok, logp, d_ids, d_pos, lab_idx);
}
int tst_k_attn_extend(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_cands, int n_rows, void* out, int64_t ldo, int H,
                      int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_extend<bf16_t>(nullptr, (const bf16_t*)q, (long)ldq, (const bf16_t*)kcache, (const bf16_t*)vcache, geo, n_cands, n_rows, (bf16_t*)out, (long)ldo, H, Hkv,
                             dh, scale, (long)cap_rows);
}
int tst_k_attn_extend_f32(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* geo, int n_cands, int n_rows, void* out, int64_t ldo,
                          int H, int Hkv, int dh, float scale, int64_t cap_rows) {
  return attn_extend<float>(nullptr, (const float*)q, (long)ldq, (const float*)kcache, (const float*)vcache, geo, n_cands, n_rows, (float*)out, (long)ldo, H, Hkv, dh,
                            scale, (long)cap_rows);
}
int tst_k_cand_logp(const float* logits, int64_t ld, int V, const float* stats, int n_rows, const int32_t* src, int n, int phase, float* out) {
  return cand_logp(nullptr, logits, (long)ld, V, stats, n_rows, src, n, phase, out);
}
int tst_k_swiglu_fwd_f32(const void* gu, void* act, int T, int F) { return swiglu_fwd<float>(nullptr, (const float*)gu, (float*)act, T, F); }
int tst_k_swiglu_bwd_f32(const void* dact, const void* gu, void* dgu, int T, int F) {
  return swiglu_bwd<float>(nullptr, (const float*)dact, (const float*)gu, (float*)dgu, T, F);
}

}  // extern "C"
