// K2 + K10 in one pass: RMSNorm forward (modeling_llama.py:62-67: fp32 mean square, rsqrt, cast, x weight) fused with the rank-axis contraction that reads
// its result -- the LoRA A side of the projections that consume the normed stream:
//
//   y[T, d]  = w . bf16( x . rsqrt(mean(x^2) + eps) )          and   us[T, N] = alpha . y . Ag^T      (Ag [N][d]: q|k|v group behind the attention norm,
//                                                                                                     gate|up group behind the MLP norm)
//
// Why (the pattern of swiglu_rank.hip): gemm_rank_lds read the 29 MB the norm had just written, for < 0.1 % of the step's FLOPs, as a launch of its own that
// waits for free CUs between two projection tiles (8 us alone, 41 us under the two-stream bench). Here the normed row is consumed where it is produced.
//   * workgroup = up to 16 token rows of ONE slot (tiles are cut at the slot boundaries of stacked folds) x the slot's rank block (<= 64 columns); the 4 waves
//     split the d columns. A wave keeps its 16 rows x d / 4 columns in registers (128 VGPRs at d = 4096): every load of the tile is in flight at once,
//     the row statistic needs no second read;
//   * row statistic: lane sum over its k-steps and elements in order, xor-1/2/4 butterfly over the 8 lanes of a row segment, the 4 waves' partials added in
//     wave order through LDS. The SAME code computes it when no rank block is attached (N = 0): rmsnorm_fwd routes here for these widths, so y and rstd of
//     the fused and the unfused form are bit-identical by construction;
//   * second pass, k-step by k-step: y = w . bf16(x . rstd) is rounded, stored, dropped into the wave's private swizzled LDS image and read back as the MFMA
//     operand against the matching k-step of Ag (staged the same way, D steps of loads in flight, L2-resident); no barrier in the loop;
//   * the 4 partial tiles meet in LDS once, are summed in wave order (bit-reproducible), scaled, rounded and stored; the other slots' rank blocks of the
//     tile's rows are exact zeros.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int NR_BM = 16;         // token rows per workgroup
constexpr int NR_PITCH = 68;      // floats per row of a partial tile in LDS
constexpr int NR_NW = 4;          // waves = K slices

struct NrParams {
  const bf16_t* x; const bf16_t* w; bf16_t* y; float* rstd;
  const bf16_t* B; long ldb;      // Ag [N][d] (null: no rank part)
  bf16_t* C;                      // us [T][N]
  int M, N, d;
  float eps, alpha;
  int width, nslot;               // stacked folds: rank columns per slot (0: one slot, all N columns)
  int bm;                         // token rows per workgroup (<= 16)
  SlotEnds ends;
  int tile0[TST_MAX_STACK + 1];   // first workgroup of each slot; tile0[nslot] = grid size
};

__device__ __forceinline__ void nr_unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(v[e] << 16); f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
}
__device__ __forceinline__ u32x4 nr_pack8(const float* f) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack2bf(f[2 * e], f[2 * e + 1]);
  return o;
}

// KS: k-steps (64 columns) per wave = d / 256; NB: 16-column blocks of the slot's rank block (0: plain RMSNorm); D: k-steps of B loads in flight;
// RP: 8-row pieces of the tile a lane holds -- 2: 16 token rows per workgroup; 1: 8 rows (rows 8-15 of the MFMA tile are never written, read or stored): half the
// registers, twice the workgroups, several of them resident per CU, so that one workgroup's loads overlap another one's stores (a single generation of 16-row
// workgroups first reads everything, then writes everything: 18.7 us for 58 MB against 16.5 us of the wave-per-row kernel)
template <int KS, int NB, int D, int RP>
__global__ __launch_bounds__(NR_NW * 64) void rmsnorm_rank_kernel(NrParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int slot = 0;
#pragma unroll
  for (int q = 1; q < TST_MAX_STACK; ++q) slot += (q < p.nslot && (int)blockIdx.x >= p.tile0[q]) ? 1 : 0;
  const int r_lo = slot ? p.ends.t_end[slot - 1] : 0;
  const int m0 = r_lo + ((int)blockIdx.x - p.tile0[slot]) * p.bm;
  const int r_hi = min(slot < p.nslot - 1 ? p.ends.t_end[slot] : p.M, m0 + p.bm);   // end of this tile's rows (rows of the 16-row tile beyond it redo the last one)
  const int c_lo = p.width ? slot * p.width : 0;
  const int ncol = p.width ? p.width : p.N;
  const long d = p.d;
  const int kbase = w * KS * 64;                                  // this wave's first column

  // this lane's two 16-byte pieces of a 16-row x 64-column k-step: piece j = (row 8 j + lane / 8, chunk lane % 8) -- 8 lanes fetch one 128-byte row segment
  const int ch = lane & 7;
  const bf16_t* xsrc[RP];
  bf16_t* ydst[RP];
  int aoff[RP];
  bool live[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) {
    const int row = 8 * j + (lane >> 3);
    const long gr = min(m0 + row, r_hi - 1);                       // rows beyond the tile's end redo its last row: same loads, same values stored to the same place
    live[j] = m0 + row < r_hi;
    xsrc[j] = p.x + gr * d + kbase + ch * 8;
    ydst[j] = p.y + gr * d + kbase + ch * 8;
    aoff[j] = row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
  }
  // ---- pass 1: the whole tile into registers, every load in flight at once; row statistic
  u32x4 X[KS][RP];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < RP; ++j) X[ks][j] = *(const u32x4*)(xsrc[j] + ks * 64);
  float ss[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) ss[j] = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      float f[8];
      nr_unpack8(X[ks][j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss[j] += f[e] * f[e];
    }
#pragma unroll
  for (int j = 0; j < RP; ++j) {
    ss[j] += __shfl_xor(ss[j], 1, 64);
    ss[j] += __shfl_xor(ss[j], 2, 64);
    ss[j] += __shfl_xor(ss[j], 4, 64);
  }
  float* ssq = (float*)smem;                                      // [NR_NW][16]
  if (ch == 0) {
#pragma unroll
    for (int j = 0; j < RP; ++j) ssq[w * 16 + 8 * j + (lane >> 3)] = ss[j];
  }
  __syncthreads();
  float rstd[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) {
    const int row = 8 * j + (lane >> 3);
    const float tot = ((ssq[row] + ssq[16 + row]) + ssq[32 + row]) + ssq[48 + row];
    rstd[j] = 1.0f / sqrtf(tot / (float)p.d + p.eps);
    if (w == 0 && ch == 0 && live[j] && p.rstd) p.rstd[m0 + row] = rstd[j];
  }
  __syncthreads();                                                // (the images below reuse the LDS of the partial sums)

  // ---- pass 2: y = w . bf16(x . rstd), stored and -- with a rank block attached -- contracted against Ag k-step by k-step
  char* wl = smem + w * ((1 + (NB ? NB : 0)) * 2048);             // this wave's images: A 16 rows x 128 B, B NB x 16 rows x 128 B
  char* sA = wl;
  char* sB = wl + 2048;
  f32x4 acc[NB ? NB : 1];
#pragma unroll
  for (int ni = 0; ni < (NB ? NB : 1); ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* bsrc[NB ? NB * 2 : 1];
  int boff[NB ? NB * 2 : 1];
  if constexpr (NB > 0) {
#pragma unroll
    for (int j = 0; j < NB * 2; ++j) {
      const int row = 8 * j + (lane >> 3);
      bsrc[j] = p.B + (long)(c_lo + row) * p.ldb + kbase + ch * 8;
      boff[j] = row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
    }
  }
  struct Stage { u32x4 wv; u32x4 b[NB ? NB * 2 : 1]; };
  Stage S[D];
  auto issue = [&](Stage& s, int ks) {
    s.wv = *(const u32x4*)(p.w + kbase + ks * 64 + ch * 8);
    if constexpr (NB > 0) {
#pragma unroll
      for (int j = 0; j < NB * 2; ++j) s.b[j] = *(const u32x4*)(bsrc[j] + ks * 64);
    }
  };
  auto consume = [&](Stage& s, const u32x4 (&xk)[RP], int ks) {
    float wf[8];
    nr_unpack8(s.wv, wf);
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      float f[8];
      nr_unpack8(xk[j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = wf[e] * rnd_as<bf16_t>(f[e] * rstd[j]);
      const u32x4 o = nr_pack8(f);
      *(u32x4*)(ydst[j] + ks * 64) = o;
      if constexpr (NB > 0) *(u32x4*)(sA + aoff[j]) = o;
    }
    if constexpr (NB > 0) {
#pragma unroll
      for (int j = 0; j < NB * 2; ++j) *(u32x4*)(sB + boff[j]) = s.b[j];
      __builtin_amdgcn_wave_barrier();                            // (the wave reads what its own lanes wrote: LDS serves a wave's accesses in order)
      bf16x8 af[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) af[kk] = *(const bf16x8*)(sA + fr * 128 + (((kk * 4 + fg) ^ ((fr >> 1) & 7)) << 4));
#pragma unroll
      for (int ni = 0; ni < NB; ++ni) {
        const int row = ni * 16 + fr;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const bf16x8 bq = *(const bf16x8*)(sB + row * 128 + (((kk * 4 + fg) ^ ((row >> 1) & 7)) << 4));
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, af[kk], acc[ni], 0, 0, 0);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  };
  // straight-line code (KS and D are compile-time): no branch around a memory instruction, the compiler's s_waitcnt counts stay exact
#pragma unroll
  for (int dd = 0; dd < D; ++dd) issue(S[dd], dd < KS ? dd : KS - 1);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    consume(S[ks % D], X[ks], ks);
    if (ks + D < KS) issue(S[ks % D], ks + D);
  }
  if constexpr (NB > 0) {
    // partial tiles -> LDS (over the images): lane holds C[row fr][col ni * 16 + 4 fg + r]
    float* red = (float*)smem;                                    // [NR_NW][16][NR_PITCH]
    __syncthreads();
#pragma unroll
    for (int ni = 0; ni < NB; ++ni) *(f32x4*)(red + ((long)w * NR_BM + fr) * NR_PITCH + ni * 16 + 4 * fg) = acc[ni];
    __syncthreads();
    const int orow = tid >> 4, ocol = (tid & 15) << 2;            // 256 threads: 16 rows x 64 columns
    const int gm = m0 + orow;
    if (orow < 8 * RP && gm < r_hi && ocol < ncol) {
      f32x4 s = *(const f32x4*)(red + (long)orow * NR_PITCH + ocol);
#pragma unroll
      for (int ww = 1; ww < NR_NW; ++ww) s += *(const f32x4*)(red + ((long)ww * NR_BM + orow) * NR_PITCH + ocol);
      s *= p.alpha;
      uint2 o;
      o.x = pack2bf(s[0], s[1]); o.y = pack2bf(s[2], s[3]);
      *(uint2*)(p.C + (long)gm * p.N + c_lo + ocol) = o;
    }
    // the other slots' rank blocks (and padding columns) of these rows: exact zeros
    if (ncol < p.N) {
      const int n4 = p.N >> 2;
      for (int e = tid; e < 8 * RP * n4; e += NR_NW * 64) {
        const int row = e / n4, c = (e % n4) << 2;
        if (m0 + row < r_hi && (c < c_lo || c >= c_lo + ncol)) *(uint2*)(p.C + (long)(m0 + row) * p.N + c) = make_uint2(0u, 0u);
      }
    }
  }
}

// RP from nb as rmsnorm_rank_fwd sets p.bm: 16-row blocks (RP = 2) for nb >= 3, 8-row blocks (RP = 1) below
template <int KS>
int nr_launch_ks(hipStream_t st, const NrParams& p, int tiles, int nb) {
  const size_t images = (size_t)NR_NW * (1 + nb) * 2048, partial = (size_t)NR_NW * NR_BM * NR_PITCH * sizeof(float);
  const size_t lds = nb ? (images > partial ? images : partial) : 256;
  switch (nb) {
    case 0: hipLaunchKernelGGL((rmsnorm_rank_kernel<KS, 0, 2, 1>), dim3(tiles), dim3(NR_NW * 64), lds, st, p); break;
    case 1: hipLaunchKernelGGL((rmsnorm_rank_kernel<KS, 1, 4, 1>), dim3(tiles), dim3(NR_NW * 64), lds, st, p); break;
    case 2: hipLaunchKernelGGL((rmsnorm_rank_kernel<KS, 2, 4, 1>), dim3(tiles), dim3(NR_NW * 64), lds, st, p); break;
    case 3: hipLaunchKernelGGL((rmsnorm_rank_kernel<KS, 3, 3, 2>), dim3(tiles), dim3(NR_NW * 64), lds, st, p); break;
    case 4: hipLaunchKernelGGL((rmsnorm_rank_kernel<KS, 4, 2, 2>), dim3(tiles), dim3(NR_NW * 64), lds, st, p); break;
    default: return TST_EINVAL;
  }
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

// ---- RMSNorm backward with the norm-weight gradient in the same pass (full fine-tune): dx = dres + rstd (g - xhat mean(g xhat)), g = dy w, xhat = x rstd, AND
// the slice sums part[workgroup][c] = sum over the workgroup's 8 rows of dy[t, c] bf16(x[t, c] rstd[t]) (colred_finish2_kernel adds the slices in slice order: no
// atomics, bit-reproducible). Same tile as the forward: 8 rows per workgroup, the 4 waves split the columns, x and dy of the tile in registers (every load in flight
// at once), the residual gradient streamed in the second pass. It replaces rmsnorm_dw_kernel + colred_finish + rmsnorm_bwd_kernel: the two reduction launches sat
// on the backward's critical chain (the dX stream), stretched ~3x by the weight-gradient tiles beside them, and re-read dy and x.
struct NbParams {
  const bf16_t* dy; const bf16_t* x; const float* rstd; const bf16_t* w; const bf16_t* dres; bf16_t* dx;
  float* part;                    // [ceil(T / 8)][d] slice sums (null: no weight gradient)
  int T, d;
};

template <int KS, bool DW, int D>
__global__ __launch_bounds__(NR_NW * 64) void rmsnorm_bwd_tile_kernel(NbParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = lane & 7, row = lane >> 3;
  const int m0 = (int)blockIdx.x * 8;
  const long d = p.d;
  const int kbase = w * KS * 64;
  const long gr = min(m0 + row, p.T - 1);                          // rows beyond the batch redo its last row (their stores hit the same bytes with the same values)
  const bool live = m0 + row < p.T;
  const bf16_t* xsrc = p.x + gr * d + kbase + ch * 8;
  const bf16_t* dsrc = p.dy + gr * d + kbase + ch * 8;
  const bf16_t* rsrc = p.dres ? p.dres + gr * d + kbase + ch * 8 : xsrc;   // no residual gradient: the (cached) x piece is read instead and not used
  const bf16_t* wsrc = p.w + kbase + ch * 8;
  bf16_t* dst = p.dx + gr * d + kbase + ch * 8;
  u32x4 X[KS], DY[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) { X[ks] = *(const u32x4*)(xsrc + ks * 64); DY[ks] = *(const u32x4*)(dsrc + ks * 64); }
  const float rstd = p.rstd[gr];
  // ---- pass 1: dot = sum_c (dy w)(x rstd)
  float dot = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float fx[8], fd[8], fw[8];
    nr_unpack8(X[ks], fx);
    nr_unpack8(DY[ks], fd);
    nr_unpack8(*(const u32x4*)(wsrc + ks * 64), fw);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot += (fd[e] * fw[e]) * (fx[e] * rstd);
  }
  dot += __shfl_xor(dot, 1, 64);
  dot += __shfl_xor(dot, 2, 64);
  dot += __shfl_xor(dot, 4, 64);
  float* dsum = (float*)smem;                                      // [NR_NW][8]
  if (ch == 0) dsum[w * 8 + row] = dot;
  __syncthreads();
  dot = (((dsum[row] + dsum[8 + row]) + dsum[16 + row]) + dsum[24 + row]) / (float)p.d;
  // ---- pass 2: dx, and the slice sums of the weight gradient
  struct Stage { u32x4 r, wv; };
  Stage S[D];
#pragma unroll
  for (int dd = 0; dd < D; ++dd) {
    const int ks = dd < KS ? dd : KS - 1;
    S[dd].r = *(const u32x4*)(rsrc + ks * 64);
    S[dd].wv = *(const u32x4*)(wsrc + ks * 64);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float fx[8], fd[8], fw[8], fr[8], o[8];
    nr_unpack8(X[ks], fx);
    nr_unpack8(DY[ks], fd);
    nr_unpack8(S[ks % D].wv, fw);
    nr_unpack8(S[ks % D].r, fr);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = rstd * (fd[e] * fw[e] - (fx[e] * rstd) * dot);
      if (p.dres) v += fr[e];
      o[e] = v;
    }
    *(u32x4*)(dst + ks * 64) = nr_pack8(o);
    if constexpr (DW) {
      float pw[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = live ? fd[e] * rnd_as<bf16_t>(fx[e] * rstd) : 0.f;
        v += __shfl_xor(v, 8, 64);                                 // over the tile's 8 rows: lanes that differ in bits 3..5 hold the same columns of different rows
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        pw[e] = v;
      }
      if (row == 0) {
        float* dp = p.part + (long)blockIdx.x * d + kbase + ks * 64 + ch * 8;
        *(f32x4*)dp = f32x4{pw[0], pw[1], pw[2], pw[3]};
        *(f32x4*)(dp + 4) = f32x4{pw[4], pw[5], pw[6], pw[7]};
      }
    }
    if (ks + D < KS) {
      S[ks % D].r = *(const u32x4*)(rsrc + (ks + D) * 64);
      S[ks % D].wv = *(const u32x4*)(wsrc + (ks + D) * 64);
    }
  }
}

// out[c] += sum over the slices, in slice order: 64 columns per workgroup, its 4 waves take the slices b = q, q + 4, ... and meet in LDS (fixed order: reproducible)
__global__ __launch_bounds__(256) void colred_finish2_kernel(const float* __restrict__ part, int nslices, int n, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  float s = 0.f;
  if (c < n)
    for (int b = q; b < nslices; b += 4) s += part[(long)b * n + c];
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q == 0 && c < n) out[c] += ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

template <int KS>
int nb_launch(hipStream_t st, const NbParams& p) {
  const int tiles = tst_ceil_div(p.T, 8);
  if (p.part) hipLaunchKernelGGL((rmsnorm_bwd_tile_kernel<KS, true, 4>), dim3(tiles), dim3(NR_NW * 64), 256, st, p);
  else hipLaunchKernelGGL((rmsnorm_bwd_tile_kernel<KS, false, 4>), dim3(tiles), dim3(NR_NW * 64), 256, st, p);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

}  // namespace

// dx (as rmsnorm_bwd) and, with dw != null, dw[c] += sum_t dy[t, c] bf16(x[t, c] rstd[t]) in one pass + one finish launch; ws: colred_ws_floats(T, d) floats
int rmsnorm_bwd_dw(hipStream_t st, const bf16_t* dy, const bf16_t* x, const float* rstd, const bf16_t* w, const bf16_t* dres, bf16_t* dx, float* dw, int T, int d, float* ws) {
  if (!rmsnorm_rank_width_ok(d) || (dw && !ws)) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  NbParams p;
  p.dy = dy; p.x = x; p.rstd = rstd; p.w = w; p.dres = dres; p.dx = dx; p.part = dw ? ws : nullptr; p.T = T; p.d = d;
  int rc;
  switch (d >> 8) {
    case 1: rc = nb_launch<1>(st, p); break;
    case 2: rc = nb_launch<2>(st, p); break;
    case 4: rc = nb_launch<4>(st, p); break;
    case 8: rc = nb_launch<8>(st, p); break;
    case 12: rc = nb_launch<12>(st, p); break;
    case 14: rc = nb_launch<14>(st, p); break;
    case 16: rc = nb_launch<16>(st, p); break;
    default: return TST_EINVAL;
  }
  if (rc != TST_OK || !dw) return rc;
  hipLaunchKernelGGL(colred_finish2_kernel, dim3(tst_ceil_div(d, 64)), dim3(256), 0, st, ws, tst_ceil_div(T, 8), d, dw);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

// widths the kernel is instantiated for: d = 256 KS with KS in {1, 2, 4, 8, 12, 14, 16} (256, 512: the test models; 1024, 2048, 3072, 3584 = Qwen2.5-7B, 4096 = Llama-3-8B)
bool rmsnorm_rank_width_ok(int d) { return d == 256 || d == 512 || d == 1024 || d == 2048 || d == 3072 || d == 3584 || d == 4096; }

bool rmsnorm_rank_supported(int T, int d, const NormRank* r) {
  if (T <= 0 || !rmsnorm_rank_width_ok(d)) return false;
  if (!r || !r->B) return true;   // plain RMSNorm
  if (!r->C || (r->ldb & 7) || r->N < 16 || (r->N & 15)) return false;
  if (r->mask_width) return (r->mask_width & 15) == 0 && r->mask_width <= 64 && r->mask_nslot >= 1 && r->mask_nslot <= TST_MAX_STACK && r->mask_nslot * r->mask_width <= r->N;
  return r->N <= 64;
}

int rmsnorm_rank_fwd(hipStream_t st, const bf16_t* x, const bf16_t* w, bf16_t* y, float* rstd, int T, int d, float eps, const NormRank* r) {
  if (!rmsnorm_rank_supported(T, d, r)) return TST_EINVAL;
  NrParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.w = w; p.y = y; p.rstd = rstd; p.M = T; p.d = d; p.eps = eps;
  const bool rank = r && r->B;
  if (rank) {
    p.B = r->B; p.ldb = r->ldb; p.C = r->C; p.N = r->N; p.alpha = r->alpha;
    p.width = r->mask_width; p.nslot = r->mask_width ? r->mask_nslot : 1; p.ends = r->mask_ends;
  } else {
    p.nslot = 1;
  }
  // rows per workgroup: 8 for the plain norm and rank blocks of <= 32 columns (alone on T = 3555 x 4096: 16.3 / 19.2 us against 18.6 / 19.7 with 16 rows), 16 for
  // wider blocks (nb >= 3 blocks of 16 columns), where the 8-row form re-reads twice the Ag bytes and sits at 256 registers (24.2 against 22.9 us)
  const int nb = rank ? (p.width ? p.width : p.N) >> 4 : 0;
  p.bm = nb >= 3 ? NR_BM : 8;
  int tiles = 0;
  for (int s = 0; s < p.nslot; ++s) {
    const int lo = s ? p.ends.t_end[s - 1] : 0, hi = s < p.nslot - 1 ? p.ends.t_end[s] : T;
    if (lo < 0 || hi < lo || hi > T) return TST_EINVAL;
    p.tile0[s] = tiles;
    tiles += tst_ceil_div(hi - lo, p.bm);
  }
  for (int s = p.nslot; s <= TST_MAX_STACK; ++s) p.tile0[s] = tiles;
  if (tiles == 0) return TST_OK;
  switch (d >> 8) {
    case 1: return nr_launch_ks<1>(st, p, tiles, nb);
    case 2: return nr_launch_ks<2>(st, p, tiles, nb);
    case 4: return nr_launch_ks<4>(st, p, tiles, nb);
    case 8: return nr_launch_ks<8>(st, p, tiles, nb);
    case 12: return nr_launch_ks<12>(st, p, tiles, nb);
    case 14: return nr_launch_ks<14>(st, p, tiles, nb);
    case 16: return nr_launch_ks<16>(st, p, tiles, nb);
  }
  return TST_EINVAL;
}
