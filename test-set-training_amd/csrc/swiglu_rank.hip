// K5 + K10 in one pass: SwiGLU (modeling_llama.py:175, activations.py silu) fused with the rank-axis contraction that consumes its result.
//
//   forward : act[T, F]   = silu(gate) * up            and  us[T, N] = alpha * act . Ag^T   (Ag  [N][F]:  the down projection's LoRA A side)
//   backward: dgu[T, 2F]  = d(gate | up) from d(act)   and  du[T, N] = alpha * dgu . BgT^T  (BgT [N][2F]: the gate|up projection's LoRA B side)
//
// Why: both contractions read a [T, F]-sized tensor that the elementwise kernel has just written -- 102 MB (forward, gemm_rank_lds: 24 us alone) and 204 MB
// (backward: K = 28672 took the tiled split-K path, 51 + 13 us alone) per layer and step for < 0.1 % of the FLOPs. Here the elementwise result is consumed
// where it is produced: a wave loads its (rows x 64 columns) pieces of gate, up (and d act) with whole 128-byte row segments per 8 lanes, computes the SwiGLU
// values in registers, stores them, drops the same 16-byte pieces into a private swizzled LDS image (the layout of gemm_rank.hip's LDS-staged form) and reads
// them back as MFMA fragments against the matching k-step of B, which it stages the same way (B is L2-resident). Arithmetic of act / dgu: swiglu_of /
// sigmoid_of (common.h), the same expressions as swiglu_fwd_kernel / swiglu_bwd_kernel (elementwise.hip), bit for bit; the contraction sums the same bf16
// products as gemm_rank / gemm_nt in another order (fp32).
//   * workgroup = up to 16 token rows of ONE slot (row tiles are cut at the slot boundaries of stacked folds: no tile straddles two rank blocks) x the slot's
//     rank block (<= 64 columns). Rows per workgroup are chosen so that the grid covers the CUs (sr_launch): M = 3555 -> 14 rows, 255 workgroups;
//   * the 4 waves split the K axis (the gate columns); each keeps 3 - 4 stages of loads in flight in registers; no barrier in the main loop (a wave reads
//     only LDS it wrote itself) and NO BRANCH around a memory instruction in the steady state -- behind a conditional load the compiler's s_waitcnt pass must
//     assume the load was not issued and waits vmcnt(0), which left one stage in flight (81 -> 71 us);
//   * backward: Bg of the gate|up group is block diagonal by module, so a gate step meets the gate module's rank rows only and an up step the up module's
//     (SwiRank.block_diag): half the B traffic, 124 -> 108 us;
//   * the 4 partial tiles meet in LDS once, are summed in wave order (bit-reproducible), scaled, rounded and stored; the other slots' rank blocks
//     of the tile's rows are exact zeros.
// Alone on the benchmark's micro-batch: forward 60 - 66 us (swiglu 51 + rank 24 before), backward 97 - 108 us (86 + 51 + 13 before): 85 - 88 % of the
// elementwise kernels' HBM rate; the stores, not the arithmetic, are the rest of the time (profiles/r04_swiglu_rank_ab.txt). +1.15 % on the two-stream bench.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int SR_BM = 16;         // token rows per workgroup
constexpr int SR_PITCH = 68;      // floats per row of a partial tile in LDS

struct SrParams {
  const bf16_t* gu;               // [T][2F]: gate | up
  const bf16_t* dact;             // backward: d act [T][F]
  bf16_t* out;                    // forward: act [T][F]; backward: dgu [T][2F]
  const bf16_t* B; long ldb;      // forward: Ag [N][F]; backward: BgT [N][2F]
  bf16_t* C;                      // [T][N]
  int M, N, F;
  float alpha;
  int width, nslot;               // stacked folds: rank columns per slot (0: one slot, all N columns)
  int bm;                         // token rows per workgroup (<= 16): chosen so that the grid covers the CUs (see sr_launch)
  int bd;                         // backward: B is block diagonal by module -- the first half of a rank block meets gate columns only, the second half up columns only
  SlotEnds ends;
  int tile0[TST_MAX_STACK + 1];   // first workgroup of each slot; tile0[nslot] = grid size
};

__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(v[e] << 16); f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack2bf(f[2 * e], f[2 * e + 1]);
  return o;
}

template <int MODE, int NB, bool BD>
struct SrRegs {
  u32x4 g[2], u[2], d[2];
  u32x4 b[BD ? NB * 2 : (MODE ? 2 : 1) * NB * 2];   // BD: NB / 2 blocks for the gate step + NB / 2 for the up step
};

// MODE 0: forward, 1: backward. NB: 16-column blocks of the slot's rank block. D: stages of loads in flight.
template <int MODE, int NB, int D, bool BD = false>
__device__ __forceinline__ void sr_body(const SrParams& p, char* wl, int m0, int r_hi, int c_lo, int ks0, int ks1, int lane, f32x4 (&acc)[NB]) {
  constexpr int KS = MODE ? 2 : 1;                                // k-steps of the contraction per stage: backward takes a gate step and its up partner
  const int fr = lane & 15, fg = lane >> 4;
  const long F = p.F;
  // this lane's two 16-byte pieces of a 16-row x 64-column tile: piece j = (row 8 j + lane / 8, chunk lane % 8) -- 8 lanes fetch one 128-byte row segment
  const bf16_t* gsrc[2];
  const bf16_t* dsrc[2];
  bf16_t* dst[2];
  int aoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 8 * j + (lane >> 3), ch = lane & 7;
    const long gr = min(m0 + row, r_hi - 1);                       // rows beyond the slot's end redo its last row: same loads, same values stored to the same place
    gsrc[j] = p.gu + gr * 2 * F + ch * 8;
    dsrc[j] = MODE ? p.dact + gr * F + ch * 8 : nullptr;
    dst[j] = p.out + gr * (MODE ? 2 * F : F) + ch * 8;
    aoff[j] = row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
  }
  const bf16_t* bsrc[NB * 2];
  int boff[NB * 2];
#pragma unroll
  for (int j = 0; j < NB * 2; ++j) {
    const int row = 8 * j + (lane >> 3), ch = lane & 7;
    bsrc[j] = p.B + (long)(c_lo + row) * p.ldb + ch * 8;
    boff[j] = row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
  }
  char* sA = wl;                                                  // KS images of 16 rows x 128 B
  char* sB = wl + KS * 2048;                                      // KS images of NB * 16 rows x 128 B
  constexpr int NH = NB / 2;                                      // BD: 16-column blocks per module
  SrRegs<MODE, NB, BD> R[D];
  auto issue = [&](SrRegs<MODE, NB, BD>& r, int ks) {
    const long kc = (long)ks << 6;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      r.g[j] = *(const u32x4*)(gsrc[j] + kc);
      r.u[j] = *(const u32x4*)(gsrc[j] + F + kc);
      if constexpr (MODE) r.d[j] = *(const u32x4*)(dsrc[j] + kc);
    }
#pragma unroll
    for (int j = 0; j < NB * 2; ++j) {
      if constexpr (BD) r.b[j] = *(const u32x4*)(bsrc[j] + (j < NH * 2 ? 0 : F) + kc);   // rows of the gate module: the gate step; of the up module: the up step
      else {
        r.b[j] = *(const u32x4*)(bsrc[j] + kc);
        if constexpr (MODE) r.b[NB * 2 + j] = *(const u32x4*)(bsrc[j] + F + kc);
      }
    }
  };
  auto consume = [&](SrRegs<MODE, NB, BD>& r, int ks) {
    const long kc = (long)ks << 6;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float g[8], u[8];
      unpack8(r.g[j], g);
      unpack8(r.u[j], u);
      if constexpr (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = swiglu_of<bf16_t>(g[e], u[e]);
#ifdef SWR_NO_MATH   // (probe builds only: tools/probes/swr_probe_build.sh)
        const u32x4 o = r.g[j] ^ r.u[j];
#else
        const u32x4 o = pack8(g);
#endif
#ifndef SWR_NO_STORE
        *(u32x4*)(dst[j] + kc) = o;
#endif
        *(u32x4*)(sA + aoff[j]) = o;
      } else {
        float da[8], dg[8], du[8];
        unpack8(r.d[j], da);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float sg = sigmoid_of<bf16_t>(g[e]);
          dg[e] = da[e] * u[e] * sg * (1.0f + g[e] * (1.0f - sg));
          du[e] = da[e] * g[e] * sg;
        }
#ifdef SWR_NO_MATH
        const u32x4 og = r.g[j] ^ r.d[j], ou = r.u[j] ^ r.d[j];
#else
        const u32x4 og = pack8(dg), ou = pack8(du);
#endif
#ifndef SWR_NO_STORE
        *(u32x4*)(dst[j] + kc) = og;
        *(u32x4*)(dst[j] + F + kc) = ou;
#endif
        *(u32x4*)(sA + aoff[j]) = og;
        *(u32x4*)(sA + 2048 + aoff[j]) = ou;
      }
    }
#pragma unroll
    for (int j = 0; j < NB * 2; ++j) {
      *(u32x4*)(sB + boff[j]) = r.b[j];
      if constexpr (MODE && !BD) *(u32x4*)(sB + NB * 2048 + boff[j]) = r.b[NB * 2 + j];
    }
    __builtin_amdgcn_wave_barrier();                              // (the wave reads what its own lanes wrote: LDS serves a wave's accesses in order)
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      bf16x8 af[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) af[kk] = *(const bf16x8*)(sA + t * 2048 + fr * 128 + (((kk * 4 + fg) ^ ((fr >> 1) & 7)) << 4));
#pragma unroll
      for (int ni = 0; ni < NB; ++ni) {
        if constexpr (BD) { if ((ni < NH) != (t == 0)) continue; }   // one image of B: its first NH blocks belong to the gate step, the others to the up step
        const int row = ni * 16 + fr;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const bf16x8 bq = *(const bf16x8*)(sB + (BD ? 0 : t * NB * 2048) + row * 128 + (((kk * 4 + fg) ^ ((row >> 1) & 7)) << 4));
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, af[kk], acc[ni], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  // No branch around a memory instruction in the steady state: the compiler's s_waitcnt counts are exact only on straight-line code (behind a conditional
  // load it must assume the load was NOT issued and waits for everything: vmcnt(0), one stage in flight). Steps beyond the slice re-load its last step.
  const int n = ks1 - ks0;                                         // >= 1
#pragma unroll
  for (int d = 0; d < D; ++d) issue(R[d], min(ks0 + d, ks1 - 1));
  int i = 0;
  for (; i + D <= n; i += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      consume(R[d], ks0 + i + d);
      issue(R[d], min(ks0 + i + d + D, ks1 - 1));
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (i + d < n) consume(R[d], ks0 + i + d);
}

template <int MODE, int SR_NW>   // SR_NW: waves per workgroup = K slices
__global__ __launch_bounds__(SR_NW * 64) void swiglu_rank_kernel(SrParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the slot of this row tile and its rows [m0, min(m0 + 16, r_hi))
  int slot = 0;
#pragma unroll
  for (int q = 1; q < TST_MAX_STACK; ++q) slot += (q < p.nslot && (int)blockIdx.x >= p.tile0[q]) ? 1 : 0;
  const int r_lo = slot ? p.ends.t_end[slot - 1] : 0;
  const int m0 = r_lo + ((int)blockIdx.x - p.tile0[slot]) * p.bm;
  const int r_hi = min(slot < p.nslot - 1 ? p.ends.t_end[slot] : p.M, m0 + p.bm);   // end of this tile's rows (rows of the 16-row MFMA tile beyond it redo the last one)
  const int c_lo = p.width ? slot * p.width : 0;
  const int ncol = p.width ? p.width : p.N;                       // a multiple of 16, at most 64
  const int nb = ncol >> 4;
  const int nk = p.F >> 6;                                        // gate k-steps of 64 columns
  const int ks0 = (int)(((long)w * nk) / SR_NW), ks1 = (int)(((long)(w + 1) * nk) / SR_NW);
  constexpr int D = MODE ? 3 : 4, DW = 2;                         // stages in flight: narrow blocks (NB <= 2: the product's shapes) / wide ones (registers)
  char* wl = smem + w * ((MODE ? 2 : 1) * (1 + nb) * 2048);       // this wave's images
  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nb == 1) {
    f32x4 a1[1] = {acc[0]};
    sr_body<MODE, 1, D>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, a1);
    acc[0] = a1[0];
  } else if (nb == 2) {
    f32x4 a2[2] = {acc[0], acc[1]};
    if (MODE == 1 && p.bd) sr_body<MODE, 2, D, MODE == 1>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, a2);
    else sr_body<MODE, 2, D>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, a2);
    acc[0] = a2[0]; acc[1] = a2[1];
  } else if (nb == 3) {
    f32x4 a3[3] = {acc[0], acc[1], acc[2]};
    sr_body<MODE, 3, DW>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, a3);
    acc[0] = a3[0]; acc[1] = a3[1]; acc[2] = a3[2];
  } else {
    if (MODE == 1 && p.bd) sr_body<MODE, 4, D, MODE == 1>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, acc);
    else sr_body<MODE, 4, DW>(p, wl, m0, r_hi, c_lo, ks0, ks1, lane, acc);
  }
  // partial tiles -> LDS (over the images): lane holds C[row fr][col ni * 16 + 4 fg + r]
  float* red = (float*)smem;                                      // [SR_NW][16][SR_PITCH]
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    if (ni < nb) *(f32x4*)(red + ((long)w * SR_BM + fr) * SR_PITCH + ni * 16 + 4 * fg) = acc[ni];
  __syncthreads();
  const int orow = tid >> 4, ocol = (tid & 15) << 2;              // the first 256 threads: 16 rows x 64 columns
  const int gm = m0 + orow;
  if (orow < SR_BM && gm < r_hi && ocol < ncol) {
    f32x4 s = *(const f32x4*)(red + (long)orow * SR_PITCH + ocol);
#pragma unroll
    for (int ww = 1; ww < SR_NW; ++ww) s += *(const f32x4*)(red + ((long)ww * SR_BM + orow) * SR_PITCH + ocol);
    s *= p.alpha;
    uint2 o;
    o.x = pack2bf(s[0], s[1]); o.y = pack2bf(s[2], s[3]);
    *(uint2*)(p.C + (long)gm * p.N + c_lo + ocol) = o;
  }
  // the other slots' rank blocks (and padding columns) of these rows: exact zeros
  if (ncol < p.N) {
    const int n4 = p.N >> 2;
    for (int e = tid; e < SR_BM * n4; e += SR_NW * 64) {
      const int row = e / n4, c = (e % n4) << 2;
      if (m0 + row < r_hi && (c < c_lo || c >= c_lo + ncol)) *(uint2*)(p.C + (long)(m0 + row) * p.N + c) = make_uint2(0u, 0u);
    }
  }
}

template <int NW>
int sr_launch_nw(hipStream_t st, int mode, const SrParams& p, int tiles, int nb) {
  const size_t images = (size_t)NW * (mode ? 2 : 1) * (1 + nb) * 2048, partial = (size_t)NW * SR_BM * SR_PITCH * sizeof(float);
  const size_t lds = images > partial ? images : partial;
  static TstLdsAttr attr;
  if (tst_set_max_lds(attr, {{(const void*)swiglu_rank_kernel<0, NW>, NW * 5 * 2048}, {(const void*)swiglu_rank_kernel<1, NW>, NW * 10 * 2048}}) != TST_OK) return TST_EHIP;
  if (mode == 0) hipLaunchKernelGGL((swiglu_rank_kernel<0, NW>), dim3(tiles), dim3(NW * 64), lds, st, p);
  else hipLaunchKernelGGL((swiglu_rank_kernel<1, NW>), dim3(tiles), dim3(NW * 64), lds, st, p);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

int sr_launch(hipStream_t st, int mode, const bf16_t* gu, const bf16_t* dact, bf16_t* out, int T, int F, const SwiRank& r) {
  if (!swiglu_rank_supported(T, F, r)) return TST_EINVAL;
  SrParams p;
  p.gu = gu; p.dact = dact; p.out = out; p.B = r.B; p.ldb = r.ldb; p.C = r.C;
  p.M = T; p.N = r.N; p.F = F; p.alpha = r.alpha;
  p.width = r.mask_width; p.nslot = r.mask_width ? r.mask_nslot : 1; p.ends = r.mask_ends;
  const int ncol = r.mask_width ? r.mask_width : r.N;
  p.bd = (mode == 1 && r.block_diag && (ncol & 31) == 0) ? 1 : 0;
  // Rows per workgroup: 16 (one MFMA tile) when that fills the GPU; fewer when 16-row tiles would leave CUs idle -- a CU streams ~30 GB/s through its vector
  // memory path whatever the kernel does, so 223 workgroups (T = 3555) cap the launch at 87 % of what 254 reach, and the extra B re-reads cost less than that
  static const int bm_env = [] { const char* e = getenv("TST_SWR_BM"); return e ? atoi(e) : 0; }();
  static const int ncu = [] {   // (asked once: the GPUs of a node are alike)
    int dev = 0;
    hipDeviceProp_t pr;
    return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
  }();
  p.bm = SR_BM;
  if (T < SR_BM * ncu) { p.bm = tst_ceil_div(T, ncu); if (p.bm < 8) p.bm = 8; }
  if (bm_env >= 1 && bm_env <= SR_BM) p.bm = bm_env;
  int tiles = 0;
  for (int s = 0; s <= TST_MAX_STACK; ++s) p.tile0[s] = 0;
  for (int s = 0; s < p.nslot; ++s) {
    const int lo = s ? p.ends.t_end[s - 1] : 0, hi = s < p.nslot - 1 ? p.ends.t_end[s] : T;
    if (lo < 0 || hi < lo || hi > T) return TST_EINVAL;
    p.tile0[s] = tiles;
    tiles += tst_ceil_div(hi - lo, p.bm);
  }
  for (int s = p.nslot; s <= TST_MAX_STACK; ++s) p.tile0[s] = tiles;
  if (tiles == 0) return TST_OK;
  const int nb = (p.width ? p.width : p.N) >> 4;
  return sr_launch_nw<4>(st, mode, p, tiles, nb);   // (8 waves per workgroup: forward the same, backward 144 vs 124 us)
}

}  // namespace

bool swiglu_rank_supported(int T, int F, const SwiRank& r) {
  if (T <= 0 || (F & 63) || (F >> 6) < 4 || !r.B || !r.C || (r.ldb & 7) || r.N < 16 || (r.N & 15)) return false;
  if (r.mask_width) return (r.mask_width & 15) == 0 && r.mask_width <= 64 && r.mask_nslot >= 1 && r.mask_nslot <= TST_MAX_STACK && r.mask_nslot * r.mask_width <= r.N;
  return r.N <= 64;
}

int swiglu_rank_fwd(hipStream_t st, const bf16_t* gu, bf16_t* act, int T, int F, const SwiRank& r) { return sr_launch(st, 0, gu, nullptr, act, T, F, r); }
int swiglu_rank_bwd(hipStream_t st, const bf16_t* dact, const bf16_t* gu, bf16_t* dgu, int T, int F, const SwiRank& r) { return sr_launch(st, 1, gu, dact, dgu, T, F, r); }
