// K10 (rank axis): C[M, N] (bf16) = alpha * A[M, K] . B[N, K]^T for the SKINNY side of the LoRA term -- u = x . Ag^T (N = padded group rank,
// K = d_in) in the forward and du = dy . Bg (K = d_out) in the backward: N = 64 .. 512, M = the step's tokens, K = 4096 .. 28672.
//
// Why its own kernel (variant 8): on the tiled families these launches are neither MFMA- nor HBM-bound but LATENCY-bound -- a 128x64 tile
// walks 64 .. 448 dependent k-steps, so the tile policy split K over workgroups into an fp32 slab and a second launch reduced it
// (profiles/r02_final_default_sweep_kernel_stats.csv: gemm_nt<128,64> 39.5 us + splitk_reduce 20 us per contraction under the two-stream
// bench, 11.8 % of all kernel time for < 2 % of the FLOPs). Here the K axis is split over the 8 WAVES of one workgroup instead:
//   * workgroup = BM (16 or 32) token rows x ALL needed columns; wave w owns the k-steps [w nk / 8, (w + 1) nk / 8);
//   * no LDS staging and no barrier in the main loop: every lane loads its MFMA fragments straight from global memory. The 64 elements of
//     a k-step of one row are one 128-byte line; lane (fr, fg) takes bytes [32 fg, 32 fg + 32) of row fr -- 4 lanes fetch a whole line --
//     and uses the first 16 bytes as the fragment of MFMA half 0 and the second 16 as half 1. A and B use the same (lane, half, element)
//     -> k map, so the contraction pairs up correctly although neither half is a contiguous 32-k window;
//   * register double buffering: the loads of k-step s + 1 are in flight during the MFMAs of step s;
//   * the 8 partial tiles meet in LDS once, are summed in wave order (fixed order: bit-reproducible), scaled, rounded to bf16, masked
//     and stored: one launch, no slab, no reduce kernel.
// Stacked folds: a token row keeps only its slot's rank block (GemmParams.mask_*), and the other blocks are exact zeros -- so a row tile
// that lies inside one slot computes that slot's columns only (B rows [slot w, (slot + 1) w)) and stores zeros elsewhere: 1 / n_stack of
// the MFMA work and of the B traffic. A tile that straddles a slot boundary computes the union of its slots' blocks.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int RK_NW = 8;          // waves per workgroup = K slices
constexpr int RK_PITCH = 68;      // floats per row of a partial tile in LDS (64 + 4: spreads the f32x4 stores over the banks)

// one 64-column chunk (NB blocks of 16 columns) of a row tile: this wave's k-steps [ks0, ks1) into acc
template <int MI, int NB>
__device__ __forceinline__ void rank_chunk(const char* const (&Ab)[MI], const char* const (&Bb)[4], int ks0, int ks1, f32x4 (&acc)[MI][4]) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  u32x4 ra0[MI][2], rb0[NB][2], ra1[MI][2], rb1[NB][2];
#define RK_ISSUE(RA, RB, KS)                                              \
  do {                                                                    \
    const long o_ = (long)(KS) << 7; /* 64 elements = 128 bytes per k-step */ \
    _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) {                   \
      RA[mi][0] = *(const u32x4*)(Ab[mi] + o_);                           \
      RA[mi][1] = *(const u32x4*)(Ab[mi] + o_ + 16);                      \
    }                                                                     \
    _Pragma("unroll") for (int ni = 0; ni < NB; ++ni) {                   \
      RB[ni][0] = *(const u32x4*)(Bb[ni] + o_);                           \
      RB[ni][1] = *(const u32x4*)(Bb[ni] + o_ + 16);                      \
    }                                                                     \
  } while (0)
#define RK_CONSUME(RA, RB)                                                \
  do {                                                                    \
    _Pragma("unroll") for (int h = 0; h < 2; ++h)                         \
      _Pragma("unroll") for (int ni = 0; ni < NB; ++ni) {                 \
        const bf16x8 bq_ = __builtin_bit_cast(bf16x8, RB[ni][h]);         \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                 \
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq_, __builtin_bit_cast(bf16x8, RA[mi][h]), acc[mi][ni], 0, 0, 0); \
      }                                                                   \
  } while (0)
  if (ks0 >= ks1) return;
  RK_ISSUE(ra0, rb0, ks0);
  int ks = ks0;
  for (; ks + 2 <= ks1 - 1; ks += 2) {   // two steps per trip: register double buffering, the loads of the next step fly during the MFMAs of this one
    RK_ISSUE(ra1, rb1, ks + 1);
    RK_CONSUME(ra0, rb0);
    RK_ISSUE(ra0, rb0, ks + 2);
    RK_CONSUME(ra1, rb1);
  }
  if (ks + 1 < ks1) {                    // two steps left
    RK_ISSUE(ra1, rb1, ks + 1);
    RK_CONSUME(ra0, rb0);
    RK_CONSUME(ra1, rb1);
  } else {                               // one step left
    RK_CONSUME(ra0, rb0);
  }
#undef RK_ISSUE
#undef RK_CONSUME
}

template <int MI>                 // BM = 16 * MI token rows per workgroup
__global__ __launch_bounds__(RK_NW * 64) void gemm_rank_kernel(GemmParams p) {
  constexpr int BM = 16 * MI;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // float [RK_NW][BM][RK_PITCH]
  float* red = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int m0 = blockIdx.x * BM;
  // column range this tile needs (multiples of 16)
  int c_lo = 0, c_hi = p.N;
  if (p.mask_width) {
    int s_lo = 0, s_hi = 0;
    const int m_last = min(m0 + BM, p.M) - 1;
#pragma unroll
    for (int q = 0; q < TST_MAX_STACK - 1; ++q) {
      s_lo += (q < p.mask_nslot - 1 && m0 >= p.mask_ends.t_end[q]) ? 1 : 0;
      s_hi += (q < p.mask_nslot - 1 && m_last >= p.mask_ends.t_end[q]) ? 1 : 0;
    }
    c_lo = (s_lo * p.mask_width) & ~15;
    c_hi = min(p.N, ((s_hi + 1) * p.mask_width + 15) & ~15);
  }
  const int nk = p.K >> 6;                                   // k-steps of 64
  const int ks0 = (int)(((long)w * nk) / RK_NW), ks1 = (int)(((long)(w + 1) * nk) / RK_NW);
  const char* Ab[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) Ab[mi] = (const char*)(p.A + (long)min(m0 + mi * 16 + fr, p.M - 1) * p.lda) + 32 * fg;
  const int orow = tid >> 4, ocol = (tid & 15) << 2;          // epilogue: thread -> (row, 4 columns) of a 64-column chunk; 512 threads cover 32 rows

  for (int c0 = c_lo; c0 < c_hi; c0 += 64) {
    const int nb = min(4, (c_hi - c0) >> 4);                  // 16-column blocks of this chunk (workgroup-uniform)
    const char* Bb[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) Bb[ni] = (const char*)(p.B + (long)min(c0 + ni * 16 + fr, p.N - 1) * p.ldb) + 32 * fg;
    f32x4 acc[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nb == 4) rank_chunk<MI, 4>(Ab, Bb, ks0, ks1, acc);
    else if (nb == 3) rank_chunk<MI, 3>(Ab, Bb, ks0, ks1, acc);
    else if (nb == 2) rank_chunk<MI, 2>(Ab, Bb, ks0, ks1, acc);
    else rank_chunk<MI, 1>(Ab, Bb, ks0, ks1, acc);
    // partial tiles -> LDS: lane holds C[row = mi*16 + fr][col = ni*16 + 4 fg + r]
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        *(f32x4*)(red + ((long)w * BM + mi * 16 + fr) * RK_PITCH + ni * 16 + 4 * fg) = acc[mi][ni];
    __syncthreads();
    if (orow < BM) {
      const int gm = m0 + orow;
      if (gm < p.M && c0 + ocol < c_hi) {
        f32x4 s = *(const f32x4*)(red + (long)orow * RK_PITCH + ocol);
#pragma unroll
        for (int ww = 1; ww < RK_NW; ++ww) s += *(const f32x4*)(red + ((long)ww * BM + orow) * RK_PITCH + ocol);
        s *= p.alpha;
        uint2 o;
        o.x = pack2bf(s[0], s[1]); o.y = pack2bf(s[2], s[3]);
        if (p.mask_width) {
          int slot = 0;
#pragma unroll
          for (int q = 0; q < TST_MAX_STACK - 1; ++q) slot += (q < p.mask_nslot - 1 && gm >= p.mask_ends.t_end[q]) ? 1 : 0;
          if ((c0 + ocol) / p.mask_width != slot) o.x = o.y = 0u;
        }
        *(uint2*)((bf16_t*)p.C + (long)gm * p.ldc + c0 + ocol) = o;
      }
    }
    __syncthreads();                                          // the next chunk's partial tiles reuse the buffer
  }
  // the columns outside [c_lo, c_hi) are other slots' blocks (or padding): exact zeros
  if (c_lo > 0 || c_hi < p.N) {
    const int n4 = p.N >> 2;
    for (int e = tid; e < BM * n4; e += RK_NW * 64) {
      const int row = e / n4, c = (e % n4) << 2;
      if (m0 + row < p.M && (c < c_lo || c >= c_hi)) *(uint2*)((bf16_t*)p.C + (long)(m0 + row) * p.ldc + c) = make_uint2(0u, 0u);
    }
  }
}

// ---- the LDS-staged form (the default): the direct-to-register loads above put 16 different rows into every quarter-wave of a load
// instruction (an MFMA operand lane IS a row), which the memory pipeline serves at a fraction of its rate: 0.8 - 1.4 TB/s measured
// (profiles/r03_rank_axis_kernel_microbench.txt: 248 us against 50 us for the tiled path on K = 28672). Here every wave still owns a K slice
// and runs WITHOUT barriers, but it streams its slice through a private three-stage LDS ring with buffer_load ... lds (8 lanes per
// 128-byte row segment: whole lines) and reads the MFMA fragments back with ds_read_b128 (XOR-swizzled 16-byte chunks, the image of
// gemm.hip). Ordering inside a wave is s_waitcnt vmcnt only: the DMA of step s + 2 is issued, then the wait leaves exactly the two younger
// stages in flight. 4 waves x 3 stages x (32 rows of A + up to 64 rows of B) x 128 B = 144 KB of LDS, one workgroup per CU.
constexpr int RL_NW = 4, RL_BM = 32, RL_STAGES = 3;
constexpr int RL_STAGE_BYTES = (RL_BM + 64) * 128;              // 12 KB: A tile then B tile
constexpr int RL_LDS = RL_NW * RL_STAGES * RL_STAGE_BYTES;      // 147456

template <int NB>   // 16-column blocks of the chunk: 1 .. 4
__device__ __forceinline__ void rank_chunk_lds(const GemmParams& p, char* ring, int m0, int c0, int ks0, int ks1, int lane, f32x4 (&acc)[2][4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int PA = RL_BM / 8, PB = NB * 2, P = PA + PB;       // DMA instructions per stage (1 KB = 8 rows each)
  const int fr = lane & 15, fg = lane >> 4;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, 0x7fffffff, 0x00020000);
  int voA[PA], voB[PB];                                          // loop-invariant byte offsets of this lane's 16-byte pieces at k = 0
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int row = j * 8 + (lane >> 3), lc = (lane & 7) ^ ((row >> 1) & 7);
    voA[j] = (int)(((long)min(m0 + row, p.M - 1) * p.lda + lc * 8) * 2);
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int row = j * 8 + (lane >> 3), lc = (lane & 7) ^ ((row >> 1) & 7);
    voB[j] = (int)(((long)min(c0 + row, p.N - 1) * p.ldb + lc * 8) * 2);
  }
  auto issue = [&](int ks) {
    char* st = ring + (ks % RL_STAGES) * RL_STAGE_BYTES;
    const int so = ks << 7;                                      // 64 elements = 128 bytes per k-step
#pragma unroll
    for (int j = 0; j < PA; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(st + j * 1024), 16, voA[j], so, 0, 0);
#pragma unroll
    for (int j = 0; j < PB; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(st + RL_BM * 128 + j * 1024), 16, voB[j], so, 0, 0);
  };
  const int n = ks1 - ks0;
  if (n <= 0) return;
  issue(ks0);
  if (n > 1) issue(ks0 + 1);
  for (int i = 0; i < n; ++i) {
    if (i + 2 < n) {
      issue(ks0 + i + 2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P) : "memory");   // two younger stages may still fly: stage i has landed
    } else if (i + 1 < n) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const char* sA = ring + ((ks0 + i) % RL_STAGES) * RL_STAGE_BYTES;
    const char* sB = sA + RL_BM * 128;
    bf16x8 af[2][2], bq[NB][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int row = mi * 16 + fr, sw = (row >> 1) & 7;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) af[mi][kk] = *(const bf16x8*)(sA + row * 128 + (((kk * 4 + fg) ^ sw) << 4));
    }
#pragma unroll
    for (int ni = 0; ni < NB; ++ni) {
      const int row = ni * 16 + fr, sw = (row >> 1) & 7;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) bq[ni][kk] = *(const bf16x8*)(sB + row * 128 + (((kk * 4 + fg) ^ sw) << 4));
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int ni = 0; ni < NB; ++ni)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[ni][kk], af[mi][kk], acc[mi][ni], 0, 0, 0);
  }
#endif
}

__global__ __launch_bounds__(RL_NW * 64) void gemm_rank_lds_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * RL_BM;
  int c_lo = 0, c_hi = p.N;
  if (p.mask_width) {
    int s_lo = 0, s_hi = 0;
    const int m_last = min(m0 + RL_BM, p.M) - 1;
#pragma unroll
    for (int q = 0; q < TST_MAX_STACK - 1; ++q) {
      s_lo += (q < p.mask_nslot - 1 && m0 >= p.mask_ends.t_end[q]) ? 1 : 0;
      s_hi += (q < p.mask_nslot - 1 && m_last >= p.mask_ends.t_end[q]) ? 1 : 0;
    }
    c_lo = (s_lo * p.mask_width) & ~15;
    c_hi = min(p.N, ((s_hi + 1) * p.mask_width + 15) & ~15);
  }
  const int nk = p.K >> 6;
  const int ks0 = (int)(((long)w * nk) / RL_NW), ks1 = (int)(((long)(w + 1) * nk) / RL_NW);
  char* ring = smem + w * (RL_STAGES * RL_STAGE_BYTES);
  float* red = (float*)smem;                                    // [RL_NW][RL_BM][RK_PITCH] partial tiles, after the main loop (34 KB of the ring)
  const int orow = tid >> 4, ocol = (tid & 15) << 2;            // 256 threads: 16 rows x 64 columns per pass, two passes
  for (int c0 = c_lo; c0 < c_hi; c0 += 64) {
    const int nb = min(4, (c_hi - c0) >> 4);
    f32x4 acc[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nb == 4) rank_chunk_lds<4>(p, ring, m0, c0, ks0, ks1, lane, acc);
    else if (nb == 3) rank_chunk_lds<3>(p, ring, m0, c0, ks0, ks1, lane, acc);
    else if (nb == 2) rank_chunk_lds<2>(p, ring, m0, c0, ks0, ks1, lane, acc);
    else rank_chunk_lds<1>(p, ring, m0, c0, ks0, ks1, lane, acc);
    __syncthreads();                                            // every wave is done with its ring: the partial tiles take its place
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        *(f32x4*)(red + ((long)w * RL_BM + mi * 16 + fr) * RK_PITCH + ni * 16 + 4 * fg) = acc[mi][ni];
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int row = ps * 16 + orow, gm = m0 + row;
      if (gm < p.M && c0 + ocol < c_hi) {
        f32x4 s = *(const f32x4*)(red + (long)row * RK_PITCH + ocol);
#pragma unroll
        for (int ww = 1; ww < RL_NW; ++ww) s += *(const f32x4*)(red + ((long)ww * RL_BM + row) * RK_PITCH + ocol);
        s *= p.alpha;
        uint2 o;
        o.x = pack2bf(s[0], s[1]); o.y = pack2bf(s[2], s[3]);
        if (p.mask_width) {
          int slot = 0;
#pragma unroll
          for (int q = 0; q < TST_MAX_STACK - 1; ++q) slot += (q < p.mask_nslot - 1 && gm >= p.mask_ends.t_end[q]) ? 1 : 0;
          if ((c0 + ocol) / p.mask_width != slot) o.x = o.y = 0u;
        }
        *(uint2*)((bf16_t*)p.C + (long)gm * p.ldc + c0 + ocol) = o;
      }
    }
    __syncthreads();                                            // the next chunk's DMA overwrites the partial tiles
  }
  if (c_lo > 0 || c_hi < p.N) {
    const int n4 = p.N >> 2;
    for (int e = tid; e < RL_BM * n4; e += RL_NW * 64) {
      const int row = e / n4, c = (e % n4) << 2;
      if (m0 + row < p.M && (c < c_lo || c >= c_hi)) *(uint2*)((bf16_t*)p.C + (long)(m0 + row) * p.ldc + c) = make_uint2(0u, 0u);
    }
  }
}

}  // namespace

bool gemm_rank_supported(const GemmParams& p) {
  return p.M > 0 && p.N >= 16 && p.N <= 512 && (p.N & 15) == 0 && p.K >= 64 && (p.K & 63) == 0 && p.K2 == 0 && !p.out_f32 && !p.R && !p.bias &&
         (p.lda & 7) == 0 && (p.ldb & 7) == 0 && (p.ldc & 3) == 0 && (!p.mask_width || ((p.mask_width & 3) == 0 && p.mask_nslot >= 1 && p.mask_nslot <= TST_MAX_STACK));
}

// rows per workgroup: 16 gives 2x the workgroups (M = 3555: 223 for 256 CUs) at 2x the B re-reads from L2; TST_RANK_BM overrides (A/B switch)
int gemm_rank(hipStream_t st, GemmParams p, int form) {
  if (!gemm_rank_supported(p)) return TST_EINVAL;
  // form 0: the LDS-staged kernel (needs 31-bit byte offsets from the operand bases: buffer addressing) unless TST_RANK_DIRECT=1; 1: the
  // register-loading kernel (variant 9: tests and A/B)
  static const bool direct_env = [] { const char* e = getenv("TST_RANK_DIRECT"); return e && atoi(e) != 0; }();
  const bool direct = direct_env || form == 1;
  const long lim = 0x7fffffffL;
  if (!direct && ((long)p.M * p.lda + p.K) * 2 < lim && ((long)p.N * p.ldb + p.K) * 2 < lim) {
    static TstLdsAttr attr;
    if (tst_set_max_lds(attr, (const void*)gemm_rank_lds_kernel, RL_LDS) != TST_OK) return TST_EHIP;
    hipLaunchKernelGGL(gemm_rank_lds_kernel, dim3(tst_ceil_div(p.M, RL_BM)), dim3(RL_NW * 64), RL_LDS, st, p);
    return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
  }
  static const int bm_env = [] { const char* e = getenv("TST_RANK_BM"); return e ? atoi(e) : 0; }();
  const int bm = (bm_env == 16 || bm_env == 32) ? bm_env : (p.M > 8192 ? 32 : 16);
  if (bm == 32) {
    static TstLdsAttr attr;   // 8 x 32 x 68 floats = 68 KB of partial tiles
    if (tst_set_max_lds(attr, (const void*)gemm_rank_kernel<2>, RK_NW * 32 * RK_PITCH * (int)sizeof(float)) != TST_OK) return TST_EHIP;
    hipLaunchKernelGGL(gemm_rank_kernel<2>, dim3(tst_ceil_div(p.M, 32)), dim3(RK_NW * 64), RK_NW * 32 * RK_PITCH * sizeof(float), st, p);
  } else {
    hipLaunchKernelGGL(gemm_rank_kernel<1>, dim3(tst_ceil_div(p.M, 16)), dim3(RK_NW * 64), RK_NW * 16 * RK_PITCH * sizeof(float), st, p);
  }
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
