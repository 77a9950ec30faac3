// K1: bf16 MFMA GEMM for gfx950 (hand-written, no BLAS).
//
//   C[M,N] = alpha * ( A[M,K] . B[N,K]^T  +  A2[M,K2] . B2[N,K2]^T )  (+ R[M,N])
//
// Both operands are K-contiguous ("NT"): this is the only dense contraction the hot path needs,
// because every frozen weight is kept in HBM in both orientations (W for the forward, W^T for dX)
// and the few K-strided operands (dY^T, X^T for adapter gradients) go through transpose_bf16.
// The optional second K segment (A2,B2) carries the LoRA low-rank term s*u*B^T inside the same
// fp32 accumulator, so adapters cost one extra 64-deep K step instead of a read-modify-write pass.
//
// Oracle lines this replaces: nn.Linear in modeling_llama.py:254-256, 280, 175, 480.
//
// Structure (cdna_hip_programming.md §5): BMxBNx64 tile, 256 threads = 4 waves, v_mfma_f32_16x16x32_bf16,
// operands staged HBM->LDS with global_load_lds_dwordx4 (LDS image linear, XOR swizzle applied to the
// SOURCE chunk and to the ds_read_b128 address), two LDS buffers, one barrier per K step.
// The MFMA is issued with operands swapped (D = Btile . Atile^T) so that every lane ends up with four
// consecutive N columns of one M row: the epilogue stages the tile through LDS and writes whole
// 128/256-byte rows.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "lds_image.h"

namespace {

// TN = true: C[M,N] = sum_t A[t,M] * B[t,N] -- both operands are [k rows][cols] in memory; their tiles are staged as
// 128-column panels in the row/transposed-read image of lds_image.h and consumed with ds_read_b64_tr_b16, so the
// adapter gradients (contraction over the token axis) need no transposed copies. Rows >= kvalid of the last k-step
// are masked in registers (operands must be readable, and finite, up to K = roundup64(kvalid) rows).
// BUF = true: tiles are staged with buffer_load ... lds: the per-thread part of each address is loop-invariant (one VGPR per
// 16-byte piece), the k position travels in the scalar offset -- no vector arithmetic per piece (gemm_pp.hip measured the
// flat-address form at ~9 VALU instructions per piece). BUF = false keeps 64-bit flat addresses for operands beyond 2 GiB.
template <int BM, int BN, int WARPS_M, int WARPS_N, bool TN, bool BUF>
__device__ __forceinline__ void gemm_nt_body(const GemmParams& p, const int bid, const int z, char* smem) {
#if defined(__HIP_DEVICE_COMPILE__)   // buffer-resource types exist only in the device pass
  constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
  constexpr int MI = WM / 16, NI = WN / 16;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  static_assert(WARPS_M * WARPS_N == 4, "4 waves");
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WARPS_N, wc = wave % WARPS_N;

  // XCD-aware, bijective block->tile map: blocks with equal (id % 8) share an XCD/L2 and get a
  // contiguous run of tiles; inside a run the M tile moves fastest so neighbours share the B panel.
  const int nwg = p.mtiles * p.ntiles;
  const int xcd = bid & 7, idx = bid >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  // skinny N (adapter rank axis: 1-4 column tiles): the big operand is A, so the column tiles of one row block are neighbours
  // in the run and the XCD's L2 serves A once; otherwise the M tile moves fastest and neighbours share the B panel
  const bool nfast = p.ntiles <= 4 && p.mtiles > p.ntiles;
  const int tm = nfast ? tile / p.ntiles : tile % p.mtiles, tn = nfast ? tile % p.ntiles : tile / p.mtiles;
  const int m0 = tm * BM, n0 = tn * BN;

  const int nt1 = p.K >> 6, nt2 = p.K2 >> 6, nt = nt1 + nt2;
  const int per = (nt + p.splitk - 1) / p.splitk;
  const int t_begin = z * per;
  const int t_end = min(nt, t_begin + per);

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- buffer addressing (BUF): resources + loop-invariant per-thread byte offsets
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.K2 ? p.A2 : p.A), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.K2 ? p.B2 : p.B), 0, 0x7fffffff, 0x00020000);
  auto nt_off = [&](int j, bool isA, long ld) {   // NT: row (clamped) x ld + swizzled chunk, at k = 0
    const int row = j * 32 + (tid >> 3), pc = tid & 7;
    const int lc = pc ^ ((row >> 1) & 7);
    const int gr = isA ? min(m0 + row, p.M - 1) : min(n0 + row, p.N - 1);
    return (int)(((long)gr * ld + lc * 8) * 2);
  };
  auto tn_off = [&](int j, bool isA, long ld) {   // TN: k-row within the tile x ld + swizzled column chunk, at k-tile 0
    const int q = j * 256 + tid;
    const int panel = q >> 10, row = (q >> 4) & 63, phys = q & 15;
    const int gc = isA ? min((m0 >> 3) + panel * 16 + (phys ^ swz(row)), (p.M >> 3) - 1) : min((n0 >> 3) + panel * 16 + (phys ^ swz(row)), (p.N >> 3) - 1);
    return (int)(((long)row * ld + gc * 8) * 2);
  };
  int voffA[BM / 32], voffB[BN / 32];
  if constexpr (BUF) {
#pragma unroll
    for (int j = 0; j < BM / 32; ++j) voffA[j] = TN ? tn_off(j, true, p.lda) : nt_off(j, true, p.lda);
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) voffB[j] = TN ? tn_off(j, false, p.ldb) : nt_off(j, false, p.ldb);
  }

  auto stage = [&](int buf, int t) {
    if constexpr (BUF) {
      char* sA = smem + buf * STAGE + wave_s * 1024;
      char* sB = sA + A_BYTES;
      if constexpr (TN) {
        const int soA = (int)((long)(t << 6) * p.lda * 2), soB = (int)((long)(t << 6) * p.ldb * 2);
#pragma unroll
        for (int j = 0; j < BM / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + j * 4096), 16, voffA[j], soA, 0, 0);
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + j * 4096), 16, voffB[j], soB, 0, 0);
      } else if (t < nt1) {
        const int so = t << 7;
#pragma unroll
        for (int j = 0; j < BM / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, LDS_PTR(sA + j * 4096), 16, voffA[j], so, 0, 0);
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, LDS_PTR(sB + j * 4096), 16, voffB[j], so, 0, 0);
      } else {   // second K segment (LoRA): one or two tiles, offsets computed on the spot
        const int so = (t - nt1) << 7;
#pragma unroll
        for (int j = 0; j < BM / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA2, LDS_PTR(sA + j * 4096), 16, nt_off(j, true, p.lda2), so, 0, 0);
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB2, LDS_PTR(sB + j * 4096), 16, nt_off(j, false, p.ldb2), so, 0, 0);
      }
      return;
    }
    const bf16_t* Ap;
    const bf16_t* Bp;
    long lda, ldb;
    int k0;
    if (t < nt1) {
      Ap = p.A; Bp = p.B; lda = p.lda; ldb = p.ldb; k0 = t << 6;
    } else {
      Ap = p.A2; Bp = p.B2; lda = p.lda2; ldb = p.ldb2; k0 = (t - nt1) << 6;
    }
    char* sA = smem + buf * STAGE;
    char* sB = sA + A_BYTES;
    if constexpr (TN) {
#pragma unroll
      for (int j = 0; j < BM / 32; ++j) {
        const int q = j * 256 + tid;
        const int panel = q >> 10, row = (q >> 4) & 63, phys = q & 15;
        const int gc = min((m0 >> 3) + panel * 16 + (phys ^ swz(row)), (p.M >> 3) - 1);
        __builtin_amdgcn_global_load_lds(GLB_PTR(p.A + (long)((t << 6) + row) * p.lda + gc * 8), LDS_PTR(sA + (j * 256 + wave * 64) * 16), 16, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < BN / 32; ++j) {
        const int q = j * 256 + tid;
        const int panel = q >> 10, row = (q >> 4) & 63, phys = q & 15;
        const int gc = min((n0 >> 3) + panel * 16 + (phys ^ swz(row)), (p.N >> 3) - 1);
        __builtin_amdgcn_global_load_lds(GLB_PTR(p.B + (long)((t << 6) + row) * p.ldb + gc * 8), LDS_PTR(sB + (j * 256 + wave * 64) * 16), 16, 0, 0);
      }
      return;
    }
    const int prow = tid >> 3, pc = tid & 7;
#pragma unroll
    for (int j = 0; j < BM / 32; ++j) {
      const int row = j * 32 + prow;
      const int lc = pc ^ ((row >> 1) & 7);
      const int gr = min(m0 + row, p.M - 1);
      const bf16_t* src = Ap + (long)gr * lda + k0 + lc * 8;
      char* dst = sA + (j * 256 + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(dst), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) {
      const int row = j * 32 + prow;
      const int lc = pc ^ ((row >> 1) & 7);
      const int gr = min(n0 + row, p.N - 1);
      const bf16_t* src = Bp + (long)gr * ldb + k0 + lc * 8;
      char* dst = sB + (j * 256 + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(dst), 16, 0, 0);
    }
  };

  if (t_begin < t_end) {
    stage(0, t_begin);
    __syncthreads();
    int cur = 0;
    const int fr = lane & 15, fg = lane >> 4;
    for (int t = t_begin; t < t_end; ++t) {
      if (t + 1 < t_end) stage(cur ^ 1, t + 1);
      const char* sA = smem + cur * STAGE;
      const char* sB = sA + A_BYTES;
      bf16x8 af[MI][2], bq[NI][2];
      if constexpr (TN) {
        const bool tail = ((t + 1) << 6) > p.kvalid;  // wave-uniform: k-step reaches past the real contraction rows
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int col = wr * WM + mi * 16;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            af[mi][kk] = tr_frag(sA + (col >> 7) * 16384, kk, col & 127, lane);
            if (tail) {
              const int tbase = (t << 6) + 32 * kk + 4 * fg;
#pragma unroll
              for (int e = 0; e < 8; ++e)
                af[mi][kk][e] = (tbase + 16 * (e >> 2) + (e & 3) >= p.kvalid) ? (__bf16)0.0f : af[mi][kk][e];
            }
          }
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          const int col = wc * WN + ni * 16;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) bq[ni][kk] = tr_frag(sB + (col >> 7) * 16384, kk, col & 127, lane);
        }
      } else {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int row = wr * WM + mi * 16 + fr;
        const int sw = (row >> 1) & 7;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          af[mi][kk] = *(const bf16x8*)(sA + row * 128 + (((kk * 4 + fg) ^ sw) << 4));
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = wc * WN + ni * 16 + fr;
        const int sw = (row >> 1) & 7;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          bq[ni][kk] = *(const bf16x8*)(sB + row * 128 + (((kk * 4 + fg) ^ sw) << 4));
      }
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[ni][kk], af[mi][kk], acc[mi][ni], 0, 0, 0);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue: fp32 tile -> LDS (XOR-swizzled 16-B chunks) -> whole-row global stores ----
  float* Cs = (float*)smem;
  {
    const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = wr * WM + mi * 16 + fr;
        const int ch = (wc * WN + ni * 16 + fg * 4) >> 2;
        f32x4 v = acc[mi][ni];
        v *= p.alpha;
        *(f32x4*)(Cs + row * BN + ((ch ^ (row & 7)) << 2)) = v;
      }
  }
  __syncthreads();

  if (p.splitk > 1 || p.out_f32) {
    float* dst;
    long ld;
    if (p.splitk > 1) { dst = p.slab + (long)z * p.M * p.N; ld = p.N; }
    else { dst = (float*)p.C; ld = p.ldc; }
    constexpr int TPR = BN / 4;           // threads per row
    constexpr int RPP = 256 / TPR;        // rows per pass
    const int c4 = tid % TPR, r0 = tid / TPR;
#pragma unroll 4
    for (int pass = 0; pass < BM / RPP; ++pass) {
      const int row = pass * RPP + r0;
      const int gm = m0 + row, gn = n0 + c4 * 4;
      if (gm < p.M && gn < p.N) {
        f32x4 v = *(const f32x4*)(Cs + row * BN + ((c4 ^ (row & 7)) << 2));
        *(f32x4*)(dst + (long)gm * ld + gn) = v;
      }
    }
  } else {
    bf16_t* dst = (bf16_t*)p.C;
    constexpr int TPR = BN / 8;
    constexpr int RPP = 256 / TPR;
    const int c8 = tid % TPR, r0 = tid / TPR;
#pragma unroll 4
    for (int pass = 0; pass < BM / RPP; ++pass) {
      const int row = pass * RPP + r0;
      const int gm = m0 + row, gn = n0 + c8 * 8;
      if (gm < p.M && gn < p.N) {
        f32x4 v0 = *(const f32x4*)(Cs + row * BN + (((2 * c8) ^ (row & 7)) << 2));
        f32x4 v1 = *(const f32x4*)(Cs + row * BN + (((2 * c8 + 1) ^ (row & 7)) << 2));
        if (p.R) {
          const uint4 rr = *(const uint4*)(p.R + (long)gm * p.ldr + gn);
          v0[0] += __uint_as_float(rr.x << 16); v0[1] += __uint_as_float(rr.x & 0xffff0000u);
          v0[2] += __uint_as_float(rr.y << 16); v0[3] += __uint_as_float(rr.y & 0xffff0000u);
          v1[0] += __uint_as_float(rr.z << 16); v1[1] += __uint_as_float(rr.z & 0xffff0000u);
          v1[2] += __uint_as_float(rr.w << 16); v1[3] += __uint_as_float(rr.w & 0xffff0000u);
        }
        if (p.bias) {
          const uint4 rr = *(const uint4*)(p.bias + gn);
          v0[0] += __uint_as_float(rr.x << 16); v0[1] += __uint_as_float(rr.x & 0xffff0000u);
          v0[2] += __uint_as_float(rr.y << 16); v0[3] += __uint_as_float(rr.y & 0xffff0000u);
          v1[0] += __uint_as_float(rr.z << 16); v1[1] += __uint_as_float(rr.z & 0xffff0000u);
          v1[2] += __uint_as_float(rr.w << 16); v1[3] += __uint_as_float(rr.w & 0xffff0000u);
        }
        uint4 o;
        o.x = pack2bf(v0[0], v0[1]); o.y = pack2bf(v0[2], v0[3]);
        o.z = pack2bf(v1[0], v1[1]); o.w = pack2bf(v1[2], v1[3]);
        if (p.mask_width) {   // stacked folds: a token keeps the rank block of its own slot (block widths are multiples of 8 columns)
          int slot = 0;
#pragma unroll
          for (int q = 0; q < TST_MAX_STACK - 1; ++q) slot += (q < p.mask_nslot - 1 && gm >= p.mask_ends.t_end[q]) ? 1 : 0;
          if (gn / p.mask_width != slot) o = make_uint4(0u, 0u, 0u, 0u);
        }
        *(uint4*)(dst + (long)gm * p.ldc + gn) = o;
      }
    }
  }
#endif
}

template <int BM, int BN, int WARPS_M, int WARPS_N, bool TN = false, bool BUF = true>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_body<BM, BN, WARPS_M, WARPS_N, TN, BUF>(p, blockIdx.x, blockIdx.y, smem);
}

// Several TN contractions in ONE launch (the adapter gradients dB = dy^T.us, dA = s du^T.x of a layer's four module groups): each
// of them alone has too few 128x128 tiles for 256 CUs and was split over K with a slab reduce behind it; together they fill the
// chip without any split, so a layer's 8 contractions + 8 reduces become one launch. Workgroup b works on problem g with
// first[g] <= b < first[g+1], tile b - first[g].
struct GroupedGemm {
  GemmParams p[TST_MAX_GROUPED];
  int first[TST_MAX_GROUPED + 1];
  int n;
};
__global__ __launch_bounds__(256) void gemm_tn_grouped_kernel(GroupedGemm g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int idx = 0;
#pragma unroll
  for (int i = 1; i < TST_MAX_GROUPED; ++i) idx += (i < g.n && (int)blockIdx.x >= g.first[i]) ? 1 : 0;
  gemm_nt_body<128, 128, 2, 2, true, true>(g.p[idx], (int)blockIdx.x - g.first[idx], 0, smem);
}

// out[m][n] = sum_z slab[z][m][n] (+R) ; 4 columns per thread
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, int splitk, int M, int N,
                                                            void* C, long ldc, const bf16_t* R, long ldr, int out_f32, const bf16_t* bias,
                                                            int mask_width, int mask_nslot, SlotEnds ends) {
  const long n4 = N >> 2;
  const long total = (long)M * n4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / n4, c = (i % n4) << 2;
    f32x4 s = *(const f32x4*)(slab + m * N + c);
    for (int z0 = 1; z0 < splitk; z0 += 8) {   // eight partials in flight at a time (a plain loop waits for each load before it issues the next); same order of adds
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(slab + ((long)min(z0 + u, splitk - 1) * M + m) * N + c);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (z0 + u < splitk) s += v[u];        // (wave-uniform)
    }
    if (out_f32) {
      *(f32x4*)((float*)C + m * ldc + c) = s;
    } else {
      if (R) {
        const uint2 rr = *(const uint2*)(R + m * ldr + c);
        s[0] += __uint_as_float(rr.x << 16); s[1] += __uint_as_float(rr.x & 0xffff0000u);
        s[2] += __uint_as_float(rr.y << 16); s[3] += __uint_as_float(rr.y & 0xffff0000u);
      }
      if (bias) {
        const uint2 rr = *(const uint2*)(bias + c);
        s[0] += __uint_as_float(rr.x << 16); s[1] += __uint_as_float(rr.x & 0xffff0000u);
        s[2] += __uint_as_float(rr.y << 16); s[3] += __uint_as_float(rr.y & 0xffff0000u);
      }
      uint2 o;
      o.x = pack2bf(s[0], s[1]); o.y = pack2bf(s[2], s[3]);
      if (mask_width) {   // stacked folds: a token keeps the rank block of its own slot (widths are multiples of 8 columns)
        int slot = 0;
#pragma unroll
        for (int q = 0; q < TST_MAX_STACK - 1; ++q) slot += (q < mask_nslot - 1 && m >= ends.t_end[q]) ? 1 : 0;
        if ((int)c / mask_width != slot) o.x = o.y = 0u;
      }
      *(uint2*)((bf16_t*)C + m * ldc + c) = o;
    }
  }
}

// Naive reference contraction (one thread per output, fp32 accumulate) -- used by the GPU tests to
// cross-check the MFMA kernels on arbitrary layouts; never on the product path.
__global__ void gemm_ref_kernel(const bf16_t* A, long sam, long sak, const bf16_t* B, long sbn, long sbk, float* C,
                                long ldc, int M, int N, int K) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += bf2f(A[m * sam + k * sak]) * bf2f(B[n * sbn + k * sbk]);
  C[(long)m * ldc + n] = s;
}

// 64x64 LDS-tiled transpose, out[c][r] = in[r][c] for r < R, 0 for R <= r < R_pad (zero K padding for the
// contractions over the token axis)
template <typename AT>
__global__ __launch_bounds__(256) void transpose_kernel(const AT* __restrict__ in, long ldi, AT* __restrict__ out,
                                                        long ldo, int R, int C, int R_pad) {
  __shared__ AT tile[64][sizeof(AT) == 2 ? 66 : 65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? in[(long)r * ldi + c] : (AT)0;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < R_pad) out[(long)c * ldo + r] = tile[tx][i];
  }
}

// every operand byte must be reachable with a 31-bit offset from its base for the buffer form
template <bool TN>
bool buffer_addressable(const GemmParams& p) {
  const long lim = 0x7fffffffL;
  if (TN) return ((long)p.K * p.lda + p.M) * 2 < lim && ((long)p.K * p.ldb + p.N) * 2 < lim;
  auto fits = [&](long rows, long ld, long k) { return (rows * ld + k) * 2 < lim; };
  return fits(p.M, p.lda, p.K) && fits(p.N, p.ldb, p.K) && (!p.K2 || (fits(p.M, p.lda2, p.K2) && fits(p.N, p.ldb2, p.K2)));
}

template <int BM, int BN, int WARPS_M, int WARPS_N, bool TN, bool BUF>
int launch_variant_impl(hipStream_t st, GemmParams& p) {
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int LDS = (2 * STAGE > BM * BN * 4) ? 2 * STAGE : BM * BN * 4;
  static TstLdsAttr attr_set;   // per device
  auto kfn = gemm_nt_kernel<BM, BN, WARPS_M, WARPS_N, TN, BUF>;
  if (tst_set_max_lds(attr_set, (const void*)kfn, LDS) != TST_OK) return TST_EHIP;
  p.mtiles = tst_ceil_div(p.M, BM);
  p.ntiles = tst_ceil_div(p.N, BN);
  dim3 grid(p.mtiles * p.ntiles, p.splitk);
  hipLaunchKernelGGL(kfn, grid, dim3(256), LDS, st, p);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

template <int BM, int BN, int WARPS_M, int WARPS_N, bool TN = false>
int launch_variant(hipStream_t st, GemmParams& p) {
  static const bool flat = [] { const char* e = getenv("TST_FLAT_ADDR"); return e && atoi(e) != 0; }();   // A/B switch for measurements
  if (!flat && buffer_addressable<TN>(p)) return launch_variant_impl<BM, BN, WARPS_M, WARPS_N, TN, true>(st, p);
  return launch_variant_impl<BM, BN, WARPS_M, WARPS_N, TN, false>(st, p);
}

}  // namespace

// process-wide tile policy: 0 = 128x128 tiles (best for one fold alone on the GPU), 1 = projections on the 256x256
// pipelined tile (best with >= 2 resident folds per GPU), 2 = only projections with N >= 6144. level < 0 reads it.
// Default from the environment variable TST_BIG_TILE.
int gemm_big_tile_level(int level) {
  static int cur = [] { const char* e = getenv("TST_BIG_TILE"); return e ? atoi(e) : 0; }();
  if (level >= 0) cur = level;
  return cur;
}

size_t gemm_slab_bytes(int M, int N, int splitk) { return splitk > 1 ? (size_t)splitk * M * N * sizeof(float) : 0; }

// Tile/split-K heuristic. 512 = 256 CUs x 2 resident workgroups (64 KB LDS each).
void gemm_plan(int M, int N, int K, int K2, int* variant, int* splitk) {
  int v;
  if (N <= 64 || (N <= 320 && (N & 127) == 64)) v = 1;   // 128x64 (also N = 192, 320: no half-empty 128-column tile)
  else if (M <= 64) v = 2;       // 64x128
  else v = 0;                    // 128x128
  // adapter rank axis (N = 64 .. 320): a 32 x 64 tile (variant 7) gives M / 32 x N / 64 workgroups without splitting K -- no fp32 slab round trip, no
  // reduce launch. Measured SLOWER than the split 128 x 64 tile + reduce (34.7 vs 21-22 us at M 3555, N 192, K 4096: 64 dependent k-steps of a
  // tiny tile are latency-bound; profiles/r02_skinny_tile_ab.txt), so it stays an opt-in (TST_SKINNY_TILE=1) and a forced variant for the tests
  static const bool skinny_env = [] { const char* e = getenv("TST_SKINNY_TILE"); return e && atoi(e) != 0; }();
  if (skinny_env && N <= 320 && (N & 63) == 0 && (K + K2) <= 8192 && (long)tst_ceil_div(M, 32) * (N / 64) >= 192) { *variant = 7; *splitk = 1; return; }
  const int bm = (v == 2) ? 64 : 128, bn = (v == 1) ? 64 : 128;
  const long tiles = (long)tst_ceil_div(M, bm) * tst_ceil_div(N, bn);
  const int nt = (K + K2) / 64;
  // TST_BIG_TILE=1: projections go to the 256x256 pipelined tile (meant for several resident folds per GPU, where other
  // folds' kernels fill the holes its coarse tile grid leaves)
  const int big = gemm_big_tile_level(-1);
  if (big && v == 0 && M > 256 && N >= (big == 2 ? 6144 : 1024)) { *variant = 4; *splitk = 1; return; }
  int sk = 1;
  // A/B switch: rank-axis contractions (N <= 320) WITHOUT split-K (one launch, mask in the tile's epilogue, no slab, no reduce launch)
  static const bool rank_nosplit = [] { const char* e = getenv("TST_RANK_NOSPLIT"); return e && atoi(e) != 0; }();
  if (rank_nosplit && N <= 320 && K2 == 0) { *variant = v; *splitk = 1; return; }
  if (tiles >= 256 && tiles < 448 && nt >= 192) {
    // 1.0-1.75 waves of tiles on 256 CUs x 2 and a long K: a 4-way split fills the last wave and its fp32 slab
    // round trip is small against >= 12k-deep dot products (measured: profiles/r01_gemm_sweep_*.txt, rows down / dX_gate_up)
    sk = 4;
  } else if (tiles < 256) {
    sk = (int)((384 + tiles - 1) / tiles);
    int maxsk = nt / 4; if (maxsk < 1) maxsk = 1;
    if (sk > maxsk) sk = maxsk;
    if (sk > 64) sk = 64;
  }
  *variant = v; *splitk = sk;
}

// split factor of the ping-pong tile: a projection with N = 4096 gives one micro-batch only 80 tiles of 256x256 for 256
// CUs; splitting its long K two- to four-ways fills the chip (TST_PP_SPLITK=0 turns it off)
int gemm_pp_splitk(int M, int N, int Ktot) {
  // measured on Llama-3-8B LoRA (profiles/r01_g_splitk_*.json): alone on the GPU +28 % (49.0 -> 62.8 QA-pairs/s); with three
  // resident folds the other folds' kernels already fill the chip and the slab round trips cost 7 % (90.6 -> 84.2): tile
  // policy level 3 (one fold per GPU) splits, level 1 (several folds) does not
  if (gemm_big_tile_level(-1) != 3) return 1;
  const long tiles = (long)tst_ceil_div(M, 256) * tst_ceil_div(N, 256);
  const int nt = Ktot / 64;
  int sk = (int)(256 / tiles);
  if (sk > 4) sk = 4;
  if (sk > nt / 16) sk = nt / 16;   // at least 16 k-tiles per slice: the pipeline prologue and the slab round trip stay small
  return sk < 1 ? 1 : sk;
}

static int run_pp(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int sk, int* used) {
  if (sk > (p.K + p.K2) / 64) sk = (p.K + p.K2) / 64;
  if (sk < 1) sk = 1;
  while (sk > 1 && gemm_slab_bytes(p.M, p.N, sk) > slab_ws_bytes) --sk;
  if (!gemm_pp_supported(p)) sk = 1;
  p.splitk = sk;
  p.slab = slab_ws;
  p.slab_cap = slab_ws_bytes;
  if (used) { used[0] = 5; used[1] = sk; }
  int rc = gemm_pp(st, p);
  if (rc != TST_OK) return rc;
  if (sk > 1) {
    const long total = (long)p.M * (p.N / 4);
    int blocks = (int)((total + 255) / 256); if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, slab_ws, sk, p.M, p.N, p.C, p.ldc, p.R, p.ldr, p.out_f32, p.bias, p.mask_width, p.mask_nslot,
                       p.mask_ends);
    if (hipGetLastError() != hipSuccess) return TST_EHIP;
  }
  return TST_OK;
}

// the K-major members of the 256x256 ping-pong tile (gemm_pp.hip): TN (p.ta && p.tb, p.kvalid real rows, p.K derived) and NN (p.tb)
int gemm_pp_kmajor(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int force_splitk, int* used) {
  if (p.M <= 0 || p.N <= 0) return TST_EINVAL;
  if (p.ta && p.tb && p.kvalid > 0) p.K = (p.kvalid + 63) / 64 * 64;
  if (p.out_f32 ? (p.ldc & 3) : (p.ldc & 7)) return TST_EINVAL;
  if (p.R && (p.ldr & 7)) return TST_EINVAL;
  if (!gemm_pp_kmajor_supported(p)) return TST_EINVAL;
  return run_pp(st, p, slab_ws, slab_ws_bytes, force_splitk > 0 ? force_splitk : (p.no_splitk ? 1 : gemm_pp_splitk(p.M, p.N, p.K)), used);
}

int gemm_nt(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int force_variant, int force_splitk, int* used) {
  if (p.M <= 0 || p.N <= 0 || (p.K + p.K2) <= 0) return TST_EINVAL;
  if (p.ta || p.tb) return TST_EINVAL;   // K-major operands: gemm_pp_kmajor
  if ((p.K & 63) || (p.K2 & 63) || (p.N & 7)) return TST_EINVAL;
  if ((p.lda & 7) || (p.ldb & 7) || (p.K2 && ((p.lda2 & 7) || (p.ldb2 & 7)))) return TST_EINVAL;
  if (p.out_f32 ? (p.ldc & 3) : (p.ldc & 7)) return TST_EINVAL;
  if (p.R && (p.ldr & 7)) return TST_EINVAL;
  if (p.mask_width) {   // stacked folds: slot mask on a bf16 output; fused into the split-K reduce of the plain tiles, a pass of its own otherwise
    if (p.out_f32 || (p.mask_width & 7) || p.mask_nslot < 1 || p.mask_nslot > TST_MAX_STACK) return TST_EINVAL;
    int v0, s0;
    gemm_plan(p.M, p.N, p.K, p.K2, &v0, &s0);
    if ((force_variant >= 4 && force_variant != 7 && force_variant != 8 && force_variant != 9) || (force_variant < 0 && v0 == 4)) {
      GemmParams q = p;
      q.mask_width = 0;
      const int rc = gemm_nt(st, q, slab_ws, slab_ws_bytes, force_variant, force_splitk, used);
      return rc != TST_OK ? rc : rank_mask(st, (bf16_t*)p.C, (int)p.ldc, p.M, p.mask_width, p.mask_nslot, p.mask_ends);
    }
  }
  if (force_variant >= 10 || force_variant == 6) return TST_EINVAL;   // (ids of the stream-K and four-wave families: measured, rejected, removed in round 3)
  if (force_variant == 4) {  // 256x256 software-pipelined tile (gemm_big.hip)
    if (used) { used[0] = 4; used[1] = 1; }
    return gemm_big(st, p);
  }
  if (force_variant == 5) {  // 256x256 ping-pong tile (gemm_pp.hip), optional split-K through the slab workspace
    return run_pp(st, p, slab_ws, slab_ws_bytes, force_splitk > 0 ? force_splitk : 1, used);
  }
  // rank axis of the LoRA term (u = x.Ag^T, du = dy.Bg: N = the padded group rank): its own kernel, K split over the waves of a workgroup,
  // no slab and no reduce launch (gemm_rank.hip). TST_RANK_KERNEL=0 keeps the split 128x64 / 128x128 tiles + splitk_reduce (A/B switch).
  // Measured (profiles/r03_rank_axis_kernel_microbench_masked.txt, alone on the GPU, M = 3555, three slots): 8.0 vs 15.7 us at K = 4096, 24.1 vs
  // 26.7 at K = 14336, 62 vs 51 at K = 28672 (there the tiled path's 4 TB/s stream wins: HBM-bound either way) -- hence the K limit; on the
  // two-stream bench +0.3 ... +0.5 % (profiles/r03_ab_rank_kernel_lds.txt: the time these launches free is refilled by the other stream's tiles).
  static const bool rank_env = [] { const char* e = getenv("TST_RANK_KERNEL"); return !e || atoi(e) != 0; }();
  static const int rank_kmax = [] { const char* e = getenv("TST_RANK_KMAX"); return e ? atoi(e) : 16384; }();
  if (force_variant == 9) return gemm_rank_supported(p) ? gemm_rank(st, p, 1) : TST_EINVAL;
  if (force_variant == 8 || (force_variant < 0 && rank_env && p.K <= rank_kmax && (p.N <= 256 || p.mask_width) && p.N <= 512 && gemm_rank_supported(p))) {
    if (!gemm_rank_supported(p)) return TST_EINVAL;
    if (used) { used[0] = 8; used[1] = 1; }
    return gemm_rank(st, p);
  }
  int v, sk;
  gemm_plan(p.M, p.N, p.K, p.K2, &v, &sk);
  if (force_variant < 0 && v == 4) {
    // the 256x256 family: the ping-pong member (variant 5) unless TST_BIG_KIND=4 asks for the one-barrier pipeline or an
    // operand is too large for its 32-bit buffer offsets
    static const int kind = [] { const char* e = getenv("TST_BIG_KIND"); return e ? atoi(e) : 5; }();
    if (kind == 5 && gemm_pp_supported(p))
      return run_pp(st, p, slab_ws, slab_ws_bytes, force_splitk > 0 ? force_splitk : (p.no_splitk ? 1 : gemm_pp_splitk(p.M, p.N, p.K + p.K2)), used);
    if (used) { used[0] = 4; used[1] = 1; }
    return gemm_big(st, p);
  }
  if (force_variant >= 0) v = force_variant;
  if (force_splitk > 0) sk = force_splitk;
  while (sk > 1 && gemm_slab_bytes(p.M, p.N, sk) > slab_ws_bytes) --sk;
  p.splitk = sk;
  p.slab = slab_ws;
  if (used) { used[0] = v; used[1] = sk; }
  int rc;
  switch (v) {
    case 0: rc = launch_variant<128, 128, 2, 2>(st, p); break;
    case 1: rc = launch_variant<128, 64, 2, 2>(st, p); break;
    case 2: rc = launch_variant<64, 128, 1, 4>(st, p); break;
    case 7: rc = launch_variant<32, 64, 2, 2>(st, p); break;
    case 3:  // TN (contraction over the row axis of both operands)
      if (p.K2 || (p.M & 7) || p.kvalid <= 0 || p.kvalid > p.K || p.R) return TST_EINVAL;
      rc = launch_variant<128, 128, 2, 2, true>(st, p);
      break;
    default: return TST_EINVAL;
  }
  if (rc != TST_OK) return rc;
  if (sk > 1) {
    const long total = (long)p.M * (p.N / 4);
    int blocks = (int)((total + 255) / 256); if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, slab_ws, sk, p.M, p.N, p.C, p.ldc, p.R, p.ldr, p.out_f32, p.bias, p.mask_width, p.mask_nslot,
                       p.mask_ends);
    if (hipGetLastError() != hipSuccess) return TST_EHIP;
  }   // (unsplit launches apply the slot mask in their own epilogue)
  return TST_OK;
}

// C[M,N] = alpha * sum_{t<kvalid} A[t,M] * B[t,N]: tile-per-workgroup TN kernel + split-K over the token axis
// (no persistent / spinning workgroups: safe when several folds' streams share the GPU)
int gemm_tn(hipStream_t st, GemmParams p, float* slab_ws, size_t slab_ws_bytes, int* used) {
  p.K = (p.kvalid + 63) / 64 * 64;
  p.K2 = 0;
  const long tiles = (long)tst_ceil_div(p.M, 128) * tst_ceil_div(p.N, 128);
  const int nt = p.K / 64;
  int sk = (int)((384 + tiles - 1) / tiles);
  int maxsk = nt / 2; if (maxsk < 1) maxsk = 1;
  if (sk > maxsk) sk = maxsk;
  if (sk > 32) sk = 32;
  return gemm_nt(st, p, slab_ws, slab_ws_bytes, 3, sk, used);
}

int gemm_ref(hipStream_t st, const bf16_t* A, long sam, long sak, const bf16_t* B, long sbn, long sbk, float* C, long ldc,
             int M, int N, int K) {
  const long total = (long)M * N;
  hipLaunchKernelGGL(gemm_ref_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, A, sam, sak, B, sbn, sbk, C, ldc, M, N, K);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

template <typename AT>
int transpose_mat(hipStream_t st, const AT* in, long ldi, AT* out, long ldo, int R, int C, int R_pad) {
  if (R_pad < R) R_pad = R;
  dim3 grid(tst_ceil_div(C, 64), tst_ceil_div(R_pad, 64));
  hipLaunchKernelGGL(transpose_kernel<AT>, grid, dim3(256), 0, st, in, ldi, out, ldo, R, C, R_pad);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
template int transpose_mat<bf16_t>(hipStream_t, const bf16_t*, long, bf16_t*, long, int, int, int);
template int transpose_mat<float>(hipStream_t, const float*, long, float*, long, int, int, int);

// n <= TST_MAX_GROUPED TN contractions C_i[M_i,N_i] (fp32) = alpha_i * sum_{t<kvalid_i} A_i[t,M_i] * B_i[t,N_i] in one launch, no split-K.
// Falls back to one launch each when an operand is beyond the 32-bit buffer offsets.
int gemm_tn_grouped(hipStream_t st, const GemmParams* ps, int n, float* slab_ws, size_t slab_ws_bytes) {
  if (n <= 0) return TST_OK;
  if (n > TST_MAX_GROUPED) return TST_EINVAL;
  GroupedGemm g;
  memset(&g, 0, sizeof(g));
  bool ok = true;
  int total = 0;
  for (int i = 0; i < n; ++i) {
    GemmParams p = ps[i];
    if (p.M <= 0 || p.N <= 0 || p.kvalid <= 0 || (p.M & 7) || (p.N & 7) || (p.lda & 7) || (p.ldb & 7) || (p.ldc & 3) || !p.out_f32 || p.R || p.K2) return TST_EINVAL;
    p.K = (p.kvalid + 63) / 64 * 64;
    p.splitk = 1;
    p.slab = nullptr;
    p.mtiles = tst_ceil_div(p.M, 128);
    p.ntiles = tst_ceil_div(p.N, 128);
    ok = ok && buffer_addressable<true>(p);
    g.p[i] = p;
    g.first[i] = total;
    total += p.mtiles * p.ntiles;
  }
  g.first[n] = total;
  g.n = n;
  if (!ok) {
    for (int i = 0; i < n; ++i) {
      const int rc = gemm_tn(st, ps[i], slab_ws, slab_ws_bytes, nullptr);
      if (rc != TST_OK) return rc;
    }
    return TST_OK;
  }
  constexpr int LDS = 2 * (128 + 128) * 128;
  static TstLdsAttr attr_set;   // per device
  if (tst_set_max_lds(attr_set, (const void*)gemm_tn_grouped_kernel, LDS) != TST_OK) return TST_EHIP;
  hipLaunchKernelGGL(gemm_tn_grouped_kernel, dim3(total), dim3(256), LDS, st, g);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
