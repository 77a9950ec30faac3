// K8/K9: global-norm clip + fused AdamW over flat fp32 parameter/gradient/moment buffers (HBM-bound),
// and the LoRA adapter pack/unpack between the logical fp32 masters and the padded bf16 MFMA operands.
//
// Oracle lines: torch/nn/utils/clip_grad.py:106-108,165-169 (total_norm, clip_coef = max_norm/(norm+1e-6),
// clamped to 1.0); torch/optim/adam.py:414-476 single-tensor math == the fused kernel's math
// (p *= 1-lr*wd; m = lerp(m,g,1-b1); v = b2*v + (1-b2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)).
#include "common.h"
#include "kernels.h"

namespace {

// stage 1: per-block partial sums of squares (fixed assignment of elements to blocks => reproducible)
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long n, float* __restrict__ partial) {
  __shared__ float red[4];
  float s = 0.f;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = *(const f32x4*)(g + i * 4);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0) for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += g[i] * g[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// stage 2: out[0] = ||g||_2, out[1] = clip coefficient. One workgroup of 1024 threads, 16 bytes per lane: a full fine-tune hands over ~330 k partial sums
// (one per weight-gradient tile), which 256 threads reading one float each took 0.54 ms to add; fixed assignment of partials to lanes: reproducible.
__global__ __launch_bounds__(1024) void clip_finalize_kernel(const float* __restrict__ partial, int nparts, float max_norm, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  const int n4 = ((((unsigned long long)partial) & 15ull) == 0) ? (nparts >> 2) : 0;
  for (int i = threadIdx.x; i < n4; i += 1024) {
    const f32x4 v = ((const f32x4*)partial)[i];
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  for (int i = (n4 << 2) + threadIdx.x; i < nparts; i += 1024) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0.f;
    for (int w = 0; w < 16; ++w) s += red[w];
    const float norm = sqrtf(s);
    float coef = 1.0f;
    if (max_norm > 0.f) { coef = max_norm / (norm + 1e-6f); if (coef > 1.0f) coef = 1.0f; }
    out[0] = norm;
    out[1] = coef;
  }
}

// optimizer-state sharding: out[0] = sum of the partials (the shard's sum of squares, all-reduced over the group before clip_from_sumsq)
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[0] = s;
}
__global__ void clip_from_sumsq_kernel(const float* __restrict__ sumsq, float max_norm, float* __restrict__ out) {
  const float norm = sqrtf(sumsq[0]);
  float coef = 1.0f;
  if (max_norm > 0.f) { coef = max_norm / (norm + 1e-6f); if (coef > 1.0f) coef = 1.0f; }
  out[0] = norm;
  out[1] = coef;
}

// one element of the fused AdamW update (adam.py:414-476, see the header of this file); returns the new parameter
__device__ __forceinline__ float adamw_elem(float p, float g, float& m, float& v, float coef, float decay, float step_size, float beta1, float beta2, float eps,
                                            float bc2_sqrt) {
  const float gi = g * coef;
  float pi = p * decay;
  m = m + (1.0f - beta1) * (gi - m);
  v = beta2 * v + (1.0f - beta2) * gi * gi;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  pi -= step_size * (m / denom);
  return pi;
}

// shadow != nullptr (full fine-tune): the updated fp32 master is also rounded into the bf16 compute copy of the weight.
// 16 bytes per lane and array (four elements) while the buffers are 16-byte aligned: a quarter of the memory instructions of the
// scalar form -- what a CU can stream is bounded by the memory instructions it issues, and the full fine-tune runs this kernel on a
// SUBSET of the CUs beside the next forward (engine.hip, tst_ctx::opt_stream), where every CU has to pull its share of the HBM rate.
// U independent 16-byte pieces per lane and array, all loaded before the first is used: what ONE CU streams is bounded by the bytes its waves keep in
// flight (32 waves x 4 loads x 1 KB = 128 KB at U = 1: 37 GB/s per CU at the ~3.5 us a load takes beside other traffic), and the full fine-tune's optimizer
// has a SHARE of the CUs to reach the HBM rate with. NT: non-temporal loads and stores -- every byte is touched once per step, the next forward's weights and
// activations keep the L2 / Infinity Cache lines.
template <typename AT, int U, bool NT>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    long n, const float* __restrict__ clip, float lr, float beta1, float beta2, float eps, float wd,
                                                    float bc1, float bc2_sqrt, AT* __restrict__ shadow) {
  const float coef = clip ? clip[1] : 1.0f;
  const float step_size = lr / bc1;
  const float decay = 1.0f - lr * wd;
  const bool al = ((((unsigned long long)p | (unsigned long long)g | (unsigned long long)m | (unsigned long long)v) & 15ull) == 0) &&
                  (!shadow || ((unsigned long long)shadow & (4 * sizeof(AT) - 1)) == 0);
  const long n4 = al ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * 256;
  auto ld = [](const float* base, long i) -> f32x4 {
    if constexpr (NT) return __builtin_nontemporal_load((const f32x4*)base + i);
    else return ((const f32x4*)base)[i];
  };
  auto stv = [](float* base, long i, f32x4 x) {
    if constexpr (NT) __builtin_nontemporal_store(x, (f32x4*)base + i);
    else ((f32x4*)base)[i] = x;
  };
#pragma nounroll
  for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += stride * U) {
    f32x4 pi[U], mi[U], vi[U], gi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i < n4) { pi[u] = ld(p, i); mi[u] = ld(m, i); vi[u] = ld(v, i); gi[u] = ld(g, i); }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i >= n4) break;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = mi[u][j], vj = vi[u][j];
        o[j] = adamw_elem(pi[u][j], gi[u][j], mj, vj, coef, decay, step_size, beta1, beta2, eps, bc2_sqrt);
        mi[u][j] = mj; vi[u][j] = vj;
      }
      stv(p, i, f32x4{o[0], o[1], o[2], o[3]});
      stv(m, i, mi[u]);
      stv(v, i, vi[u]);
      if (shadow) st4(shadow + i * 4, o);   // the compute copy is the next forward's operand: default policy
    }
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float mi = m[i], vi = v[i];
    const float pi = adamw_elem(p[i], g[i], mi, vi, coef, decay, step_size, beta1, beta2, eps, bc2_sqrt);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (shadow) st1(shadow + i, pi);
  }
}

// Full fine-tune, weight matrices: the same update on one row-major [rows, cols] matrix, 64x64 tiles, writing the bf16
// compute copy AND its transpose (the dX contractions' operand) -- saves the separate W -> W^T pass over all weights after every
// optimizer step (2 B/param extra write here against 4 B/param of traffic there).
// A thread owns a 4 x 4 block of the tile (wave w: rows 16w .. 16w+15; lane = (q, cl): rows 16w + 4q .. +3, columns 4cl .. +3): every global
// access is 16 bytes per lane (8 for the bf16 row of the compute copy); the transpose goes through an LDS image [64 columns][64 rows] written as
// 4-row pieces and read back as whole 16-byte pieces of a W^T row (128-byte segments of W^T per 8 lanes). 34 memory instructions per thread and
// 16 elements instead of 144.
template <typename AT>
__global__ __launch_bounds__(256) void adamw_tiled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          int rows, int cols, const float* __restrict__ clip, float lr, float beta1, float beta2, float eps,
                                                          float wd, float bc1, float bc2_sqrt, AT* __restrict__ shadow, AT* __restrict__ shadowT) {
  constexpr int PITCH = 64 + 16 / (int)sizeof(AT);   // elements per image row: 16-byte aligned rows, 144 / 272 bytes
  __shared__ __attribute__((aligned(16))) AT tileT[64 * PITCH];
  const float coef = clip ? clip[1] : 1.0f;
  const float step_size = lr / bc1;
  const float decay = 1.0f - lr * wd;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane >> 4, cl = lane & 15;
  const int tiles_c = cols >> 6;
  const int r0 = (blockIdx.x / tiles_c) << 6, c0 = (blockIdx.x % tiles_c) << 6;
  const int rl = 16 * w + 4 * q;   // first of this thread's four tile rows
  f32x4 pp[4], gg[4], mm[4], vv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long idx = (long)(r0 + rl + i) * cols + c0 + 4 * cl;
    pp[i] = *(const f32x4*)(p + idx); gg[i] = *(const f32x4*)(g + idx); mm[i] = *(const f32x4*)(m + idx); vv[i] = *(const f32x4*)(v + idx);
  }
  float o[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mm[i][j], vj = vv[i][j];
      o[i][j] = adamw_elem(pp[i][j], gg[i][j], mj, vj, coef, decay, step_size, beta1, beta2, eps, bc2_sqrt);
      mm[i][j] = mj; vv[i][j] = vj;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long idx = (long)(r0 + rl + i) * cols + c0 + 4 * cl;
    *(f32x4*)(p + idx) = f32x4{o[i][0], o[i][1], o[i][2], o[i][3]};
    *(f32x4*)(m + idx) = mm[i];
    *(f32x4*)(v + idx) = vv[i];
    st4(shadow + idx, o[i]);
  }
  // the thread's 4 x 4 block, transposed: image row 4cl + j holds tile column 4cl + j, its elements rl .. rl+3 are this thread's rows
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float colv[4] = {o[0][j], o[1][j], o[2][j], o[3][j]};
    st4(tileT + (4 * cl + j) * PITCH + rl, colv);
  }
  __syncthreads();
  constexpr int E = 16 / (int)sizeof(AT);     // elements per 16-byte piece
  constexpr int PPR = 64 / E;                 // pieces per image row
#pragma unroll
  for (int it = 0; it < (64 * PPR) / 256; ++it) {
    const int pc = it * 256 + threadIdx.x;
    const int c = pc / PPR, r = (pc % PPR) * E;
    *(uint4*)(shadowT + (long)(c0 + c) * rows + r0 + r) = *(const uint4*)(tileT + c * PITCH + r);
  }
}

// which enabled module of the group owns output row n of the fused projection (row ranges [seg_row0, seg_row1)), and which of its rows that is; mod = -1: none
template <typename AT>
__device__ __forceinline__ void row_owner(const LoraGroupDescT<AT>& gd, int n, int& mod, int& local) {
  mod = -1;
  local = 0;
  for (int s2 = 0; s2 < gd.nmod; ++s2)
    if (n >= gd.seg_row0[s2] && n < gd.seg_row1[s2]) { mod = s2; local = n - gd.seg_row0[s2]; }
}

// ---- LoRA pack: logical fp32 masters -> padded, grouped bf16 operands (see engine.cpp for the group layout) ----
//   segment seg = slot * nmod + module (one slot unless folds are stacked in the context); rank columns seg*r .. seg*r+r-1
//   Ag  [RP, din]   rows seg*r + j  = A_seg[j, :]                 (LoRA-down operand, u = x.Ag^T)
//   AgT [din, RP]   AgT[k, seg*r+j] = bf16(scale * A_seg[j, k])   (dX second segment)
//   Bg  [dout, RP]  Bg[n, seg*r+j]  = B_seg[n - off_seg, j] for rows of segment seg, 0 elsewhere
//   BgT [RP, dout]  transpose of Bg                                (du = dy.Bg)
// grid = (64-wide tiles along the long axis, 2 parts {A, B}, groups); a workgroup packs a 64 x 64 tile per rank chunk. Round 4: a thread owns 8 consecutive
// elements of a row, so every global access is 16 bytes per lane (the scalar form wrote 2 bytes per lane and ran the 1.5 GB of a Llama-3-8B repack at 1 TB/s:
// 0.89 ms per optimizer step with nothing of the context to hide it behind); the transposed copies go through a 64 x 64 fp32 LDS tile and leave as whole
// 16-byte pieces too.
template <typename AT>
__global__ __launch_bounds__(256) void lora_pack_tiled_kernel(const LoraGroupDescT<AT>* __restrict__ descs, const float* __restrict__ master) {
  __shared__ float tile[64][65];
  // a reference, not a by-value copy: the offset arrays are indexed at run time, and a private copy of a
  // runtime-indexed array lands in scratch memory (cdna_hip_programming.md §5.4 rule 20)
  const LoraGroupDescT<AT>& gd = descs[blockIdx.z];
  const int r8 = threadIdx.x >> 3, c8 = (threadIdx.x & 7) * 8;   // row 0 .. 31 of a pass, first of this thread's 8 columns
  const int x0 = blockIdx.x * 64;
  const bool vec = (gd.r & 7) == 0;   // 8 consecutive rank indices lie in one segment (lora_r 8 .. 64): the B master is read 32 bytes at a time
  if (blockIdx.y == 0) {
    if (x0 >= gd.din) return;
    for (int jb = 0; jb < gd.RP; jb += 64) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int jj = pass * 32 + r8, j = jb + jj, seg = j / gd.r;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (seg < gd.nseg) {
          const float* src = master + gd.a_off[seg] + (long)(j % gd.r) * gd.din + x0 + c8;
          const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
          v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
        }
        st8(&gd.Ag[(long)j * gd.din + x0 + c8], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[jj][c8 + e] = v[e];
      }
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int kk = pass * 32 + r8;
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = tile[c8 + e][kk] * gd.scale;
        st8(&gd.AgT[(long)(x0 + kk) * gd.RP + jb + c8], t);
      }
      __syncthreads();
    }
  } else {
    if (x0 >= gd.dout) return;
    for (int jb = 0; jb < gd.RP; jb += 64) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int nn = pass * 32 + r8, n = x0 + nn, j0 = jb + c8;
        int mod, local;
        row_owner(gd, n, mod, local);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (mod >= 0) {
          if (vec) {
            const int seg = j0 / gd.r;   // = slot * nmod + module
            if (seg < gd.nseg && seg % gd.nmod == mod) {
              const float* src = master + gd.b_off[seg] + (long)local * gd.r + j0 % gd.r;
              const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
              v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int j = j0 + e, seg = j / gd.r;
              if (seg < gd.nseg && seg % gd.nmod == mod) v[e] = master[gd.b_off[seg] + (long)local * gd.r + j % gd.r];
            }
          }
        }
        st8(&gd.Bg[(long)n * gd.RP + j0], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[nn][c8 + e] = v[e];
      }
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int jj = pass * 32 + r8;
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = tile[c8 + e][jj];
        st8(&gd.BgT[(long)(jb + jj) * gd.dout + x0 + c8], t);
      }
      __syncthreads();
    }
  }
}

// ---- LoRA unpack: padded fp32 group gradients -> logical flat gradient ----
template <typename AT>
__global__ __launch_bounds__(256) void lora_unpack_grad_kernel(const LoraGroupDescT<AT>* __restrict__ descs, float* __restrict__ grad) {
  const LoraGroupDescT<AT>& gd = descs[blockIdx.y];
  const long nA = (long)gd.nseg * gd.r * gd.din;
  const long nB = (long)gd.dout * gd.r;   // upper bound: rows outside every segment are skipped
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (long)gridDim.x * 256) {
    if (i < nA) {
      const int j = (int)(i / gd.din), k = (int)(i % gd.din);
      const int seg = j / gd.r, jj = j % gd.r;
      grad[gd.a_off[seg] + (long)jj * gd.din + k] = gd.dAg[(long)j * gd.din + k];
    } else {
      const long e = i - nA;
      const int n = (int)(e / gd.r), jj = (int)(e % gd.r);
      int mod, local;
      row_owner(gd, n, mod, local);
      if (mod >= 0)
        for (int seg = mod; seg < gd.nseg; seg += gd.nmod)   // every slot's copy of this module
          grad[gd.b_off[seg] + (long)local * gd.r + jj] = gd.dBg[(long)n * gd.RP + seg * gd.r + jj];
    }
  }
}

inline int nblocks(long work, int cap) {
  long b = (work + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
// sumsq_partial_kernel has no scalar form for an unaligned g (kernels.h): the host refuses it
inline bool aligned16(const void* p) { return (((unsigned long long)p) & 15ull) == 0; }

// gradient accumulation (HF/trainer.py:1740-1758: backward of every micro-batch adds into .grad): acc = first ? g : acc + g
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, int first) {
  const long n4 = ((((unsigned long long)acc | (unsigned long long)g) & 15ull) == 0) ? (n >> 2) : 0;   // 16-byte accesses only on aligned buffers
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 v = ((const f32x4*)g)[i];
    if (!first) v += ((const f32x4*)acc)[i];
    ((f32x4*)acc)[i] = v;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc[i] = first ? g[i] : acc[i] + g[i];
}
}  // namespace
int grad_accumulate(hipStream_t st, float* acc, const float* g, long n, int first) {
  if (n <= 0) return TST_OK;
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, st, acc, g, n, first);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

int grad_clip_coef(hipStream_t st, const float* g, long n, float max_norm, float* partial_ws, int nparts, float* out2) {
  if (nparts < 1 || nparts > 4096 || !aligned16(g)) return TST_EINVAL;
  // one block per partial; a full fine-tune streams 32 GB of gradients here: 256 blocks reached 2.3 TB/s, 4096 fill the chip
  const long want = (n / 4 + 255) / 256;
  if (want < nparts) nparts = want < 1 ? 1 : (int)want;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nparts), dim3(256), 0, st, g, n, partial_ws);
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(1024), 0, st, partial_ws, nparts, max_norm, out2);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
// the two stages of grad_clip_coef on their own (full fine-tune: the weight-gradient contractions leave their own partial sums)
int sumsq_partial(hipStream_t st, const float* g, long n, float* partial, int nparts) {
  if (nparts < 1 || n <= 0 || !aligned16(g)) return TST_EINVAL;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nparts), dim3(256), 0, st, g, n, partial);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
int clip_finalize(hipStream_t st, const float* partial, int nparts, float max_norm, float* out2) {
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, nparts, max_norm, out2);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
int sum_partials(hipStream_t st, const float* partial, int nparts, float* out1) {
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, partial, nparts, out1);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
int clip_from_sumsq(hipStream_t st, const float* sumsq1, float max_norm, float* out2) {
  hipLaunchKernelGGL(clip_from_sumsq_kernel, dim3(1), dim3(1), 0, st, sumsq1, max_norm, out2);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
template <typename AT>
int adamw_step(hipStream_t st, float* p, const float* g, float* m, float* v, long n, const float* clip, float lr, float beta1, float beta2, float eps,
               float wd, float bc1, float bc2_sqrt, AT* shadow) {
  if (n <= 0) return TST_OK;
  // 2 pieces in flight per lane and array; TST_ADAMW_NT = 1 / 0 non-temporal accesses on / off (A/B switch; the same arithmetic on the same elements in
  // either form: bit-identical results PER ELEMENT TYPE AT -- the bf16_t and the float instance differ from each other in the last bit of m on a few per cent of
  // the second piece's elements, profiles/optim_kernel_parity.txt; a context never mixes the two). Default: non-temporal for the full fine-tune's 30 B/param stream (shadow != nullptr) -- measured on config 3, one GPU,
  // two rounds: 23.87 QA/s (1 piece, default policy) | 24.29 (1, nt) | 24.51 (2, nt); unrolling alone changes nothing (profiles/r05_full_adamw_ab.txt).
  constexpr int unroll = 2;
  static const int nt_env = [] { const char* e = getenv("TST_ADAMW_NT"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
  const bool nt = nt_env >= 0 ? nt_env != 0 : shadow != nullptr;
  const dim3 grid(nblocks(((n + 3) / 4 + unroll - 1) / unroll, 8192)), blk(256);
#define TST_ADAMW_LAUNCH(NT) hipLaunchKernelGGL((adamw_kernel<AT, unroll, NT>), grid, blk, 0, st, p, g, m, v, n, clip, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, shadow)
  if (nt) TST_ADAMW_LAUNCH(true);
  else TST_ADAMW_LAUNCH(false);
#undef TST_ADAMW_LAUNCH
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
template <typename AT>
int adamw_step_matrix(hipStream_t st, float* p, const float* g, float* m, float* v, int rows, int cols, const float* clip, float lr, float beta1,
                      float beta2, float eps, float wd, float bc1, float bc2_sqrt, AT* shadow, AT* shadowT) {
  if ((rows & 63) || (cols & 63) || !shadow || !shadowT) return TST_EINVAL;
  hipLaunchKernelGGL(adamw_tiled_kernel<AT>, dim3((unsigned)((rows >> 6) * (cols >> 6))), dim3(256), 0, st, p, g, m, v, rows, cols, clip, lr, beta1, beta2, eps, wd,
                     bc1, bc2_sqrt, shadow, shadowT);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
template <typename AT>
int lora_pack(hipStream_t st, const LoraGroupDescT<AT>* descs_dev, int ngroups, const float* master, long max_long_axis) {
  if (ngroups <= 0) return TST_OK;
  hipLaunchKernelGGL(lora_pack_tiled_kernel<AT>, dim3((unsigned)((max_long_axis + 63) / 64), 2, ngroups), dim3(256), 0, st, descs_dev, master);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
template <typename AT>
int lora_unpack_grad(hipStream_t st, const LoraGroupDescT<AT>* descs_dev, int ngroups, float* grad, long max_elems) {
  if (ngroups <= 0) return TST_OK;
  hipLaunchKernelGGL(lora_unpack_grad_kernel<AT>, dim3(nblocks(max_elems, 256), ngroups), dim3(256), 0, st, descs_dev, grad);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

#define TST_INST(AT)                                                                                                                          \
  template int adamw_step<AT>(hipStream_t, float*, const float*, float*, float*, long, const float*, float, float, float, float, float, float, float, AT*); \
  template int adamw_step_matrix<AT>(hipStream_t, float*, const float*, float*, float*, int, int, const float*, float, float, float, float, float, float,    \
                                     float, AT*, AT*);                                                                                        \
  template int lora_pack<AT>(hipStream_t, const LoraGroupDescT<AT>*, int, const float*, long);                                                \
  template int lora_unpack_grad<AT>(hipStream_t, const LoraGroupDescT<AT>*, int, float*, long);
TST_INST(bf16_t)
TST_INST(float)
#undef TST_INST
