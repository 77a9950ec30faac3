// Per-head q/k RMSNorm of the Qwen3 family (modeling_qwen3.py:237-238, 252-253): every query head and every key head of the fused q|k|v projection
// is RMS-normalised over head_dim = 128 behind the projection and before RoPE, with ONE learned [128] vector for all query heads (q_norm) and one for
// all key heads (k_norm). Forward and backward run in place on the q|k columns of the [T, (H + 2 Hkv) 128] activation / gradient; v is never touched.
//
// Shape: HBM-bound streaming. A row is 128 elements = 16 lanes x 8 elements (one 16-byte load per lane in bf16), so a wave64 covers four rows per
// iteration and a 256-thread workgroup sixteen; the row statistic is four DPP rotations inside the 16-lane row (no LDS, no barrier); the half-split RoPE
// partner j +- 64 lives 8 lanes away in the same row. q_norm / k_norm sit in registers (8 + 8 floats per lane). Grid-stride over the T (H + Hkv) rows.
//
// Rounding points (bf16 path; the fp32 strict path rounds nowhere): y = bf16(w * bf16(x * rstd)) as RMSNorm everywhere in this library
// (modeling_llama.py:62-67), statistics fp32. With pos / cosT / sinT the rotation of rope_kernel (elementwise.hip) follows in the same traversal on the
// ROUNDED y, with rope_kernel's own expressions: bit-identical to head norm followed by rope_apply. Backward: un-rotate, round, then the norm backward.
//
// The backward reads the RAW projection output x, which the training forward copies into `stash` (the in-place forward destroys it): x_hat = x * rstd is
// re-formed from it, so nothing is ever divided by w (a zero weight element is legal) and dx is the arithmetic of rmsnorm_bwd_kernel.
// Weight gradients (full fine-tune): per-workgroup partial sums [grid][256] (q | k) and an ordered finish -- no atomics, bit-reproducible.
#include "kernels.h"

// The fused and the two-pass forms must agree bit for bit, and so must the four instantiations of each kernel among themselves: the compiler's own choice of
// which multiply-add pairs to contract differs from one instantiation to the next (measured: the un-rotation of the fp32 backward fused the OTHER product than
// rope_kernel does). So contraction is off in this file and every fused multiply-add is written out.
#pragma clang fp contract(off)

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP)

// lane i <- lane (i + n) % 16 of its row of 16 lanes (DPP row_ror:n)
template <int N> __device__ __forceinline__ float row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, true));
}
// sum over the 16 lanes of a row, the same bits in every lane (every lane adds the same pairs at each step; fp32 addition is commutative)
__device__ __forceinline__ float row16_sum(float v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  return v;
}

// rotation of this lane's 8 elements of a 128-row; the partner element j +- 64 is 8 lanes away. rope_kernel (elementwise.hip) computes o1 = a co - b si,
// o2 = b co + a si with si = sin * sign, which hipcc contracts to fma(a, co, -(b si)) and fma(b, co, a si) in both precisions: own * co is the fused product,
// partner * (si or -si) a rounded one. The same operations are spelled out here (tests/test_head_norm_gpu.py pins the two kernels to each other bit for bit).
__device__ __forceinline__ void rotate8(float* f, int sub, const int* __restrict__ pos, unsigned t, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                        float sign) {
  const int c = (sub & 7) * 8;
  const long o = (long)pos[t] * 64 + c;
  float co[8], sn[8];
  ld8(cosT + o, co);
  ld8(sinT + o, sn);
  const float sg = (sub & 8) ? -sign : sign;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float partner = row_ror<8>(f[j]);
    const float t = partner * (sn[j] * sg);
    f[j] = __builtin_fmaf(f[j], co[j], -t);
  }
}

template <typename AT, bool ROPE>
__global__ __launch_bounds__(256) void head_norm_fwd_kernel(AT* __restrict__ qkv, long ld, const AT* __restrict__ wq, const AT* __restrict__ wk,
                                                            float* __restrict__ rstd_out, AT* __restrict__ stash, unsigned total, int H, int HK, unsigned magic,
                                                            float eps, const int* __restrict__ pos, const float* __restrict__ cosT,
                                                            const float* __restrict__ sinT) {
  const int sub = threadIdx.x & 15;
  float fwq[8], fwk[8];
  ld8(wq + sub * 8, fwq);
  ld8(wk + sub * 8, fwk);
  const unsigned stride = gridDim.x * 16;
  for (unsigned r = blockIdx.x * 16 + (threadIdx.x >> 4); r < total; r += stride) {
    const unsigned t = __umulhi(r, magic);   // r / HK (exact: the launcher checks total * HK < 2^32)
    const int h = (int)(r - t * (unsigned)HK);
    AT* p = qkv + (long)t * ld + h * 128 + sub * 8;
    float f[8];
    ld8(p, f);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
    ss = row16_sum(ss);
    const float rstd = 1.0f / sqrtf(ss / 128.0f + eps);
    if (sub == 0) rstd_out[r] = rstd;
    if (stash) st8(stash + (long)r * 128 + sub * 8, f);
    const bool isq = h < H;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = rnd_as<AT>((isq ? fwq[j] : fwk[j]) * rnd_as<AT>(f[j] * rstd));
    if constexpr (ROPE) rotate8(f, sub, pos, t, cosT, sinT, 1.0f);
    st8(p, f);
  }
}

// dx = rstd (g - x_hat mean(g x_hat)), g = dy w, x_hat = x rstd; DW: part[block][0..127] = sum over the block's query rows of dy bf16(x_hat), [128..255] the key rows
template <typename AT, bool ROPE, bool DW>
__global__ __launch_bounds__(256) void head_norm_bwd_kernel(AT* __restrict__ dqkv, long ld, const AT* __restrict__ wq, const AT* __restrict__ wk,
                                                            const float* __restrict__ rstd_in, const AT* __restrict__ stash, unsigned total, int H, int HK,
                                                            unsigned magic, const int* __restrict__ pos, const float* __restrict__ cosT,
                                                            const float* __restrict__ sinT, float* __restrict__ part) {
  const int sub = threadIdx.x & 15;
  float fwq[8], fwk[8];
  ld8(wq + sub * 8, fwq);
  ld8(wk + sub * 8, fwk);
  float aq[8], ak[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) aq[j] = ak[j] = 0.f;
  const unsigned stride = gridDim.x * 16;
  for (unsigned r = blockIdx.x * 16 + (threadIdx.x >> 4); r < total; r += stride) {
    const unsigned t = __umulhi(r, magic);
    const int h = (int)(r - t * (unsigned)HK);
    AT* p = dqkv + (long)t * ld + h * 128 + sub * 8;
    float g[8], x[8];
    ld8(p, g);
    ld8(stash + (long)r * 128 + sub * 8, x);
    const float rstd = rstd_in[r];
    if constexpr (ROPE) {
      rotate8(g, sub, pos, t, cosT, sinT, -1.0f);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = rnd_as<AT>(g[j]);   // (the stand-alone pass stores its result before the norm backward reads it)
    }
    const bool isq = h < H;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = x[j] * rstd;
      if constexpr (DW) {
        const float v = g[j] * rnd_as<AT>(xh);
        aq[j] += isq ? v : 0.f;
        ak[j] += isq ? 0.f : v;
      }
      g[j] = g[j] * (isq ? fwq[j] : fwk[j]);
      dot = __builtin_fmaf(g[j], xh, dot);
      x[j] = xh;
    }
    dot = row16_sum(dot) / 128.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = rstd * __builtin_fmaf(-x[j], dot, g[j]);
    st8(p, g);
  }
  if constexpr (DW) {
    // the four rows of a wave, then the four waves through LDS, always in the same order
    __shared__ float red[4][256];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      aq[j] += __shfl_xor(aq[j], 16, 64); aq[j] += __shfl_xor(aq[j], 32, 64);
      ak[j] += __shfl_xor(ak[j], 16, 64); ak[j] += __shfl_xor(ak[j], 32, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        red[wave][sub * 8 + j] = aq[j];
        red[wave][128 + sub * 8 + j] = ak[j];
      }
    }
    __syncthreads();
    part[(long)blockIdx.x * 256 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// dwq[c] += sum_b part[b][c], dwk[c] += sum_b part[b][128 + c]: one workgroup per column; thread i sums the slices i, i + 256, ... in slice order, then a tree
// over the 256 threads in a fixed order -- the same bits on every run
__global__ __launch_bounds__(256) void head_norm_dw_finish_kernel(const float* __restrict__ part, int nslices, float* __restrict__ dwq, float* __restrict__ dwk) {
  __shared__ float red[256];
  const int c = blockIdx.x, i = threadIdx.x;
  float s = 0.f;
  for (int b = i; b < nslices; b += 256) s += part[(long)b * 256 + c];
  red[i] = s;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (i < o) red[i] += red[i + o];
    __syncthreads();
  }
  if (i == 0) {
    if (c < 128) dwq[c] += red[0];
    else dwk[c - 128] += red[0];
  }
}

// exact r / HK by multiply-high for every r with r * HK < 2^32
inline bool row_magic(long total, int HK, unsigned* magic) {
  if (HK < 2 || total <= 0 || (double)total * HK >= 4294967296.0) return false;
  *magic = (unsigned)((4294967296ULL + (unsigned)HK - 1) / (unsigned)HK);
  return true;
}

}  // namespace

template <typename AT>
int head_norm_fwd(hipStream_t st, AT* qkv, long ld, const AT* wq, const AT* wk, float* rstd, AT* stash, int T, int H, int Hkv, float eps, const int* pos,
                  const float* cosT, const float* sinT) {
  if (T <= 0) return TST_OK;
  const int HK = H + Hkv;
  const long total = (long)T * HK;
  unsigned magic;
  if (H < 1 || Hkv < 1 || (ld & 7) || ld < (long)(H + 2 * Hkv) * 128 || !qkv || !wq || !wk || !rstd || !row_magic(total, HK, &magic)) return TST_EINVAL;
  const bool rope = pos != nullptr;
  if (rope && (!cosT || !sinT)) return TST_EINVAL;
  const long want = (total + 15) / 16;
  const dim3 grid((unsigned)(want < 2048 ? want : 2048));
  if (rope) hipLaunchKernelGGL((head_norm_fwd_kernel<AT, true>), grid, dim3(256), 0, st, qkv, ld, wq, wk, rstd, stash, (unsigned)total, H, HK, magic, eps, pos, cosT, sinT);
  else hipLaunchKernelGGL((head_norm_fwd_kernel<AT, false>), grid, dim3(256), 0, st, qkv, ld, wq, wk, rstd, stash, (unsigned)total, H, HK, magic, eps, pos, cosT, sinT);
  return CHECK_LAUNCH();
}

template <typename AT>
int head_norm_bwd(hipStream_t st, AT* dqkv, long ld, const AT* wq, const AT* wk, const float* rstd, const AT* stash, int T, int H, int Hkv, const int* pos,
                  const float* cosT, const float* sinT, float* dwq, float* dwk, float* ws) {
  if (T <= 0) return TST_OK;
  const int HK = H + Hkv;
  const long total = (long)T * HK;
  unsigned magic;
  if (H < 1 || Hkv < 1 || (ld & 7) || ld < (long)(H + 2 * Hkv) * 128 || !dqkv || !wq || !wk || !rstd || !stash || !row_magic(total, HK, &magic)) return TST_EINVAL;
  const bool rope = pos != nullptr, dw = dwq != nullptr;
  if ((rope && (!cosT || !sinT)) || (dw && (!dwk || !ws))) return TST_EINVAL;
  const long want = (total + 15) / 16;
  const long cap = dw ? HEAD_NORM_WS_FLOATS / 256 : 2048;
  const dim3 grid((unsigned)(want < cap ? want : cap));
#define HN_BWD(R, D) hipLaunchKernelGGL((head_norm_bwd_kernel<AT, R, D>), grid, dim3(256), 0, st, dqkv, ld, wq, wk, rstd, stash, (unsigned)total, H, HK, magic, pos, cosT, sinT, ws)
  if (rope && dw) HN_BWD(true, true);
  else if (rope) HN_BWD(true, false);
  else if (dw) HN_BWD(false, true);
  else HN_BWD(false, false);
#undef HN_BWD
  if (dw) hipLaunchKernelGGL(head_norm_dw_finish_kernel, dim3(256), dim3(256), 0, st, ws, (int)grid.x, dwq, dwk);
  return CHECK_LAUNCH();
}

#define INSTANTIATE(AT)                                                                                                                                   \
  template int head_norm_fwd<AT>(hipStream_t, AT*, long, const AT*, const AT*, float*, AT*, int, int, int, float, const int*, const float*, const float*); \
  template int head_norm_bwd<AT>(hipStream_t, AT*, long, const AT*, const AT*, const float*, const AT*, int, int, int, const int*, const float*,           \
                                 const float*, float*, float*, float*);
INSTANTIATE(bf16_t)
INSTANTIATE(float)
