// HBM-bound kernels of the TsT hot path (K2,K3,K5,K6,K7,K11 of SURVEY.md §2), gfx950 only.
// All traffic is eight elements per lane (16 B of bf16, cdna_hip_programming.md Guideline 13; 32 B of fp32 in strict mode);
// arithmetic in fp32 with a single rounding to the storage type at each tensor boundary (the numerics contract mirrored
// by oracle/ops_np.py). Every kernel exists for AT = bf16_t (product path) and AT = float (fp32 "strict" parity mode).
#include "common.h"
#include "kernels.h"

namespace {

template <typename AT> __device__ __forceinline__ void cp8(AT* dst, const AT* src) {
  if constexpr (sizeof(AT) == 2) {
    *(uint4*)dst = *(const uint4*)src;
  } else {
    *(uint4*)dst = *(const uint4*)src;
    *(uint4*)((char*)dst + 16) = *(const uint4*)((const char*)src + 16);
  }
}



// ---------------- K7 embedding gather: modeling_llama.py:353,381 ----------------
template <typename AT>
__global__ __launch_bounds__(256) void embed_kernel(const int* __restrict__ ids, const AT* __restrict__ E, AT* __restrict__ out,
                                                    int T, int d, int vocab) {
  const int c8n = d >> 3;
  const long total = (long)T * c8n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / c8n), c = (int)(i % c8n);
    int id = ids[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    cp8(out + (long)t * d + c * 8, E + (long)id * d + c * 8);
  }
}

// out[i,:] = in[idx[i],:]   /  out[idx[i],:] = in[i,:]
template <typename AT>
__global__ __launch_bounds__(256) void gather_rows_kernel(const AT* __restrict__ in, const int* __restrict__ idx, AT* __restrict__ out,
                                                          int n, int d, int scatter) {
  const int c8n = d >> 3;
  const long total = (long)n * c8n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = (int)(i / c8n), c = (int)(i % c8n);
    const int s = idx[r];
    if (scatter) cp8(out + (long)s * d + c * 8, in + (long)r * d + c * 8);
    else cp8(out + (long)r * d + c * 8, in + (long)s * d + c * 8);
  }
}

// ---------------- K2 RMSNorm: modeling_llama.py:62-67 ----------------
// y = bf16( w * bf16( x * rsqrt(mean(x^2)+eps) ) ), statistics in fp32; one wave per row.
template <typename AT>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const AT* __restrict__ x, const AT* __restrict__ w, AT* __restrict__ y,
                                                          float* __restrict__ rstd_out, int T, int d, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int lane = threadIdx.x & 63;
  const AT* xr = x + (long)row * d;
  AT* yr = y + (long)row * d;
  float ss = 0.f;
  if (sizeof(AT) == 2 && d <= 4096) {   // (the fp32 strict mode keeps the streaming loops below: its trajectories are pinned to their exact rounding)
    // the row lives in registers between the statistic and the scaling: every chunk is loaded once and all eight loads are in flight together
    // (the streaming loop below waits for each 16-byte load before issuing the next: 23.7 us for 58 MB); same summation order: bit-identical
    // Loads are UNCONDITIONAL (chunks beyond d re-read chunk 0 and are masked by a select): under `if (c < d)` the compiler branches around every
    // load and waits for it inside the branch, which serialises the eight latencies again.
    float f[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512;
      ld8(xr + (c < d ? c : 0), f[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool in = lane * 8 + i * 512 < d;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += in ? f[i][j] * f[i][j] : 0.f;
    }
    ss = wave_sum(ss);
    const float rstd = 1.0f / sqrtf(ss / (float)d + eps);
    if (lane == 0 && rstd_out) rstd_out[row] = rstd;
    float g[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512;
      ld8(w + (c < d ? c : 0), g[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] = g[i][j] * rnd_as<AT>(f[i][j] * rstd);
      if (c < d) st8(yr + c, f[i]);
    }
    return;
  }
  for (int c = lane * 8; c < d; c += 512) {
    float f[8];
    ld8(xr + c, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
  }
  ss = wave_sum(ss);
  const float rstd = 1.0f / sqrtf(ss / (float)d + eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
  for (int c = lane * 8; c < d; c += 512) {
    float f[8], g[8];
    ld8(xr + c, f);
    ld8(w + c, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = g[j] * rnd_as<AT>(f[j] * rstd);
    st8(yr + c, f);
  }
}

// dx = bf16( dres + rstd * (g - xhat * mean(g*xhat)) ),  g = dy*w, xhat = x*rstd   (fp32 inside)
template <typename AT>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const AT* __restrict__ dy, const AT* __restrict__ x, const float* __restrict__ rstd_in,
                                                          const AT* __restrict__ w, const AT* __restrict__ dres, AT* __restrict__ dx,
                                                          int T, int d) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int lane = threadIdx.x & 63;
  const AT* xr = x + (long)row * d;
  const AT* dyr = dy + (long)row * d;
  const float rstd = rstd_in[row];
  float dot = 0.f;
  AT* dxr = dx + (long)row * d;
  if (sizeof(AT) == 2 && d <= 4096) {   // (the fp32 strict mode keeps the streaming loops below: its trajectories are pinned to their exact rounding)
    // x, dy and w of the row are loaded ONCE, all loads in flight together and unconditional (see rmsnorm_fwd_kernel); g = dy * w stays in
    // registers between the row statistic and the output; same summation order as the streaming loop below: bit-identical
    float fx[8][8], fg[8][8], fr[8][8];
    const AT* rr = dres ? dres + (long)row * d : xr;   // no residual gradient: the (cached) x row is read instead and not used
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512, cc = c < d ? c : 0;
      ld8(xr + cc, fx[i]);
      ld8(dyr + cc, fg[i]);
      ld8(rr + cc, fr[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512;
      const bool in = c < d;
      float fw[8];
      ld8(w + (in ? c : 0), fw);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        fg[i][j] = fg[i][j] * fw[j];
        dot += in ? fg[i][j] * (fx[i][j] * rstd) : 0.f;
      }
    }
    dot = wave_sum(dot) / (float)d;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane * 8 + i * 512;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = rstd * (fg[i][j] - (fx[i][j] * rstd) * dot);
        if (dres) v += fr[i][j];
        fx[i][j] = v;
      }
      if (c < d) st8(dxr + c, fx[i]);
    }
    return;
  }
  for (int c = lane * 8; c < d; c += 512) {
    float fx[8], fd[8], fw[8];
    ld8(xr + c, fx);
    ld8(dyr + c, fd);
    ld8(w + c, fw);
#pragma unroll
    for (int j = 0; j < 8; ++j) dot += fd[j] * fw[j] * (fx[j] * rstd);
  }
  dot = wave_sum(dot) / (float)d;
  for (int c = lane * 8; c < d; c += 512) {
    float fx[8], fd[8], fw[8], fr[8];
    ld8(xr + c, fx);
    ld8(dyr + c, fd);
    ld8(w + c, fw);
    if (dres) ld8(dres + (long)row * d + c, fr);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = rstd * (fd[j] * fw[j] - (fx[j] * rstd) * dot);
      if (dres) v += fr[j];
      fx[j] = v;
    }
    st8(dxr + c, fx);
  }
}

// Column reductions of the full fine-tune (norm-weight and bias gradients) are two launches and NO atomics, so a full fine-tune is reproducible
// bit for bit: every block writes the sum of its slice of rows to part[blockIdx.y][c]; colred_finish_kernel adds the slices in slice order.
__global__ __launch_bounds__(256) void colred_finish_kernel(const float* __restrict__ part, int nslices, int n, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int b = 0; b < nslices; ++b) s += part[(long)b * n + c];
  out[c] += s;
}
// part[slice][c] = sum_{t in slice} dy[t,c] * bf16(x[t,c]*rstd[t])  (full fine-tune only)
template <typename AT>
__global__ __launch_bounds__(256) void rmsnorm_dw_kernel(const AT* __restrict__ dy, const AT* __restrict__ x, const float* __restrict__ rstd_in,
                                                         float* __restrict__ dw, int T, int d, int rows_per_block) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  const int t0 = blockIdx.y * rows_per_block;
  const int t1 = min(T, t0 + rows_per_block);
  float s = 0.f;
  for (int t = t0; t < t1; ++t) s += ld1(&dy[(long)t * d + c]) * rnd_as<AT>(ld1(&x[(long)t * d + c]) * rstd_in[t]);
  dw[(long)blockIdx.y * d + c] = s;
}

// ---------------- LayerNorm (GPT-2 family): modeling_gpt2.py:252-254,497 = torch F.layer_norm ----------------
// y = bf16( (x - mean) * rstd * w + b ), biased variance, fp32 statistics, ONE rounding; one wave per row.
// stats[2*row] = mean, stats[2*row+1] = rstd.
template <typename AT>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const AT* __restrict__ x, const AT* __restrict__ w, const AT* __restrict__ b,
                                                            AT* __restrict__ y, float* __restrict__ stats, int T, int d, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int lane = threadIdx.x & 63;
  const AT* xr = x + (long)row * d;
  float s = 0.f;
  for (int c = lane * 8; c < d; c += 512) {
    float f[8];
    ld8(xr + c, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += f[j];
  }
  const float mean = wave_sum(s) / (float)d;
  float ss = 0.f;
  for (int c = lane * 8; c < d; c += 512) {
    float f[8];
    ld8(xr + c, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (f[j] - mean) * (f[j] - mean);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)d + eps);
  if (lane == 0 && stats) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  AT* yr = y + (long)row * d;
  for (int c = lane * 8; c < d; c += 512) {
    float f[8], g[8], h[8];
    ld8(xr + c, f);
    ld8(w + c, g);
    ld8(b + c, h);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (f[j] - mean) * rstd * g[j] + h[j];
    st8(yr + c, f);
  }
}

// dx = bf16( dres + rstd * (g - mean(g) - xhat * mean(g*xhat)) ),  g = dy*w, xhat = (x-mean)*rstd
template <typename AT>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const AT* __restrict__ dy, const AT* __restrict__ x, const float* __restrict__ stats,
                                                            const AT* __restrict__ w, const AT* __restrict__ dres, AT* __restrict__ dx,
                                                            int T, int d) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int lane = threadIdx.x & 63;
  const AT* xr = x + (long)row * d;
  const AT* dyr = dy + (long)row * d;
  const float mean = stats[2 * row], rstd = stats[2 * row + 1];
  float sg = 0.f, sgx = 0.f;
  for (int c = lane * 8; c < d; c += 512) {
    float fx[8], fd[8], fw[8];
    ld8(xr + c, fx);
    ld8(dyr + c, fd);
    ld8(w + c, fw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = fd[j] * fw[j];
      sg += g;
      sgx += g * ((fx[j] - mean) * rstd);
    }
  }
  sg = wave_sum(sg) / (float)d;
  sgx = wave_sum(sgx) / (float)d;
  AT* dxr = dx + (long)row * d;
  for (int c = lane * 8; c < d; c += 512) {
    float fx[8], fd[8], fw[8], fr[8];
    ld8(xr + c, fx);
    ld8(dyr + c, fd);
    ld8(w + c, fw);
    if (dres) ld8(dres + (long)row * d + c, fr);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = rstd * (fd[j] * fw[j] - sg - ((fx[j] - mean) * rstd) * sgx);
      if (dres) v += fr[j];
      fx[j] = v;
    }
    st8(dxr + c, fx);
  }
}

// slice sums of dw[c] = sum_t dy[t,c] * xhat[t,c] and db[c] = sum_t dy[t,c]  (full fine-tune only; dw / db here = the two partial buffers)
template <typename AT>
__global__ __launch_bounds__(256) void layernorm_dwdb_kernel(const AT* __restrict__ dy, const AT* __restrict__ x, const float* __restrict__ stats,
                                                             float* __restrict__ dw, float* __restrict__ db, int T, int d, int rows_per_block) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  const int t0 = blockIdx.y * rows_per_block;
  const int t1 = min(T, t0 + rows_per_block);
  float s = 0.f, sb = 0.f;
  for (int t = t0; t < t1; ++t) {
    const float g = ld1(&dy[(long)t * d + c]);
    s += g * ((ld1(&x[(long)t * d + c]) - stats[2 * t]) * stats[2 * t + 1]);
    sb += g;
  }
  dw[(long)blockIdx.y * d + c] = s;
  db[(long)blockIdx.y * d + c] = sb;
}

// ---------------- gelu_new (GPT-2 MLP): HF/activations.py:65-66 ----------------
__device__ __forceinline__ float gelu_tanh_arg(float x) { return 0.7978845608028654f * (x + 0.044715f * x * x * x); }
template <typename AT>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const AT* __restrict__ x, AT* __restrict__ y, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float f[8];
    ld8(x + i * 8, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = 0.5f * f[j] * (1.0f + tanhf(gelu_tanh_arg(f[j])));
    st8(y + i * 8, f);
  }
}
template <typename AT>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const AT* __restrict__ dy, const AT* __restrict__ x, AT* __restrict__ dx, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float f[8], g[8];
    ld8(x + i * 8, f);
    ld8(dy + i * 8, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = tanhf(gelu_tanh_arg(f[j]));
      f[j] = g[j] * (0.5f * (1.0f + t) + 0.5f * f[j] * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * f[j] * f[j]));
    }
    st8(dx + i * 8, f);
  }
}

// ---------------- token + learned position embedding (GPT-2): modeling_gpt2.py:569-577 ----------------
template <typename AT>
__global__ __launch_bounds__(256) void embed_pos_kernel(const int* __restrict__ ids, const int* __restrict__ pos, const AT* __restrict__ E,
                                                        const AT* __restrict__ P, AT* __restrict__ out, int T, int d, int vocab, int npos) {
  const int c8n = d >> 3;
  const long total = (long)T * c8n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / c8n), c = (int)(i % c8n);
    int id = ids[t], p = pos[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    p = p < 0 ? 0 : (p >= npos ? npos - 1 : p);
    float a[8], b[8];
    ld8(E + (long)id * d + c * 8, a);
    ld8(P + (long)p * d + c * 8, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += b[j];
    st8(out + (long)t * d + c * 8, a);
  }
}

// ---------------- K3 RoPE (half-split rotate_half): modeling_llama.py:122-160 ----------------
// In place on the packed [T, (H+2*Hkv)*dh] projection buffer; q and k heads only. cos/sin tables are
// [max_pos, dh/2] fp32 already rounded to bf16 precision (HF casts cos/sin to the activation dtype, :108).
// sign=+1 forward, -1 backward (transpose of the rotation).
template <typename AT>
__global__ __launch_bounds__(256) void rope_kernel(AT* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ cosT,
                                                   const float* __restrict__ sinT, int T, int nheads_rot, int dh, long ld, float sign) {
  const int half = dh >> 1;
  const int c8n = half >> 3;
  const long total = (long)T * nheads_rot * c8n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % c8n);
    const int h = (int)((i / c8n) % nheads_rot);
    const int t = (int)(i / ((long)c8n * nheads_rot));
    AT* p = qkv + (long)t * ld + (long)h * dh + c * 8;
    const float* cs = cosT + (long)pos[t] * half + c * 8;
    const float* sn = sinT + (long)pos[t] * half + c * 8;
    float a[8], b[8];
    ld8(p, a);
    ld8(p + half, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float co = cs[j], si = sn[j] * sign;
      const float o1 = a[j] * co - b[j] * si;
      const float o2 = b[j] * co + a[j] * si;
      a[j] = o1; b[j] = o2;
    }
    st8(p, a);
    st8(p + half, b);
  }
}

// ---------------- K5 SwiGLU: modeling_llama.py:175, activations.py (silu) ----------------
// grid (column chunks of 256 x 8 elements, row slices): a thread keeps its 8 columns and walks rows blockIdx.y, + gridDim.y, ... -- no index division (the flat
// 64-bit i / c8n, i % c8n of the first form cost more VALU instructions than the arithmetic, which is what these kernels are short of beside the projection
// tiles of the other stream)
template <typename AT>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const AT* __restrict__ gu, AT* __restrict__ act, int T, int F) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (F >> 3)) return;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    float g[8], u[8];
    ld8(gu + (long)t * 2 * F + c * 8, g);
    ld8(gu + (long)t * 2 * F + F + c * 8, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = swiglu_of<AT>(g[j], u[j]);
    st8(act + (long)t * F + c * 8, g);
  }
}
template <typename AT>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const AT* __restrict__ dact, const AT* __restrict__ gu, AT* __restrict__ dgu, int T, int F) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (F >> 3)) return;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    float g[8], u[8], da[8], dg[8], du[8];
    ld8(gu + (long)t * 2 * F + c * 8, g);
    ld8(gu + (long)t * 2 * F + F + c * 8, u);
    ld8(dact + (long)t * F + c * 8, da);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sg = sigmoid_of<AT>(g[j]);
      dg[j] = da[j] * u[j] * sg * (1.0f + g[j] * (1.0f - sg));
      du[j] = da[j] * g[j] * sg;
    }
    st8(dgu + (long)t * 2 * F + c * 8, dg);
    st8(dgu + (long)t * 2 * F + F + c * 8, du);
  }
}

// ---------------- K6 / K11 fp32-logit row statistics, cross-entropy and d(logits) ----------------
// loss_utils.py:39-46,59-70: CE over rows whose label != -100, sum / num_items_in_batch (rows are already the
// labelled rows; target[r] is the shifted label). One workgroup per row.
//   stats[r] = {lse, logit[target], argmax (as float bits of int), max}
//   dlogits[r,:] = (softmax - onehot) * inv_items   (bf16), if dlogits != nullptr
//   optl[r, j]  = logit[r, opt_ids[j]]              if opt_ids != nullptr  (restricted-softmax s(x))
template <typename AT>
__global__ __launch_bounds__(256) void logit_rows_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ target, int V,
                                                         float* __restrict__ stats, AT* __restrict__ dlogits, long ldd, float inv_items,
                                                         const int* __restrict__ opt_ids, int n_opt, float* __restrict__ optl) {
  __shared__ float red[4];
  __shared__ int redi[4];
  const int r = blockIdx.x;
  const float* lr = logits + (long)r * ld;
  const int tid = threadIdx.x;
  float m = -INFINITY;
  int am = 0;
  for (int c = tid * 4; c < V; c += 1024) {
    const f32x4 v = *(const f32x4*)(lr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < V && v[j] > m) { m = v[j]; am = c + j; }   // V need not be a multiple of 4 (GPT-2: 50257); ld is
  }
  // block argmax (first index of the maximum, as torch.argmax on CPU)
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  if ((tid & 63) == 0) { red[tid >> 6] = m; redi[tid >> 6] = am; }
  __syncthreads();
  float bm = red[0]; int ba = redi[0];
  for (int w = 1; w < 4; ++w)
    if (red[w] > bm || (red[w] == bm && redi[w] < ba)) { bm = red[w]; ba = redi[w]; }
  __syncthreads();
  float s = 0.f;
  for (int c = tid * 4; c < V; c += 1024) {
    const f32x4 v = *(const f32x4*)(lr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (c + j < V) ? expf(v[j] - bm) : 0.f;
  }
  s = block_sum_256(s, red);
  const float lse = bm + logf(s);
  const int tg = target[r];
  if (tid == 0) {
    stats[r * 4 + 0] = lse;
    stats[r * 4 + 1] = lr[tg];
    stats[r * 4 + 2] = __int_as_float(ba);
    stats[r * 4 + 3] = bm;
  }
  if (opt_ids && tid < n_opt) optl[(long)r * n_opt + tid] = lr[opt_ids[tid]];
  if (dlogits) {
    AT* dr = dlogits + (long)r * ldd;
    for (int c = tid * 4; c < V; c += 1024) {
      const f32x4 v = *(const f32x4*)(lr + c);
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = expf(v[j] - lse);
        if (c + j == tg) pj -= 1.0f;
        o[j] = (c + j < V) ? pj * inv_items : 0.f;
      }
      st4(dr + c, o);
    }
  }
}

// loss = sum_r (lse - logit[target]) * inv_items  (single workgroup, fixed order => bitwise reproducible)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ stats, int n, float inv_items, float* __restrict__ loss_out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) s += stats[r * 4 + 0] - stats[r * 4 + 1];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) loss_out[0] = s * inv_items;
}

// embedding backward (full fine-tune): dE[ids[t], :] += dx[t, :]. A token id may repeat in a batch, so the rows of one id are added by ONE
// workgroup per column slice, in token order (no atomics: reproducible): workgroup (t, s) does nothing unless t is the first occurrence of its id; then it takes
// its 4 columns per thread of dE[id] into registers, walks the later positions 1024 at a time (the four waves' ballots meet in LDS), adds every matching row -- up to four
// rows' loads in flight, added in token order -- and stores once. The same sums in the same order as a read-modify-write per row, without the dependent
// load -> add -> store chain through memory that made a frequent id (a prompt template's tokens) a serial tail of one workgroup: the bench's 1185-token
// micro-batch with Zipf-distributed ids took the old form 230 us, this one 38 us; 16384 tokens with one id on a quarter of them 9.6 ms against 1.5 ms
// (profiles/r05_embed_bwd_skewed_ids.txt; with all-distinct ids both forms are bound by every workgroup's scan of the id vector: 13 / 18 us and 0.7 / 1.6 ms).
template <typename AT>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int* __restrict__ ids, const AT* __restrict__ dx, float* __restrict__ dE,
                                                        int T, int d, int vocab) {
  __shared__ unsigned long long masks[2][16];     // the 16 ballots of a 1024-position step, double-buffered (one barrier per step)
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto clampid = [&](int id) { return id < 0 ? 0 : (id >= vocab ? vocab - 1 : id); };
  const int id = clampid(ids[t]);
  // first occurrence? all 256 threads look at the earlier positions, 1024 per step (four independent loads per thread)
  int hit = 0;
  for (int base = 0; base < t; base += 1024) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + 256 * u + tid;
      hit |= (j < t && clampid(ids[j]) == id) ? 1 : 0;
    }
  }
  if (__syncthreads_or(hit)) return;
  const int c0 = blockIdx.y * 1024 + tid * 4;
  const bool live = c0 < d;                       // d % 4 == 0 (host check)
  float* __restrict__ row = dE + (long)id * d + (live ? c0 : 0);
  const AT* __restrict__ col = dx + (live ? c0 : 0);
  f32x4 acc = live ? *(const f32x4*)row : f32x4{0.f, 0.f, 0.f, 0.f};
  int buf = 0;
  for (int base = t; base < T; base += 1024, buf ^= 1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {                 // 64-position chunk 4u + w of this step
      const int j = base + 256 * u + tid;
      const unsigned long long m = __ballot(j < T && clampid(ids[j]) == id);
      if (lane == 0) masks[buf][4 * u + w] = m;
    }
    __syncthreads();
    for (int c = 0; c < 16; ++c) {
      const unsigned long long mv = masks[buf][c];
      unsigned long long hits = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mv >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)(mv & 0xffffffffull));
      const int cb = base + 64 * c;
      while (hits) {   // workgroup-uniform: up to four rows per trip, loaded together, added in token order
        int tt[4];
        float x[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          tt[u] = hits ? cb + __builtin_ctzll(hits) : -1;
          hits &= hits - 1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (tt[u] >= 0 && live) ld4(col + (long)tt[u] * d, x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (tt[u] >= 0 && live) { acc[0] += x[u][0]; acc[1] += x[u][1]; acc[2] += x[u][2]; acc[3] += x[u][3]; }
      }
    }
  }
  if (live) *(f32x4*)row = acc;
}
// the read-modify-write form of rounds 4 (TST_EMBED_BWD=0: the 'before' arm of the timing record)
template <typename AT>
__global__ __launch_bounds__(256) void embed_bwd_rmw_kernel(const int* __restrict__ ids, const AT* __restrict__ dx, float* __restrict__ dE,
                                                            int T, int d, int vocab) {
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  auto clampid = [&](int id) { return id < 0 ? 0 : (id >= vocab ? vocab - 1 : id); };
  const int id = clampid(ids[t]);
  for (int base = 0; base < t; base += 64) {
    const int j = base + lane;
    if (__ballot(j < t && clampid(ids[j]) == id)) return;
  }
  float* __restrict__ row = dE + (long)id * d;
  for (int base = t; base < T; base += 64) {
    const int j = base + lane;
    unsigned long long hits = __ballot(j < T && clampid(ids[j]) == id);
    while (hits) {
      const int tt = base + __builtin_ctzll(hits);
      hits &= hits - 1;
      for (int c = threadIdx.x; c < d; c += 256) row[c] += ld1(&dx[(long)tt * d + c]);
    }
  }
}
template <typename AT>
__global__ __launch_bounds__(256) void cast_to_f32_kernel(const AT* __restrict__ in, float* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = ld1(in + i);
}

// bias gradient (full fine-tune, Qwen2 q/k/v bias): slice sums of out[c] = sum_t x[t,c]
template <typename AT>
__global__ __launch_bounds__(256) void colsum_kernel(const AT* __restrict__ x, long ld, float* __restrict__ out, int T, int n, int rows_per_block) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int t0 = blockIdx.y * rows_per_block, t1 = min(T, t0 + rows_per_block);
  float s = 0.f;
  for (int t = t0; t < t1; ++t) s += ld1(&x[(long)t * ld + c]);
  out[(long)blockIdx.y * n + c] = s;
}

// ---------------- misc ----------------
template <typename AT>
__global__ __launch_bounds__(256) void cast_from_f32_kernel(const float* __restrict__ in, AT* __restrict__ out, long n, float scale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) st1(out + i, in[i] * scale);
}

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// N(0, std^2) bf16 fill, counter-based (Box-Muller on two hashed uniforms): weights for the synthetic benchmark.
// (strict mode stores the SAME bf16-representable values as fp32, so both precisions start from identical weights)
template <typename AT>
__global__ __launch_bounds__(256) void randn_kernel(AT* __restrict__ out, long n, unsigned seed, float stdv) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const unsigned lo = (unsigned)i, hi = (unsigned)(i >> 32);
    const unsigned a = hash32(lo ^ hash32(hi + 0x9e3779b9U) ^ seed);
    const unsigned b = hash32(a ^ 0x85ebca6bU ^ (seed * 0x27d4eb2fU + 1U));
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530718f * u2);
    st1(out + i, bf2f(f2bf(z * stdv)));
  }
}
// lora_A of one module at a fold's reset: U(-bound, bound); element i is draw i of the splitmix64 stream that starts at state0. A draw only adds the
// stream's constant to the state, so draw i is a function of i: the same values, bit for bit, as the serial host loop this replaces (21 M draws per fold)
__global__ __launch_bounds__(256) void lora_a_init_kernel(float* __restrict__ out, long n, unsigned long long state0, float bound) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    unsigned long long z = state0 + (unsigned long long)(i + 1) * 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    const float u = (float)((double)(z >> 40) + 0.5) * (1.0f / 16777216.0f);   // (0, 1)
    out[i] = (2.0f * u - 1.0f) * bound;
  }
}
template <typename AT>
__global__ __launch_bounds__(256) void fill_kernel(AT* __restrict__ out, long n, float v) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) st1(out + i, v);
}

// stacked folds: the adapter rank axis holds one block of `width` columns per slot; a token keeps its own slot's block only
// (u = x.Ag^T and du = dy.Bg are computed for every slot's adapters at once, this zeroes the cross-fold terms)
__global__ __launch_bounds__(256) void rank_mask_kernel(bf16_t* __restrict__ u, int ld, int T, int width, int nslot, SlotEnds ends) {
  const int per_row = ld >> 3;   // 16-byte pieces per row
  const long total = (long)T * per_row;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / per_row), c = (int)(i % per_row) << 3;
    int slot = 0;
#pragma unroll
    for (int s = 0; s < TST_MAX_STACK - 1; ++s) slot += (s < nslot - 1 && t >= ends.t_end[s]) ? 1 : 0;
    if (c / width != slot) *(uint4*)(u + (long)t * ld + c) = make_uint4(0u, 0u, 0u, 0u);
  }
}

inline int nblocks(long work, int cap = 2048) {
  long b = (work + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP)

}  // namespace

template <typename AT> int embed_fwd(hipStream_t st, const int* ids, const AT* E, AT* out, int T, int d, int vocab) {
  if (d & 7) return TST_EINVAL;
  hipLaunchKernelGGL(embed_kernel<AT>, dim3(nblocks((long)T * (d / 8))), dim3(256), 0, st, ids, E, out, T, d, vocab);
  return CHECK_LAUNCH();
}
template <typename AT> int embed_bwd(hipStream_t st, const int* ids, const AT* dx, float* dE, int T, int d, int vocab) {
  if (T <= 0) return TST_OK;
  static const bool rmw = [] { const char* e = getenv("TST_EMBED_BWD"); return e && atoi(e) == 0; }();
  if (rmw || (d & 3)) hipLaunchKernelGGL(embed_bwd_rmw_kernel<AT>, dim3((unsigned)T), dim3(256), 0, st, ids, dx, dE, T, d, vocab);
  else hipLaunchKernelGGL(embed_bwd_kernel<AT>, dim3((unsigned)T, (unsigned)((d + 1023) / 1024)), dim3(256), 0, st, ids, dx, dE, T, d, vocab);
  return CHECK_LAUNCH();
}
// ws: colred_ws_floats(T, n) floats of scratch for the slice sums (ordered behind earlier users by the stream)
template <typename AT> int colsum(hipStream_t st, const AT* x, long ld, float* out, int T, int n, float* ws) {
  if (T <= 0) return TST_OK;
  if (!ws) return TST_EINVAL;
  const int ns = (T + 63) / 64;
  hipLaunchKernelGGL(colsum_kernel<AT>, dim3((n + 255) / 256, ns), dim3(256), 0, st, x, ld, ws, T, n, 64);
  hipLaunchKernelGGL(colred_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws, ns, n, out);
  return CHECK_LAUNCH();
}
long colred_ws_floats(int T, int n) { return (long)((T + 7) / 8) * n; }   // (slices of 8 rows: rmsnorm_bwd_dw; the 64-row slices of the other reductions use a part of it)
template <typename AT> int cast_to_f32(hipStream_t st, const AT* in, float* out, long n) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(cast_to_f32_kernel<AT>, dim3(nblocks(n, 8192)), dim3(256), 0, st, in, out, n);
  return CHECK_LAUNCH();
}
template <typename AT> int gather_rows(hipStream_t st, const AT* in, const int* idx, AT* out, int n, int d, int scatter) {
  if (d & 7) return TST_EINVAL;
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(gather_rows_kernel<AT>, dim3(nblocks((long)n * (d / 8))), dim3(256), 0, st, in, idx, out, n, d, scatter);
  return CHECK_LAUNCH();
}
template <typename AT> int rmsnorm_fwd(hipStream_t st, const AT* x, const AT* w, AT* y, float* rstd, int T, int d, float eps) {
  if (d & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  if constexpr (sizeof(AT) == 2) {
    // the widths norm_rank.hip is built for go through ITS kernel (16 rows per workgroup, the tile in registers), with or without a rank block attached: one
    // definition of the row statistic's summation order, so the fused and the unfused form agree bit for bit. TST_NORM_TILE=0: the wave-per-row kernel below (A/B)
    static const bool tile_env = [] { const char* e = getenv("TST_NORM_TILE"); return !e || atoi(e) != 0; }();
    if (tile_env && rmsnorm_rank_width_ok(d)) return rmsnorm_rank_fwd(st, x, w, y, rstd, T, d, eps, nullptr);
  }
  hipLaunchKernelGGL(rmsnorm_fwd_kernel<AT>, dim3((T + 3) / 4), dim3(256), 0, st, x, w, y, rstd, T, d, eps);
  return CHECK_LAUNCH();
}
template <typename AT> int rmsnorm_bwd(hipStream_t st, const AT* dy, const AT* x, const float* rstd, const AT* w, const AT* dres, AT* dx, int T, int d) {
  if (d & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(rmsnorm_bwd_kernel<AT>, dim3((T + 3) / 4), dim3(256), 0, st, dy, x, rstd, w, dres, dx, T, d);
  return CHECK_LAUNCH();
}
template <typename AT> int rmsnorm_dw(hipStream_t st, const AT* dy, const AT* x, const float* rstd, float* dw, int T, int d, float* ws) {
  if (T <= 0) return TST_OK;
  if (!ws) return TST_EINVAL;
  const int rpb = 64, ns = (T + rpb - 1) / rpb;
  hipLaunchKernelGGL(rmsnorm_dw_kernel<AT>, dim3((d + 255) / 256, ns), dim3(256), 0, st, dy, x, rstd, ws, T, d, rpb);
  hipLaunchKernelGGL(colred_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, ws, ns, d, dw);
  return CHECK_LAUNCH();
}
template <typename AT> int layernorm_fwd(hipStream_t st, const AT* x, const AT* w, const AT* b, AT* y, float* stats, int T, int d, float eps) {
  if (d & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(layernorm_fwd_kernel<AT>, dim3((T + 3) / 4), dim3(256), 0, st, x, w, b, y, stats, T, d, eps);
  return CHECK_LAUNCH();
}
template <typename AT> int layernorm_bwd(hipStream_t st, const AT* dy, const AT* x, const float* stats, const AT* w, const AT* dres, AT* dx, int T, int d) {
  if (d & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(layernorm_bwd_kernel<AT>, dim3((T + 3) / 4), dim3(256), 0, st, dy, x, stats, w, dres, dx, T, d);
  return CHECK_LAUNCH();
}
template <typename AT> int layernorm_dwdb(hipStream_t st, const AT* dy, const AT* x, const float* stats, float* dw, float* db, int T, int d, float* ws) {
  if (T <= 0) return TST_OK;
  if (!ws) return TST_EINVAL;
  const int rpb = 64, ns = (T + rpb - 1) / rpb;
  float* ws_b = ws + (long)ns * d;   // (2 * colred_ws_floats(T, d))
  hipLaunchKernelGGL(layernorm_dwdb_kernel<AT>, dim3((d + 255) / 256, ns), dim3(256), 0, st, dy, x, stats, ws, ws_b, T, d, rpb);
  hipLaunchKernelGGL(colred_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, ws, ns, d, dw);
  hipLaunchKernelGGL(colred_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, ws_b, ns, d, db);
  return CHECK_LAUNCH();
}
template <typename AT> int gelu_fwd(hipStream_t st, const AT* x, AT* y, long n) {
  if (n & 7) return TST_EINVAL;
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(gelu_fwd_kernel<AT>, dim3(nblocks(n / 8, 4096)), dim3(256), 0, st, x, y, n / 8);
  return CHECK_LAUNCH();
}
template <typename AT> int gelu_bwd(hipStream_t st, const AT* dy, const AT* x, AT* dx, long n) {
  if (n & 7) return TST_EINVAL;
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(gelu_bwd_kernel<AT>, dim3(nblocks(n / 8, 4096)), dim3(256), 0, st, dy, x, dx, n / 8);
  return CHECK_LAUNCH();
}
template <typename AT> int embed_pos_fwd(hipStream_t st, const int* ids, const int* pos, const AT* E, const AT* P, AT* out, int T, int d, int vocab, int npos) {
  if (d & 7) return TST_EINVAL;
  hipLaunchKernelGGL(embed_pos_kernel<AT>, dim3(nblocks((long)T * (d / 8))), dim3(256), 0, st, ids, pos, E, P, out, T, d, vocab, npos);
  return CHECK_LAUNCH();
}
template <typename AT> int rope_apply(hipStream_t st, AT* qkv, const int* pos, const float* cosT, const float* sinT, int T, int nheads_rot, int dh, long ld, int backward) {
  if ((dh & 15) || (ld & 7)) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(rope_kernel<AT>, dim3(nblocks((long)T * nheads_rot * (dh / 16))), dim3(256), 0, st, qkv, pos, cosT, sinT, T, nheads_rot, dh, ld,
                     backward ? -1.0f : 1.0f);
  return CHECK_LAUNCH();
}
// column chunks x row slices: about 4096 workgroups, every thread 1 .. T / slices rows
static dim3 swiglu_grid(int T, int F) {
  const int gx = ((F >> 3) + 255) / 256;
  int gy = 4096 / gx;
  if (gy < 1) gy = 1;
  if (gy > T) gy = T;
  return dim3(gx, gy);
}
template <typename AT> int swiglu_fwd(hipStream_t st, const AT* gu, AT* act, int T, int F) {
  if (F & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(swiglu_fwd_kernel<AT>, swiglu_grid(T, F), dim3(256), 0, st, gu, act, T, F);
  return CHECK_LAUNCH();
}
template <typename AT> int swiglu_bwd(hipStream_t st, const AT* dact, const AT* gu, AT* dgu, int T, int F) {
  if (F & 7) return TST_EINVAL;
  if (T <= 0) return TST_OK;
  hipLaunchKernelGGL(swiglu_bwd_kernel<AT>, swiglu_grid(T, F), dim3(256), 0, st, dact, gu, dgu, T, F);
  return CHECK_LAUNCH();
}
template <typename AT> int logit_rows(hipStream_t st, const float* logits, long ld, const int* target, int n_rows, int V, float* stats, AT* dlogits, long ldd,
                                      float inv_items, const int* opt_ids, int n_opt, float* optl) {
  if ((ld & 3) || ld < ((V + 3) & ~3) || (dlogits && ((ldd & 3) || ldd < ((V + 3) & ~3))) || n_opt > 256) return TST_EINVAL;
  if (n_rows <= 0) return TST_OK;
  hipLaunchKernelGGL(logit_rows_kernel<AT>, dim3(n_rows), dim3(256), 0, st, logits, ld, target, V, stats, dlogits, ldd, inv_items, opt_ids, n_opt, optl);
  return CHECK_LAUNCH();
}
// token ids that arrive as a DEVICE pointer (TST_BATCH_DEVICE_IDS) cannot be checked on the host: one pass sets *flag when an id lies
// outside [0, vocab) (the embedding kernels clamp, so nothing faults; the step's result is reported as invalid at the next fetch)
__global__ __launch_bounds__(256) void ids_check_kernel(const int* __restrict__ ids, int T, int vocab, int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < T && (ids[i] < 0 || ids[i] >= vocab)) *flag = 1;
}
// the device-side batch of a TST_BATCH_DEVICE_IDS call when it is not the caller's token for token (trim_last_token): ids[i] holds the SOURCE index of
// device token i on entry and its id on exit (src is checked as a whole by ids_check first, so the index is the only thing trusted here)
__global__ __launch_bounds__(256) void ids_gather_kernel(const int* __restrict__ src, int* __restrict__ ids, int n, int n_src) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int j = ids[i];
    ids[i] = (j >= 0 && j < n_src) ? src[j] : 0;
  }
}
int ids_gather(hipStream_t st, const int* src, int* ids, int n, int n_src) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(ids_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, ids, n, n_src);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}
int ids_check(hipStream_t st, const int* ids, int T, int vocab, int* flag) {
  hipLaunchKernelGGL(ids_check_kernel, dim3((T + 255) / 256), dim3(256), 0, st, ids, T, vocab, flag);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

int loss_reduce(hipStream_t st, const float* stats, int n, float inv_items, float* loss_out) {
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, st, stats, n, inv_items, loss_out);
  return CHECK_LAUNCH();
}
template <typename AT> int cast_from_f32(hipStream_t st, const float* in, AT* out, long n, float scale) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(cast_from_f32_kernel<AT>, dim3(nblocks(n)), dim3(256), 0, st, in, out, n, scale);
  return CHECK_LAUNCH();
}
template <typename AT> int randn_fill(hipStream_t st, AT* out, long n, unsigned seed, float stdv) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(randn_kernel<AT>, dim3(nblocks(n, 8192)), dim3(256), 0, st, out, n, seed, stdv);
  return CHECK_LAUNCH();
}
int rank_mask(hipStream_t st, bf16_t* u, int ld, int T, int width, int nslot, SlotEnds ends) {
  if ((ld & 7) || (width & 7) || width <= 0 || nslot < 1 || nslot > TST_MAX_STACK) return TST_EINVAL;
  if (T <= 0 || nslot == 1) return TST_OK;
  hipLaunchKernelGGL(rank_mask_kernel, dim3(nblocks((long)T * (ld >> 3), 4096)), dim3(256), 0, st, u, ld, T, width, nslot, ends);
  return CHECK_LAUNCH();
}
int lora_a_init(hipStream_t st, float* out, long n, unsigned long long state0, float bound) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(lora_a_init_kernel, dim3(nblocks(n, 1024)), dim3(256), 0, st, out, n, state0, bound);
  return CHECK_LAUNCH();
}
template <typename AT> int fill_const(hipStream_t st, AT* out, long n, float v) {
  if (n <= 0) return TST_OK;
  hipLaunchKernelGGL(fill_kernel<AT>, dim3(nblocks(n, 8192)), dim3(256), 0, st, out, n, v);
  return CHECK_LAUNCH();
}

// both precisions of every launcher
#define TST_INST(AT)                                                                                                                        \
  template int embed_fwd<AT>(hipStream_t, const int*, const AT*, AT*, int, int, int);                                                       \
  template int embed_bwd<AT>(hipStream_t, const int*, const AT*, float*, int, int, int);                                                    \
  template int colsum<AT>(hipStream_t, const AT*, long, float*, int, int, float*);                                                                \
  template int cast_to_f32<AT>(hipStream_t, const AT*, float*, long);                                                                       \
  template int gather_rows<AT>(hipStream_t, const AT*, const int*, AT*, int, int, int);                                                     \
  template int rmsnorm_fwd<AT>(hipStream_t, const AT*, const AT*, AT*, float*, int, int, float);                                            \
  template int rmsnorm_bwd<AT>(hipStream_t, const AT*, const AT*, const float*, const AT*, const AT*, AT*, int, int);                       \
  template int rmsnorm_dw<AT>(hipStream_t, const AT*, const AT*, const float*, float*, int, int, float*);                                         \
  template int layernorm_fwd<AT>(hipStream_t, const AT*, const AT*, const AT*, AT*, float*, int, int, float);                               \
  template int layernorm_bwd<AT>(hipStream_t, const AT*, const AT*, const float*, const AT*, const AT*, AT*, int, int);                     \
  template int layernorm_dwdb<AT>(hipStream_t, const AT*, const AT*, const float*, float*, float*, int, int, float*);                             \
  template int gelu_fwd<AT>(hipStream_t, const AT*, AT*, long);                                                                             \
  template int gelu_bwd<AT>(hipStream_t, const AT*, const AT*, AT*, long);                                                                  \
  template int embed_pos_fwd<AT>(hipStream_t, const int*, const int*, const AT*, const AT*, AT*, int, int, int, int);                       \
  template int rope_apply<AT>(hipStream_t, AT*, const int*, const float*, const float*, int, int, int, long, int);                          \
  template int swiglu_fwd<AT>(hipStream_t, const AT*, AT*, int, int);                                                                       \
  template int swiglu_bwd<AT>(hipStream_t, const AT*, const AT*, AT*, int, int);                                                            \
  template int logit_rows<AT>(hipStream_t, const float*, long, const int*, int, int, float*, AT*, long, float, const int*, int, float*);    \
  template int cast_from_f32<AT>(hipStream_t, const float*, AT*, long, float);                                                              \
  template int randn_fill<AT>(hipStream_t, AT*, long, unsigned, float);                                                                     \
  template int fill_const<AT>(hipStream_t, AT*, long, float);
TST_INST(bf16_t)
TST_INST(float)
#undef TST_INST
