// Token attribution (include/tst_hip.h tst_attribute_async): the two kernels a backward pass seeded with J = sum_i log s(x_i) adds to the training one.
//   attr_seed   d J / d logits of the labelled rows, in place of logit_rows + loss_reduce (whose seed is the training loss)
//   token_attr  per token, gradient x input and the gradient's 2-norm of the embedding-layer output
// and the two that integrated gradients (tst_attribute_ig_async) add to those:
//   embed_interp  the embedding-layer output on the straight path from a baseline prompt to the real one
//   token_ig      per token, one term of the path's Riemann sum, accumulated over the steps
// All are HBM-trivial beside the contractions between them; none uses atomics, so two runs agree bit for bit.
#include "common.h"
#include "kernels.h"

// One workgroup per labelled row r, w = row_w[r] (1 / labelled rows of the row's sequence):
//   kind 0 (open form)    dlogits[r, c] = w (onehot(target)[c] - softmax(z_r)[c])                                    c < V
//   kind 1 (option form)  dlogits[r, c] = w (onehot(target)[c] - softmax over the option ids [c]) at the option columns, 0 at every other one
// The whole padded row (Vp columns) is written, the padding as exact zeros. An id listed twice in opt_ids counts twice in the option logsumexp, as it does
// in the host's restricted softmax; its column then receives the sum of its entries. stats[r] = {lse, logit[target], option logsumexp (kind 1; else 0), max}.
template <typename AT>
__global__ __launch_bounds__(256) void attr_seed_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ target, const float* __restrict__ row_w,
                                                        const int* __restrict__ row_kind, const int* __restrict__ opt_ids, int n_opt, int V, int Vp,
                                                        float* __restrict__ stats, AT* __restrict__ dlogits, long ldd) {
  __shared__ float red[4];
  __shared__ int s_id[256];
  __shared__ float s_p[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* lr = logits + (long)r * ld;
  AT* dr = dlogits + (long)r * ldd;
  const int tg = target[r];
  const float w = row_w[r];
  const bool option = row_kind[r] != 0;   // (uniform over the workgroup)
  float m = -INFINITY;
  for (int c = tid * 4; c < V; c += 1024) {
    const f32x4 v = *(const f32x4*)(lr + c);   // (ld is padded past V: the vector stays inside the row)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < V) m = fmaxf(m, v[j]);
  }
  const float bm = block_max_256(m, red);
  float s = 0.f;
  for (int c = tid * 4; c < V; c += 1024) {
    const f32x4 v = *(const f32x4*)(lr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (c + j < V) ? expf(v[j] - bm) : 0.f;
  }
  s = block_sum_256(s, red);
  const float zt = lr[tg];
  if (!option) {
    if (tid == 0) {
      stats[r * 4 + 0] = bm + logf(s);
      stats[r * 4 + 1] = zt;
      stats[r * 4 + 2] = 0.f;
      stats[r * 4 + 3] = bm;
    }
    const float ws = w / s;
    for (int c = tid * 4; c < Vp; c += 1024) {
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (c < V) {
        const f32x4 v = *(const f32x4*)(lr + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c + j >= V) continue;
          const float p = expf(v[j] - bm) * ws;
          o[j] = (c + j == tg) ? w - p : -p;
        }
      }
      st4(dr + c, o);
    }
    return;
  }
  // option form: softmax over the (at most 256) option logits
  const bool mine = tid < n_opt;
  const int id = mine ? opt_ids[tid] : -1;
  const float z = mine ? lr[id] : -INFINITY;
  const float om = block_max_256(z, red);
  const float e = mine ? expf(z - om) : 0.f;
  const float os = block_sum_256(e, red);
  s_id[tid] = id;
  s_p[tid] = e / os;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = tid * 4; c < Vp; c += 1024) st4(dr + c, zero);
  if (tid == 0) {
    stats[r * 4 + 0] = bm + logf(s);
    stats[r * 4 + 1] = zt;
    stats[r * 4 + 2] = om + logf(os);
    stats[r * 4 + 3] = bm;
  }
  __syncthreads();   // the zeros of the whole row are written (and s_id / s_p are complete) before the option columns are
  if (mine) {
    bool first = true;
    float p = 0.f;
    for (int j = 0; j < n_opt; ++j)
      if (s_id[j] == id) {
        if (j < tid) first = false;
        p += s_p[j];
      }
    if (first) st1(dr + id, w * ((id == tg ? 1.0f : 0.0f) - p));
  }
}

// One wave per token t: gxi[t] = sum_c g[t, c] e[t, c], gnorm[t] = sqrt(sum_c g[t, c]^2); fp32 accumulation over 16-byte loads (d a multiple of 8), then the
// cross-lane butterfly of wave_sum: a fixed summation order.
template <typename AT>
__global__ __launch_bounds__(256) void token_attr_kernel(const AT* __restrict__ g, const AT* __restrict__ e, int T, int d, float* __restrict__ gxi,
                                                         float* __restrict__ gnorm) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;   // (whole waves leave: the shuffles below run on full waves)
  const AT* gr = g + (long)t * d;
  const AT* er = e + (long)t * d;
  float dot = 0.f, ss = 0.f;
  for (int c = lane * 8; c < d; c += 512) {
    float a[8], b[8];
    ld8(gr + c, a);
    ld8(er + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dot = fmaf(a[j], b[j], dot);
      ss = fmaf(a[j], a[j], ss);
    }
  }
  dot = wave_sum(dot);
  ss = wave_sum(ss);
  if (lane == 0) {
    gxi[t] = dot;
    gnorm[t] = sqrtf(ss);
  }
}

// Integrated gradients, the path: one wave per token t, x[t, :] = b + alpha (e - b) with e = E[ids[t]] and b = E[bids[t]] (ids clamped as the embedding kernels
// clamp them), evaluated in fp32 as written -- the difference, its product with alpha and the sum, each rounded to fp32, no contraction -- and rounded ONCE to the
// activation type. The ends, and a token whose baseline is its own id, take no arithmetic at all: the table row is copied (alpha == 1: E[ids[t]], what embed_fwd
// writes; alpha == 0: E[bids[t]]) -- fp32 would lose e against a b many binades larger, and a -0 of the table stays -0. GPT-2 (P != nullptr) adds P[pos[t]] in fp32
// before the one rounding, like embed_pos_fwd. The row choice is uniform over the wave.
template <typename AT>
__global__ __launch_bounds__(256) void embed_interp_kernel(const int* __restrict__ ids, const int* __restrict__ bids, const int* __restrict__ pos,
                                                           const AT* __restrict__ E, const AT* __restrict__ P, AT* __restrict__ out, int T, int d, int vocab,
                                                           int npos, float alpha) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  int id = ids[t], bid = bids[t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  bid = bid < 0 ? 0 : (bid >= vocab ? vocab - 1 : bid);
  const AT* er = E + (long)id * d;
  const AT* br = E + (long)bid * d;
  const AT* one = (id == bid || alpha == 1.0f) ? er : (alpha == 0.0f ? br : nullptr);   // the row that is the result as it stands
  const AT* pr = nullptr;
  if (P) {
    int p = pos[t];
    p = p < 0 ? 0 : (p >= npos ? npos - 1 : p);
    pr = P + (long)p * d;
  }
  AT* orow = out + (long)t * d;
  for (int c = lane * 8; c < d; c += 512) {
#pragma clang fp contract(off)   // every product and sum below is rounded to fp32 on its own: no fused multiply-add
    if (one && !pr) {   // a plain gather: bits, not values
      if constexpr (sizeof(AT) == 2) {
        *(uint4*)(orow + c) = *(const uint4*)(one + c);
      } else {
        *(uint4*)(orow + c) = *(const uint4*)(one + c);
        *(uint4*)(orow + c + 4) = *(const uint4*)(one + c + 4);
      }
      continue;
    }
    float a[8];
    if (one) ld8(one + c, a);
    else {
      float b[8];
      ld8(er + c, a);
      ld8(br + c, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = b[j] + alpha * (a[j] - b[j]);
    }
    if (pr) {
      float q[8];
      ld8(pr + c, q);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = a[j] + q[j];
    }
    st8(orow + c, a);
  }
}

// Integrated gradients, one step of the sum: one wave per token t, v = w sum_c g[t, c] (E[ids[t], c] - E[bids[t], c]), the difference taken in fp32 from the
// table rows (GPT-2's position term cancels in it); acc[t] = v when `first`, acc[t] + v otherwise -- the caller's steps run in stream order, so the adds happen in
// that order and the sum is bit-reproducible. A token whose baseline is its own id gets exactly 0 without reading g. Same summation order as token_attr.
template <typename AT>
__global__ __launch_bounds__(256) void token_ig_kernel(const AT* __restrict__ g, const AT* __restrict__ E, const int* __restrict__ ids, const int* __restrict__ bids,
                                                       int T, int d, int vocab, float w, int first, float* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;   // (whole waves leave: the shuffles below run on full waves)
  int id = ids[t], bid = bids[t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  bid = bid < 0 ? 0 : (bid >= vocab ? vocab - 1 : bid);
  float dot = 0.f;
  if (id != bid) {   // (uniform over the wave)
    const AT* gr = g + (long)t * d;
    const AT* er = E + (long)id * d;
    const AT* br = E + (long)bid * d;
    for (int c = lane * 8; c < d; c += 512) {
      float a[8], e[8], b[8];
      ld8(gr + c, a);
      ld8(er + c, e);
      ld8(br + c, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) dot = fmaf(a[j], e[j] - b[j], dot);
    }
    dot = wave_sum(dot);
  }
  if (lane == 0) {
#pragma clang fp contract(off)   // w dot is rounded before it is added: the sum over the steps is the fp32 sum of the steps' own results
    const float v = w * dot;
    acc[t] = first ? v : acc[t] + v;
  }
}

template <typename AT>
int attr_seed(hipStream_t st, const float* logits, long ld, const int* target, const float* row_w, const int* row_kind, const int* opt_ids, int n_opt, int n_rows,
              int V, int Vp, float* stats, AT* dlogits, long ldd) {
  if (n_rows <= 0) return TST_OK;
  if (!logits || !target || !row_w || !row_kind || !stats || !dlogits) return TST_EINVAL;
  if (V <= 0 || Vp < V || (Vp & 3) || ld < Vp || ldd < Vp || (ld & 3) || (ldd & 3) || n_opt < 0 || n_opt > 256 || (n_opt > 0 && !opt_ids)) return TST_EINVAL;
  hipLaunchKernelGGL(attr_seed_kernel<AT>, dim3(n_rows), dim3(256), 0, st, logits, ld, target, row_w, row_kind, opt_ids, n_opt, V, Vp, stats, dlogits, ldd);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

template <typename AT>
int token_attr(hipStream_t st, const AT* g, const AT* e, int T, int d, float* gxi, float* gnorm) {
  if (T <= 0) return TST_OK;
  if (!g || !e || !gxi || !gnorm || d <= 0 || (d & 7) || d > 8192) return TST_EINVAL;
  hipLaunchKernelGGL(token_attr_kernel<AT>, dim3(tst_ceil_div(T, 4)), dim3(256), 0, st, g, e, T, d, gxi, gnorm);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

template <typename AT>
int embed_interp(hipStream_t st, const int* ids, const int* bids, const int* pos, const AT* E, const AT* P, AT* out, int T, int d, int vocab, int npos, float alpha) {
  if (T <= 0) return TST_OK;
  if (!ids || !bids || !E || !out || d <= 0 || (d & 7) || vocab <= 0 || (P && (!pos || npos <= 0)) || !(alpha >= 0.0f && alpha <= 1.0f)) return TST_EINVAL;
  hipLaunchKernelGGL(embed_interp_kernel<AT>, dim3(tst_ceil_div(T, 4)), dim3(256), 0, st, ids, bids, pos, E, P, out, T, d, vocab, npos, alpha);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

template <typename AT>
int token_ig(hipStream_t st, const AT* g, const AT* E, const int* ids, const int* bids, int T, int d, int vocab, float w, bool first, float* acc) {
  if (T <= 0) return TST_OK;
  if (!g || !E || !ids || !bids || !acc || d <= 0 || (d & 7) || vocab <= 0) return TST_EINVAL;
  hipLaunchKernelGGL(token_ig_kernel<AT>, dim3(tst_ceil_div(T, 4)), dim3(256), 0, st, g, E, ids, bids, T, d, vocab, w, first ? 1 : 0, acc);
  return hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP;
}

#define INSTANTIATE(AT)                                                                                                                                  \
  template int attr_seed<AT>(hipStream_t, const float*, long, const int*, const float*, const int*, const int*, int, int, int, int, float*, AT*, long); \
  template int token_attr<AT>(hipStream_t, const AT*, const AT*, int, int, float*, float*);                                                            \
  template int embed_interp<AT>(hipStream_t, const int*, const int*, const int*, const AT*, const AT*, AT*, int, int, int, int, float);                \
  template int token_ig<AT>(hipStream_t, const AT*, const AT*, const int*, const int*, int, int, int, float, bool, float*);
INSTANTIATE(bf16_t)
INSTANTIATE(float)
#undef INSTANTIATE
