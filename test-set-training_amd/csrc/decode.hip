// Generation (tst_generate_async, tst_sample_async): the kernels a decode step adds to the model graph of forward(). Greedy generation has three:
//
//   kv_append    copies the k and v columns of qkv [T, ld] -- behind the head norm and RoPE, i.e. as attention reads them -- into one layer's cache
//                kcache / vcache [rows, Hkv dh] at given row indices. One 16-byte vector per lane, nothing else.
//   attn_decode  ONE query token per sequence against that sequence's cached keys 0 .. n-1. HBM / L2-bound streaming: K and V are read exactly once.
//                One workgroup per (sequence, kv head); the G = H / Hkv <= 8 query heads that share the kv head sit in registers. A cache row of dh elements
//                is dh / 8 lanes x 8 elements (the lane shape of head_norm.hip: 16 lanes per 128-wide row, one 16-byte load per lane in bf16, two in fp32), so
//                the 256 threads hold 16 (dh 128) or 32 (dh 64) "row groups"; row group r takes the keys r, r + 16, ... . The row dot product ends in DPP
//                inside the row group. Every row group keeps a running max, sum and accumulator in fp32 (online softmax, P never rounded: there is no MFMA
//                to feed); the row groups of a wave are merged by lane exchanges, the four waves once through LDS, in a fixed order: bit-reproducible.
//                No atomics. Cache rows >= n of a sequence are never read.
//   next_token   turns the {lse, logit[target], argmax, max} rows logit_rows leaves in `stats` into the step's outputs and the next step's inputs, on the
//                device: tok[s, j] = argmax, logp[s, j] = max - lse, d_ids[s] = argmax, d_pos[s] = len[s] + j, lab_idx[s] = s.
//
// Sampled generation (tst_sample_async) adds two:
//   attn_decode, SHARED  the same kernel reading a prompt's cache rows, which the n samples of that prompt share, and behind them the decode row's own tail
//   sample_rows          logit_rows + next_token of a sampled step in ONE pass over the logits row: the log-sum-exp of logit / temperature and a Gumbel-max
//                        draw from softmax(logits / temperature), noise from Philox4x32-10
//
// Candidate scoring (tst_score_candidates_async) adds two:
//   attn_extend          attn_decode, SHARED for ALL positions of a given continuation at once: the register sets hold (position, query head) pairs
//   cand_logp            log p of every candidate token from the prefill's logits (first tokens) and the extend pass's row statistics (the rest)
//
// The generation's geometry travels in one small device array `meta` (host_logic.h plan_generate writes it):
//   meta[0] = n_seqs S, meta[1] = max_new, meta[2 .. 2 + S] = cu_seqlens of the prompts, meta[3 + S .. 3 + 2 S) = their lengths.
// Cache row of (sequence s, position p) = cu[s] + s max_new + p: the packed prompts with room for max_new tokens behind each.
#include "kernels.h"

// the merges below rely on both partner lanes forming the same two products and one sum: no contraction the compiler may apply to one side only; every fused
// multiply-add is written out
#pragma clang fp contract(off)

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? TST_OK : TST_EHIP)

template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the LPR (8 or 16) lanes of a row group, the same bits in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
template <int LPR> __device__ __forceinline__ float rowgroup_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  if constexpr (LPR == 16) v += dpp_mov<0x140>(v);
  return v;
}

// bf16 path: v_exp_f32 of x log2(e), as the probabilities of attn.hip; fp32 strict path: the library expf, as attn_f32.hip
template <typename AT> __device__ __forceinline__ float exp_of(float x) {
  if constexpr (sizeof(AT) == 2) return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
  else return expf(x);
}

// The partial results (row groups of a wave, then the four waves) are merged in MT: fp32 on the bf16 path; fp64 on the fp32 strict path, where the merges'
// roundings would otherwise be the largest error of the kernel -- a sequence whose softmax sits on ONE key has |out| ~ |v| of that key, and each of the six
// merges and the normalisation rounds at that magnitude (measured against fp64 attention: 7.6e-7 with fp32 merges, 2.8e-7 with fp64 merges, 4.1e-7 the causal
// fp32 kernel's last rows; tests/test_decode_kernels_gpu.py). A few dozen operations per lane, once per workgroup.
template <typename AT> struct MergeT { typedef float type; };
template <> struct MergeT<float> { typedef double type; };
__device__ __forceinline__ float merge_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ double merge_exp(double x) { return exp(x); }

template <typename AT>
__global__ __launch_bounds__(256) void kv_append_kernel(const AT* __restrict__ qkv, long ld, int k_off, int wkv, const int* __restrict__ rows,
                                                        AT* __restrict__ kcache, AT* __restrict__ vcache, int T, long cap_rows) {
  constexpr int EPV = 16 / (int)sizeof(AT);   // elements per 16-byte vector
  const int vpr = 2 * wkv / EPV;              // vectors per token: k then v
  const long total = (long)T * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / vpr), c = (int)(i - (long)t * vpr);
    const int is_v = c >= (vpr >> 1);
    const int col = (c - is_v * (vpr >> 1)) * EPV;
    const long row = rows[t];
    if (row < 0 || row >= cap_rows) continue;   // (plan_generate keeps every row inside the cache: never taken)
    const uint4 v = *(const uint4*)(qkv + (long)t * ld + k_off + is_v * wkv + col);
    *(uint4*)((is_v ? vcache : kcache) + row * wkv + col) = v;
  }
}

// SHARED = false: the greedy generation's contiguous rows (meta as above). SHARED = true: the sampled generation (tst_sample_async) -- `meta` is the geometry
// array of plan_sample, rows | max_new | n_samples | {pre_row0, len, tail_row0} per decode row; key k of decode row r lies at cache row
// k < len ? pre_row0 + k : tail_row0 + k - len: the prompt's rows, which the n samples of that prompt share, then the row's own tail. Lane shape, loads per trip
// and merge order are the one code below, so the same keys give the same bits in either layout.
template <typename AT, int DH, int GP, bool SHARED>
__global__ __launch_bounds__(256) void attn_decode_kernel(const AT* __restrict__ q, long ldq, const AT* __restrict__ kcache, const AT* __restrict__ vcache,
                                                          const int* __restrict__ meta, int step, AT* __restrict__ out, long ldo, int G, int Hkv, float scale,
                                                          long cap_rows) {
  constexpr int LPR = DH / 8;     // lanes per cache row
  constexpr int NG = 256 / LPR;   // row groups per workgroup
  typedef typename MergeT<AT>::type MT;
  __shared__ MT red[4][GP][LPR * 8 + 2];
  const int s = blockIdx.x, kvh = blockIdx.y;
  int n, len = 0;
  long row0, tail0 = 0;
  if constexpr (SHARED) {
    row0 = meta[3 + 3 * s];                                    // cache row of the prompt's key 0
    len = meta[4 + 3 * s];
    tail0 = meta[5 + 3 * s];                                   // cache row of this decode row's first own token
    n = len + step;
    // (plan_sample keeps the prompt and every tail inside the cache: never taken)
    if (len <= 0 || step < 0 || row0 < 0 || row0 + len > cap_rows || tail0 < 0 || tail0 + step > cap_rows) return;
  } else {
    const int S = meta[0], max_new = meta[1];
    n = meta[3 + S + s] + step;                                // keys of this sequence, the new token's included
    row0 = (long)meta[2 + s] + (long)s * max_new;              // cache row of its key 0
    if (n <= 0 || row0 < 0 || row0 + n > cap_rows) return;     // (plan_generate keeps every sequence inside the cache: never taken)
  }
  const int tid = threadIdx.x, sub = tid % LPR, grp = tid / LPR;
  const int wkv = Hkv * DH;
  float qf[GP][8], acc[GP][8], m[GP], l[GP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { acc[g][i] = 0.f; qf[g][i] = 0.f; }
    if (g < G) ld8(q + (long)s * ldq + (long)(kvh * G + g) * DH + sub * 8, qf[g]);
  }
  const AT* kp = kcache + row0 * wkv + (long)kvh * DH + sub * 8;
  const AT* vp = vcache + row0 * wkv + (long)kvh * DH + sub * 8;
  // element offset of key k from kp / vp
  auto key_off = [&](int k) -> long {
    if constexpr (SHARED) return (k < len ? (long)k : tail0 - row0 + (k - len)) * wkv;
    else return (long)k * wkv;
  };
  auto one_key = [&](const float* kf, const float* vf) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      if (g < G) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = __builtin_fmaf(qf[g][i], kf[i], d);
        const float sc = rowgroup_sum<LPR>(d) * scale;
        const float mn = fmaxf(m[g], sc);
        const float corr = exp_of<AT>(m[g] - mn);   // exactly 1 while the maximum stands (0 for the first key: m = -inf)
        const float p = exp_of<AT>(sc - mn);
        l[g] = __builtin_fmaf(l[g], corr, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(p, vf[i], acc[g][i] * corr);   // (acc * 1 is exact: one rounding per key while the maximum stands)
        m[g] = mn;
      }
    }
  };
  // two keys per trip: the loads of both are in flight before the first is used
  for (int j = grp; j < n; j += 2 * NG) {
    float k0[8], v0[8], k1[8], v1[8];
    const bool two = j + NG < n;
    ld8(kp + key_off(j), k0);
    ld8(vp + key_off(j), v0);
    if (two) {
      ld8(kp + key_off(j + NG), k1);
      ld8(vp + key_off(j + NG), v1);
    }
    one_key(k0, v0);
    if (two) one_key(k1, v1);
  }
  // merge the row groups of a wave (lanes LPR, 2 LPR, .. 32 apart): both partners add the same two products, so every lane ends with the same bits
  MT am[GP], al[GP], aa[GP][8];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    am[g] = (MT)m[g];
    al[g] = (MT)l[g];
#pragma unroll
    for (int i = 0; i < 8; ++i) aa[g][i] = (MT)acc[g][i];
  }
  const MT NEG_INF = (MT)(-INFINITY);
#pragma unroll
  for (int o = LPR; o < 64; o <<= 1) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      if (g < G) {
        const MT mo = __shfl_xor(am[g], o, 64), lo = __shfl_xor(al[g], o, 64);
        const MT M = am[g] > mo ? am[g] : mo;
        const MT wa = am[g] == NEG_INF ? (MT)0 : merge_exp(am[g] - M), wb = mo == NEG_INF ? (MT)0 : merge_exp(mo - M);
        al[g] = al[g] * wa + lo * wb;
#pragma unroll
        for (int i = 0; i < 8; ++i) aa[g][i] = aa[g][i] * wa + __shfl_xor(aa[g][i], o, 64) * wb;
        am[g] = M;
      }
    }
  }
  // the four waves, once through LDS, merged in wave order
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < LPR) {
#pragma unroll
    for (int g = 0; g < GP; ++g) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][g][sub * 8 + i] = aa[g][i];
      if (sub == 0) { red[wave][g][LPR * 8] = am[g]; red[wave][g][LPR * 8 + 1] = al[g]; }
    }
  }
  __syncthreads();
  if (tid < G * LPR) {
    const int g = tid / LPR;   // (sub = tid % LPR as above)
    MT M = NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = red[w][g][LPR * 8] > M ? red[w][g][LPR * 8] : M;
    MT L = 0, o8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o8[i] = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const MT mw = red[w][g][LPR * 8];
      const MT ww = mw == NEG_INF ? (MT)0 : merge_exp(mw - M);
      L += red[w][g][LPR * 8 + 1] * ww;
#pragma unroll
      for (int i = 0; i < 8; ++i) o8[i] += red[w][g][sub * 8 + i] * ww;
    }
    float of[8];   // n >= 1: at least one key carries weight exp(0) = 1, so L >= 1
#pragma unroll
    for (int i = 0; i < 8; ++i) of[i] = (float)(o8[i] / L);
    st8(out + (long)s * ldo + (long)(kvh * G + g) * DH + sub * 8, of);
  }
}

__global__ __launch_bounds__(256) void next_token_kernel(const float* __restrict__ stats, const int* __restrict__ meta, int j, int* __restrict__ tok,
                                                         float* __restrict__ logp, int* __restrict__ d_ids, int* __restrict__ d_pos, int* __restrict__ lab_idx) {
  const int S = meta[0], max_new = meta[1];
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S || j < 0 || j >= max_new) return;
  const int am = __float_as_int(stats[s * 4 + 2]);
  tok[(long)s * max_new + j] = am;
  logp[(long)s * max_new + j] = stats[s * 4 + 3] - stats[s * 4 + 0];
  d_ids[s] = am;
  d_pos[s] = meta[3 + S + s] + j;   // position of the token just chosen
  lab_idx[s] = s;                   // the head reads every row of a decode step
}

// ---- sampled generation: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out; the four output words of
// counter (c0, c1, c2, c3) under key (k0, k1)
struct U4 { unsigned x, y, z, w; };
__device__ __forceinline__ U4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}
// Gumbel noise of one 32-bit word: u = ((x >> 9) + 0.5) 2^-23 has 24 significant bits (exact in fp32, never 0 or 1), g = -log(-log u)
__device__ __forceinline__ float gumbel_of(unsigned x) {
  const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

// One workgroup per output row r = s n_samples + i: ONE pass over the fp32 logits row src (step 0: the prefill's row s, read by its n samples; afterwards row r)
// carries the online max / sum of z = logit inv_temp (the log-sum-exp of the tempered row) and the arg-max of fmaf(logit, inv_temp, g) -- Gumbel-max, an exact
// draw from softmax(logits / temperature). Noise word v & 3 of Philox counter (v >> 2, step, i, 0) under the sequence's seed belongs to vocabulary entry v:
// one call serves the four columns of a load. Columns >= V (the padding up to ld) are loaded with their vector and never become candidates. Ties go to the
// first index, as in logit_rows; the partial results are merged in a fixed order: no atomics, bit-reproducible.
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ logits, long ld, int V, const int* __restrict__ geo,
                                                          const int* __restrict__ seeds, int j, float inv_temp, int* __restrict__ tok, float* __restrict__ logp,
                                                          int* __restrict__ d_ids, int* __restrict__ d_pos, int* __restrict__ lab_idx) {
  __shared__ float red_b[4], red_m[4], red_l[4];
  __shared__ int red_i[4];
  const int R = geo[0], max_new = geo[1], n_samples = geo[2];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= R || j < 0 || j >= max_new || n_samples < 1) return;
  const int s = r / n_samples, i = r - s * n_samples;
  const float* lr = logits + (long)(j == 0 ? s : r) * ld;
  const unsigned k0 = (unsigned)seeds[2 * s], k1 = (unsigned)seeds[2 * s + 1];
  float best = -INFINITY, m = -INFINITY, l = 0.f;
  int bi = 0;
  for (int c = tid * 4; c < V; c += 1024) {
    const f32x4 v = *(const f32x4*)(lr + c);
    const U4 x = philox4x32_10((unsigned)(c >> 2), (unsigned)j, (unsigned)i, 0u, k0, k1);
    const unsigned xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e < V) {
        const float sc = __builtin_fmaf(v[e], inv_temp, gumbel_of(xs[e]));
        if (sc > best) { best = sc; bi = c + e; }   // (ascending columns: the first index of a thread's maximum)
        const float z = v[e] * inv_temp;
        const float ex = expf(-fabsf(z - m));       // one exponential per entry: the old sum's correction, or the entry's own term (first entry: exp(-inf) = 0)
        if (z > m) { l = l * ex + 1.0f; m = z; }
        else l += ex;
      }
    }
  }
  auto merge = [](float& ma, float& la, float mb, float lb) {
    const float M = fmaxf(ma, mb);
    const float wa = ma == -INFINITY ? 0.f : expf(ma - M), wb = mb == -INFINITY ? 0.f : expf(mb - M);
    la = la * wa + lb * wb;   // (both partners of an exchange form the same two products and one sum)
    ma = M;
  };
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    merge(m, l, om, ol);
  }
  if ((tid & 63) == 0) { red_b[tid >> 6] = best; red_i[tid >> 6] = bi; red_m[tid >> 6] = m; red_l[tid >> 6] = l; }
  __syncthreads();
  if (tid == 0) {
    float bb = red_b[0], M = red_m[0], L = red_l[0];
    int ba = red_i[0];
    for (int w = 1; w < 4; ++w) {
      if (red_b[w] > bb || (red_b[w] == bb && red_i[w] < ba)) { bb = red_b[w]; ba = red_i[w]; }
      merge(M, L, red_m[w], red_l[w]);
    }
    tok[(long)r * max_new + j] = ba;
    logp[(long)r * max_new + j] = lr[ba] * inv_temp - (M + logf(L));
    d_ids[r] = ba;
    d_pos[r] = geo[4 + 3 * r] + j;   // position of the token just chosen: the prompt's length + j
    lab_idx[r] = r;                  // the head reads every row of a decode step
  }
}

// ---- candidate scoring (tst_score_candidates_async): every position of a given continuation in ONE launch per layer. geo = {pre_row0, len, tail_row0, q_row0,
// n_pos} per candidate with at least two tokens (host_logic.h plan_candidates): the prompt lies at cache rows [pre_row0, pre_row0 + len), the candidate's own
// tokens 0 .. n_pos - 1 at [tail_row0, tail_row0 + n_pos), their queries at rows q_row0 .. q_row0 + n_pos - 1 of q / out. The GP register sets of attn_decode hold
// (position, query head) pairs: set e = pl Gpad + g (Gpad = 1 << gsh, G rounded up to 1, 2, 4, 8), so one pass over the keys serves P = GP / Gpad consecutive
// positions; pair (p, g) takes the keys 0 .. len + p and skips the later ones. Per pair the keys a row group sees, their order, the products and every merge are
// those of attn_decode_kernel<.., SHARED> at step = p + 1: the same bits.
template <typename AT, int DH, int GP>
__global__ __launch_bounds__(256) void attn_extend_kernel(const AT* __restrict__ q, long ldq, const AT* __restrict__ kcache, const AT* __restrict__ vcache,
                                                          const int* __restrict__ geo, int n_rows, AT* __restrict__ out, long ldo, int G, int gsh, int Hkv, float scale,
                                                          long cap_rows) {
  constexpr int LPR = DH / 8;     // lanes per cache row
  constexpr int NG = 256 / LPR;   // row groups per workgroup
  typedef typename MergeT<AT>::type MT;
  __shared__ MT red[4][GP][LPR * 8 + 2];
  const int c = blockIdx.x, kvh = blockIdx.y;
  const long row0 = geo[5 * c];
  const int len = geo[5 * c + 1];
  const long tail0 = geo[5 * c + 2], q0 = geo[5 * c + 3];
  const int n_pos = geo[5 * c + 4];
  // (plan_candidates keeps the prompt, every tail and every query row in range: never taken)
  if (len <= 0 || n_pos < 1 || row0 < 0 || row0 + len > cap_rows || tail0 < 0 || tail0 + n_pos > cap_rows || q0 < 0 || q0 + n_pos > n_rows) return;
  const int tid = threadIdx.x, sub = tid % LPR, grp = tid / LPR;
  const int wkv = Hkv * DH;
  const int P = GP >> gsh, gmask = (1 << gsh) - 1;
  const AT* kp = kcache + row0 * wkv + (long)kvh * DH + sub * 8;
  const AT* vp = vcache + row0 * wkv + (long)kvh * DH + sub * 8;
  auto key_off = [&](int k) -> long { return (k < len ? (long)k : tail0 - row0 + (k - len)) * wkv; };
  const MT NEG_INF = (MT)(-INFINITY);
  for (int p0 = 0; p0 < n_pos; p0 += P) {
    float qf[GP][8], acc[GP][8], m[GP], l[GP];
    int ne[GP];   // keys of set e (0: the set is empty -- a padded head, or a position behind the candidate's last)
#pragma unroll
    for (int e = 0; e < GP; ++e) {
      const int pl = e >> gsh, g = e & gmask;
      ne[e] = (g < G && p0 + pl < n_pos) ? len + p0 + pl + 1 : 0;
      m[e] = -INFINITY;
      l[e] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { acc[e][i] = 0.f; qf[e][i] = 0.f; }
      if (ne[e]) ld8(q + (q0 + p0 + pl) * ldq + (long)(kvh * G + g) * DH + sub * 8, qf[e]);
    }
    const int n = len + (p0 + P < n_pos ? p0 + P : n_pos);   // keys of the pass's last position
    auto one_key = [&](int j, const float* kf, const float* vf) {
#pragma unroll
      for (int e = 0; e < GP; ++e) {
        if (j < ne[e]) {
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) d = __builtin_fmaf(qf[e][i], kf[i], d);
          const float sc = rowgroup_sum<LPR>(d) * scale;
          const float mn = fmaxf(m[e], sc);
          const float corr = exp_of<AT>(m[e] - mn);
          const float p = exp_of<AT>(sc - mn);
          l[e] = __builtin_fmaf(l[e], corr, p);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[e][i] = __builtin_fmaf(p, vf[i], acc[e][i] * corr);
          m[e] = mn;
        }
      }
    };
    // two keys per trip, as attn_decode: row group r takes the keys r, r + NG, .. in ascending order
    for (int j = grp; j < n; j += 2 * NG) {
      float k0[8], v0[8], k1[8], v1[8];
      const bool two = j + NG < n;
      ld8(kp + key_off(j), k0);
      ld8(vp + key_off(j), v0);
      if (two) {
        ld8(kp + key_off(j + NG), k1);
        ld8(vp + key_off(j + NG), v1);
      }
      one_key(j, k0, v0);
      if (two) one_key(j + NG, k1, v1);
    }
    MT am[GP], al[GP], aa[GP][8];
#pragma unroll
    for (int e = 0; e < GP; ++e) {
      am[e] = (MT)m[e];
      al[e] = (MT)l[e];
#pragma unroll
      for (int i = 0; i < 8; ++i) aa[e][i] = (MT)acc[e][i];
    }
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < GP; ++e) {
        if (ne[e]) {
          const MT mo = __shfl_xor(am[e], o, 64), lo = __shfl_xor(al[e], o, 64);
          const MT M = am[e] > mo ? am[e] : mo;
          const MT wa = am[e] == NEG_INF ? (MT)0 : merge_exp(am[e] - M), wb = mo == NEG_INF ? (MT)0 : merge_exp(mo - M);
          al[e] = al[e] * wa + lo * wb;
#pragma unroll
          for (int i = 0; i < 8; ++i) aa[e][i] = aa[e][i] * wa + __shfl_xor(aa[e][i], o, 64) * wb;
          am[e] = M;
        }
      }
    }
    const int wave = tid >> 6, lane = tid & 63;
    if (lane < LPR) {
#pragma unroll
      for (int e = 0; e < GP; ++e) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wave][e][sub * 8 + i] = aa[e][i];
        if (sub == 0) { red[wave][e][LPR * 8] = am[e]; red[wave][e][LPR * 8 + 1] = al[e]; }
      }
    }
    __syncthreads();
    if (tid < GP * LPR) {
      const int e = tid / LPR, pl = e >> gsh, g = e & gmask;   // (sub = tid % LPR as above)
      if (g < G && p0 + pl < n_pos) {
        MT M = NEG_INF;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = red[w][e][LPR * 8] > M ? red[w][e][LPR * 8] : M;
        MT L = 0, o8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o8[i] = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const MT mw = red[w][e][LPR * 8];
          const MT ww = mw == NEG_INF ? (MT)0 : merge_exp(mw - M);
          L += red[w][e][LPR * 8 + 1] * ww;
#pragma unroll
          for (int i = 0; i < 8; ++i) o8[i] += red[w][e][sub * 8 + i] * ww;
        }
        float of[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) of[i] = (float)(o8[i] / L);
        st8(out + (q0 + p0 + pl) * ldo + (long)(kvh * G + g) * DH + sub * 8, of);
      }
    }
    __syncthreads();   // the next pass writes `red` again
  }
}

// One thread per candidate token t: src[2 t] = row, src[2 t + 1] = tok. tok >= 0: a candidate's FIRST token, read from the prefill's logits row of its prompt,
// logits[row, tok] - lse[row] (phase 0, before the extend pass overwrites logits and stats); tok < 0: a later token, logit[target] - lse of extend row `row` as
// logit_rows left them in stats (phase 1).
__global__ __launch_bounds__(256) void cand_logp_kernel(const float* __restrict__ logits, long ld, int V, const float* __restrict__ stats, int n_rows,
                                                        const int* __restrict__ src, int n, int phase, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int row = src[2 * t], tok = src[2 * t + 1];
  if (row < 0 || row >= n_rows || tok >= V) return;   // (plan_candidates keeps both in range: never taken)
  if (phase == 0) {
    if (tok >= 0) out[t] = logits[(long)row * ld + tok] - stats[(long)row * 4];
  } else if (tok < 0) out[t] = stats[(long)row * 4 + 1] - stats[(long)row * 4];
}

}  // namespace

template <typename AT>
int kv_append(hipStream_t st, const AT* qkv, long ld, int k_off, const int* rows, AT* kcache, AT* vcache, int T, int Hkv, int dh, long cap_rows) {
  if (T <= 0) return TST_OK;
  constexpr int EPV = 16 / (int)sizeof(AT);
  if (!qkv || !rows || !kcache || !vcache || Hkv < 1 || (dh != 64 && dh != 128) || (ld % EPV) || (k_off % EPV) || k_off < 0 || ld < (long)k_off + 2L * Hkv * dh ||
      cap_rows <= 0)
    return TST_EINVAL;
  const int wkv = Hkv * dh;
  const long want = ((long)T * (2 * wkv / EPV) + 255) / 256;
  hipLaunchKernelGGL(kv_append_kernel<AT>, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, st, qkv, ld, k_off, wkv, rows, kcache, vcache, T, cap_rows);
  return CHECK_LAUNCH();
}

template <typename AT>
int attn_decode(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* meta, int n_seqs, int step, AT* out, long ldo, int H, int Hkv,
                int dh, float scale, long cap_rows) {
  if (n_seqs <= 0) return TST_OK;
  if (!q || !kcache || !vcache || !meta || !out || Hkv < 1 || H < Hkv || H % Hkv || H / Hkv > 8 || (dh != 64 && dh != 128) || (ldq & 7) || (ldo & 7) ||
      ldq < (long)H * dh || ldo < (long)H * dh || step < 0 || cap_rows <= 0 || Hkv > 65535)
    return TST_EINVAL;
  const int G = H / Hkv;
  const dim3 grid((unsigned)n_seqs, (unsigned)Hkv);
#define AD_LAUNCH(DH, GP) \
  hipLaunchKernelGGL((attn_decode_kernel<AT, DH, GP, false>), grid, dim3(256), 0, st, q, ldq, kcache, vcache, meta, step, out, ldo, G, Hkv, scale, cap_rows)
#define AD_DH(GP) do { if (dh == 128) AD_LAUNCH(128, GP); else AD_LAUNCH(64, GP); } while (0)
  if (G == 1) AD_DH(1);
  else if (G == 2) AD_DH(2);
  else if (G <= 4) AD_DH(4);
  else AD_DH(8);
#undef AD_DH
#undef AD_LAUNCH
  return CHECK_LAUNCH();
}

template <typename AT>
int attn_decode_shared(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* geo, int n_rows, int step, AT* out, long ldo, int H,
                       int Hkv, int dh, float scale, long cap_rows) {
  if (n_rows <= 0) return TST_OK;
  if (!q || !kcache || !vcache || !geo || !out || Hkv < 1 || H < Hkv || H % Hkv || H / Hkv > 8 || (dh != 64 && dh != 128) || (ldq & 7) || (ldo & 7) ||
      ldq < (long)H * dh || ldo < (long)H * dh || step < 0 || cap_rows <= 0 || Hkv > 65535)
    return TST_EINVAL;
  const int G = H / Hkv;
  const dim3 grid((unsigned)n_rows, (unsigned)Hkv);
#define AD_LAUNCH(DH, GP) \
  hipLaunchKernelGGL((attn_decode_kernel<AT, DH, GP, true>), grid, dim3(256), 0, st, q, ldq, kcache, vcache, geo, step, out, ldo, G, Hkv, scale, cap_rows)
#define AD_DH(GP) do { if (dh == 128) AD_LAUNCH(128, GP); else AD_LAUNCH(64, GP); } while (0)
  if (G == 1) AD_DH(1);
  else if (G == 2) AD_DH(2);
  else if (G <= 4) AD_DH(4);
  else AD_DH(8);
#undef AD_DH
#undef AD_LAUNCH
  return CHECK_LAUNCH();
}

template <typename AT>
int attn_extend(hipStream_t st, const AT* q, long ldq, const AT* kcache, const AT* vcache, const int* geo, int n_cands, int n_rows, AT* out, long ldo, int H, int Hkv,
                int dh, float scale, long cap_rows) {
  if (n_cands <= 0) return TST_OK;
  if (!q || !kcache || !vcache || !geo || !out || Hkv < 1 || H < Hkv || H % Hkv || H / Hkv > 8 || (dh != 64 && dh != 128) || (ldq & 7) || (ldo & 7) ||
      ldq < (long)H * dh || ldo < (long)H * dh || n_rows < 1 || cap_rows <= 0 || Hkv > 65535)
    return TST_EINVAL;
  const int G = H / Hkv;
  const int gsh = G == 1 ? 0 : G == 2 ? 1 : G <= 4 ? 2 : 3;
  const dim3 grid((unsigned)n_cands, (unsigned)Hkv);
#define AE_LAUNCH(DH) \
  hipLaunchKernelGGL((attn_extend_kernel<AT, DH, 8>), grid, dim3(256), 0, st, q, ldq, kcache, vcache, geo, n_rows, out, ldo, G, gsh, Hkv, scale, cap_rows)
  if (dh == 128) AE_LAUNCH(128);
  else AE_LAUNCH(64);
#undef AE_LAUNCH
  return CHECK_LAUNCH();
}

int cand_logp(hipStream_t st, const float* logits, long ld, int V, const float* stats, int n_rows, const int* src, int n, int phase, float* out) {
  if (n <= 0) return TST_OK;
  if (!logits || !stats || !src || !out || V < 1 || ld < V || n_rows < 1 || (phase != 0 && phase != 1)) return TST_EINVAL;
  hipLaunchKernelGGL(cand_logp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, ld, V, stats, n_rows, src, n, phase, out);
  return CHECK_LAUNCH();
}

int next_token(hipStream_t st, const float* stats, const int* meta, int n_seqs, int j, int* tok, float* logp, int* d_ids, int* d_pos, int* lab_idx) {
  if (n_seqs <= 0) return TST_OK;
  if (!stats || !meta || !tok || !logp || !d_ids || !d_pos || !lab_idx || j < 0) return TST_EINVAL;
  hipLaunchKernelGGL(next_token_kernel, dim3((unsigned)((n_seqs + 255) / 256)), dim3(256), 0, st, stats, meta, j, tok, logp, d_ids, d_pos, lab_idx);
  return CHECK_LAUNCH();
}

int sample_rows(hipStream_t st, const float* logits, long ld, int V, const int* geo, const int* seeds, int n_rows, int j, float inv_temp, int* tok, float* logp,
                int* d_ids, int* d_pos, int* lab_idx) {
  if (n_rows <= 0) return TST_OK;
  if (!logits || !geo || !seeds || !tok || !logp || !d_ids || !d_pos || !lab_idx || j < 0 || V < 1 || (ld & 3) || ld < (((long)V + 3) & ~3L) || !(inv_temp > 0.f))
    return TST_EINVAL;
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)n_rows), dim3(256), 0, st, logits, ld, V, geo, seeds, j, inv_temp, tok, logp, d_ids, d_pos, lab_idx);
  return CHECK_LAUNCH();
}

#define INSTANTIATE(AT)                                                                                                           \
  template int kv_append<AT>(hipStream_t, const AT*, long, int, const int*, AT*, AT*, int, int, int, long);                      \
  template int attn_decode<AT>(hipStream_t, const AT*, long, const AT*, const AT*, const int*, int, int, AT*, long, int, int, int, \
                               float, long);                                                                                        \
  template int attn_decode_shared<AT>(hipStream_t, const AT*, long, const AT*, const AT*, const int*, int, int, AT*, long, int, int, \
                                      int, float, long);                                                                             \
  template int attn_extend<AT>(hipStream_t, const AT*, long, const AT*, const AT*, const int*, int, int, AT*, long, int, int, int, float, long);
INSTANTIATE(bf16_t)
INSTANTIATE(float)
