"""GPU parity of the general bf16 attention path: batches whose longest sequence has more than 128 tokens (csrc/attn.hip attn_fwd_kernel,
attn_delta_kernel, attn_bwd_dkdv_kernel, attn_bwd_dq_kernel). Every case is checked twice:
  * against the oracle's bf16 mirror (oracle/ops_np.py, the same 64-key tiles, running max and bf16 rounding of P / dS) at the tolerances of
    tests/test_kernels_gpu.py: out 2 ulp + 5e-3 rms, lse 1e-4, gradients 4 ulp + 2e-2 rms;
  * against exact float64 attention on the same bf16 inputs (written here, not in the pinned oracle): an error the kernel and the mirror share
    would pass the first check only. The kernel must sit no farther from fp64 than 1.5 x the mirror's own distance plus one bf16 ulp x rms.
Long sequences carry planted extremes that make the running max move across key tiles: a row whose largest score lies in its LAST key tile (the
accumulators of every earlier tile are rescaled by a tiny alpha), a key of tile 0 that dominates a block of rows (later tiles underflow to ~0), and a
head whose scores reach magnitude ~50. Outputs are poisoned before every launch, so an element no workgroup writes is caught.
The two kernel families (shared-staging / single backward kernel for max_len <= 128, general kernels above) are also run on the SAME inputs:
max_len is only an upper bound for the hooks, so lengths <= 128 launched with max_len = 129 take the general kernels."""
import numpy as np
import pytest

from oracle import ops_np as O
from test_kernels_gpu import BF_ULP, L, assert_close, err_stats, report  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

POISON = 0x7f   # 0x7f7f bf16 / 0x7f7f7f7f fp32: ~3.4e38, far from any result


# ------------------------------------------------------------------------------------------------ exact reference (float64)
def exact_attention_fwd(q, k, v, cu):
    """causal softmax attention per packed sequence in float64. q [T,H,dh], k/v [T,Hkv,dh] -> out [T,H,dh], lse [H,T]"""
    T, H, dh = q.shape
    G = H // k.shape[1]
    scale = 1.0 / np.sqrt(dh)
    out, lse = np.zeros((T, H, dh)), np.zeros((H, T))
    for b in range(len(cu) - 1):
        s0, s1 = int(cu[b]), int(cu[b + 1])
        mask = np.tril(np.ones((s1 - s0, s1 - s0), bool))
        for h in range(H):
            S = np.where(mask, (q[s0:s1, h].astype(np.float64) @ k[s0:s1, h // G].astype(np.float64).T) * scale, -np.inf)
            m = S.max(-1, keepdims=True)
            p = np.exp(S - m)
            l = p.sum(-1, keepdims=True)
            out[s0:s1, h] = (p / l) @ v[s0:s1, h // G].astype(np.float64)
            lse[h, s0:s1] = (m + np.log(l))[:, 0]
    return out, lse


def exact_attention_bwd(q, k, v, dout, cu):
    """gradients of sum(out * dout) of exact_attention_fwd, float64"""
    T, H, dh = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    scale = 1.0 / np.sqrt(dh)
    dq, dk, dv = np.zeros((T, H, dh)), np.zeros((T, Hkv, dh)), np.zeros((T, Hkv, dh))
    for b in range(len(cu) - 1):
        s0, s1 = int(cu[b]), int(cu[b + 1])
        mask = np.tril(np.ones((s1 - s0, s1 - s0), bool))
        for h in range(H):
            hk = h // G
            qh, kh, vh = (x.astype(np.float64) for x in (q[s0:s1, h], k[s0:s1, hk], v[s0:s1, hk]))
            do = dout[s0:s1, h].astype(np.float64)
            S = np.where(mask, (qh @ kh.T) * scale, -np.inf)
            P = np.exp(S - S.max(-1, keepdims=True))
            P /= P.sum(-1, keepdims=True)
            dP = do @ vh.T
            dS = P * (dP - (dP * P).sum(-1, keepdims=True)) * scale   # rowsum(P dP) = rowsum(dO * out)
            dv[s0:s1, hk] += P.T @ do
            dk[s0:s1, hk] += dS.T @ qh
            dq[s0:s1, h] = dS @ kh
    return dq, dk, dv


def check_vs_exact(name, got, mirror, exact):
    """|kernel - fp64| <= 1.5 |mirror - fp64| + one bf16 ulp x rms(fp64), both as the largest element distance"""
    exact = np.asarray(exact, np.float64)
    rms = float(np.sqrt(np.mean(exact * exact)))
    dk = float(np.abs(np.asarray(got, np.float64) - exact).max())
    dm = float(np.abs(np.asarray(mirror, np.float64) - exact).max())
    report(name + " vs fp64", kernel_max_abs=dk, mirror_max_abs=dm, rms=rms)
    assert dk <= 1.5 * dm + BF_ULP * rms, f"{name}: kernel {dk:.3e} from fp64, the bf16 mirror {dm:.3e} (rms {rms:.3e})"


def assert_close_but_rare_flips(name, a, b, rtol, atol_rms, max_frac=4e-6, slack=3.0):
    """the gradient tolerance of tests/test_kernels_gpu.py (|a-b| <= rtol |b| + atol_rms rms(b)), of which at most max_frac of the elements (about two
    per million) may miss by up to `slack` times. Why wider than the short-sequence check: in the planted head whose scores reach ~50, P = exp(S - lse)
    is ~1 on a row's dominant key, and the kernel's S (MFMA summation order) and the mirror's (BLAS order) differ in their last fp32 bits; where that
    moves bf16(P) or bf16(dS) across a rounding boundary, dq / dk move by one bf16 ulp of the dominant term, which can exceed the bound at an element
    whose value cancels to near zero (measured: 1 element of 525824 at (1024, 3), 7.8e-3 against a bound of 3e-3). check_vs_exact bounds the whole
    tensor against fp64 at the same time, so a systematic error cannot hide in the allowance."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.isfinite(a).all(), f"{name}: non-finite output"
    rms = float(np.sqrt(np.mean(b * b))) + 1e-30
    tol = rtol * np.abs(b) + atol_rms * rms
    d = np.abs(a - b)
    mx, mxr, rel = err_stats(a, b)
    n_bad = int((d > tol).sum())
    report(name, max_abs=mx, max_over_rms=mxr, rel_l2=rel, beyond_tol=n_bad)
    assert n_bad <= max_frac * d.size and (d <= slack * tol).all(), \
        f"{name}: {n_bad}/{d.size} elements out of tolerance, worst {float((d / tol).max()):.2f} x the bound"


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(lengths, H, Hkv, dh, seed, plant=True):
    """bf16-exact packed qkv [T, (H + 2 Hkv) dh] and dO [T, H dh]; plant=True: extremes inside every sequence of more than 128 tokens"""
    rng = np.random.default_rng(seed)
    T = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    G = H // Hkv
    q = rng.standard_normal((T, H, dh)).astype(np.float32)
    k = rng.standard_normal((T, Hkv, dh)).astype(np.float32)
    v = rng.standard_normal((T, Hkv, dh)).astype(np.float32)
    for b in range(len(lengths)):
        s0, n = int(cu[b]), int(lengths[b])
        if not plant or n <= 128:
            continue
        # (1) the last row of head 0 meets its largest score (~2 |q|^2 / sqrt(dh) ~ 23 vs ~6 elsewhere) at its own position, in its last key tile
        r = s0 + n - 1
        k[r, 0] = 2.0 * q[r, 0]
        # (2) key 1 (tile 0) dominates rows 130.. of head 1 by ~24: the later tiles' probabilities fall to ~e^-24
        u = rng.standard_normal(dh).astype(np.float32)
        k[s0 + 1, 1 // G] = u
        rows = slice(s0 + 130, s0 + min(n, 170))
        q[rows, 1] = 3.0 * u + 0.3 * rng.standard_normal((len(range(*rows.indices(T))), dh)).astype(np.float32)
        # (3) the last head's scores reach magnitude ~50
        q[s0:s0 + n, H - 1] *= 12.0
    qkv = O.rbf(np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1))
    do = O.rbf(rng.standard_normal((T, H * dh)).astype(np.float32))
    return qkv, do, cu


def split(qkv, T, H, Hkv, dh):
    return (qkv[:, : H * dh].reshape(T, H, dh), qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh),
            qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh))


def run_kernels(L, qkv, do, cu, H, Hkv, dh, max_len):
    """tst_k_attn_fwd + tst_k_attn_bwd with every output poisoned first; returns out [T,H,dh], lse [H,T], dqkv [T, ld] (host)"""
    T, ld = qkv.shape
    lib = L.load_lab()
    n = len(cu) - 1
    scale = 1.0 / np.sqrt(dh)
    qkv_, cu_, do_ = L.dev_bf16(qkv), L.DevBuf(cu), L.dev_bf16(do)
    out_, lse_, delta_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4)
    dqkv_ = L.DevBuf(nbytes=T * ld * 2)
    for buf in (out_, lse_, delta_, dqkv_):
        assert lib.tst_dev_memset(buf.ptr, POISON, buf.nbytes) == 0
    assert lib.tst_k_attn_fwd(qkv_.ptr, ld, cu_.ptr, n, max_len, out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    assert lib.tst_k_attn_bwd(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, n, max_len, dqkv_.ptr, T, H, Hkv, dh,
                              scale) == 0
    return out_.get_bf16((T, H, dh)), lse_.get(np.float32, (H, T)), dqkv_.get_bf16((T, ld))


# ------------------------------------------------------------------------------------------------ 1. the general kernels, bf16
LONG_CASES = [
    ((1, 7, 129, 64, 300, 65), 4, 1, 128),      # several sequences, the grid sized by the longest; a one-token sequence
    ((1, 7, 129, 64, 300, 65), 7, 1, 128),      # Qwen2.5-7B's GQA group of 7
    ((1, 7, 129, 64, 300, 65), 12, 12, 64),     # GPT-2: head_dim 64, no grouping
    ((191, 192, 193), 8, 2, 128),               # tile edges past 128
    ((255, 256, 257), 8, 2, 128),
    ((512,), 4, 1, 128),
    ((1024, 3), 4, 1, 128),
    ((2048,), 4, 1, 128),                       # 32 key tiles: the online-softmax rescale over many tiles
    ((1024,), 12, 12, 64),                      # GPT-2's n_positions
]


@pytest.mark.parametrize("lengths,H,Hkv,dh", LONG_CASES)
def test_general_attention_long_sequences(L, lengths, H, Hkv, dh):
    T = sum(lengths)
    qkv, do, cu = make_inputs(lengths, H, Hkv, dh, seed=T + 13 * H + dh)
    out, lse, dqkv = run_kernels(L, qkv, do, cu, H, Hkv, dh, max(lengths))
    q, k, v = split(qkv, T, H, Hkv, dh)
    dO = do.reshape(T, H, dh)
    out_m, lse_m = O.attention_fwd(q, k, v, cu, bf16=True)
    dq_m, dk_m, dv_m = O.attention_bwd(q, k, v, out_m, dO, lse_m, cu, bf16=True)
    out_x, lse_x = exact_attention_fwd(q, k, v, cu)
    dq_x, dk_x, dv_x = exact_attention_bwd(q, k, v, dO, cu)
    dq, dk, dv = split(dqkv, T, H, Hkv, dh)
    tag = f"general L{'_'.join(map(str, lengths))} H{H}/{Hkv} dh{dh}"
    for name, a in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert np.isfinite(a).all(), f"{name} {tag}: non-finite element"
    assert_close("attn_out " + tag, out, out_m, 2 * BF_ULP, 5e-3)
    assert_close("attn_lse " + tag, lse, lse_m, 1e-4, 1e-4)
    assert_close_but_rare_flips("attn_dq " + tag, dq, dq_m, 4 * BF_ULP, 2e-2)
    assert_close_but_rare_flips("attn_dk " + tag, dk, dk_m, 4 * BF_ULP, 2e-2)
    assert_close_but_rare_flips("attn_dv " + tag, dv, dv_m, 4 * BF_ULP, 2e-2)
    check_vs_exact("attn_out " + tag, out, out_m, out_x)
    check_vs_exact("attn_lse " + tag, lse, lse_m, lse_x)
    check_vs_exact("attn_dq " + tag, dq, dq_m, dq_x)
    check_vs_exact("attn_dk " + tag, dk, dk_m, dk_x)
    check_vs_exact("attn_dv " + tag, dv, dv_m, dv_x)


def test_planted_extremes_are_in_place():
    """the planted rows really put their maxima where the docstring says (a guard on make_inputs, CPU only)"""
    lengths, H, Hkv, dh = (300,), 4, 1, 128
    qkv, _, cu = make_inputs(lengths, H, Hkv, dh, seed=5)
    q, k, _ = split(qkv, 300, H, Hkv, dh)
    S0 = (q[:, 0].astype(np.float64) @ k[:, 0].astype(np.float64).T) / np.sqrt(dh)
    assert int(np.argmax(S0[299, :300])) == 299 and S0[299, 299] - np.sort(S0[299, :299])[-1] > 10
    S1 = (q[:, 1].astype(np.float64) @ k[:, 0].astype(np.float64).T) / np.sqrt(dh)
    for r in range(130, 170):
        row = S1[r, : r + 1]
        assert int(np.argmax(row)) == 1 and row[1] - np.delete(row, 1).max() > 10
    S3 = (q[:, 3].astype(np.float64) @ k[:, 0].astype(np.float64).T) / np.sqrt(dh)
    assert np.abs(np.tril(S3)).max() > 40


# ------------------------------------------------------------------------------------------------ 2. the two kernel families on the same inputs
SHORT_CASES = [((7, 48, 100), 2, 1, 128), ((64, 65, 128, 1), 4, 2, 128), ((33, 64, 12, 50), 8, 2, 128), ((128, 127, 66), 4, 1, 128),
               ((80, 81, 16, 112), 14, 2, 128), ((5, 64, 17), 2, 2, 64), ((128, 70, 1), 4, 4, 64)]   # those of test_attention_backward_single_kernel


@pytest.mark.parametrize("lengths,H,Hkv,dh", SHORT_CASES)
def test_short_and_general_families_agree(L, lengths, H, Hkv, dh):
    T = sum(lengths)
    qkv, do, cu = make_inputs(lengths, H, Hkv, dh, seed=sum(lengths) + 31 * H + dh, plant=False)
    q, k, v = split(qkv, T, H, Hkv, dh)
    out_m, lse_m = O.attention_fwd(q, k, v, cu, bf16=True)
    dq_m, dk_m, dv_m = O.attention_bwd(q, k, v, out_m, do.reshape(T, H, dh), lse_m, cu, bf16=True)
    grads_m = np.concatenate([dq_m.reshape(T, -1), dk_m.reshape(T, -1), dv_m.reshape(T, -1)], 1)
    tag = f"L{'_'.join(map(str, lengths))} H{H}/{Hkv} dh{dh}"
    res = {}
    for fam, max_len in (("short", max(lengths)), ("general", 129)):
        out, lse, dqkv = run_kernels(L, qkv, do, cu, H, Hkv, dh, max_len)
        assert np.isfinite(out).all() and np.isfinite(lse).all() and np.isfinite(dqkv).all()
        assert_close(f"attn_out[{fam}] " + tag, out, out_m, 2 * BF_ULP, 5e-3)
        assert_close(f"attn_lse[{fam}] " + tag, lse, lse_m, 1e-4, 1e-4)
        assert_close(f"attn_dqkv[{fam}] " + tag, dqkv, grads_m, 4 * BF_ULP, 2e-2)
        res[fam] = (out, lse, dqkv)
    for i, (name, ulps) in enumerate((("out", 2), ("lse", 2), ("dqkv", 4))):
        a, b = res["general"][i].astype(np.float64), res["short"][i].astype(np.float64)
        mx, mxr, rel = err_stats(a, b)
        report(f"attn_short_vs_general {name} " + tag, max_abs=mx, max_over_rms=mxr, rel_l2=rel)
        assert mx <= ulps * BF_ULP * max(1.0, float(np.abs(b).max())), (name, mx)


@pytest.mark.parametrize("max_len,dh", [(129, 128), (300, 128), (100, 64)])
def test_rope_in_attention_is_refused_where_it_does_not_apply(L, max_len, dh):
    """RoPE inside the kernels exists for the short family at head_dim 128 only: the hooks return an error and leave every output untouched"""
    lengths = (max_len,) if max_len <= 128 else (max_len - 7, 7)
    H, Hkv, T = 2, 1, sum(lengths)
    qkv, do, cu = make_inputs(lengths, H, Hkv, dh, seed=3, plant=False)
    ld = qkv.shape[1]
    cos, sin = O.rope_tables(np.arange(512), dh, 10000.0, True)
    lib = L.load_lab()
    qkv_, cu_, do_, cos_, sin_ = L.dev_bf16(qkv), L.DevBuf(cu), L.dev_bf16(do), L.DevBuf(cos), L.DevBuf(sin)
    out_, lse_, delta_, dqkv_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=T * ld * 2)
    for buf in (out_, lse_, delta_, dqkv_):
        assert lib.tst_dev_memset(buf.ptr, POISON, buf.nbytes) == 0
    scale = 1.0 / np.sqrt(dh)
    assert lib.tst_k_attn_fwd_rope(qkv_.ptr, ld, cu_.ptr, len(lengths), max_len, out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale, cos_.ptr, sin_.ptr) != 0
    assert lib.tst_k_attn_bwd_rope(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, len(lengths), max_len, dqkv_.ptr, T, H,
                                   Hkv, dh, scale, cos_.ptr, sin_.ptr) != 0
    for buf in (out_, lse_, delta_, dqkv_):
        assert (buf.get(np.uint8, (buf.nbytes,)) == POISON).all(), "a refused launch wrote to an output"
    np.testing.assert_array_equal(qkv_.get_bf16(qkv.shape), qkv)

