"""GPU parity of the candidate-scoring kernels of csrc/decode.hip through their lab hooks: attn_extend (all positions of every candidate in one launch) and
cand_logp (the log-probability of every candidate token from the prefill's logits and the extend pass's row statistics).

attn_extend's contract is bit-identity, bf16 and fp32, with attn_decode_shared run once per position with step = p + 1 on the same cache. One launch holds
prompts of 1, 15, 16, 17, 33, 128 and 257 tokens and candidates of 1, 2, 3, 5 and 15 positions (fewer than P positions, a non-multiple of P, several passes),
two candidates sharing one prompt, laid out with gaps between the prompts and between the tails. Every cache row outside the prompts and tails, every tail row
behind a candidate's last position, and the whole output are NaN: a read past a candidate's keys or an element no lane writes shows. One case is also held to
exact float64 attention inside the bound of tests/test_decode_kernels_gpu.py (at most 1.5 x the causal kernel's distance from fp64 on the same rows plus one
ulp x rms)."""
import numpy as np
import pytest

from oracle import ops_np as O
from test_decode_kernels_gpu import exact_last_rows, split
from test_kernels_gpu import BF_ULP, L, report  # noqa: F401  (L: the module fixture)

gpu = pytest.mark.gpu

LENS = (1, 15, 16, 17, 33, 128, 257)
# (prompt, positions): every count of positions on a short and on a long prompt; prompts 2, 5 and 6 carry two candidates each
CANDS = [(0, 15), (0, 1), (1, 2), (2, 3), (2, 5), (3, 1), (4, 5), (5, 15), (5, 2), (6, 3), (6, 15)]
CASES = [(4, 2, 128), (2, 2, 64), (6, 2, 128), (7, 1, 128), (8, 1, 64)]   # G = 2 (P = 4), 1 (8), 3 padded to 4 (2), 7 (1), 8 (1)
GAP = 2   # unused cache rows behind every prompt and every tail


def layout():
    """geo [n, 5] = {pre_row0, len, tail_row0, q_row0, n_pos} and the cache's row count"""
    pre0, row = [], 0
    for n in LENS:
        pre0.append(row)
        row += n + GAP
    geo, q0 = [], 0
    for s, n_pos in CANDS:
        geo.append((pre0[s], LENS[s], row, q0, n_pos))
        row += n_pos + GAP
        q0 += n_pos
    return np.array(geo, np.int32), row, q0


def make_inputs(H, Hkv, dh, seed, bf16):
    """queries [R, H, dh] of every (candidate, position); keys / values of the prompts [sum LENS, Hkv, dh] and of the candidates' own rows [R, Hkv, dh]. Planted:
    position 0 of the first candidate on the 257-token prompt has its largest score for head 0 on its OWN row (the last key: every accumulator is rescaled at the
    end), its position 1 on the prompt's key 0"""
    rng = np.random.default_rng(seed)
    geo, _, R = layout()
    Tp = sum(LENS)
    q = rng.standard_normal((R, H, dh)).astype(np.float32)
    kp, vp = rng.standard_normal((Tp, Hkv, dh)).astype(np.float32), rng.standard_normal((Tp, Hkv, dh)).astype(np.float32)
    kt, vt = rng.standard_normal((R, Hkv, dh)).astype(np.float32), rng.standard_normal((R, Hkv, dh)).astype(np.float32)
    c = [i for i, (s, _) in enumerate(CANDS) if s == 6][0]
    q0 = int(geo[c, 3])
    kt[q0, 0] = 2.0 * q[q0, 0]
    kp[sum(LENS[:6]), 0] = 3.0 * q[q0 + 1, 0]
    r = (lambda a: O.rbf(a)) if bf16 else (lambda a: a)
    return r(q), r(kp), r(vp), r(kt), r(vt)


def build_cache(L, geo, cap, kp, vp, kt, vt, bf16):
    wkv = kp.shape[1] * kp.shape[2]
    kc = np.full((cap, wkv), np.nan, np.float32)
    vc = kc.copy()
    o = 0
    for s, n in enumerate(LENS):
        r0 = int(geo[[i for i, (ps, _) in enumerate(CANDS) if ps == s][0], 0])
        kc[r0:r0 + n], vc[r0:r0 + n] = kp[o:o + n].reshape(n, wkv), vp[o:o + n].reshape(n, wkv)
        o += n
    for pre0, ln, tail0, q0, n_pos in geo:
        kc[tail0:tail0 + n_pos], vc[tail0:tail0 + n_pos] = kt[q0:q0 + n_pos].reshape(n_pos, wkv), vt[q0:q0 + n_pos].reshape(n_pos, wkv)
    if bf16:
        kb, vb = L.to_bf16_bits(np.nan_to_num(kc)), L.to_bf16_bits(np.nan_to_num(vc))
        kb[np.isnan(kc)] = 0x7FC0
        vb[np.isnan(vc)] = 0x7FC0
        return kb, vb
    return kc, vc


def run_extend(L, H, Hkv, dh, bf16, seed):
    lib = L.load_lab()
    geo, cap, R = layout()
    q, kp, vp, kt, vt = make_inputs(H, Hkv, dh, seed, bf16)
    kc, vc = build_cache(L, geo, cap, kp, vp, kt, vt, bf16)
    esz, ld = (2 if bf16 else 4), (H + 2 * Hkv) * dh   # the queries sit in the q columns of a qkv-wide row, as in the engine
    qrow = np.zeros((R, ld), np.float32)
    qrow[:, : H * dh] = q.reshape(R, H * dh)
    dev = L.dev_bf16 if bf16 else L.dev_f32
    bits = (lambda b, shape: b.get(np.uint16, shape)) if bf16 else (lambda b, shape: b.get(np.uint32, shape))
    kc_, vc_, q_, geo_ = L.DevBuf(kc), L.DevBuf(vc), dev(qrow), L.DevBuf(geo)
    scale = 1.0 / np.sqrt(dh)
    nan_out = np.full((R, H * dh), 0x7FC0 if bf16 else 0x7FC00000, np.uint16 if bf16 else np.uint32)
    o_ = L.DevBuf(nan_out)
    ext = lib.tst_k_attn_extend if bf16 else lib.tst_k_attn_extend_f32
    assert ext(q_.ptr, ld, kc_.ptr, vc_.ptr, geo_.ptr, len(geo), R, o_.ptr, H * dh, H, Hkv, dh, scale, cap) == 0
    got = bits(o_, (R, H * dh))
    # the cache is read-only
    np.testing.assert_array_equal(kc_.get(kc.dtype, kc.shape).view(np.uint8), kc.view(np.uint8))
    return dict(lib=lib, geo=geo, cap=cap, R=R, q=q, kp=kp, vp=vp, kt=kt, vt=vt, kc_=kc_, vc_=vc_, qrow=qrow, got=got, ld=ld, scale=scale, dev=dev, bits=bits)


def as_float(L, bits, bf16):
    return L.from_bf16_bits(bits) if bf16 else bits.view(np.float32)


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,Hkv,dh", CASES)
def test_attn_extend_is_bit_identical_to_one_shared_decode_step_per_position(L, H, Hkv, dh, bf16):
    x = run_extend(L, H, Hkv, dh, bf16, seed=11 * H + Hkv + dh)
    lib, geo, R, got = x["lib"], x["geo"], x["R"], x["got"]
    assert np.isfinite(as_float(L, got, bf16)).all(), "NaN reached the output: a read outside a candidate's keys or an element no lane writes"
    dec = lib.tst_k_attn_decode_shared if bf16 else lib.tst_k_attn_decode_shared_f32
    n_checked = 0
    for p in range(int(geo[:, 4].max())):
        live = [c for c in range(len(geo)) if geo[c, 4] > p]
        rows = np.array([geo[c, 3] + p for c in live])
        g = np.concatenate([[len(live), 16, 1]] + [geo[c, :3] for c in live]).astype(np.int32)
        q_, g_ = x["dev"](np.ascontiguousarray(x["qrow"][rows])), L.DevBuf(g)
        o_ = L.DevBuf(nbytes=len(live) * H * dh * got.itemsize)
        assert dec(q_.ptr, x["ld"], x["kc_"].ptr, x["vc_"].ptr, g_.ptr, len(live), p + 1, o_.ptr, H * dh, H, Hkv, dh, x["scale"], x["cap"]) == 0
        want = x["bits"](o_, (len(live), H * dh))
        assert np.isfinite(as_float(L, want, bf16)).all()
        np.testing.assert_array_equal(got[rows], want, err_msg=f"position {p}")
        n_checked += len(live)
    assert n_checked == R


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_attn_extend_against_fp64_and_the_causal_kernel(L, bf16):
    H, Hkv, dh = 4, 2, 128
    x = run_extend(L, H, Hkv, dh, bf16, seed=5)
    lib, geo, R = x["lib"], x["geo"], x["R"]
    got = as_float(L, x["got"], bf16).reshape(R, H, dh)
    # every (candidate, position) as a causal sequence of its own: the prompt's rows, then the candidate's rows 0 .. p; only its last row is compared
    starts = np.concatenate([[0], np.cumsum(LENS)])
    q_l, k_l, v_l, cu = [], [], [], [0]
    rng = np.random.default_rng(1)
    for (s, n_pos), (pre0, ln, tail0, q0, _) in zip(CANDS, geo):
        for p in range(n_pos):
            n = ln + p + 1
            qq = rng.standard_normal((n, H, dh)).astype(np.float32)
            qq = O.rbf(qq) if bf16 else qq
            qq[-1] = x["q"][q0 + p]
            q_l.append(qq)
            k_l.append(np.concatenate([x["kp"][starts[s]:starts[s] + ln], x["kt"][q0:q0 + p + 1]]))
            v_l.append(np.concatenate([x["vp"][starts[s]:starts[s] + ln], x["vt"][q0:q0 + p + 1]]))
            cu.append(cu[-1] + n)
    q, k, v, cu = np.concatenate(q_l), np.concatenate(k_l), np.concatenate(v_l), np.array(cu, np.int32)
    T = len(q)
    exact = exact_last_rows(q, k, v, cu)
    qkv = np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1)
    esz = 2 if bf16 else 4
    qkv_, cu_ = x["dev"](qkv), L.DevBuf(cu)
    out_, lse_ = L.DevBuf(nbytes=T * H * dh * esz), L.DevBuf(nbytes=H * T * 4)
    fwd = lib.tst_k_attn_fwd if bf16 else lib.tst_k_attn_fwd_f32
    assert fwd(qkv_.ptr, qkv.shape[1], cu_.ptr, R, int(np.diff(cu).max()), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, x["scale"]) == 0
    causal = (out_.get_bf16((T, H, dh)) if bf16 else out_.get(np.float32, (T, H, dh)))[cu[1:] - 1]
    rms = float(np.sqrt(np.mean(exact * exact)))
    d_ext = float(np.abs(got.astype(np.float64) - exact).max())
    d_causal = float(np.abs(causal.astype(np.float64) - exact).max())
    ulp = BF_ULP if bf16 else 2.0 ** -23
    report(f"attn_extend {'bf16' if bf16 else 'f32'} H{H}/{Hkv} dh{dh}", extend_max_abs=d_ext, causal_max_abs=d_causal, rms=rms)
    print(f"attn_extend {'bf16' if bf16 else 'f32'}: extend {d_ext:.3e} causal kernel {d_causal:.3e} from fp64, rms {rms:.3e}")
    assert d_ext <= 1.5 * d_causal + ulp * rms, f"extend {d_ext:.3e} from fp64, the causal kernel's last rows {d_causal:.3e} (rms {rms:.3e})"


@gpu
def test_attn_extend_hook_refuses_shapes_the_kernel_does_not_cover(L):
    lib = L.load_lab()
    b = L.DevBuf(nbytes=4096)
    assert lib.tst_k_attn_extend(b.ptr, 1152, b.ptr, b.ptr, b.ptr, 1, 1, b.ptr, 1152, 9, 1, 128, 1.0, 4) != 0   # 9 query heads per kv head
    assert lib.tst_k_attn_extend(b.ptr, 96, b.ptr, b.ptr, b.ptr, 1, 1, b.ptr, 96, 1, 1, 96, 1.0, 4) != 0        # head_dim 96
    assert lib.tst_k_attn_extend_f32(b.ptr, 132, b.ptr, b.ptr, b.ptr, 1, 1, b.ptr, 128, 1, 1, 128, 1.0, 4) != 0  # ld not a multiple of 8
    # a candidate whose rows lie outside the cache or the query rows is skipped: the output stays as it was
    geo = np.array([[0, 2, 3, 0, 2], [0, 2, 2, 1, 1]], np.int32)   # tail 3 .. 5 of a 4-row cache; query row 1 of 1
    o = np.full((2, 128), 0x7FC0, np.uint16)
    z = L.DevBuf(np.zeros((4, 128), np.uint16))
    g_, o_ = L.DevBuf(geo), L.DevBuf(o)
    assert lib.tst_k_attn_extend(z.ptr, 128, z.ptr, z.ptr, g_.ptr, 2, 1, o_.ptr, 128, 1, 1, 128, 1.0, 4) == 0
    np.testing.assert_array_equal(o_.get(np.uint16, o.shape), o)


@gpu
@pytest.mark.parametrize("V", [5, 517, 128256])
def test_cand_logp_against_numpy(L, V):
    lib = L.load_lab()
    rng = np.random.default_rng(V)
    ld = (V + 63) // 64 * 64 + 64   # padded rows
    S, Re = 3, 7
    logits0 = np.full((S, ld), np.nan, np.float32)
    logits0[:, :V] = rng.standard_normal((S, V)).astype(np.float32) * 3
    stats0 = rng.standard_normal((S, 4)).astype(np.float32)
    stats1 = rng.standard_normal((Re, 4)).astype(np.float32)
    # candidates: {prompt, first token, later tokens}: the first one starts on the LAST vocabulary entry; a one-token candidate; two on one prompt
    firsts = [(0, V - 1, 3), (0, 0, 0), (1, V // 2, 2), (2, min(3, V - 1), 2), (2, V - 1, 0)]
    src, want, r = [], [], 0
    for s, tok, n_later in firsts:
        src.append((s, tok))
        want.append(np.float32(logits0[s, tok]) - stats0[s, 0])
        for _ in range(n_later):
            src.append((r, -1))
            want.append(stats1[r, 1] - stats1[r, 0])
            r += 1
    assert r == Re
    src, want = np.array(src, np.int32), np.array(want, np.float32)
    n = len(src)
    lg_, s0_, s1_, src_ = L.DevBuf(logits0), L.DevBuf(stats0), L.DevBuf(stats1), L.DevBuf(src)
    out_ = L.DevBuf(np.full(n, np.nan, np.float32))
    assert lib.tst_k_cand_logp(lg_.ptr, ld, V, s0_.ptr, S, src_.ptr, n, 0, out_.ptr) == 0
    half = out_.get(np.float32, (n,))
    first = src[:, 1] >= 0
    np.testing.assert_array_equal(half[first], want[first])
    assert np.isnan(half[~first]).all(), "phase 0 wrote a later token"
    # phase 1 reads the extend pass's statistics; the logits buffer is overwritten by then (NaN here): it must not be read
    lg2_ = L.DevBuf(np.full((Re, ld), np.nan, np.float32))
    assert lib.tst_k_cand_logp(lg2_.ptr, ld, V, s1_.ptr, Re, src_.ptr, n, 1, out_.ptr) == 0
    np.testing.assert_array_equal(out_.get(np.float32, (n,)), want)
    # refused: a padded width below V, an unknown phase
    assert lib.tst_k_cand_logp(lg_.ptr, V - 1, V, s0_.ptr, S, src_.ptr, n, 0, out_.ptr) != 0
    assert lib.tst_k_cand_logp(lg_.ptr, ld, V, s0_.ptr, S, src_.ptr, n, 2, out_.ptr) != 0
