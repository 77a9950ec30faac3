"""GPU parity of the generation kernels of csrc/decode.hip through their lab hooks: kv_append (bit-exact copy into the cache's row map) and attn_decode
(one query token per sequence against its cached keys), bf16 and fp32.

attn_decode is checked against TWO references on the same inputs: exact float64 attention of every sequence's last query, and the last row per sequence of
the existing causal kernels (tst_k_attn_fwd / tst_k_attn_fwd_f32) -- the last token of a causal sequence attends to all of its keys, which is what a decode
step computes. The bound has the form of tests/test_attention_long_gpu.py check_vs_exact: the decode kernel's largest distance from fp64 is at most 1.5 x
that of the existing kernel's last rows plus one ulp x rms (bf16: 2^-7; fp32: 2^-23). The yardstick is measured in the same test.
One launch holds sequences of 1, 2, 63, 64, 65, 127, 128, 129, 200 and 257 keys (one key, the 16- and 32-key trips of the row groups, partial trips, and
lengths past the 64- and 128-key tiles of the existing kernels), laid out in a cache with room for new tokens behind every sequence. Everything outside the
valid cache rows, and the whole output, is poisoned with 0x7f bytes (~3.4e38): a read past a sequence's keys or an element no lane writes shows."""
import numpy as np
import pytest

from oracle import ops_np as O
from test_kernels_gpu import BF_ULP, L, report  # noqa: F401  (L: the module fixture)

gpu = pytest.mark.gpu   # (test_planted_extremes_are_in_place is a CPU-only guard on the inputs)

POISON = 0x7f
KEYS = (1, 2, 63, 64, 65, 127, 128, 129, 200, 257)
MAX_NEW = 3   # room behind every sequence in the cache: the row map is not the packed one
CASES = [(2, 1, 128), (4, 2, 128), (7, 1, 128), (8, 1, 128), (2, 2, 64), (4, 1, 64)]


def make_inputs(H, Hkv, dh, seed, bf16):
    """packed qkv [T, (H + 2 Hkv) dh] for sequences of KEYS tokens. Planted: in the 200-key sequence the last query's largest score of head 0 is its LAST
    key (every row group's accumulator is rescaled at the end); in the 257-key sequence key 0 dominates head 1's last query (the rest underflows to ~e^-24)"""
    rng = np.random.default_rng(seed)
    T = sum(KEYS)
    cu = np.concatenate([[0], np.cumsum(KEYS)]).astype(np.int32)
    G = H // Hkv
    q = rng.standard_normal((T, H, dh)).astype(np.float32)
    k = rng.standard_normal((T, Hkv, dh)).astype(np.float32)
    v = rng.standard_normal((T, Hkv, dh)).astype(np.float32)
    last = cu[1:] - 1
    i200, i257 = KEYS.index(200), KEYS.index(257)
    k[last[i200], 0] = 2.0 * q[last[i200], 0]
    u = rng.standard_normal(dh).astype(np.float32)
    k[cu[i257], 1 // G] = u
    q[last[i257], 1] = 3.0 * u + 0.3 * rng.standard_normal(dh).astype(np.float32)
    qkv = np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1)
    return (O.rbf(qkv) if bf16 else qkv.astype(np.float32)), cu


def split(qkv, H, Hkv, dh):
    T = qkv.shape[0]
    return (qkv[:, : H * dh].reshape(T, H, dh), qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh))


def exact_last_rows(q, k, v, cu):
    """float64 attention of every sequence's LAST query over all of its keys: [S, H, dh]"""
    S, H, dh = len(cu) - 1, q.shape[1], q.shape[2]
    G = H // k.shape[1]
    out = np.zeros((S, H, dh))
    for s in range(S):
        s0, s1 = int(cu[s]), int(cu[s + 1])
        for h in range(H):
            sc = (k[s0:s1, h // G].astype(np.float64) @ q[s1 - 1, h].astype(np.float64)) / np.sqrt(dh)
            p = np.exp(sc - sc.max())
            out[s, h] = (p / p.sum()) @ v[s0:s1, h // G].astype(np.float64)
    return out


def cache_rows(cu, max_new):
    """cache row of every packed token: cu[s] + s max_new + p"""
    return np.concatenate([np.arange(int(cu[s]), int(cu[s + 1])) + s * max_new for s in range(len(cu) - 1)]).astype(np.int32)


def meta_of(cu, max_new, lens=None):
    S = len(cu) - 1
    lens = np.diff(cu) if lens is None else lens
    return np.concatenate([[S, max_new], cu, lens]).astype(np.int32)


def test_planted_extremes_are_in_place():
    """a guard on make_inputs (CPU only): the maxima sit where the docstring says"""
    H, Hkv, dh = 4, 2, 128
    qkv, cu = make_inputs(H, Hkv, dh, 1, True)
    q, k, _ = split(qkv, H, Hkv, dh)
    i200, i257 = KEYS.index(200), KEYS.index(257)
    s0, s1 = int(cu[i200]), int(cu[i200 + 1])
    sc = (k[s0:s1, 0].astype(np.float64) @ q[s1 - 1, 0]) / np.sqrt(dh)
    assert int(np.argmax(sc)) == 199 and sc[199] - np.sort(sc)[-2] > 10
    s0, s1 = int(cu[i257]), int(cu[i257 + 1])
    sc = (k[s0:s1, 0].astype(np.float64) @ q[s1 - 1, 1]) / np.sqrt(dh)
    assert int(np.argmax(sc)) == 0 and sc[0] - np.sort(sc)[-2] > 10


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,Hkv,dh", CASES)
def test_attn_decode_against_fp64_and_the_causal_kernel(L, H, Hkv, dh, bf16):
    lib = L.load_lab()
    qkv, cu = make_inputs(H, Hkv, dh, seed=7 * H + Hkv + dh, bf16=bf16)
    T, ld = qkv.shape
    S, wkv, esz = len(KEYS), Hkv * dh, 2 if bf16 else 4
    scale = 1.0 / np.sqrt(dh)
    dev = L.dev_bf16 if bf16 else L.dev_f32
    get = (lambda b, shape: b.get_bf16(shape)) if bf16 else (lambda b, shape: b.get(np.float32, shape))
    q, k, v = split(qkv, H, Hkv, dh)
    exact = exact_last_rows(q, k, v, cu)
    # the yardstick: the existing causal kernel's last row of every sequence
    qkv_, cu_ = dev(qkv), L.DevBuf(cu)
    out_, lse_ = L.DevBuf(nbytes=T * H * dh * esz), L.DevBuf(nbytes=H * T * 4)
    fwd = lib.tst_k_attn_fwd if bf16 else lib.tst_k_attn_fwd_f32
    assert fwd(qkv_.ptr, ld, cu_.ptr, S, max(KEYS), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    causal = get(out_, (T, H, dh))[cu[1:] - 1]
    # the cache: valid rows at cu[s] + s MAX_NEW + p, poison everywhere else
    cap = T + S * MAX_NEW
    rows = cache_rows(cu, MAX_NEW)
    if bf16:
        kc = np.full((cap, wkv), POISON * 257, np.uint16)
        vc = kc.copy()
        kc[rows], vc[rows] = L.to_bf16_bits(k.reshape(T, wkv)), L.to_bf16_bits(v.reshape(T, wkv))
    else:
        kc = np.full((cap, wkv), POISON * 0x01010101, np.uint32).view(np.float32)
        vc = kc.copy()
        kc[rows], vc[rows] = k.reshape(T, wkv), v.reshape(T, wkv)
    kc_, vc_ = L.DevBuf(kc), L.DevBuf(vc)
    q_ = dev(np.ascontiguousarray(qkv[cu[1:] - 1]))   # the step's qkv rows [S, ld]: q columns first
    dec = lib.tst_k_attn_decode if bf16 else lib.tst_k_attn_decode_f32
    res = {}
    # step = 0 with the full lengths, and step = 1 with lengths one shorter: the same keys either way
    for step in (0, 1):
        meta_ = L.DevBuf(meta_of(cu, MAX_NEW, np.diff(cu) - step))
        o_ = L.DevBuf(nbytes=S * H * dh * esz)
        assert lib.tst_dev_memset(o_.ptr, POISON, o_.nbytes) == 0
        assert dec(q_.ptr, ld, kc_.ptr, vc_.ptr, meta_.ptr, S, step, o_.ptr, H * dh, H, Hkv, dh, scale, cap) == 0
        res[step] = get(o_, (S, H, dh))
        assert np.isfinite(res[step]).all() and np.abs(res[step]).max() < 1e6, "poison reached the output: a read past a sequence's keys or an unwritten element"
    np.testing.assert_array_equal(res[0], res[1])
    got = res[0]
    rms = float(np.sqrt(np.mean(exact * exact)))
    d_dec = float(np.abs(got.astype(np.float64) - exact).max())
    d_causal = float(np.abs(causal.astype(np.float64) - exact).max())
    ulp = BF_ULP if bf16 else 2.0 ** -23
    report(f"attn_decode {'bf16' if bf16 else 'f32'} H{H}/{Hkv} dh{dh}", decode_max_abs=d_dec, causal_max_abs=d_causal, rms=rms)
    print(f"attn_decode {'bf16' if bf16 else 'f32'} H{H}/{Hkv} dh{dh}: decode {d_dec:.3e} causal kernel {d_causal:.3e} from fp64, rms {rms:.3e}")
    assert d_dec <= 1.5 * d_causal + ulp * rms, f"decode {d_dec:.3e} from fp64, the causal kernel's last rows {d_causal:.3e} (rms {rms:.3e})"
    # the input buffers are read-only
    np.testing.assert_array_equal(kc_.get(kc.dtype, kc.shape).view(np.uint8), kc.view(np.uint8))


@gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,Hkv,dh", [(4, 2, 128), (2, 2, 64), (7, 1, 128)])
def test_kv_append_is_a_bit_exact_copy_into_the_row_map(L, H, Hkv, dh, bf16):
    lib = L.load_lab()
    lens = (1, 5, 64, 130)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, S, wkv, ld = int(cu[-1]), len(lens), Hkv * dh, (H + 2 * Hkv) * dh
    rng = np.random.default_rng(H + dh)
    x = rng.standard_normal((T, ld)).astype(np.float32)
    bits = L.to_bf16_bits(x) if bf16 else x.view(np.uint32)
    cap = T + S * MAX_NEW
    kc_, vc_ = L.DevBuf(nbytes=cap * wkv * bits.itemsize), L.DevBuf(nbytes=cap * wkv * bits.itemsize)
    for b in (kc_, vc_):
        assert lib.tst_dev_memset(b.ptr, POISON, b.nbytes) == 0
    app = lib.tst_k_kv_append if bf16 else lib.tst_k_kv_append_f32
    # the prefill's rows, then one decode step's (row behind each prompt) fed from the first S rows of the same buffer
    rows = cache_rows(cu, MAX_NEW)
    x_, rows_ = L.DevBuf(bits), L.DevBuf(rows)
    assert app(x_.ptr, ld, H * dh, rows_.ptr, kc_.ptr, vc_.ptr, T, Hkv, dh, cap) == 0
    drows = (cu[1:] + np.arange(S) * MAX_NEW).astype(np.int32)
    drows_ = L.DevBuf(drows)
    assert app(x_.ptr, ld, H * dh, drows_.ptr, kc_.ptr, vc_.ptr, S, Hkv, dh, cap) == 0
    want_k = np.full((cap, wkv), POISON * (257 if bf16 else 0x01010101), bits.dtype)
    want_v = want_k.copy()
    want_k[rows], want_v[rows] = bits[:, H * dh: H * dh + wkv], bits[:, H * dh + wkv:]
    want_k[drows], want_v[drows] = bits[:S, H * dh: H * dh + wkv], bits[:S, H * dh + wkv:]
    np.testing.assert_array_equal(kc_.get(bits.dtype, (cap, wkv)), want_k)
    np.testing.assert_array_equal(vc_.get(bits.dtype, (cap, wkv)), want_v)
    np.testing.assert_array_equal(x_.get(bits.dtype, bits.shape), bits)
    # a row outside the cache is skipped, nothing else is touched
    bad_ = L.DevBuf(np.array([cap, -1], np.int32))
    assert app(x_.ptr, ld, H * dh, bad_.ptr, kc_.ptr, vc_.ptr, 2, Hkv, dh, cap) == 0
    np.testing.assert_array_equal(kc_.get(bits.dtype, (cap, wkv)), want_k)


@gpu
def test_decode_hooks_refuse_shapes_the_kernels_do_not_cover(L):
    lib = L.load_lab()
    b = L.DevBuf(nbytes=4096)
    assert lib.tst_k_attn_decode(b.ptr, 1152, b.ptr, b.ptr, b.ptr, 1, 0, b.ptr, 1152, 9, 1, 128, 1.0, 4) != 0    # 9 query heads per kv head
    assert lib.tst_k_attn_decode(b.ptr, 96, b.ptr, b.ptr, b.ptr, 1, 0, b.ptr, 96, 1, 1, 96, 1.0, 4) != 0         # head_dim 96
    assert lib.tst_k_kv_append(b.ptr, 100, 36, b.ptr, b.ptr, b.ptr, 1, 1, 64, 4) != 0                              # ld not a multiple of a 16-byte vector
