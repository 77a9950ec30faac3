"""GPU parity of the sampled generation's kernels of csrc/decode.hip through their lab hooks: sample_rows (Gumbel-max draw + log-probability of a fp32 logits
row, Philox4x32-10 noise) and attn_decode_shared (a decode row against its prompt's shared cache rows, then its own tail), bf16 and fp32.

sample_rows is held against tests/sample_oracle.py: the same Philox words, the noise and the scores in float64. A draw is decidable when the reference's top-1 /
top-2 gap exceeds sample_oracle.band(temperature); every decidable draw must be equal, at most 1 % of a case's draws may be undecidable (the reference for the
seeds used here has none, asserted), logp within 1e-5 max(1, |logp|) of float64.

attn_decode_shared is held (a) bit for bit against tst_k_attn_decode[_f32] on a cache that holds the same keys contiguously, and (b) against exact float64
attention with the bound tests/test_decode_kernels_gpu.py uses for attn_decode: at most 1.5 x the distance of the existing causal kernel's last rows plus one ulp
x rms. Cache rows no key lives in are NaN."""
import numpy as np
import pytest

import sample_oracle as SO
from oracle import ops_np as O
from test_kernels_gpu import BF_ULP, L  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

MAX_NEW = 8
SEEDS = np.array([0x0123456789ABCDEF, 0xFFFFFFFF00000001, 7], np.uint64)   # one per source row: both key words differ, one high word is 0
LENS = (10, 1, 130)


def geo_of(n, lens=LENS, max_new=MAX_NEW):
    S = len(lens)
    T = int(np.sum(lens))
    cu = np.concatenate([[0], np.cumsum(lens)])
    rows = [(int(cu[s]), int(lens[s]), T + (s * n + i) * max_new) for s in range(S) for i in range(n)]
    return np.concatenate([[S * n, max_new, n], np.array(rows).reshape(-1)]).astype(np.int32)


def seed_words(seeds):
    s = np.asarray(seeds, np.uint64)
    return np.stack([s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)], 1).astype(np.uint32).view(np.int32).reshape(-1)


def run_sample_rows(L, logits, V, n, step, temperature, seeds=SEEDS):
    lib = L.load_lab()
    R = len(seeds) * n
    ld = logits.shape[1]
    geo_, seeds_, lg_ = L.DevBuf(geo_of(n)), L.DevBuf(seed_words(seeds)), L.DevBuf(np.ascontiguousarray(logits, np.float32))
    tok_, logp_ = L.DevBuf(np.full((R, MAX_NEW), -7, np.int32)), L.DevBuf(np.full((R, MAX_NEW), 7.0, np.float32))
    ids_, pos_, lab_ = (L.DevBuf(np.full(R, -7, np.int32)) for _ in range(3))
    assert lib.tst_k_sample_rows(lg_.ptr, ld, V, geo_.ptr, seeds_.ptr, R, step, 1.0 / temperature, tok_.ptr, logp_.ptr, ids_.ptr, pos_.ptr, lab_.ptr) == 0
    return (tok_.get(np.int32, (R, MAX_NEW)), logp_.get(np.float32, (R, MAX_NEW)), ids_.get(np.int32, (R,)), pos_.get(np.int32, (R,)), lab_.get(np.int32, (R,)))


def reference(logits, V, n, step, temperature, seeds=SEEDS):
    S = len(seeds)
    src = np.repeat(np.arange(S), n) if step == 0 else np.arange(S * n)
    g = np.stack([SO.gumbel(seeds[r // n], V, step, r % n) for r in range(S * n)])
    return SO.draw(np.asarray(logits[src, :V], np.float64), temperature, g)


def make_logits(V, rows, pad, seed):
    ld = (V + 3) // 4 * 4 + pad
    lg = np.full((rows, ld), 1e30, np.float32)   # padding columns V <= c < ld: never candidates
    lg[:, :V] = (1.5 * np.random.default_rng(seed).standard_normal((rows, V))).astype(np.float32)
    return lg


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("V,pad", [(5, 0), (257, 4), (50257, 0), (128256, 8)])
def test_sample_rows_against_the_numpy_gumbel_argmax(L, V, pad, n, step, temperature):
    S = len(SEEDS)
    R = S * n
    lg = make_logits(V, S if step == 0 else R, pad, seed=V + 10 * n + step)
    ref_tok, ref_logp, gap = reference(lg, V, n, step, temperature)
    assert (gap > SO.band(temperature)).all(), "the reference of this case has an undecidable draw: choose other inputs"
    tok, logp, d_ids, d_pos, lab = run_sample_rows(L, lg, V, n, step, temperature)
    decidable = gap > SO.band(temperature)
    d = np.abs(logp[:, step] - ref_logp) / np.maximum(1.0, np.abs(ref_logp))
    print(f"sample_rows V={V} ld={lg.shape[1]} n={n} step={step} T={temperature}: equal {int((tok[:, step] == ref_tok).sum())}/{R}, smallest gap {gap.min():.3e}, "
          f"|d logp| / max(1, |logp|) <= {d.max():.3e}")
    assert (~decidable).sum() <= 0.01 * R
    np.testing.assert_array_equal(tok[decidable, step], ref_tok[decidable])
    assert (tok[:, step] < V).all() and (tok[:, step] >= 0).all()
    assert (d <= 1e-5).all()
    # only column `step` of the outputs is written; the next step's inputs are as specified
    other = np.arange(MAX_NEW) != step
    assert (tok[:, other] == -7).all() and (logp[:, other] == 7.0).all()
    np.testing.assert_array_equal(d_ids, tok[:, step])
    np.testing.assert_array_equal(d_pos, np.repeat(LENS, n) + step)
    np.testing.assert_array_equal(lab, np.arange(R))
    # two runs: the same bits
    tok2, logp2, _, _, _ = run_sample_rows(L, lg, V, n, step, temperature)
    np.testing.assert_array_equal(tok2, tok)
    np.testing.assert_array_equal(logp2.view(np.uint32), logp.view(np.uint32))
    if step == 0 and n > 1 and V >= 50257:
        # the samples of one prompt read the same logits row and differ through the sample index only (a small vocabulary may draw one token four times)
        assert all(len(set(tok[s * n:(s + 1) * n, 0])) > 1 for s in range(S))


def test_an_exact_tie_of_the_perturbed_scores_goes_to_the_first_index(L):
    """two columns whose Philox words agree in their upper 23 bits carry the same noise; with equal logits above everything else their scores are the same fp32
    number, and the draw is the lower column"""
    V, n, step = 50257, 1, 0
    words = SO.noise_words(SEEDS[0], V, step, 0) >> np.uint32(9)
    order = np.argsort(words, kind="stable")
    same = np.flatnonzero(words[order][1:] == words[order][:-1])
    if len(same) == 0:
        pytest.skip("no two columns of this seed share their noise")
    pairs = [(int(min(order[k], order[k + 1])), int(max(order[k], order[k + 1]))) for k in same]
    lg = make_logits(V, len(SEEDS), 0, seed=5)
    for a, b in pairs[:4]:
        x = lg.copy()
        x[0, a] = x[0, b] = 40.0
        tok, _, _, _, _ = run_sample_rows(L, x, V, n, step, 1.0)
        assert tok[0, 0] == a, f"columns {a} and {b} tie: the draw must be {a}, got {tok[0, 0]}"
        x[0, a] = np.nextafter(np.float32(40.0), np.float32(0.0))   # ... and the tie rule is not a preference for low columns
        tok, _, _, _, _ = run_sample_rows(L, x, V, n, step, 1.0)
        assert tok[0, 0] == b


def test_sample_rows_refuses_what_the_kernel_does_not_cover(L):
    lib = L.load_lab()
    b = L.DevBuf(nbytes=4096)
    args = lambda ld, V, j, it: (b.ptr, ld, V, b.ptr, b.ptr, 1, j, it, b.ptr, b.ptr, b.ptr, b.ptr, b.ptr)  # noqa: E731
    assert lib.tst_k_sample_rows(*args(6, 5, 0, 1.0)) != 0     # ld not a multiple of 4
    assert lib.tst_k_sample_rows(*args(4, 5, 0, 1.0)) != 0     # ld under V rounded up to 4
    assert lib.tst_k_sample_rows(*args(8, 5, -1, 1.0)) != 0    # negative step
    assert lib.tst_k_sample_rows(*args(8, 5, 0, 0.0)) != 0     # no temperature


# ------------------------------------------------------------------------------------------------ shared-prefix decode attention
PREFIX = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
TAILS = (0, 1, 2, 8)
N_S = 3
HKV = 2


def exact_rows(q, keys_k, keys_v, H, dh):
    """float64 attention of query q [H, dh] over keys [n, Hkv, dh]"""
    G = H // keys_k.shape[1]
    out = np.zeros((H, dh))
    for h in range(H):
        sc = (keys_k[:, h // G].astype(np.float64) @ q[h].astype(np.float64)) / np.sqrt(dh)
        p = np.exp(sc - sc.max())
        out[h] = (p / p.sum()) @ keys_v[:, h // G].astype(np.float64)
    return out


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_shared_prefix_attention_equals_the_contiguous_kernel_and_fp64(L, G, dh, bf16):
    lib = L.load_lab()
    H, wkv, esz = G * HKV, HKV * dh, 2 if bf16 else 4
    ld = (H + 2 * HKV) * dh
    scale = 1.0 / np.sqrt(dh)
    rnd = (lambda x: O.rbf(x)) if bf16 else (lambda x: x.astype(np.float32))
    dev = L.dev_bf16 if bf16 else L.dev_f32
    get = (lambda b, shape: b.get_bf16(shape)) if bf16 else (lambda b, shape: b.get(np.float32, shape))
    bits = (lambda x: L.to_bf16_bits(x)) if bf16 else (lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32))
    nan_bits = np.uint16(0x7FC0) if bf16 else np.uint32(0x7FC00000)
    rng = np.random.default_rng(100 * G + dh + int(bf16))
    P, T = len(PREFIX), int(np.sum(PREFIX))
    R = P * N_S
    cu = np.concatenate([[0], np.cumsum(PREFIX)]).astype(np.int64)
    pk, pv = rnd(rng.standard_normal((T, HKV, dh))), rnd(rng.standard_normal((T, HKV, dh)))
    tk, tv = rnd(rng.standard_normal((R, MAX_NEW, HKV, dh))), rnd(rng.standard_normal((R, MAX_NEW, HKV, dh)))
    q = rnd(rng.standard_normal((R, H, dh)))
    # the shared layout: prompts packed at rows 0 .. T, the tail of row r at T + r MAX_NEW. Per step the cache holds a row's first `step` tail rows only: the tail
    # rows behind them, which no key lives in yet, and the rows behind the last tail are NaN
    cap = T + R * MAX_NEW + 5
    kc = np.full((cap, wkv), nan_bits)
    vc = kc.copy()
    kc[:T], vc[:T] = bits(pk.reshape(T, wkv)), bits(pv.reshape(T, wkv))
    kc[T:T + R * MAX_NEW], vc[T:T + R * MAX_NEW] = bits(tk.reshape(R * MAX_NEW, wkv)), bits(tv.reshape(R * MAX_NEW, wkv))
    geo = np.concatenate([[R, MAX_NEW, N_S]] + [[int(cu[r // N_S]), PREFIX[r // N_S], T + r * MAX_NEW] for r in range(R)]).astype(np.int32)
    geo_ = L.DevBuf(geo)
    unwritten = lambda t: (T + np.arange(R)[:, None] * MAX_NEW + np.arange(t, MAX_NEW)[None]).reshape(-1)   # noqa: E731  (tail rows a step-t cache does not hold yet)
    qrows = np.zeros((R, ld), np.float32)
    qrows[:, :H * dh] = q.reshape(R, -1)
    q_ = dev(qrows)
    shared = lib.tst_k_attn_decode_shared if bf16 else lib.tst_k_attn_decode_shared_f32
    contig = lib.tst_k_attn_decode if bf16 else lib.tst_k_attn_decode_f32
    fwd = lib.tst_k_attn_fwd if bf16 else lib.tst_k_attn_fwd_f32
    for t in TAILS:
        kc_t, vc_t = kc.copy(), vc.copy()
        kc_t[unwritten(t)] = vc_t[unwritten(t)] = nan_bits
        kc_, vc_ = L.DevBuf(kc_t), L.DevBuf(vc_t)
        o_ = L.DevBuf(np.full((R, H * dh), nan_bits))
        assert shared(q_.ptr, ld, kc_.ptr, vc_.ptr, geo_.ptr, R, t, o_.ptr, H * dh, H, HKV, dh, scale, cap) == 0
        got = get(o_, (R, H, dh))
        assert np.isfinite(got).all(), "NaN reached the output: a read outside a row's keys, or an element no lane writes"
        # (a) the same keys contiguously: sequence r = its prompt's keys then its t own, with one unread NaN row behind each (max_new = 1)
        n_r = np.array([PREFIX[r // N_S] + t for r in range(R)])
        cu_c = np.concatenate([[0], np.cumsum(n_r)]).astype(np.int32)
        Tc = int(cu_c[-1])
        seq_k = [np.concatenate([pk[cu[r // N_S]:cu[r // N_S + 1]], tk[r, :t]]) for r in range(R)]
        seq_v = [np.concatenate([pv[cu[r // N_S]:cu[r // N_S + 1]], tv[r, :t]]) for r in range(R)]
        kcc = np.full((Tc + R, wkv), nan_bits)
        vcc = kcc.copy()
        rows_c = np.concatenate([np.arange(cu_c[r], cu_c[r + 1]) + r for r in range(R)])
        kcc[rows_c], vcc[rows_c] = bits(np.concatenate(seq_k).reshape(Tc, wkv)), bits(np.concatenate(seq_v).reshape(Tc, wkv))
        meta_ = L.DevBuf(np.concatenate([[R, 1], cu_c, n_r]).astype(np.int32))
        kcc_, vcc_ = L.DevBuf(kcc), L.DevBuf(vcc)
        oc_ = L.DevBuf(np.full((R, H * dh), nan_bits))
        assert contig(q_.ptr, ld, kcc_.ptr, vcc_.ptr, meta_.ptr, R, 0, oc_.ptr, H * dh, H, HKV, dh, scale, Tc + R) == 0
        want = get(oc_, (R, H, dh))
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"tail {t}")
        # (b) fp64, with the causal kernel's last rows as the yardstick (tests/test_decode_kernels_gpu.py)
        exact = np.stack([exact_rows(q[r], seq_k[r], seq_v[r], H, dh) for r in range(R)])
        qkv = np.zeros((Tc, ld), np.float32)
        qkv[:, :H * dh] = rnd(rng.standard_normal((Tc, H * dh)))
        qkv[cu_c[1:] - 1, :H * dh] = q.reshape(R, -1)
        qkv[:, H * dh:H * dh + wkv], qkv[:, H * dh + wkv:] = np.concatenate(seq_k).reshape(Tc, wkv), np.concatenate(seq_v).reshape(Tc, wkv)
        qkv_, cuc_ = dev(qkv), L.DevBuf(cu_c)
        out_, lse_ = L.DevBuf(nbytes=Tc * H * dh * esz), L.DevBuf(nbytes=H * Tc * 4)
        assert fwd(qkv_.ptr, ld, cuc_.ptr, R, int(n_r.max()), out_.ptr, H * dh, lse_.ptr, Tc, H, HKV, dh, scale) == 0
        causal = get(out_, (Tc, H, dh))[cu_c[1:] - 1]
        rms = float(np.sqrt(np.mean(exact * exact)))
        d_dec, d_causal = float(np.abs(got.astype(np.float64) - exact).max()), float(np.abs(causal.astype(np.float64) - exact).max())
        ulp = BF_ULP if bf16 else 2.0 ** -23
        print(f"attn_decode_shared {'bf16' if bf16 else 'f32'} G{G} dh{dh} tail {t}: {d_dec:.3e} from fp64, causal kernel {d_causal:.3e}, rms {rms:.3e}")
        assert d_dec <= 1.5 * d_causal + ulp * rms, f"tail {t}: {d_dec:.3e} from fp64, the causal kernel's last rows {d_causal:.3e} (rms {rms:.3e})"
    # the caches are read-only
    np.testing.assert_array_equal(kc_.get(kc.dtype, kc.shape), kc_t)


def test_shared_prefix_attention_skips_rows_outside_the_cache(L):
    """the guards return without reading: a prompt or a tail that would leave the cache leaves the output row as it was"""
    lib = L.load_lab()
    dh, H, cap = 64, 2, 16
    wkv, ld = HKV * dh, (H + 2 * HKV) * dh
    kc_ = L.dev_f32(np.ones((cap, wkv), np.float32))
    q_ = L.dev_f32(np.ones((4, ld), np.float32))
    geo = np.array([4, MAX_NEW, 1, 0, 4, 8, 14, 4, 8, 0, 4, 15, 0, 0, 8], np.int32)   # fine | prompt past the cache | tail past the cache at step 2 | len 0
    o_, geo_ = L.dev_f32(np.full((4, H * dh), 5.0, np.float32)), L.DevBuf(geo)
    assert lib.tst_k_attn_decode_shared_f32(q_.ptr, ld, kc_.ptr, kc_.ptr, geo_.ptr, 4, 2, o_.ptr, H * dh, H, HKV, dh, 1.0, cap) == 0
    out = o_.get(np.float32, (4, H * dh))
    np.testing.assert_allclose(out[0], 1.0, rtol=1e-6)
    assert (out[1:] == 5.0).all()
