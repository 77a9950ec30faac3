"""GPU parity of the fp32 "strict" precision mode (tst_model_cfg.precision = TST_PRECISION_STRICT) -- the north_star check proper:
per-sample s(x) within 1e-3 of the reference, given identical weights, with NO re-negotiated tolerance.

Reference = the installed HF / torch fp32 CPU stack (the upstream repository has no code); its outputs on the deterministic inputs
of tests/golden_inputs.py are the committed fixtures tests/golden/strict_*.npz (tools/make_golden.py `strict`).

Stated tolerances (all four model families: MHA, GQA, Qwen2-bias, GPT-2):
  * fp32 logits vs HF fp32:                       |d| <= 1e-4 absolute (logits are O(1)); argmax identical on every checked row
  * s(x) ingredients, identical weights:          |d softmax over the option ids| <= 1e-3, |d p(answer)| <= 1e-3, `correct` identical
  * 20-step trajectories (LoRA and full fine-tune; clip 1.0, AdamW wd 0.01 with HF's two parameter groups, linear decay, two
    alternating micro-batches): step 1 (identical weights, one forward/backward) within TRAJ_STEP1 relative; step t >= 2 within
    min(TRAJ_CAP, TRAJ_REL * TRAJ_GROWTH**(t-1)) relative + TRAJ_ABS absolute on the loss (the absolute term matters only once a tiny
    model has memorised its two batches: losses of 4e-5 late in a run), twice the relative and ten times the absolute term on the
    gradient norm. Two fp32 implementations
    differ by summation order (~1e-7 relative per reduction); Adam's first updates are sign-like (lr * g / (|g| + eps)), which turns
    that into O(1e-4) parameter differences wherever |g| is tiny, and training amplifies them from step to step -- so the bound grows
    with t (measured maxima over the eight runs: loss 1.3e-3, gradient norm 2.2e-3; profiles/r02_strict_report.txt). The bf16 mode's
    step-2 deviation on the same recipe is 25 %.
  * s(x) of the TRAINED models on the 32-sample held-out set: the same 1e-3 as above (the whole fold: 20 steps, then score).
Kernel-level checks of the two kernels that have their own fp32 index maps (gemm_f32.hip, attn_f32.hip) come first.
"""
import os

import numpy as np
import pytest

import golden_inputs as GI
from oracle import ops_np as O
import families as FAM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "gpurun_out", "strict_report.txt")

LOGIT_TOL = 1e-4
SX_TOL = 1e-3
TRAJ_STEP1, TRAJ_REL, TRAJ_GROWTH, TRAJ_CAP, TRAJ_ABS = 2e-6, 1e-4, 1.5, 5e-3, 2e-6


def report(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load_lab()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ kernels with their own fp32 maps
@pytest.mark.parametrize("M,N,K,K2,with_r,with_bias", [(64, 64, 32, 0, False, False), (155, 256, 256, 0, True, False), (155, 384, 256, 64, True, True),
                                                       (33, 1004, 128, 0, False, False), (1, 64, 4096, 0, False, True), (300, 192, 36, 0, False, False)])
def test_gemm_f32_nt(L, M, N, K, K2, with_r, with_bias):
    rng = np.random.default_rng(M * 7 + N + K)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    A2 = rng.standard_normal((M, K2)).astype(np.float32) if K2 else None
    B2 = rng.standard_normal((N, K2)).astype(np.float32) if K2 else None
    R = rng.standard_normal((M, N)).astype(np.float32) if with_r else None
    bias = rng.standard_normal(N).astype(np.float32) if with_bias else None
    ref = 0.75 * (A.astype(np.float64) @ B.astype(np.float64).T + (A2.astype(np.float64) @ B2.astype(np.float64).T if K2 else 0.0))
    if with_r:
        ref = ref + R
    if with_bias:
        ref = ref + bias
    d = {k: L.dev_f32(v) for k, v in dict(A=A, B=B, A2=A2, B2=B2, R=R, bias=bias).items() if v is not None}
    C_ = L.DevBuf(nbytes=M * N * 4)
    L.load_lab().tst_dev_memset(C_.ptr, 0xFF, M * N * 4)
    g = lambda k: d[k].ptr if k in d else None
    assert L.load_lab().tst_k_gemm_f32_nt(g("A"), K, g("B"), K, g("A2"), K2, g("B2"), K2, C_.ptr, N, g("R"), N, g("bias"), M, N, K, K2, 0.75) == 0
    got = C_.get(np.float32, (M, N))
    err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
    report(f"gemm_f32_nt M{M} N{N} K{K}+{K2} R{int(with_r)} b{int(with_bias)}: max|d|/max|ref| = {err:.2e}")
    assert np.isfinite(got).all() and err <= 2e-6 * max(1.0, np.sqrt(K / 64.0))   # fp32 accumulation over K, fp64 reference


@pytest.mark.parametrize("M,N,T", [(64, 64, 7), (256, 64, 155), (64, 512, 40), (1004, 128, 32), (384, 256, 300)])
def test_gemm_f32_tn(L, M, N, T):
    rng = np.random.default_rng(M + N * 3 + T)
    Tp = (T + 63) // 64 * 64
    P, Q = np.zeros((Tp, M), np.float32), np.zeros((Tp, N), np.float32)
    P[:T], Q[:T] = rng.standard_normal((T, M)), rng.standard_normal((T, N))
    P[T:], Q[T:] = 1e30, -1e30        # rows >= kvalid must not be read into the sum
    ref = 0.5 * (P[:T].astype(np.float64).T @ Q[:T].astype(np.float64))
    P_, Q_, C_ = L.dev_f32(P), L.dev_f32(Q), L.DevBuf(nbytes=M * N * 4)
    assert L.load_lab().tst_k_gemm_f32_tn(P_.ptr, M, Q_.ptr, N, C_.ptr, N, M, N, T, 0.5) == 0
    got = C_.get(np.float32, (M, N))
    err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
    report(f"gemm_f32_tn M{M} N{N} T{T}: max|d|/max|ref| = {err:.2e}")
    assert np.isfinite(got).all() and err <= 2e-6


@pytest.mark.parametrize("lengths,H,Hkv,dh", [((7, 48, 100), 2, 1, 128), ((64, 65, 128, 1), 4, 2, 128), ((130,), 4, 1, 128), ((33, 70), 2, 2, 64)])
def test_attention_f32(L, lengths, H, Hkv, dh):
    rng = np.random.default_rng(sum(lengths) + H + dh)
    T = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ld = (H + 2 * Hkv) * dh
    qkv = rng.standard_normal((T, ld)).astype(np.float32)
    qkv[5 % T, :dh] *= 6.0  # spike one query row: exercises the running-max rescale across key tiles
    do = rng.standard_normal((T, H * dh)).astype(np.float32)
    q = qkv[:, : H * dh].reshape(T, H, dh)
    k = qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh)
    v = qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh)
    out_ref, lse_ref = O.attention_fwd(q, k, v, cu, bf16=False)
    dq_ref, dk_ref, dv_ref = O.attention_bwd(q, k, v, out_ref, do.reshape(T, H, dh), lse_ref, cu, bf16=False)
    qkv_, cu_, do_ = L.dev_f32(qkv), L.DevBuf(cu), L.dev_f32(do)
    out_, lse_, delta_ = L.DevBuf(nbytes=T * H * dh * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4)
    dqkv_ = L.DevBuf(nbytes=T * ld * 4)
    lib = L.load_lab()
    scale = 1.0 / np.sqrt(dh)
    assert lib.tst_k_attn_fwd_f32(qkv_.ptr, ld, cu_.ptr, len(lengths), max(lengths), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    tag = f"L{'_'.join(map(str, lengths))} H{H}/{Hkv} dh{dh}"
    out, lse = out_.get(np.float32, (T, H, dh)), lse_.get(np.float32, (H, T))

    def chk(name, a, b, tol):
        e = float(np.abs(a - b).max() / (np.sqrt(np.mean(b.astype(np.float64) ** 2)) + 1e-30))
        report(f"attn_f32 {name} {tag}: max|d|/rms = {e:.2e}")
        assert np.isfinite(a).all() and e <= tol, (name, e)
    chk("out", out, out_ref, 2e-5)
    chk("lse", lse, lse_ref, 2e-6)
    assert lib.tst_k_attn_bwd_f32(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, len(lengths), max(lengths), dqkv_.ptr, T,
                                  H, Hkv, dh, scale) == 0
    dqkv = dqkv_.get(np.float32, (T, ld))
    chk("dq", dqkv[:, : H * dh].reshape(T, H, dh), dq_ref, 5e-5)
    chk("dk", dqkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), dk_ref, 5e-5)
    chk("dv", dqkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh), dv_ref, 5e-5)


@pytest.mark.parametrize("lengths,H,Hkv,dh", [((1, 7, 129, 64, 300, 65), 4, 1, 128), ((1, 7, 129, 64, 300, 65), 7, 1, 128), ((1, 7, 129, 64, 300, 65), 12, 12, 64),
                                             ((191, 192, 193), 8, 2, 128), ((255, 256, 257), 8, 2, 128), ((2048,), 4, 1, 128)])
@pytest.mark.parametrize("planted", [False, True])
def test_attention_f32_long_sequences(L, lengths, H, Hkv, dh, planted):
    """attn_f32.hip on batches whose longest sequence has more than 128 tokens -- several sequences, tile edges past 128, 2048 tokens -- against
    float64 attention. Every output is poisoned before its launch.
    planted=False: unit-scale inputs, the bounds of test_attention_f32 (out 2e-5, lse 2e-6, gradients 5e-5 of rms).
    planted=True: the extremes of tests/test_attention_long_gpu.py (a row maximum in the last key tile, a dominant key in tile 0, one head whose
    scores reach ~50 and beyond). Out and gradients then get twice the bound: a score S carries an fp32 rounding of ~|S| 2^-24 into P = exp(S - lse)
    as a RELATIVE error, so scores 10x larger than unit scale give proportionally larger output errors. That is not growth with n: measured out 1.75e-5
    at 300 tokens, 2.2e-5 at 191 - 257 and 2.5e-5 at 2048 (a summation term would grow ~sqrt(7) = 2.6x from 300 to 2048, a tile defect far more), dk
    5.2e-5 at 300 tokens. lse keeps its bound.
    dK, which sums G x n terms for the first keys of a sequence, is the one output whose error grows with n: measured max|d|/rms 7.3e-6 at 130 tokens,
    2.0e-5 at 300 and 1.12e-4 at 2048, i.e. n 2^-24 at every length -- the worst-case (linear) form of fp32 summation error rather than the random-walk
    sqrt(n) form, and nowhere near a tile defect (which would show as errors of order 1e-3 at tile boundaries). Gradients are therefore held to
    max(5e-5, 1.5 n 2^-24) with n the longest sequence; the linear growth itself is left for a follow-up look at the dK accumulation order."""
    from test_attention_long_gpu import POISON, exact_attention_bwd, exact_attention_fwd, make_inputs, split
    T = sum(lengths)
    qkv, do, cu = make_inputs(lengths, H, Hkv, dh, seed=T + 7 * H + dh, plant=planted)
    widen = 2.0 if planted else 1.0
    gtol = max(5e-5, 1.5 * max(lengths) * 2.0 ** -24) * widen
    q, k, v = split(qkv, T, H, Hkv, dh)
    out_ref, lse_ref = exact_attention_fwd(q, k, v, cu)
    dq_ref, dk_ref, dv_ref = exact_attention_bwd(q, k, v, do.reshape(T, H, dh), cu)
    ld = qkv.shape[1]
    lib = L.load_lab()
    qkv_, cu_, do_ = L.dev_f32(qkv), L.DevBuf(cu), L.dev_f32(do)
    out_, lse_, delta_, dqkv_ = L.DevBuf(nbytes=T * H * dh * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=T * ld * 4)
    for buf in (out_, lse_, delta_, dqkv_):
        assert lib.tst_dev_memset(buf.ptr, POISON, buf.nbytes) == 0
    scale = 1.0 / np.sqrt(dh)
    assert lib.tst_k_attn_fwd_f32(qkv_.ptr, ld, cu_.ptr, len(lengths), max(lengths), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    assert lib.tst_k_attn_bwd_f32(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, len(lengths), max(lengths), dqkv_.ptr, T,
                                  H, Hkv, dh, scale) == 0
    tag = f"long{' planted' if planted else ''} L{'_'.join(map(str, lengths))} H{H}/{Hkv} dh{dh}"
    dqkv = dqkv_.get(np.float32, (T, ld))
    dq, dk, dv = split(dqkv, T, H, Hkv, dh)

    def chk(name, a, b, tol):
        e = float(np.abs(a - b).max() / (np.sqrt(np.mean(b.astype(np.float64) ** 2)) + 1e-30))
        report(f"attn_f32 {name} {tag} vs fp64: max|d|/rms = {e:.2e}")
        assert np.isfinite(a).all() and e <= tol, (name, e)
    chk("out", out_.get(np.float32, (T, H, dh)), out_ref, 2e-5 * widen)
    chk("lse", lse_.get(np.float32, (H, T)), lse_ref, 2e-6)
    chk("dq", dq, dq_ref, gtol)
    chk("dk", dk, dk_ref, gtol)
    chk("dv", dv, dv_ref, gtol)


def test_attention_f32_matches_hf_fixture(L, golden_dir):
    """HF eager_attention_forward (fp32) fixture: forward output and all three gradients, to fp32 summation order."""
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    q, k, v = (g[n][0].transpose(1, 0, 2) for n in ("att_q", "att_k", "att_v"))
    T, H, dh = q.shape
    Hkv = k.shape[1]
    qkv = np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).astype(np.float32)
    cu = np.array([0, T], np.int32)
    do = np.ascontiguousarray(g["att_do"][0].reshape(T, H * dh), np.float32)
    qkv_, cu_, do_ = L.dev_f32(qkv), L.DevBuf(cu), L.dev_f32(do)
    out_, lse_, delta_, dqkv_ = L.DevBuf(nbytes=T * H * dh * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=qkv.nbytes)
    lib, scale, ld = L.load_lab(), 1.0 / np.sqrt(dh), qkv.shape[1]
    assert lib.tst_k_attn_fwd_f32(qkv_.ptr, ld, cu_.ptr, 1, T, out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    out = out_.get(np.float32, (T, H, dh))
    assert float(np.abs(out - g["att_o"][0]).max()) <= 1e-5
    assert lib.tst_k_attn_bwd_f32(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, 1, T, dqkv_.ptr, T, H, Hkv, dh, scale) == 0
    dqkv = dqkv_.get(np.float32, (T, ld))
    for name, got, ref in (("dq", dqkv[:, : H * dh].reshape(T, H, dh), g["att_dq"][0].transpose(1, 0, 2)),
                           ("dk", dqkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), g["att_dk"][0].transpose(1, 0, 2)),
                           ("dv", dqkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh), g["att_dv"][0].transpose(1, 0, 2))):
        e = float(np.abs(got - ref).max() / np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
        report(f"attn_f32 vs HF eager fp32 {name}: max|d|/rms = {e:.2e}")
        assert e <= 5e-5, (name, e)


def test_elementwise_f32_vs_hf_fixtures(L, golden_dir):
    """the elementwise kernels instantiated for fp32 against the HF / torch op fixtures (RMSNorm, RoPE, SwiGLU)."""
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    lib = L.load_lab()
    T, d = g["rms_x"].shape
    x_, w_, dy_ = L.dev_f32(g["rms_x"]), L.dev_f32(g["rms_w"]), L.dev_f32(g["rms_dy"])
    y_, rstd_, dx_ = L.DevBuf(nbytes=T * d * 4), L.DevBuf(nbytes=T * 4), L.DevBuf(nbytes=T * d * 4)
    assert lib.tst_k_rmsnorm_fwd_f32(x_.ptr, w_.ptr, y_.ptr, rstd_.ptr, T, d, 1e-5) == 0
    assert float(np.abs(y_.get(np.float32, (T, d)) - g["rms_y"]).max()) <= 2e-6
    assert lib.tst_k_rmsnorm_bwd_f32(dy_.ptr, x_.ptr, rstd_.ptr, w_.ptr, None, dx_.ptr, T, d) == 0
    assert float(np.abs(dx_.get(np.float32, (T, d)) - g["rms_dx"]).max()) <= 5e-6
    # RoPE: q [1, 2, 9, 128] and k [1, 1, 9, 128] as one packed [9, 3*128] buffer; the HF tables are used as they are
    q, k = g["rope_q"][0].transpose(1, 0, 2), g["rope_k"][0].transpose(1, 0, 2)
    Tn, Hn, dh = q.shape
    buf = np.concatenate([q.reshape(Tn, -1), k.reshape(Tn, -1)], 1).astype(np.float32)
    cosT, sinT = np.ascontiguousarray(g["rope_cos"][0][:, : dh // 2]), np.ascontiguousarray(g["rope_sin"][0][:, : dh // 2])
    b_, p_, c_, s_ = L.dev_f32(buf), L.DevBuf(np.arange(Tn, dtype=np.int32)), L.dev_f32(cosT), L.dev_f32(sinT)
    assert lib.tst_k_rope_f32(b_.ptr, p_.ptr, c_.ptr, s_.ptr, Tn, Hn + 1, dh, buf.shape[1], 0) == 0
    got = b_.get(np.float32, buf.shape)
    assert float(np.abs(got[:, : Hn * dh].reshape(Tn, Hn, dh) - g["rope_qe"][0].transpose(1, 0, 2)).max()) <= 2e-6
    assert float(np.abs(got[:, Hn * dh:].reshape(Tn, 1, dh) - g["rope_ke"][0].transpose(1, 0, 2)).max()) <= 2e-6
    # SwiGLU
    Ts, F = g["sw_g"].shape
    gu = np.concatenate([g["sw_g"], g["sw_u"]], 1).astype(np.float32)
    gu_, da_ = L.dev_f32(gu), L.dev_f32(g["sw_da"])
    a_, dgu_ = L.DevBuf(nbytes=Ts * F * 4), L.DevBuf(nbytes=Ts * 2 * F * 4)
    assert lib.tst_k_swiglu_fwd_f32(gu_.ptr, a_.ptr, Ts, F) == 0
    assert float(np.abs(a_.get(np.float32, (Ts, F)) - g["sw_a"]).max()) <= 2e-6
    assert lib.tst_k_swiglu_bwd_f32(da_.ptr, gu_.ptr, dgu_.ptr, Ts, F) == 0
    dgu = dgu_.get(np.float32, (Ts, 2 * F))
    assert float(np.abs(dgu[:, :F] - g["sw_dg"]).max()) <= 5e-6 and float(np.abs(dgu[:, F:] - g["sw_du"]).max()) <= 5e-6


# ------------------------------------------------------------------------------------------------ the engine in strict mode
STRICT_CASES = [("tiny", GI.TINY_CFG), ("tiny2", GI.TINY2_CFG), ("qwen", GI.QWEN_CFG), ("gpt2", GI.GPT2_CFG), ("tiny_rs", GI.TINY_RS_CFG)]   # tiny_rs: llama3 RoPE scaling


def make_ctx(cfg, mode="lora", **kw):
    from tst import lib
    ctx = lib.Context(cfg, max_tokens=1024, max_seqs=32, max_labelled=64, max_position=256 if cfg.get("arch") != "gpt2" else cfg["max_position"],
                      lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode, precision="strict", **kw)
    ctx.load_state_dict(GI.strict_weights(cfg))
    return ctx


def check_heldout(tag, what, ctx, g, prefix):
    """s(x) ingredients + logits of the 32-sample held-out set against the HF fp32 fixture, at the north_star tolerance"""
    hid, hlab, hcu = GI.strict_heldout(ctx.cfg)
    opt = list(GI.STRICT_OPT_IDS)
    logp, correct, optl, rseq = ctx.score_rows(hid, hlab, hcu, opt)
    assert len(logp) == 32 and (rseq == np.arange(32)).all()
    d_sx = float(np.abs(_softmax(optl) - _softmax(g[prefix + "_optl"])).max())
    d_p = float(np.abs(np.exp(logp) - np.exp(g[prefix + "_logp"])).max())
    lg = ctx.forward_logits(hid, hcu, g["heldout_rows"])
    d_lg = float(np.abs(lg - g[prefix + "_logits"]).max())
    agree = float((lg.argmax(-1) == g[prefix + "_logits"].argmax(-1)).mean())
    same = bool((correct == g[prefix + "_correct"]).all())
    # ... and the set on which HF's own `correct` is not all zeros (GI.strict_seen: the training answers; base model 0, trained models 1): identity of `correct`
    # there is a statement, on the fresh set above it compares zeros with zeros
    sid, slab, scu = GI.strict_seen(ctx.cfg)
    slogp, scorrect, _, _ = ctx.score_rows(sid, slab, scu, opt)
    ref_c = g[prefix + "_seen_correct"]
    d_ps = float(np.abs(np.exp(slogp) - np.exp(g[prefix + "_seen_logp"])).max())
    same_seen = bool((scorrect == ref_c).all())
    report(f"strict[{tag}] {what}: held-out |d s(x)| max={d_sx:.2e}  |d p(answer)| max={d_p:.2e}  |d logits| max={d_lg:.2e}  argmax agreement={agree:.3f}  "
           f"correct identical={same}; seen set ({int(ref_c.sum())}/{len(ref_c)} correct in HF): correct identical={same_seen}  |d p(answer)| max={d_ps:.2e}")
    return d_sx, max(d_p, d_ps), d_lg, agree, same and same_seen


@pytest.mark.parametrize("tag,cfg", STRICT_CASES)
def test_strict_logits_and_scores_identical_weights(golden_dir, tag, cfg):
    """T1: identical weights -> fp32 logits within 1e-4, s(x) within 1e-3 (north_star), `correct` and argmax identical."""
    g = np.load(os.path.join(golden_dir, f"strict_{tag}.npz"))
    ctx = make_ctx(cfg)
    ctx.reset_trainable(seed=1)      # fold-start adapters (B = 0): the base model
    ids, labels, cu = GI.strict_train_batches(cfg)[0]
    lg = ctx.forward_logits(ids, cu, g["logits0_rows"])
    d0 = float(np.abs(lg - g["logits0"]).max())
    report(f"strict[{tag}] base logits vs HF fp32: max|d|={d0:.2e} (rms {float(np.sqrt(np.mean(g['logits0'] ** 2))):.2f})")
    assert d0 <= LOGIT_TOL
    assert (lg.argmax(-1) == g["logits0"].argmax(-1)).all()
    d_sx, d_p, d_lg, agree, same = check_heldout(tag, "base", ctx, g, "base")
    assert d_sx <= SX_TOL and d_p <= SX_TOL and d_lg <= LOGIT_TOL and agree == 1.0 and same
    ctx.close()


def traj_bound(ref, t):
    """t = 0-based step index"""
    rel = TRAJ_STEP1 if t == 0 else min(TRAJ_CAP, TRAJ_REL * TRAJ_GROWTH ** t)
    return rel * abs(ref) + TRAJ_ABS


@pytest.mark.parametrize("mode", ["lora", "full"])
@pytest.mark.parametrize("tag,cfg", STRICT_CASES)
def test_strict_twenty_step_trajectory_then_heldout_scores(golden_dir, tag, cfg, mode):
    """T3 + the whole fold: 20 optimizer steps in fp32, per-step loss / gradient norm inside the stated growing bound, then the
    trained model's s(x) on the held-out set within 1e-3 of the reference's."""
    g = np.load(os.path.join(golden_dir, f"strict_{tag}.npz"))
    ctx = make_ctx(cfg, mode, weight_decay=0.01, max_grad_norm=1.0)
    if mode == "lora":
        ctx.set_trainable(GI.make_lora(cfg))
    batches = GI.strict_train_batches(cfg)
    losses, gnorms = [], []
    for step in range(GI.STRICT_STEPS):
        ids, labels, cu = batches[step % 2]
        l, gn = ctx.train_step(ids, labels, cu, O.linear_lr(step, GI.STRICT_STEPS, GI.STRICT_LR[mode]))
        losses.append(l)
        gnorms.append(gn)
    losses, gnorms = np.array(losses, np.float64), np.array(gnorms, np.float64)
    rl, rg = g[mode + "_losses"], g[mode + "_gnorms"]
    rel_l = np.abs(losses - rl) / (np.abs(rl) + 1e-30)
    rel_g = np.abs(gnorms - rg) / (np.abs(rg) + 1e-30)
    report(f"strict[{tag}] {mode} trajectory: loss rel dev step1={rel_l[0]:.1e} step5={rel_l[4]:.1e} step10={rel_l[9]:.1e} step20={rel_l[19]:.1e} (max {rel_l.max():.1e}) | "
           f"gnorm rel dev step1={rel_g[0]:.1e} step10={rel_g[9]:.1e} step20={rel_g[19]:.1e} (max {rel_g.max():.1e}) | "
           f"loss hip {losses[0]:.6f}->{losses[19]:.3e} hf {rl[0]:.6f}->{rl[19]:.3e}")
    report(f"strict[{tag}] {mode} per-step loss rel dev: " + " ".join(f"{x:.1e}" for x in rel_l))
    report(f"strict[{tag}] {mode} per-step |d gnorm|: " + " ".join(f"{x:.1e}" for x in np.abs(gnorms - rg)) + " | gnorm ref: " + " ".join(f"{x:.1e}" for x in rg))
    for t in range(GI.STRICT_STEPS):
        assert abs(losses[t] - rl[t]) <= traj_bound(rl[t], t), ("loss", t, losses[t], rl[t])
        assert abs(gnorms[t] - rg[t]) <= 2 * traj_bound(rg[t], t) + 8 * TRAJ_ABS, ("gnorm", t, gnorms[t], rg[t])
    d_sx, d_p, d_lg, agree, same = check_heldout(tag, f"after 20 {mode} steps", ctx, g, mode)
    assert d_sx <= SX_TOL and d_p <= SX_TOL and agree == 1.0 and same
    ctx.close()


def test_strict_mode_is_bit_reproducible_and_forkable():
    """same run twice -> identical losses and gradients (no atomics on the LoRA path); a fork shares the fp32 base weights"""
    cfg = GI.TINY_CFG
    ids, labels, cu = GI.strict_train_batches(cfg)[0]
    ctx = make_ctx(cfg)
    ctx.set_trainable(GI.make_lora(cfg))
    l1, g1 = ctx.forward_backward(ids, labels, cu), ctx.get_grads()
    l2, g2 = ctx.forward_backward(ids, labels, cu), ctx.get_grads()
    assert l1 == l2
    for k in g1:
        np.testing.assert_array_equal(g1[k], g2[k])
    kid = ctx.fork()
    kid.set_trainable(GI.make_lora(cfg))
    assert kid.forward_backward(ids, labels, cu) == l1
    from tst import lib
    with pytest.raises(lib.TstError, match="stacked"):
        lib.Context(cfg, precision="strict", n_stack=2)
    kid.close()
    ctx.close()


SX_BF16_FACTOR = 1.25   # the product's bf16 path may sit this much above the reference's own bf16 deviation, no further


@pytest.mark.parametrize("tag,cfg", STRICT_CASES)
def test_bf16_path_scores_inside_the_references_own_bf16_floor(golden_dir, tag, cfg):
    """What the benched bf16 path costs in s(x), stated against the reference instead of a fixed number: HF's own model.to(bfloat16) moves the
    held-out s(x) by some |d| from HF fp32 (fixture keys *_optl_hf_bf16, tools/make_golden.py strict); the HIP bf16 path, on the same weights and --
    for the trained fold -- the SAME adapters HF's 20 fp32 steps ended with, must stay within SX_BF16_FACTOR x that, in the worst sample and on
    average. ("s(x) within 1e-3" itself is a statement about fp32 arithmetic: the strict-mode tests above.)"""
    from tst import lib
    g = np.load(os.path.join(golden_dir, f"strict_{tag}.npz"))
    hid, hlab, hcu = GI.strict_heldout(cfg)
    opt = list(GI.STRICT_OPT_IDS)
    ctx = lib.Context(cfg, max_tokens=1024, max_seqs=32, max_labelled=64, max_position=256 if cfg.get("arch") != "gpt2" else cfg["max_position"],
                      lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, precision="bf16")
    ctx.load_state_dict(GI.strict_weights(cfg))   # (rounded to bf16 on the way in, like HF's .to(bfloat16))
    for prefix in ("base", "lora"):
        if prefix == "base":
            ctx.reset_trainable(seed=1)           # B = 0: the base model
        else:
            ctx.set_trainable({k[len("lora_trained/"):]: g[k] for k in g.files if k.startswith("lora_trained/")})
        optl = ctx.score_rows(hid, hlab, hcu, opt)[2]
        ref = _softmax(g[prefix + "_optl"])
        d = np.abs(_softmax(optl) - ref)
        floor = np.abs(_softmax(g[prefix + "_optl_hf_bf16"]) - ref)
        report(f"bf16 path [{tag}] {prefix}: |d s(x)| vs HF fp32 max={d.max():.2e} mean={d.mean():.2e} | HF bf16's own: max={floor.max():.2e} mean={floor.mean():.2e} "
               f"| ratio max {d.max() / floor.max():.2f} mean {d.mean() / floor.mean():.2f}")
        assert d.max() <= SX_BF16_FACTOR * floor.max(), (prefix, float(d.max()), float(floor.max()))
        assert d.mean() <= SX_BF16_FACTOR * floor.mean(), (prefix, float(d.mean()), float(floor.mean()))
    ctx.close()
