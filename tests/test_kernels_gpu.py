"""GPU parity tests of the individual HIP kernels, called through the C-ABI (tst_k_*), checked against the CPU
oracle in its bf16-mirror mode (oracle/ops_np.py). Tolerances are stated per test: bf16 outputs may differ from the
oracle by one bf16 ulp (2^-8 relative) where fp32 summation order flips a rounding; fp32 outputs by summation order only.
"""
import os

import ctypes as C

import numpy as np
import pytest

import golden_inputs as GI
from oracle import ops_np as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "gpurun_out", "kernel_report.txt")


def report(name, **kv):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()) + "\n")


def err_stats(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rms = float(np.sqrt(np.mean(b * b))) + 1e-30
    d = np.abs(a - b)
    return float(d.max()), float(d.max() / rms), float(np.sqrt(np.mean(d * d)) / rms)


def assert_close(name, a, b, rtol, atol_rms):
    """|a-b| <= rtol*|b| + atol_rms*rms(b) elementwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), f"{name}: non-finite output"
    rms = float(np.sqrt(np.mean(b * b))) + 1e-30
    mx, mxr, rel = err_stats(a, b)
    report(name, max_abs=mx, max_over_rms=mxr, rel_l2=rel)
    bad = np.abs(a - b) > rtol * np.abs(b) + atol_rms * rms
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.size} elements out of tolerance, max|d|={mx:.3e} rms(ref)={rms:.3e}"


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load_lab()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


BF_ULP = 2.0 ** -7  # one bf16 ulp relative, worst case


def test_tr_read_lane_map(L):
    """pins the ds_read_b64_tr_b16 lane map attn.hip relies on (cdna_hip_programming.md T10)."""
    for d0 in (0, 16, 112):
        out = L.DevBuf(nbytes=64 * 8 * 2)
        assert L.load_lab().tst_k_tr_probe(out.ptr, d0) == 0
        got = out.get(np.uint16, (64, 8)).astype(np.int64)
        lane = np.arange(64)
        i, g = lane & 15, lane >> 4
        exp = np.zeros((64, 8), np.int64)
        for j in range(8):
            row = 16 * (j >> 2) + 4 * g + (j & 3)
            exp[:, j] = row * 128 + d0 + i
        np.testing.assert_array_equal(got, exp)


def _gemm(L, A, B, A2=None, B2=None, R=None, alpha=1.0, out_f32=False, variant=-1, splitk=-1):
    M, K = A.shape
    N = B.shape[0]
    K2 = A2.shape[1] if A2 is not None else 0
    dA, dB = L.dev_bf16(A), L.dev_bf16(B)
    dA2 = L.dev_bf16(A2) if A2 is not None else None
    dB2 = L.dev_bf16(B2) if B2 is not None else None
    dR = L.dev_bf16(R) if R is not None else None
    dC = L.DevBuf(nbytes=M * N * (4 if out_f32 else 2))
    rc = L.load_lab().tst_k_gemm_nt(dA.ptr, K, dB.ptr, K, dA2.ptr if dA2 else None, K2, dB2.ptr if dB2 else None, K2, dC.ptr, N,
                                dR.ptr if dR else None, N, M, N, K, K2, alpha, 1 if out_f32 else 0, variant, splitk)
    assert rc == 0, f"tst_k_gemm_nt rc={rc}"
    return dC.get(np.float32, (M, N)) if out_f32 else dC.get_bf16((M, N))


def _gemm_ref_np(A, B, A2=None, B2=None, R=None, alpha=1.0, out_f32=False):
    acc = O.rbf(A) @ O.rbf(B).T
    if A2 is not None:
        acc = acc + O.rbf(A2) @ O.rbf(B2).T
    acc = acc * np.float32(alpha)
    if R is not None:
        acc = acc + O.rbf(R)
    return acc.astype(np.float32) if out_f32 else O.rbf(acc)


@pytest.mark.parametrize("M,N,K,variant,splitk", [
    (128, 128, 64, 0, 1), (128, 128, 256, 0, 1), (256, 384, 512, 0, 1), (200, 136, 192, 0, 1), (77, 72, 128, 0, 2),
    (130, 64, 256, 1, 1), (300, 64, 1024, 1, 4), (64, 256, 128, 2, 1), (33, 200, 640, 2, 3), (1, 8, 64, 0, 1),
    (512, 512, 2048, -1, -1), (2048, 64, 4096, -1, -1), (64, 4096, 2048, -1, -1),
    (256, 256, 64, 4, 1), (256, 384, 512, 4, 1), (200, 136, 192, 4, 1), (513, 264, 2048, 4, 1), (1, 8, 64, 4, 1), (1190, 1024, 1088, 4, 1),
    # ping-pong tile: 1, 2, 3 and 4 k-tiles exercise every tail of its prefetch schedule
    (256, 256, 64, 5, 1), (256, 256, 128, 5, 1), (300, 520, 192, 5, 1), (256, 384, 256, 5, 1), (256, 384, 512, 5, 1), (200, 136, 192, 5, 1),
    (513, 264, 2048, 5, 1), (1, 8, 64, 5, 1), (1190, 1024, 1088, 5, 1),
    # ... and with its split-K (fp32 slabs + reduce): uneven slices, one-tile slices, more slices asked for than k-tiles
    (513, 264, 2048, 5, 3), (256, 256, 2048, 5, 4), (300, 520, 192, 5, 2), (1190, 1024, 1088, 5, 2), (256, 256, 64, 5, 4),
])
def test_gemm_nt_shapes(L, M, N, K, variant, splitk):
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    got = _gemm(L, A, B, out_f32=True, variant=variant, splitk=splitk)
    ref = _gemm_ref_np(A, B, out_f32=True)
    assert_close(f"gemm_f32 M{M} N{N} K{K} v{variant} sk{splitk}", got, ref, 1e-4, 1e-4)
    got = _gemm(L, A, B, variant=variant, splitk=splitk)
    assert_close(f"gemm_bf16 M{M} N{N} K{K} v{variant} sk{splitk}", got, O.rbf(ref), BF_ULP, 1e-3)


@pytest.mark.parametrize("variant,splitk", [(0, 1), (0, 3), (1, 1), (2, 2), (4, 1), (5, 1), (5, 3)])
def test_gemm_nt_lora_segment_residual_alpha(L, variant, splitk):
    """second K segment (LoRA term), residual add before rounding, alpha scaling."""
    rng = np.random.default_rng(11 + variant)
    M, N, K, K2 = (190, 64, 320, 64) if variant == 1 else (190, 200, 320, 64)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    A2, B2 = rng.standard_normal((M, K2)).astype(np.float32), rng.standard_normal((N, K2)).astype(np.float32)
    R = rng.standard_normal((M, N)).astype(np.float32) * 5
    got = _gemm(L, A, B, A2, B2, R, alpha=0.5, variant=variant, splitk=splitk)
    ref = _gemm_ref_np(A, B, A2, B2, R, alpha=0.5)
    assert_close(f"gemm_seg2 v{variant} sk{splitk}", got, ref, BF_ULP, 1e-3)
    got = _gemm(L, A, B, A2, B2, None, alpha=2.0, out_f32=True, variant=variant, splitk=splitk)
    assert_close(f"gemm_seg2_f32 v{variant} sk{splitk}", got, _gemm_ref_np(A, B, A2, B2, None, 2.0, True), 1e-4, 1e-4)


def _gemm_masked(L, A, B, alpha, width, ends, variant, splitk=-1):
    M, K = A.shape
    N = B.shape[0]
    dA, dB = L.dev_bf16(A), L.dev_bf16(B)
    dC = L.DevBuf(nbytes=M * N * 2)
    L.load_lab().tst_dev_memset(dC.ptr, 0x7f, M * N * 2)   # every element must be written (also the zeros of the other slots' blocks)
    te = (C.c_int32 * 8)(*([int(e) for e in ends] + [M] * (8 - len(ends)))) if ends is not None else None
    rc = L.load_lab().tst_k_gemm_masked(dA.ptr, K, dB.ptr, K, dC.ptr, N, M, N, K, alpha, width, len(ends) if ends is not None else 0, te, variant, splitk)
    assert rc == 0, f"tst_k_gemm_masked rc={rc}"
    return dC.get_bf16((M, N))


@pytest.mark.parametrize("M,N,K,width,ends", [
    (3555, 192, 4096, 48, (1190, 2371, 3555)),      # u = x.Ag^T of the q|k|v group, three stacked folds (the benchmark's shape)
    (3555, 128, 1024, 32, (1190, 2371, 3555)),      # gate|up group
    (2370, 64, 14336, 16, (1185, 1185, 2370)),      # down projection: long K; an EMPTY middle slot
    (1200, 64, 4096, 0, None),                      # one fold per context: no mask, N = RP = 64
    (37, 64, 64, 0, None), (16, 16, 128, 0, None), (100, 256, 192, 0, None),        # fewer k-steps than waves; ragged last row tile
    (530, 384, 576, 48, (70, 70, 100, 200, 300, 301, 520, 530)),                    # eight slots, empty and one-row slots, tiles straddling several slots
    (300, 64, 512, 24, (150, 300)),                 # block width not a multiple of 16 (lora_r = 8, three modules)
])
def test_gemm_rank_axis_kernel(L, M, N, K, width, ends):
    """csrc/gemm_rank.hip (variant 8): K split over the waves of a workgroup, slot-restricted columns. Against numpy (same bf16 operands, fp32
    accumulate, one rounding) and against the tiled path with the mask in its epilogue / split-K reduce."""
    rng = np.random.default_rng(M + 3 * N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    alpha = 2.0
    ref = (O.rbf(A) @ O.rbf(B).T) * np.float32(alpha)
    if width:
        slot = np.searchsorted(np.asarray(ends), np.arange(M), side="right")
        keep = (np.arange(N)[None, :] // width) == slot[:, None]
        ref = np.where(keep, ref, 0.0)
    ref = O.rbf(ref.astype(np.float32))
    got = _gemm_masked(L, A, B, alpha, width, ends, 8)
    assert_close(f"gemm_rank M{M} N{N} K{K} w{width}", got, ref, BF_ULP, 1e-3)
    if width:
        assert (got[~keep] == 0).all(), "columns of other slots must be exact zeros"
    direct = _gemm_masked(L, A, B, alpha, width, ends, 9)          # the register-loading form of the same kernel (8 K slices instead of 4)
    assert_close(f"gemm_rank(direct) M{M} N{N} K{K} w{width}", direct, ref, BF_ULP, 1e-3)
    old = _gemm_masked(L, A, B, alpha, width, ends, 1 if N <= 64 or (N & 127) == 64 else 0)
    assert_close(f"gemm_rank vs tiled M{M} N{N} K{K}", got, old, BF_ULP, 1e-3)
    again = _gemm_masked(L, A, B, alpha, width, ends, 8)
    assert (got == again).all(), "fixed summation order: bit-reproducible"


@pytest.mark.parametrize("M,N,K,K2,w,ends", [
    (3507, 1024, 512, 192, 48, (1169, 2338, 3507)),   # q|k|v group of three stacked folds: slot blocks 0-47 / 48-95 / 96-143 of 192 columns -> 1, 2, 2 of 3 K2 k-tiles
    (2338, 512, 256, 128, 32, (1169, 2338)),          # gate|up group of two: both blocks in K2 k-tile 0
    (2338, 768, 256, 128, 32, (900, 900, 2338)),      # an EMPTY middle slot; slot 2's block 64-95 lies in k-tile 1
    (700, 256, 128, 512, 64, (1, 65, 129, 300, 301, 512, 700)),   # seven slots of 64 columns, boundaries inside and on tile rows, tiles straddling up to four slots
    (300, 256, 64, 64, 16, (100, 200, 300)),          # one tile row holds all three slots, one K2 k-tile
])
def test_gemm_pp_skips_the_k2_tiles_of_other_slots(L, M, N, K, K2, w, ends):
    """GemmParams.k2_w: rows of A2 (u / du of a stacked context) are zero outside their slot's rank block, so the ping-pong tile runs only the K2 k-tiles that
    overlap the blocks of its rows' slots. Bit-identical to running every K2 k-tile (the skipped ones add exact zeros), and equal to numpy."""
    rng = np.random.default_rng(M + N + K2)
    ns = len(ends)
    slot = np.searchsorted(np.asarray(ends), np.arange(M), side="right")
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    A2 = np.zeros((M, K2), np.float32)
    blk = (rng.standard_normal((M, w)) * 0.5).astype(np.float32)
    for t in range(M):
        A2[t, slot[t] * w:(slot[t] + 1) * w] = blk[t]
    B2 = (rng.standard_normal((N, K2)) * 0.05).astype(np.float32)
    dA, dB, dA2, dB2 = L.dev_bf16(A), L.dev_bf16(B), L.dev_bf16(A2), L.dev_bf16(B2)
    te = (C.c_int32 * 8)(*([int(e) for e in ends] + [M] * (8 - ns)))
    outs = []
    for k2_w in (0, w):
        dC = L.DevBuf(nbytes=M * N * 2)
        L.load_lab().tst_dev_memset(dC.ptr, 0x7f, M * N * 2)
        assert L.load_lab().tst_k_gemm_k2slots(dA.ptr, K, dB.ptr, K, dA2.ptr, K2, dB2.ptr, K2, dC.ptr, N, M, N, K, K2, k2_w, ns, te, 5) == 0
        outs.append(dC.get_bf16((M, N)))
    assert (outs[0] == outs[1]).all(), "skipping the other slots' K2 k-tiles must not change a bit"
    ref = O.rbf(A) @ O.rbf(B).T + O.rbf(A2) @ O.rbf(B2).T
    assert_close(f"gemm_pp k2 slots M{M} N{N} K2{K2} w{w}", outs[1], ref, BF_ULP, 1e-3)


@pytest.mark.parametrize("T,ends,w,rp,wn", [
    (3555, (1190, 2371, 3555), 48, 192, 4096),        # q|k|v group of three stacked folds: dAg / dBg against d_in = 4096
    (2370, (1185, 1185, 2370), 32, 128, 1536),        # gate|up group; an EMPTY middle slot (its block must come out as zeros)
    (1200, (1200,), 48, 64, 768),                     # one fold per context
    (700, (1, 65, 129, 300, 301, 512, 700), 16, 128, 320),   # seven slots: one-token slots, boundaries inside and on 64-token steps, wide side not a multiple of 256
    (130, (70, 130), 72, 192, 264),                   # w > 64: two rank tiles per slot (lora_r 24 x 3 modules), wn with a ragged last tile
])
@pytest.mark.parametrize("kind", [0, 1])
def test_gemm_tns_slot_restricted_adapter_gradients(L, T, ends, w, rp, wn, kind):
    """csrc/gemm_tns.hip: the adapter-gradient contraction restricted to each slot's tokens and rank block, against numpy on the same bf16
    operands (fp32 accumulate); blocks of other slots are not written (the output buffer keeps its sentinel there)."""
    rng = np.random.default_rng(T + 7 * w + wn + kind)
    Tp = (T + 63) // 64 * 64
    ns = len(ends)
    slot = np.searchsorted(np.asarray(ends), np.arange(T), side="right")
    rk = np.zeros((Tp, rp), np.float32)
    blk = (rng.standard_normal((T, w)) * 0.5).astype(np.float32)
    for t in range(T):
        rk[t, slot[t] * w:(slot[t] + 1) * w] = blk[t]                     # per token only its slot's block is non-zero (the masked du / us)
    rk[T:] = 7.0                                                          # rows past the batch hold finite garbage that must not contribute
    wd = (rng.standard_normal((Tp, wn)) * 0.5).astype(np.float32)
    wd[T:] = np.nan                                                       # ... and the wide operand's tail rows may even be non-finite (a diverged earlier batch): masked in-kernel
    alpha = 2.0 if kind == 0 else 1.0
    shape = (rp, wn) if kind == 0 else (wn, rp)
    out = L.DevBuf(np.full(shape, -123.0, np.float32))
    te = (C.c_int32 * 8)(*([int(e) for e in ends] + [T] * (8 - ns)))
    d_rk, d_wd = L.dev_bf16(rk), L.dev_bf16(wd)                            # (named: a temporary would be freed before the launch reads it)
    rc = L.load_lab().tst_k_gemm_tns(d_rk.ptr, rp, rp, d_wd.ptr, wn, wn, out.ptr, shape[1], w, alpha, kind, Tp, ns, te)
    assert rc == 0
    got = out.get(np.float32, shape)
    full = alpha * (O.rbf(rk[:T]).T @ O.rbf(wd[:T]))                        # [rp, wn]: cross-slot blocks are exact zeros by construction
    ref = np.full(shape, -123.0, np.float32)
    for s_ in range(ns):
        if kind == 0:
            ref[s_ * w:(s_ + 1) * w, :] = full[s_ * w:(s_ + 1) * w, :]
        else:
            ref[:, s_ * w:(s_ + 1) * w] = full[s_ * w:(s_ + 1) * w, :].T
    touched = ref != -123.0
    assert (got[~touched] == -123.0).all(), "columns / rows outside the slots' blocks must not be written"
    assert_close(f"gemm_tns kind{kind} T{T} w{w} wn{wn}", got[touched], ref[touched], 1e-4, 2e-4)


@pytest.mark.parametrize("variant", [3])
@pytest.mark.parametrize("M,N,T", [(64, 256, 70), (200, 64, 130), (1024, 64, 1190), (64, 4096, 1190), (136, 264, 64), (128, 128, 1)])
def test_gemm_tn(L, M, N, T, variant):
    """contraction over the token (row) axis of both operands, as the adapter gradients need it; rows in [T, roundup64(T))
    hold finite garbage that must not contribute."""
    rng = np.random.default_rng(M + N + T)
    Tp = (T + 63) // 64 * 64
    P = rng.standard_normal((Tp, M)).astype(np.float32)
    Q = rng.standard_normal((Tp, N)).astype(np.float32)
    dP, dQ, dC = L.dev_bf16(P), L.dev_bf16(Q), L.DevBuf(nbytes=M * N * 4)
    assert L.load_lab().tst_k_gemm_tn(dP.ptr, M, dQ.ptr, N, dC.ptr, N, M, N, T, 0.5, 1, variant) == 0
    ref = 0.5 * (O.rbf(P[:T]).T @ O.rbf(Q[:T]))
    assert_close(f"gemm_tn v{variant} M{M} N{N} T{T}", dC.get(np.float32, (M, N)), ref, 1e-4, 1e-4)


@pytest.mark.parametrize("M,N,T", [(256, 256, 64), (512, 768, 1185), (264, 520, 70), (1024, 256, 1), (72, 4096, 1190), (4096, 1024, 130), (6144, 4096, 1185)])
def test_gemm_pp_tn_member(L, M, N, T):
    """TN member of the 256x256 ping-pong tile (SURVEY §2 K1 `_tn`): dW[d_out, d_in] = dy^T . x straight from the row-major activations
    (HF: autograd of nn.Linear, modeling_llama.py:254-256 / 175). Rows in [T, roundup64(T)) of BOTH operands hold NaN: the kernel must never use them
    (they are out of range of the k-tile's buffer descriptor and arrive as zeros). fp32 output + the epilogue's sum of squares."""
    rng = np.random.default_rng(M + 3 * N + T)
    Tp = (T + 63) // 64 * 64
    P = rng.standard_normal((Tp, M)).astype(np.float32)
    Q = rng.standard_normal((Tp, N)).astype(np.float32)
    P[T:] = np.nan
    Q[T:] = np.nan
    dP, dQ, dC = L.dev_bf16(P), L.dev_bf16(Q), L.DevBuf(np.full((M, N), -7.0, np.float32))
    ssq = C.c_float()
    assert L.load_lab().tst_k_gemm_pp_kmajor(dP.ptr, M, dQ.ptr, N, dC.ptr, N, M, N, T, 0.5, 1, 1, 1, 1, 0, None, C.byref(ssq)) == 0
    if M * N * T <= 600 * 800 * 1300:
        ref = 0.5 * (O.rbf(P[:T]).astype(np.float64).T @ O.rbf(Q[:T]).astype(np.float64))
    else:   # big case: the naive GPU contraction over the valid rows
        dRef = L.DevBuf(nbytes=M * N * 4)
        assert L.load_lab().tst_k_gemm_ref(dP.ptr, 1, M, dQ.ptr, 1, N, dRef.ptr, N, M, N, T) == 0
        ref = 0.5 * dRef.get(np.float32, (M, N)).astype(np.float64)
    got = dC.get(np.float32, (M, N))
    assert np.isfinite(got).all(), "a padding row of the token axis reached the accumulators"
    assert_close(f"gemm_pp TN M{M} N{N} T{T}", got, ref, 1e-4, 2e-4)
    want = float((got.astype(np.float64) ** 2).sum())
    assert abs(ssq.value - want) <= 1e-4 * want + 1e-6, (ssq.value, want)


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (1185, 512, 1024), (70, 264, 192), (300, 4096, 6144), (1185, 1024, 4096)])
def test_gemm_pp_nn_member(L, M, N, K, splitk):
    """NN member (SURVEY §2 K1 `_nn`): dX[T, d_in] = dY[T, d_out] . W[d_out, d_in] from the ONE stored W (no W^T copy), bf16 output, with and
    without split-K; M (tokens) is any count, also not a multiple of 8 (the row-major operand's rows are clamped, not read past)."""
    rng = np.random.default_rng(M + 3 * N + K + splitk)
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    dA, dW = L.dev_bf16(A), L.dev_bf16(W)
    dC = L.DevBuf(nbytes=M * N * 2)
    assert L.load_lab().tst_k_gemm_pp_kmajor(dA.ptr, K, dW.ptr, N, dC.ptr, N, M, N, K, 1.0, 0, 0, 1, splitk, 0, None, None) == 0
    ref = (O.rbf(A).astype(np.float64) @ O.rbf(W).astype(np.float64)).astype(np.float32)
    assert_close(f"gemm_pp NN M{M} N{N} K{K} sk{splitk}", dC.get_bf16((M, N)), O.rbf(ref), BF_ULP, 1e-3)


def test_gemm_pp_kmajor_race_screen(L):
    """as test_gemm_256_tiles_race_screen, for the K-major members: 10 launches each, bit-identical and equal to the naive GPU contraction."""
    rng = np.random.default_rng(12)
    lib = L.load_lab()
    for (ta, M, N, K) in ((1, 4096, 4096, 1185), (1, 6144, 4096, 1185), (0, 1200, 4096, 6144), (0, 1200, 14336, 4096)):
        Kp = (K + 63) // 64 * 64
        A = (rng.standard_normal((Kp, M) if ta else (M, Kp)) * 0.5).astype(np.float32)
        B = (rng.standard_normal((Kp, N)) * 0.05).astype(np.float32)
        dA, dB = L.dev_bf16(A), L.dev_bf16(B)
        dC, dRef = L.DevBuf(nbytes=M * N * 4), L.DevBuf(nbytes=M * N * 4)
        if ta:
            assert lib.tst_k_gemm_ref(dA.ptr, 1, M, dB.ptr, 1, N, dRef.ptr, N, M, N, K) == 0
        else:
            assert lib.tst_k_gemm_ref(dA.ptr, Kp, 1, dB.ptr, 1, N, dRef.ptr, N, M, N, K) == 0
        ref = dRef.get(np.float32, (M, N))
        first = None
        for it in range(10):
            assert lib.tst_k_gemm_pp_kmajor(dA.ptr, M if ta else Kp, dB.ptr, N, dC.ptr, N, M, N, K, 1.0, 1, ta, 1, 1, 0, None, None) == 0
            got = dC.get(np.float32, (M, N))
            if first is None:
                first = got
                assert_close(f"gemm_pp kmajor ta{ta} M{M} N{N} K{K}", got, ref, 1e-3, 1e-3)
            else:
                assert np.array_equal(got, first), f"launch {it} differs from launch 0 (ta={ta} M={M} N={N} K={K})"


def test_gemm_llama_shapes_vs_gpu_reference(L):
    """Llama-3-8B projection shapes at 1 micro-batch; checked against the naive GPU contraction (CPU matmul would take minutes)."""
    rng = np.random.default_rng(3)
    lib = L.load_lab()
    for (M, N, K) in ((1280, 6144, 4096), (2048, 4096, 14336), (40, 128256, 4096)):
        A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
        B = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
        dA, dB = L.dev_bf16(A), L.dev_bf16(B)
        dC, dRef = L.DevBuf(nbytes=M * N * 4), L.DevBuf(nbytes=M * N * 4)
        assert lib.tst_k_gemm_nt(dA.ptr, K, dB.ptr, K, None, 0, None, 0, dC.ptr, N, None, 0, M, N, K, 0, 1.0, 1, -1, -1) == 0
        assert lib.tst_k_gemm_ref(dA.ptr, K, 1, dB.ptr, K, 1, dRef.ptr, N, M, N, K) == 0
        got, ref = dC.get(np.float32, (M, N)), dRef.get(np.float32, (M, N))
        assert_close(f"gemm_big M{M} N{N} K{K}", got, ref, 1e-3, 1e-3)


@pytest.mark.parametrize("variant", [4, 5])
def test_gemm_256_tiles_race_screen(L, variant):
    """the 256x256 tiles order their LDS-DMA traffic by counted vmcnt + barriers only: a mis-placed wait shows up as rare wrong
    tiles that come and go with timing. Projection shapes, 12 launches each: every launch bit-identical to the first and
    equal to the naive GPU contraction."""
    rng = np.random.default_rng(11)
    lib = L.load_lab()
    for (M, N, K, K2) in ((1200, 4096, 4096, 64), (1200, 6144, 4096, 0), (1200, 4096, 14336, 64), (3000, 2048, 1024, 0)):
        A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
        B = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
        dA, dB = L.dev_bf16(A), L.dev_bf16(B)
        dA2 = dB2 = None
        if K2:
            A2 = (rng.standard_normal((M, K2)) * 0.5).astype(np.float32)
            B2 = (rng.standard_normal((N, K2)) * 0.05).astype(np.float32)
            dA2, dB2 = L.dev_bf16(A2), L.dev_bf16(B2)
        dC, dRef = L.DevBuf(nbytes=M * N * 4), L.DevBuf(nbytes=M * N * 4)
        assert lib.tst_k_gemm_ref(dA.ptr, K, 1, dB.ptr, K, 1, dRef.ptr, N, M, N, K) == 0
        ref = dRef.get(np.float32, (M, N))
        if K2:
            ref = ref + O.rbf(A2) @ O.rbf(B2).T
        first = None
        for it in range(12):
            assert lib.tst_k_gemm_nt(dA.ptr, K, dB.ptr, K, dA2.ptr if K2 else None, K2, dB2.ptr if K2 else None, K2, dC.ptr, N, None, 0, M, N, K, K2, 1.0, 1,
                                     variant, 1) == 0
            got = dC.get(np.float32, (M, N))
            if first is None:
                first = got
                assert_close(f"gemm_v{variant}_screen M{M} N{N} K{K}+{K2}", got, ref, 1e-3, 1e-3)
            else:
                np.testing.assert_array_equal(got, first)


@pytest.mark.parametrize("M,N,K,K2,with_r,out_f32", [
    (4300, 4096, 1024, 64, True, False),    # 17 x 16 = 272 tiles: 16 tail tiles, two K slices each, second K segment + residual
    (3555, 6144, 4096, 0, False, True),     # the stacked q,k,v projection: 336 tiles, 80 tail tiles x 3 slices, fp32 output
    (2370, 14336, 4096, 64, False, False),  # two stacked folds' dX of the down projection: 560 tiles, 48 tail tiles x 5 slices
    (4100, 4104, 512, 0, True, False),      # ragged edges in both directions inside the tail tiles; 8 k-tiles: no split (falls back)
])
def test_gemm_pp_tail_split(L, M, N, K, K2, with_r, out_f32):
    """256x256 ping-pong tile with more than one wave of tiles: the tiles beyond the last full wave of 256 are contracted as K slices
    by several workgroups and finished by pp_tail_reduce_kernel (gemm_pp.hip). Every launch equals the naive GPU contraction and
    repeats bit-identically (the slices are summed in a fixed order)."""
    rng = np.random.default_rng(M + N + K)
    lib = L.load_lab()
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    dA, dB = L.dev_bf16(A), L.dev_bf16(B)
    dA2 = dB2 = dR = None
    dRef = L.DevBuf(nbytes=M * N * 4)
    assert lib.tst_k_gemm_ref(dA.ptr, K, 1, dB.ptr, K, 1, dRef.ptr, N, M, N, K) == 0
    ref = dRef.get(np.float32, (M, N))
    if K2:
        A2 = (rng.standard_normal((M, K2)) * 0.5).astype(np.float32)
        B2 = (rng.standard_normal((N, K2)) * 0.05).astype(np.float32)
        dA2, dB2 = L.dev_bf16(A2), L.dev_bf16(B2)
        ref = ref + O.rbf(A2) @ O.rbf(B2).T
    ref = ref * np.float32(0.5)
    if with_r:
        R = rng.standard_normal((M, N)).astype(np.float32)
        dR = L.dev_bf16(R)
        ref = ref + O.rbf(R)
    dC = L.DevBuf(nbytes=M * N * (4 if out_f32 else 2))
    first = None
    prev = L.set_tile_policy(-1)
    L.set_tile_policy(3)   # the tail split belongs to the one-stream policy
    try:
        for it in range(3):
            assert lib.tst_k_gemm_nt(dA.ptr, K, dB.ptr, K, dA2.ptr if K2 else None, K2, dB2.ptr if K2 else None, K2, dC.ptr, N, dR.ptr if with_r else None, N,
                                     M, N, K, K2, 0.5, 1 if out_f32 else 0, 5, 1) == 0
            got = dC.get(np.float32, (M, N)) if out_f32 else dC.get_bf16((M, N))
            if first is None:
                first = got
                if out_f32:
                    assert_close(f"gemm_pp_tail M{M} N{N} K{K}+{K2}", got, ref, 1e-3, 1e-3)
                else:
                    assert_close(f"gemm_pp_tail M{M} N{N} K{K}+{K2}", got, O.rbf(ref), BF_ULP, 2e-3)
            else:
                np.testing.assert_array_equal(got, first)
    finally:
        L.set_tile_policy(prev)


def test_transpose(L):
    rng = np.random.default_rng(2)
    R, Cc, Rp = 150, 200, 192
    x = O.rbf(rng.standard_normal((R, Cc)).astype(np.float32))
    dx = L.dev_bf16(x)
    dout = L.DevBuf(nbytes=Cc * Rp * 2)
    L.load_lab().tst_dev_memset(dout.ptr, 0xFF, Cc * Rp * 2)
    assert L.load_lab().tst_k_transpose(dx.ptr, Cc, dout.ptr, Rp, R, Cc, Rp) == 0
    got = dout.get_bf16((Cc, Rp))
    np.testing.assert_array_equal(got[:, :R], x.T)
    np.testing.assert_array_equal(got[:, R:], 0)


def test_embed(L):
    rng = np.random.default_rng(4)
    E = O.rbf(rng.standard_normal((50, 64)).astype(np.float32))
    ids = rng.integers(0, 50, 33).astype(np.int32)
    dE, dI, dO_ = L.dev_bf16(E), L.DevBuf(ids), L.DevBuf(nbytes=33 * 64 * 2)
    assert L.load_lab().tst_k_embed(dI.ptr, dE.ptr, dO_.ptr, 33, 64, 50) == 0
    np.testing.assert_array_equal(dO_.get_bf16((33, 64)), E[ids])


@pytest.mark.parametrize("T,d", [(5, 256), (130, 4096), (3, 3584)])
def test_rmsnorm(L, T, d):
    rng = np.random.default_rng(T + d)
    x = O.rbf(rng.standard_normal((T, d)).astype(np.float32) * 2)
    w = O.rbf((1 + 0.1 * rng.standard_normal(d)).astype(np.float32))
    dy = O.rbf(rng.standard_normal((T, d)).astype(np.float32))
    dres = O.rbf(rng.standard_normal((T, d)).astype(np.float32))
    dx_, dw_, dy_, dres_ = L.dev_bf16(x), L.dev_bf16(w), L.dev_bf16(dy), L.dev_bf16(dres)
    y_, rstd_, dxo_ = L.DevBuf(nbytes=T * d * 2), L.DevBuf(nbytes=T * 4), L.DevBuf(nbytes=T * d * 2)
    lib = L.load_lab()
    assert lib.tst_k_rmsnorm_fwd(dx_.ptr, dw_.ptr, y_.ptr, rstd_.ptr, T, d, 1e-5) == 0
    y_ref, rstd_ref = O.rmsnorm_fwd(x, w, 1e-5, bf16=True)
    assert_close(f"rmsnorm_fwd T{T} d{d}", y_.get_bf16((T, d)), y_ref, BF_ULP, 1e-3)
    assert_close(f"rmsnorm_rstd T{T} d{d}", rstd_.get(np.float32, (T,)), rstd_ref, 1e-5, 0)
    assert lib.tst_k_rmsnorm_bwd(dy_.ptr, dx_.ptr, rstd_.ptr, dw_.ptr, dres_.ptr, dxo_.ptr, T, d) == 0
    dx_ref, _ = O.rmsnorm_bwd(dy, x, rstd_ref, w, dres, bf16=True)
    assert_close(f"rmsnorm_bwd T{T} d{d}", dxo_.get_bf16((T, d)), dx_ref, BF_ULP, 2e-3)
    assert lib.tst_k_rmsnorm_bwd(dy_.ptr, dx_.ptr, rstd_.ptr, dw_.ptr, None, dxo_.ptr, T, d) == 0
    dx_ref, _ = O.rmsnorm_bwd(dy, x, rstd_ref, w, None, bf16=True)
    assert_close(f"rmsnorm_bwd_nores T{T} d{d}", dxo_.get_bf16((T, d)), dx_ref, BF_ULP, 2e-3)


@pytest.mark.parametrize("T,d,N,width,ends", [
    (3555, 4096, 192, 48, (1190, 2371, 3555)),     # the benchmark's stacked micro-batch: q|k|v group, three slots of 48 rank columns
    (3555, 4096, 128, 32, (1190, 2371, 3555)),     # gate|up group
    (2370, 4096, 64, 16, (1185, 1185, 2370)),      # an EMPTY middle slot
    (1200, 4096, 64, 0, ()),                       # one fold per context: no mask, N = RP = 64
    (77, 3584, 64, 48, (77,)),                     # Qwen2.5-7B width, one slot narrower than RP (padding columns: zeros), a ragged last tile
    (37, 1024, 64, 64, (37,)), (130, 2048, 16, 0, ()), (5, 3072, 32, 16, (2, 5)), (343, 256, 64, 48, (343,)), (100, 512, 192, 48, (40, 40, 100)),
])
def test_rmsnorm_rank_fwd(L, T, d, N, width, ends):
    """csrc/norm_rank.hip: RMSNorm forward (modeling_llama.py:62-67) fused with the rank-axis contraction that reads its result. y and rstd are BIT FOR BIT those
    of the same kernel without a rank block attached (the unfused form routes through it for these widths) and within one bf16 ulp / 1e-5 of the oracle;
    us = alpha y . Ag^T is the contraction of exactly that bf16 y (fp64 reference), every row keeping its slot's block only."""
    rng = np.random.default_rng(T + d + N)
    x = O.rbf(rng.standard_normal((T, d)).astype(np.float32) * 2)
    w = O.rbf((1 + 0.1 * rng.standard_normal(d)).astype(np.float32))
    Ag = O.rbf((rng.standard_normal((N, d)) * 0.05).astype(np.float32))
    alpha = 2.0
    lib = L.load_lab()
    x_, w_, Ag_ = L.dev_bf16(x), L.dev_bf16(w), L.dev_bf16(Ag)
    y_, y0_, rstd_, rstd0_ = L.DevBuf(nbytes=T * d * 2), L.DevBuf(nbytes=T * d * 2), L.DevBuf(nbytes=T * 4), L.DevBuf(nbytes=T * 4)
    us_ = L.dev_bf16(np.full((T, N), 7.0, np.float32))
    nslot = len(ends) if width else 0
    e = np.asarray(list(ends) + [T] * (8 - len(ends)), np.int32)
    assert lib.tst_k_rmsnorm_rank_fwd(x_.ptr, w_.ptr, y0_.ptr, rstd0_.ptr, T, d, 1e-5, None, 0, None, 0, 0.0, 0, 0, None) == 0      # plain norm, same kernel
    assert lib.tst_k_rmsnorm_rank_fwd(x_.ptr, w_.ptr, y_.ptr, rstd_.ptr, T, d, 1e-5, Ag_.ptr, d, us_.ptr, N, alpha, width, nslot, e.ctypes.data if width else None) == 0
    y, y0 = y_.get_bf16((T, d)), y0_.get_bf16((T, d))
    np.testing.assert_array_equal(y, y0)
    np.testing.assert_array_equal(rstd_.get(np.float32, (T,)), rstd0_.get(np.float32, (T,)))
    y_ref, rstd_ref = O.rmsnorm_fwd(x, w, 1e-5, bf16=True)
    # a last-bit difference of the fp32 statistic (another summation order than the oracle's) can move bf16(x rstd) by one ulp and, through the second rounding
    # behind the weight, y by up to two: at most a few elements per million beyond one ulp, none beyond two
    dev = np.abs(y.astype(np.float64) - y_ref) / (np.abs(y_ref) + 1e-3)
    assert (dev <= 2 * BF_ULP + 1e-6).all() and float((dev > BF_ULP).mean()) <= 5e-6, (float(dev.max()), float((dev > BF_ULP).mean()))
    report(f"rmsnorm_rank y T{T} d{d}", max_rel=float(dev.max()), frac_beyond_one_ulp=float((dev > BF_ULP).mean()))
    assert_close(f"rmsnorm_rank rstd T{T} d{d}", rstd_.get(np.float32, (T,)), rstd_ref, 1e-5, 0)
    assert lib.tst_k_rmsnorm_fwd(x_.ptr, w_.ptr, y0_.ptr, rstd0_.ptr, T, d, 1e-5) == 0      # the product's entry point for the plain norm
    np.testing.assert_array_equal(y0_.get_bf16((T, d)), y)
    keep = np.ones((T, N), bool)
    if width:
        slot = np.searchsorted(np.asarray(ends), np.arange(T), side="right")
        keep = (np.arange(N)[None, :] // width) == slot[:, None]
    us_ref = np.where(keep, alpha * (y.astype(np.float64) @ Ag.astype(np.float64).T), 0.0)
    us = us_.get_bf16((T, N))
    assert_close(f"rmsnorm_rank us T{T} d{d} N{N} w{width} {ends}", us, us_ref, BF_ULP, 1e-3)
    assert not us[~keep].any()


@pytest.mark.parametrize("T,d,res", [(1185, 4096, True), (40, 4096, False), (77, 3584, True), (343, 256, True), (9, 512, True), (8, 1024, False)])
def test_rmsnorm_bwd_dw(L, T, d, res):
    """csrc/norm_rank.hip rmsnorm_bwd_dw: the norm backward and the norm-weight gradient (full fine-tune) in ONE pass over dy and x. dx against the oracle and
    against the wave-per-row kernel (another summation order of the row statistic: a last-bit difference may move a rounding, never more than one bf16 ulp);
    dw against fp64 numpy on the same bf16 inputs, added ON TOP of what dw held; a second call gives the same bits (slice sums + ordered finish: no atomics)."""
    rng = np.random.default_rng(T + d)
    x = O.rbf(rng.standard_normal((T, d)).astype(np.float32) * 2)
    w = O.rbf((1 + 0.1 * rng.standard_normal(d)).astype(np.float32))
    dy = O.rbf(rng.standard_normal((T, d)).astype(np.float32))
    dres = O.rbf(rng.standard_normal((T, d)).astype(np.float32))
    _, rstd = O.rmsnorm_fwd(x, w, 1e-5, bf16=True)
    lib = L.load_lab()
    x_, w_, dy_, dres_, rstd_ = L.dev_bf16(x), L.dev_bf16(w), L.dev_bf16(dy), L.dev_bf16(dres), L.DevBuf(rstd.astype(np.float32))
    dx_, dx0_ = L.DevBuf(nbytes=T * d * 2), L.DevBuf(nbytes=T * d * 2)
    base = rng.standard_normal(d).astype(np.float32)
    dw_, dw2_ = L.DevBuf(base.copy()), L.DevBuf(base.copy())
    assert lib.tst_k_rmsnorm_bwd_dw(dy_.ptr, x_.ptr, rstd_.ptr, w_.ptr, dres_.ptr if res else None, dx_.ptr, dw_.ptr, T, d) == 0
    dx_ref, dw_ref = O.rmsnorm_bwd(dy, x, rstd, w, dres if res else None, bf16=True)
    dx = dx_.get_bf16((T, d))
    assert_close(f"rmsnorm_bwd_dw dx T{T} d{d}", dx, dx_ref, BF_ULP, 2e-3)
    assert lib.tst_k_rmsnorm_bwd(dy_.ptr, x_.ptr, rstd_.ptr, w_.ptr, dres_.ptr if res else None, dx0_.ptr, T, d) == 0
    dx0 = dx0_.get_bf16((T, d))
    assert float((dx != dx0).mean()) <= 2e-3 and np.abs(dx.astype(np.float64) - dx0).max() <= BF_ULP * np.abs(dx0).max()
    dw64 = (dy.astype(np.float64) * O.rbf((x.astype(np.float32) * rstd[:, None]).astype(np.float32)).astype(np.float64)).sum(0)
    got = dw_.get(np.float32, (d,)) - base
    assert_close(f"rmsnorm_bwd_dw dw T{T} d{d}", got, dw64, 1e-4, 1e-4)
    assert_close(f"rmsnorm_bwd_dw dw vs oracle T{T} d{d}", got, dw_ref, 1e-3, 1e-3)
    assert lib.tst_k_rmsnorm_bwd_dw(dy_.ptr, x_.ptr, rstd_.ptr, w_.ptr, dres_.ptr if res else None, dx0_.ptr, dw2_.ptr, T, d) == 0
    np.testing.assert_array_equal(dw2_.get(np.float32, (d,)), dw_.get(np.float32, (d,)))
    np.testing.assert_array_equal(dx0_.get_bf16((T, d)), dx)
    assert lib.tst_k_rmsnorm_bwd_dw(dy_.ptr, x_.ptr, rstd_.ptr, w_.ptr, dres_.ptr if res else None, dx0_.ptr, None, T, d) == 0      # dx only
    np.testing.assert_array_equal(dx0_.get_bf16((T, d)), dx)


@pytest.mark.parametrize("T,d,vocab,hot", [(1185, 4096, 1000, 0.25), (300, 768, 50, 0.0), (64, 1024, 7, 0.5), (1, 256, 5, 0.0), (515, 256, 128256, 0.3)])
def test_embed_bwd_token_order(L, T, d, vocab, hot):
    """csrc/elementwise.hip embed_bwd (full fine-tune, torch.nn.functional.embedding's backward = index_add over the token axis): dE[ids[t], :] += dx[t, :]
    with the rows of one id added in TOKEN ORDER on top of what dE held -- bit-exact against sequential fp32 adds in numpy; ids outside [0, vocab) clamp as the
    forward's do; a frequent id (hot = its share of the tokens) goes through one workgroup per column slice."""
    rng = np.random.default_rng(T * 7 + d)
    ids = rng.integers(0, vocab, T).astype(np.int32)
    if hot > 0:
        ids[rng.random(T) < hot] = ids[0]
    if T > 3:
        ids[1], ids[2] = -4, vocab + 9
    dx = O.rbf(rng.standard_normal((T, d)).astype(np.float32))
    rows = np.unique(np.clip(ids, 0, vocab - 1))
    base = rng.standard_normal((len(rows), d)).astype(np.float32)
    want = base.copy()
    slot = {int(r): k for k, r in enumerate(rows)}
    for t in range(T):
        k = slot[int(np.clip(ids[t], 0, vocab - 1))]
        want[k] = (want[k] + dx[t]).astype(np.float32)
    lib = L.load_lab()
    full = np.zeros((vocab, d), np.float32)
    full[rows] = base
    dE = L.DevBuf(full)
    ids_, dx_ = L.DevBuf(ids), L.dev_bf16(dx)   # held until the result is read: a temporary's buffer is freed before the launch
    assert lib.tst_k_embed_bwd(ids_.ptr, dx_.ptr, dE.ptr, T, d, vocab, 0, None) == 0
    got = dE.get(np.float32, (vocab, d))
    np.testing.assert_array_equal(got[rows], want)
    mask = np.ones(vocab, bool)
    mask[rows] = False
    assert not got[mask].any()


def test_rope(L):
    rng = np.random.default_rng(9)
    T, H, Hkv, dh = 37, 4, 2, 128
    ld = (H + 2 * Hkv) * dh
    qkv = O.rbf(rng.standard_normal((T, ld)).astype(np.float32))
    pos = rng.integers(0, 100, T).astype(np.int32)
    cos, sin = O.rope_tables(np.arange(100), dh, 500000.0, bf16=True)
    d_, p_, c_, s_ = L.dev_bf16(qkv), L.DevBuf(pos), L.DevBuf(cos), L.DevBuf(sin)
    lib = L.load_lab()
    assert lib.tst_k_rope(d_.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, dh, ld, 0) == 0
    got = d_.get_bf16((T, ld))
    ref = qkv.copy()
    rot = O.rope_apply(qkv[:, : (H + Hkv) * dh].reshape(T, H + Hkv, dh), cos[pos], sin[pos], bf16=True)
    ref[:, : (H + Hkv) * dh] = rot.reshape(T, -1)
    assert_close("rope_fwd", got, ref, BF_ULP, 1e-3)
    np.testing.assert_array_equal(got[:, (H + Hkv) * dh:], qkv[:, (H + Hkv) * dh:])  # v untouched
    assert lib.tst_k_rope(d_.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, dh, ld, 1) == 0
    back = O.rope_apply(rot, cos[pos], sin[pos], bf16=True, backward=True).reshape(T, -1)
    assert_close("rope_bwd", d_.get_bf16((T, ld))[:, : (H + Hkv) * dh], back, BF_ULP, 1e-3)


@pytest.mark.parametrize("tag", ["llama31", "linear4", "theta500k"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_rope_long_positions(L, tag, precision):
    """the stand-alone rope kernel (sequences over 128 tokens: engine.hip runs it around attention) at positions spread over 0 .. 8191, on tables
    of a Llama-3.1 scaled, a linearly scaled and a plain theta = 500000 frequency set; forward, then backward back to the input. bf16: the bound of
    test_rope; fp32: summation-free, so within a few fp32 ulps. v untouched either way."""
    rng = np.random.default_rng(8191 + len(tag))
    T, H, Hkv, dh, P = 300, 4, 2, 128, 8192
    ld = (H + 2 * Hkv) * dh
    nrot = (H + Hkv) * dh
    theta, rs = {c[0]: c[1:] for c in GI.ROPE_SCALING_CASES}.get(tag, (500000.0, None))
    bf = precision == "bf16"
    cos, sin = O.rope_tables(np.arange(P), dh, theta, bf16=bf, scaling=rs)
    pos = rng.integers(0, P, T).astype(np.int32)
    pos[:4] = (0, 1, P - 2, P - 1)
    qkv = rng.standard_normal((T, ld)).astype(np.float32)
    if bf:
        qkv = O.rbf(qkv)
    lib = L.load_lab()
    d_ = L.dev_bf16(qkv) if bf else L.dev_f32(qkv)
    p_, c_, s_ = L.DevBuf(pos), L.DevBuf(cos), L.DevBuf(sin)
    get = (lambda: d_.get_bf16((T, ld))) if bf else (lambda: d_.get(np.float32, (T, ld)))
    rope = lib.tst_k_rope if bf else lib.tst_k_rope_f32
    rtol, atol = (BF_ULP, 1e-3) if bf else (1e-6, 1e-6)
    assert rope(d_.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, dh, ld, 0) == 0
    fwd = get()
    rot = O.rope_apply(qkv[:, :nrot].reshape(T, H + Hkv, dh), cos[pos], sin[pos], bf16=bf)
    assert_close(f"rope_fwd long {tag} {precision}", fwd[:, :nrot], rot.reshape(T, -1), rtol, atol)
    np.testing.assert_array_equal(fwd[:, nrot:], qkv[:, nrot:])
    assert rope(d_.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, dh, ld, 1) == 0
    got = get()
    back = O.rope_apply(fwd[:, :nrot].reshape(T, H + Hkv, dh), cos[pos], sin[pos], bf16=bf, backward=True)
    assert_close(f"rope_bwd long {tag} {precision}", got[:, :nrot], back.reshape(T, -1), rtol, atol)
    if not bf:   # fp32 tables: cos^2 + sin^2 = 1 to fp32 precision, so the backward undoes the forward (bf16 tables are off by up to 2^-8)
        assert_close(f"rope_roundtrip long {tag} {precision}", got[:, :nrot], qkv[:, :nrot], 2 * rtol, 2 * atol)
    np.testing.assert_array_equal(got[:, nrot:], qkv[:, nrot:])


def test_swiglu(L):
    rng = np.random.default_rng(12)
    T, F = 19, 448
    gu = O.rbf(rng.standard_normal((T, 2 * F)).astype(np.float32) * 2)
    da = O.rbf(rng.standard_normal((T, F)).astype(np.float32))
    gu_, da_, a_, dgu_ = L.dev_bf16(gu), L.dev_bf16(da), L.DevBuf(nbytes=T * F * 2), L.DevBuf(nbytes=T * 2 * F * 2)
    lib = L.load_lab()
    assert lib.tst_k_swiglu_fwd(gu_.ptr, a_.ptr, T, F) == 0
    assert_close("swiglu_fwd", a_.get_bf16((T, F)), O.swiglu_fwd(gu[:, :F], gu[:, F:], bf16=True), BF_ULP, 1e-3)
    assert lib.tst_k_swiglu_bwd(da_.ptr, gu_.ptr, dgu_.ptr, T, F) == 0
    dg, du = O.swiglu_bwd(da, gu[:, :F], gu[:, F:], bf16=True)
    assert_close("swiglu_bwd", dgu_.get_bf16((T, 2 * F)), np.concatenate([dg, du], 1), BF_ULP, 1e-3)


@pytest.mark.parametrize("T,F,width,ends", [(100, 256, 0, ()), (83, 512, 16, (30, 31)), (83, 512, 32, (16, 50)), (70, 256, 16, (0, 40)), (37, 256, 64, (20,)),
                                            (300, 14336, 32, (97, 211))])
def test_swiglu_with_the_rank_contraction_in_the_same_pass(L, T, F, width, ends):
    """csrc/swiglu_rank.hip: act / dgu are bit for bit those of the elementwise kernels; us = alpha act . Ag^T and du = alpha dgu . BgT^T are the rank-axis
    contraction of those bf16 values (fp32 sums, one rounding), every row keeping its slot's block of `width` columns only and exact zeros elsewhere. Row tiles
    are cut at the slot boundaries: a one-row slot, an EMPTY slot and a boundary inside a 16-row tile are among the cases."""
    rng = np.random.default_rng(T + F + width)
    nslot = len(ends) + 1
    N = max(16, nslot * width) if width else 48
    gu = O.rbf(rng.standard_normal((T, 2 * F)).astype(np.float32) * 2)
    da = O.rbf(rng.standard_normal((T, F)).astype(np.float32))
    Ag = O.rbf(rng.standard_normal((N, F)).astype(np.float32) * 0.05)
    BgT = O.rbf(rng.standard_normal((N, 2 * F)).astype(np.float32) * 0.05)
    gu_, da_, Ag_, BgT_ = L.dev_bf16(gu), L.dev_bf16(da), L.dev_bf16(Ag), L.dev_bf16(BgT)
    a_ref_, dgu_ref_ = L.DevBuf(nbytes=T * F * 2), L.DevBuf(nbytes=T * 2 * F * 2)
    a_, dgu_ = L.DevBuf(nbytes=T * F * 2), L.DevBuf(nbytes=T * 2 * F * 2)
    us_, du_ = L.dev_bf16(np.full((T, N), 7.0, np.float32)), L.dev_bf16(np.full((T, N), 7.0, np.float32))   # poisoned: every element must be written
    lib = L.load_lab()
    assert lib.tst_k_swiglu_fwd(gu_.ptr, a_ref_.ptr, T, F) == 0
    assert lib.tst_k_swiglu_bwd(da_.ptr, gu_.ptr, dgu_ref_.ptr, T, F) == 0
    e = np.asarray(ends, np.int32)
    alpha = 2.0
    assert lib.tst_k_swiglu_rank_fwd(gu_.ptr, a_.ptr, T, F, Ag_.ptr, F, us_.ptr, N, alpha, width, nslot, e.ctypes.data if len(e) else None) == 0
    assert lib.tst_k_swiglu_rank_bwd(da_.ptr, gu_.ptr, dgu_.ptr, T, F, BgT_.ptr, 2 * F, du_.ptr, N, alpha, width, nslot, e.ctypes.data if len(e) else None, 0) == 0
    act, dgu = a_ref_.get_bf16((T, F)), dgu_ref_.get_bf16((T, 2 * F))
    np.testing.assert_array_equal(a_.get_bf16((T, F)), act)
    np.testing.assert_array_equal(dgu_.get_bf16((T, 2 * F)), dgu)
    keep = np.ones((T, N), bool)
    if width:
        slot = np.searchsorted(np.asarray(ends), np.arange(T), side="right")
        cols = np.arange(N)[None, :] // width
        keep = cols == slot[:, None]
    us_ref = np.where(keep, alpha * (act.astype(np.float64) @ Ag.astype(np.float64).T), 0.0)
    du_ref = np.where(keep, alpha * (dgu.astype(np.float64) @ BgT.astype(np.float64).T), 0.0)
    us, du = us_.get_bf16((T, N)), du_.get_bf16((T, N))
    tag = f"T{T} F{F} w{width} {ends}"
    assert_close("swiglu_rank us " + tag, us, us_ref, BF_ULP, 1e-3)
    assert_close("swiglu_rank du " + tag, du, du_ref, BF_ULP, 1e-3)
    assert not us[~keep].any() and not du[~keep].any()
    if width and width % 32 == 0:
        # the gate|up group's BgT is block diagonal by module (first half of a rank block: the gate module, zero on the up columns; second half: up): the
        # kernel then multiplies gate steps with the first half only and up steps with the second
        h = width // 2
        Bd = BgT.copy()
        for sl in range(nslot):
            Bd[sl * width: sl * width + h, F:] = 0
            Bd[sl * width + h: (sl + 1) * width, :F] = 0
        Bd_ = L.dev_bf16(Bd)
        du2_ = L.dev_bf16(np.full((T, N), 7.0, np.float32))
        assert lib.tst_k_swiglu_rank_bwd(da_.ptr, gu_.ptr, dgu_.ptr, T, F, Bd_.ptr, 2 * F, du2_.ptr, N, alpha, width, nslot, e.ctypes.data if len(e) else None, 1) == 0
        du2_ref = np.where(keep, alpha * (dgu.astype(np.float64) @ Bd.astype(np.float64).T), 0.0)
        du2 = du2_.get_bf16((T, N))
        assert_close("swiglu_rank du block-diagonal " + tag, du2, du2_ref, BF_ULP, 1e-3)
        assert not du2[~keep].any()
        np.testing.assert_array_equal(dgu_.get_bf16((T, 2 * F)), dgu)


@pytest.mark.parametrize("R,V", [(5, 256), (37, 128256)])
def test_logit_rows(L, R, V):
    rng = np.random.default_rng(R)
    logits = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    tgt = rng.integers(0, V, R).astype(np.int32)
    logits[1, tgt[1]] = 40.0  # one confidently-correct row
    opt = np.array([3, 17, 5, V - 1], np.int32)
    lg_, t_, st_, dl_, op_, ol_ = L.DevBuf(logits), L.DevBuf(tgt), L.DevBuf(nbytes=R * 16), L.DevBuf(nbytes=R * V * 2), L.DevBuf(opt), L.DevBuf(nbytes=R * 16)
    assert L.load_lab().tst_k_logit_rows(lg_.ptr, V, t_.ptr, R, V, st_.ptr, dl_.ptr, V, 1.0 / 7, op_.ptr, 4, ol_.ptr) == 0
    st = st_.get(np.float32, (R, 4))
    loss, dl, lse = O.ce_rows(logits, tgt, 7)
    assert_close(f"ce_lse R{R} V{V}", st[:, 0], lse, 1e-5, 1e-6)
    np.testing.assert_array_equal(st[:, 1], logits[np.arange(R), tgt])
    np.testing.assert_array_equal(st[:, 2].view(np.int32), logits.argmax(-1))
    assert_close(f"ce_dlogits R{R} V{V}", dl_.get_bf16((R, V)), O.rbf(dl), 2 * BF_ULP, 1e-4)
    np.testing.assert_array_equal(ol_.get(np.float32, (R, 4)), logits[:, opt])


@pytest.mark.parametrize("lengths,H,Hkv", [((7, 48, 100), 2, 1), ((64, 65, 128, 1), 4, 2), ((130,), 4, 1), ((16, 15, 17, 96, 1, 81), 7, 1)])   # last: Qwen2.5-7B's group of 7
def test_attention_fwd_bwd(L, lengths, H, Hkv):
    rng = np.random.default_rng(sum(lengths) + H)
    dh = 128
    T = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ld = (H + 2 * Hkv) * dh
    qkv = O.rbf(rng.standard_normal((T, ld)).astype(np.float32))
    qkv[5 % T, :dh] *= 6.0  # spike one query row: exercises the running-max rescale across key tiles
    qkv = O.rbf(qkv)
    do = O.rbf(rng.standard_normal((T, H * dh)).astype(np.float32))
    q = qkv[:, : H * dh].reshape(T, H, dh)
    k = qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh)
    v = qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh)
    out_ref, lse_ref = O.attention_fwd(q, k, v, cu, bf16=True)
    dq_ref, dk_ref, dv_ref = O.attention_bwd(q, k, v, out_ref, do.reshape(T, H, dh), lse_ref, cu, bf16=True)
    qkv_, cu_, do_ = L.dev_bf16(qkv), L.DevBuf(cu), L.dev_bf16(do)
    out_, lse_, delta_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4)
    dqkv_ = L.DevBuf(nbytes=T * ld * 2)
    lib = L.load_lab()
    scale = 1.0 / np.sqrt(dh)
    assert lib.tst_k_attn_fwd(qkv_.ptr, ld, cu_.ptr, len(lengths), max(lengths), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    tag = f"L{'_'.join(map(str, lengths))} H{H}/{Hkv}"
    assert_close("attn_out " + tag, out_.get_bf16((T, H, dh)), out_ref, 2 * BF_ULP, 5e-3)
    assert_close("attn_lse " + tag, lse_.get(np.float32, (H, T)), lse_ref, 1e-4, 1e-4)
    assert lib.tst_k_attn_bwd(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, len(lengths), max(lengths), dqkv_.ptr, T, H,
                              Hkv, dh, scale) == 0
    dqkv = dqkv_.get_bf16((T, ld))
    assert_close("attn_dq " + tag, dqkv[:, : H * dh].reshape(T, H, dh), dq_ref, 4 * BF_ULP, 2e-2)
    assert_close("attn_dk " + tag, dqkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), dk_ref, 4 * BF_ULP, 2e-2)
    assert_close("attn_dv " + tag, dqkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh), dv_ref, 4 * BF_ULP, 2e-2)


@pytest.mark.parametrize("lengths,H,Hkv,dh", [((7, 48, 100), 2, 1, 128), ((64, 65, 128, 1), 4, 2, 128), ((33, 64, 12, 50), 8, 2, 128), ((128, 127, 66), 4, 1, 128), ((80, 81, 16, 112), 14, 2, 128),
                                             ((5, 64, 17), 2, 2, 64), ((128, 70, 1), 4, 4, 64)])
def test_attention_backward_single_kernel(L, lengths, H, Hkv, dh):
    """sequences of at most 128 tokens: ONE backward kernel (dQ, dK, dV and delta; S and dP computed once per pair) against the oracle,
    and against the dQ + dK/dV kernel pair on the same inputs (same operand roundings: the two paths differ only in summation order)"""
    rng = np.random.default_rng(sum(lengths) + 31 * H + dh)
    T = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ld = (H + 2 * Hkv) * dh
    qkv = O.rbf(rng.standard_normal((T, ld)).astype(np.float32))
    do = O.rbf(rng.standard_normal((T, H * dh)).astype(np.float32))
    q = qkv[:, : H * dh].reshape(T, H, dh)
    k = qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh)
    v = qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh)
    out_ref, lse_ref = O.attention_fwd(q, k, v, cu, bf16=True)
    dq_ref, dk_ref, dv_ref = O.attention_bwd(q, k, v, out_ref, do.reshape(T, H, dh), lse_ref, cu, bf16=True)
    qkv_, cu_, do_ = L.dev_bf16(qkv), L.DevBuf(cu), L.dev_bf16(do)
    out_, lse_, delta_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4)
    lib = L.load_lab()
    scale = 1.0 / np.sqrt(dh)
    assert lib.tst_k_attn_fwd(qkv_.ptr, ld, cu_.ptr, len(lengths), max(lengths), out_.ptr, H * dh, lse_.ptr, T, H, Hkv, dh, scale) == 0
    res = {}
    prev = lib.tst_dev_attn_fused_bwd(0)
    try:
        for mode in (0, 1):
            lib.tst_dev_attn_fused_bwd(mode)
            dqkv_ = L.DevBuf(nbytes=T * ld * 2)
            assert lib.tst_dev_memset(dqkv_.ptr, 0x7f, T * ld * 2) == 0       # every element must be written
            assert lib.tst_k_attn_bwd(qkv_.ptr, ld, out_.ptr, H * dh, do_.ptr, H * dh, lse_.ptr, delta_.ptr, cu_.ptr, len(lengths), max(lengths), dqkv_.ptr,
                                      T, H, Hkv, dh, scale) == 0
            res[mode] = dqkv_.get_bf16((T, ld))
    finally:
        lib.tst_dev_attn_fused_bwd(prev)
    tag = f"fused L{'_'.join(map(str, lengths))} H{H}/{Hkv} dh{dh}"
    for mode in (0, 1):
        d = res[mode]
        assert np.isfinite(d).all()
        assert_close(f"attn_dq[{mode}] " + tag, d[:, : H * dh].reshape(T, H, dh), dq_ref, 4 * BF_ULP, 2e-2)
        assert_close(f"attn_dk[{mode}] " + tag, d[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), dk_ref, 4 * BF_ULP, 2e-2)
        assert_close(f"attn_dv[{mode}] " + tag, d[:, (H + Hkv) * dh:].reshape(T, Hkv, dh), dv_ref, 4 * BF_ULP, 2e-2)
    mx, mxr, rel = err_stats(res[1], res[0])
    report("attn_bwd_single_vs_pair " + tag, max_abs=mx, max_over_rms=mxr, rel_l2=rel)
    assert np.abs(res[1] - res[0]).max() <= 4 * BF_ULP * max(1.0, float(np.abs(res[0]).max()))


@pytest.mark.parametrize("lengths,H,Hkv", [((7, 48, 100), 2, 1), ((64, 65, 128, 1), 4, 2), ((33, 64, 12, 50), 8, 2), ((128, 127, 66), 4, 1), ((1, 2, 3), 2, 2)])
def test_attention_with_rope_inside_the_kernels(L, lengths, H, Hkv):
    """q and k leave the projection un-rotated and are rotated where the attention kernels stage them; dq / dk come back through
    the inverse rotation in the backward kernel's store. Against the stand-alone path on the same inputs -- rope kernel, attention, attention
    backward, rope kernel (backward) -- forward bit-identical (the same fp32 rotation of the same bf16 values, one rounding), backward within
    one rounding (the stand-alone path rounds dq / dk to bf16 BEFORE rotating them back, the fused store rotates the fp32 accumulators);
    and against the oracle (rope + attention in its bf16 mirror)."""
    rng = np.random.default_rng(sum(lengths) * 3 + H)
    dh, P = 128, 160
    T = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    pos = np.concatenate([np.arange(n) for n in lengths]).astype(np.int32)
    ld = (H + 2 * Hkv) * dh
    qkv = O.rbf(rng.standard_normal((T, ld)).astype(np.float32))
    do = O.rbf(rng.standard_normal((T, H * dh)).astype(np.float32))
    cos, sin = O.rope_tables(np.arange(P), dh, 10000.0, True)          # [P, 64] fp32, bf16-exact (what the engine builds)
    cos, sin = np.ascontiguousarray(cos[:, : dh // 2], np.float32), np.ascontiguousarray(sin[:, : dh // 2], np.float32)
    lib = L.load_lab()
    scale = 1.0 / np.sqrt(dh)
    cu_, do_, pos_, cos_, sin_ = L.DevBuf(cu), L.dev_bf16(do), L.DevBuf(pos), L.DevBuf(cos), L.DevBuf(sin)
    n, mx = len(lengths), max(lengths)
    # stand-alone: rotate q, k in place, attention, backward, rotate dq, dk back
    a_qkv = L.dev_bf16(qkv)
    assert lib.tst_k_rope(a_qkv.ptr, pos_.ptr, cos_.ptr, sin_.ptr, T, H + Hkv, dh, ld, 0) == 0
    a_out, a_lse, delta_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4), L.DevBuf(nbytes=H * T * 4)
    assert lib.tst_k_attn_fwd(a_qkv.ptr, ld, cu_.ptr, n, mx, a_out.ptr, H * dh, a_lse.ptr, T, H, Hkv, dh, scale) == 0
    a_dqkv = L.DevBuf(nbytes=T * ld * 2)
    assert lib.tst_k_attn_bwd(a_qkv.ptr, ld, a_out.ptr, H * dh, do_.ptr, H * dh, a_lse.ptr, delta_.ptr, cu_.ptr, n, mx, a_dqkv.ptr, T, H, Hkv, dh, scale) == 0
    assert lib.tst_k_rope(a_dqkv.ptr, pos_.ptr, cos_.ptr, sin_.ptr, T, H + Hkv, dh, ld, 1) == 0
    # fused
    b_qkv = L.dev_bf16(qkv)
    b_out, b_lse = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4)
    assert lib.tst_k_attn_fwd_rope(b_qkv.ptr, ld, cu_.ptr, n, mx, b_out.ptr, H * dh, b_lse.ptr, T, H, Hkv, dh, scale, cos_.ptr, sin_.ptr) == 0
    b_dqkv = L.DevBuf(nbytes=T * ld * 2)
    assert lib.tst_dev_memset(b_dqkv.ptr, 0x7f, T * ld * 2) == 0
    assert lib.tst_k_attn_bwd_rope(b_qkv.ptr, ld, b_out.ptr, H * dh, do_.ptr, H * dh, b_lse.ptr, delta_.ptr, cu_.ptr, n, mx, b_dqkv.ptr, T, H, Hkv, dh, scale,
                                   cos_.ptr, sin_.ptr) == 0
    tag = f"rope-in-attn L{'_'.join(map(str, lengths))} H{H}/{Hkv}"
    np.testing.assert_array_equal(b_out.get(np.uint16, (T, H * dh)), a_out.get(np.uint16, (T, H * dh)))
    np.testing.assert_array_equal(b_lse.get(np.float32, (H, T)), a_lse.get(np.float32, (H, T)))
    da, db = a_dqkv.get_bf16((T, ld)), b_dqkv.get_bf16((T, ld))
    assert np.isfinite(db).all()
    np.testing.assert_array_equal(db[:, (H + Hkv) * dh:], da[:, (H + Hkv) * dh:])                       # dV: no rotation involved
    mxd, mxr, rel = err_stats(db, da)
    report("attn_rope_fused_vs_standalone " + tag, max_abs=mxd, max_over_rms=mxr, rel_l2=rel)
    assert np.abs(db - da).max() <= 3 * BF_ULP * max(1.0, float(np.abs(da).max())) and rel < 4e-3
    # oracle: rope (bf16 mirror) -> attention -> backward -> rope backward
    cf, sf = cos[pos], sin[pos]
    q = O.rope_apply(qkv[:, : H * dh].reshape(T, H, dh), cf, sf, True)
    k = O.rope_apply(qkv[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), cf, sf, True)
    v = qkv[:, (H + Hkv) * dh:].reshape(T, Hkv, dh)
    out_ref, lse_ref = O.attention_fwd(q, k, v, cu, bf16=True)
    dq_ref, dk_ref, dv_ref = O.attention_bwd(q, k, v, out_ref, do.reshape(T, H, dh), lse_ref, cu, bf16=True)
    dq_ref, dk_ref = O.rope_apply(dq_ref, cf, sf, True, backward=True), O.rope_apply(dk_ref, cf, sf, True, backward=True)
    assert_close("attn_out " + tag, b_out.get_bf16((T, H, dh)), out_ref, 2 * BF_ULP, 5e-3)
    assert_close("attn_dq " + tag, db[:, : H * dh].reshape(T, H, dh), dq_ref, 4 * BF_ULP, 2e-2)
    assert_close("attn_dk " + tag, db[:, H * dh: (H + Hkv) * dh].reshape(T, Hkv, dh), dk_ref, 4 * BF_ULP, 2e-2)
    assert_close("attn_dv " + tag, db[:, (H + Hkv) * dh:].reshape(T, Hkv, dh), dv_ref, 4 * BF_ULP, 2e-2)


def test_attention_matches_hf_fixture(L, golden_dir):
    """same inputs as the HF eager-attention fixture (fp32): bf16 kernel within bf16 noise of the HF fp32 result."""
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    q, k, v = (g[n][0].transpose(1, 0, 2) for n in ("att_q", "att_k", "att_v"))
    T, H, dh = q.shape
    qkv = np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1)
    cu = np.array([0, T], np.int32)
    qkv_, cu_ = L.dev_bf16(qkv), L.DevBuf(cu)
    out_, lse_ = L.DevBuf(nbytes=T * H * dh * 2), L.DevBuf(nbytes=H * T * 4)
    assert L.load_lab().tst_k_attn_fwd(qkv_.ptr, qkv.shape[1], cu_.ptr, 1, T, out_.ptr, H * dh, lse_.ptr, T, H, 1, dh, 1.0 / np.sqrt(dh)) == 0
    assert_close("attn_vs_hf_fp32", out_.get_bf16((T, H, dh)), g["att_o"][0], 0.05, 0.03)


def test_adamw_clip(L, golden_dir):
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    n = 1000
    p_, m_, v_ = L.DevBuf(g["ad_p0"].copy()), L.DevBuf(nbytes=n * 4), L.DevBuf(nbytes=n * 4)
    nc_, ws_ = L.DevBuf(nbytes=8), L.DevBuf(nbytes=1024)
    for s in range(3):
        g_ = L.DevBuf(g["ad_g"][s].copy())
        assert L.load_lab().tst_k_adamw(p_.ptr, g_.ptr, m_.ptr, v_.ptr, n, 1.0, 3e-3, 0.9, 0.999, 1e-8, 0.05, s + 1, nc_.ptr, ws_.ptr) == 0
        nc = nc_.get(np.float32, (2,))
        assert abs(nc[0] - g["ad_norm"][s]) <= 1e-5 * g["ad_norm"][s]
        assert_close(f"adamw_step{s + 1}_vs_torch_fused", p_.get(np.float32, (n,)), g["ad_p"][s], 2e-6, 1e-6)


@pytest.mark.parametrize("M,F,K", [(300, 256, 128), (1200, 512, 256), (257, 1024, 64)])
def test_swiglu_behind_both_tile_families_is_bit_identical(L, M, F, K):
    """gate|up projection ([gate | up]) and the down projection's dX on the 256x256 ping-pong tile (variant 5) and on the 128x128 tile (variant 0),
    each followed by the elementwise SwiGLU kernel: the two tile families give bit-identical results, and both follow the oracle's swiglu."""
    rng = np.random.default_rng(M + F + K)
    lib = L.load_lab()
    x = O.rbf(rng.standard_normal((M, K)).astype(np.float32))
    Wg, Wu = (O.rbf(0.2 * rng.standard_normal((F, K)).astype(np.float32)) for _ in range(2))
    x_, W_ = L.dev_bf16(x), L.dev_bf16(np.concatenate([Wg, Wu], 0))
    outs = {}
    for v, sk in ((5, 1), (0, -1)):
        gu_, act_ = L.DevBuf(nbytes=M * 2 * F * 2), L.DevBuf(nbytes=M * F * 2)
        assert lib.tst_k_gemm_nt(x_.ptr, K, W_.ptr, K, None, 0, None, 0, gu_.ptr, 2 * F, None, 0, M, 2 * F, K, 0, 1.0, 0, v, sk) == 0
        assert lib.tst_k_swiglu_fwd(gu_.ptr, act_.ptr, M, F) == 0
        outs[v] = (gu_.get(np.uint16, (M, 2 * F)), act_.get(np.uint16, (M, F)))
    np.testing.assert_array_equal(outs[5][0], outs[0][0])
    np.testing.assert_array_equal(outs[5][1], outs[0][1])
    g_ref, u_ref = O.rbf(x @ Wg.T), O.rbf(x @ Wu.T)
    act_ref = O.swiglu_fwd(g_ref, u_ref, bf16=True)
    from tst.lib import from_bf16_bits
    assert_close(f"swiglu_fwd behind the tile M{M} F{F}", from_bf16_bits(outs[5][1]), act_ref, 2 * BF_ULP, 1e-3)
    # backward: dy [M, Kd] . WdT [F, Kd]^T -> d(act) -> d(gate|up)
    Kd = K
    dy = O.rbf(rng.standard_normal((M, Kd)).astype(np.float32))
    WdT = O.rbf(0.2 * rng.standard_normal((F, Kd)).astype(np.float32))
    dy_, WdT_, gu_ = L.dev_bf16(dy), L.dev_bf16(WdT), L.DevBuf(outs[5][0])
    res = {}
    for v, sk in ((5, 1), (0, -1)):
        dgu_, dact_ = L.DevBuf(nbytes=M * 2 * F * 2), L.DevBuf(nbytes=M * F * 2)
        assert lib.tst_k_gemm_nt(dy_.ptr, Kd, WdT_.ptr, Kd, None, 0, None, 0, dact_.ptr, F, None, 0, M, F, Kd, 0, 1.0, 0, v, sk) == 0
        assert lib.tst_k_swiglu_bwd(dact_.ptr, gu_.ptr, dgu_.ptr, M, F) == 0
        res[v] = dgu_.get(np.uint16, (M, 2 * F))
    np.testing.assert_array_equal(res[5], res[0])
    dact = O.rbf(dy @ WdT.T)
    dg_ref, du_ref = O.swiglu_bwd(dact, g_ref, u_ref, bf16=True)
    for v in (5, 0):
        assert_close(f"swiglu_bwd behind the tile M{M} F{F} variant {v}", from_bf16_bits(res[v]), np.concatenate([dg_ref, du_ref], 1), 4 * BF_ULP, 2e-3)
