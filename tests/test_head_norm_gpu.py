"""GPU parity of the Qwen3 per-head q/k RMSNorm kernels (csrc/head_norm.hip), through the lab hooks tst_k_head_norm_fwd / _bwd and their _f32 twins.

Reference: oracle.ops_np.rmsnorm_fwd / rmsnorm_bwd on the [T * heads, 128] view of the q|k columns (bf16-mirror mode for the bf16 kernels). Bounds are those
tests/test_kernels_gpu.py states for the row-wide RMSNorm (test_rmsnorm: BF_ULP, 1e-3 forward; 1e-5 on rstd; BF_ULP, 2e-3 backward; test_rmsnorm_bwd_dw for
the weight gradients) and tests/test_strict_gpu.py for the fp32 norm kernels (2e-6 forward, 5e-6 backward, absolute, on O(1) values). The fused-RoPE form is
compared BIT FOR BIT with head norm followed by tst_k_rope."""
import numpy as np
import pytest

import golden_inputs as GI
from oracle import ops_np as O

pytestmark = pytest.mark.gpu

BF_ULP = 2.0 ** -7  # one bf16 ulp relative, worst case (tests/test_kernels_gpu.py)


def assert_close(name, a, b, rtol, atol_rms):
    """|a-b| <= rtol*|b| + atol_rms*rms(b) elementwise (the check of tests/test_kernels_gpu.py); prints the figures before it asserts"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), f"{name}: non-finite output"
    rms = float(np.sqrt(np.mean(b * b))) + 1e-30
    d = np.abs(a - b)
    print(f"{name}: max|d|={d.max():.3e} max|d|/rms={d.max() / rms:.3e} rel_l2={np.sqrt(np.mean(d * d)) / rms:.3e}")
    bad = d > rtol * np.abs(b) + atol_rms * rms
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.size} elements out of tolerance, max|d|={d.max():.3e} rms(ref)={rms:.3e}"

SHAPES = [(37, 4, 2), (1185, 32, 8), (3555, 32, 8), (1, 7, 1)]
EPS = 1e-6


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load_lab()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def _inputs(T, H, Hkv, bf16, seed=0):
    rng = np.random.default_rng(1000 * T + 10 * H + Hkv + seed)
    ld = (H + 2 * Hkv) * 128
    rb = O.rbf if bf16 else (lambda a: a)
    qkv = rb(rng.standard_normal((T, ld)).astype(np.float32) * 2)
    dqkv = rb(rng.standard_normal((T, ld)).astype(np.float32))
    wq = rb((1 + 0.1 * rng.standard_normal(128)).astype(np.float32))
    wk = rb((1 + 0.1 * rng.standard_normal(128)).astype(np.float32))
    wq[5], wk[77] = 0.0, 0.0   # a zero weight element is legal
    return qkv, dqkv, wq, wk, ld


def _ref(qkv, dqkv, wq, wk, T, H, Hkv, bf16):
    """y, rstd [T, H + Hkv], dx over the q|k columns, dwq, dwk from the oracle on the reshaped rows"""
    nq, nk = H * 128, Hkv * 128
    yq, rq = O.rmsnorm_fwd(qkv[:, :nq].reshape(-1, 128), wq, EPS, bf16=bf16)
    yk, rk = O.rmsnorm_fwd(qkv[:, nq:nq + nk].reshape(-1, 128), wk, EPS, bf16=bf16)
    dxq, dwq = O.rmsnorm_bwd(dqkv[:, :nq].reshape(-1, 128), qkv[:, :nq].reshape(-1, 128), rq, wq, None, bf16=bf16)
    dxk, dwk = O.rmsnorm_bwd(dqkv[:, nq:nq + nk].reshape(-1, 128), qkv[:, nq:nq + nk].reshape(-1, 128), rk, wk, None, bf16=bf16)
    y = np.concatenate([yq.reshape(T, nq), yk.reshape(T, nk)], 1)
    dx = np.concatenate([dxq.reshape(T, nq), dxk.reshape(T, nk)], 1)
    rstd = np.concatenate([rq.reshape(T, H), rk.reshape(T, Hkv)], 1)
    return y, rstd, dx, dwq, dwk


class _Dev:
    """device copies of one problem in either precision"""

    def __init__(self, L, bf16, qkv, dqkv, wq, wk, T, H, Hkv):
        up = L.dev_bf16 if bf16 else L.dev_f32
        self.L, self.bf16, self.T, self.H, self.Hkv, self.ld = L, bf16, T, H, Hkv, qkv.shape[1]
        self.es = 2 if bf16 else 4
        self.qkv, self.dqkv, self.wq, self.wk = up(qkv), up(dqkv), up(wq), up(wk)
        self.rstd = L.DevBuf(nbytes=T * (H + Hkv) * 4)
        self.stash = L.DevBuf(nbytes=T * (H + Hkv) * 128 * self.es)
        self.ws = L.DevBuf(nbytes=L.HEAD_NORM_WS_FLOATS * 4)   # caller-owned scratch of the weight-gradient form
        lab = L.load_lab()
        self.fwd = lab.tst_k_head_norm_fwd if bf16 else lab.tst_k_head_norm_fwd_f32
        self.bwd = lab.tst_k_head_norm_bwd if bf16 else lab.tst_k_head_norm_bwd_f32
        self.rope = lab.tst_k_rope if bf16 else lab.tst_k_rope_f32

    def get(self, buf, shape):
        return buf.get_bf16(shape) if self.bf16 else buf.get(np.float32, shape)

    def run_fwd(self, stash=True, rope=None):
        p, c, s = rope if rope else (None, None, None)
        assert self.fwd(self.qkv.ptr, self.ld, self.wq.ptr, self.wk.ptr, self.rstd.ptr, self.stash.ptr if stash else None, self.T, self.H, self.Hkv, EPS,
                        p.ptr if p else None, c.ptr if c else None, s.ptr if s else None) == 0
        return self.get(self.qkv, (self.T, self.ld))

    def run_bwd(self, rope=None, dwq=None, dwk=None):
        p, c, s = rope if rope else (None, None, None)
        assert self.bwd(self.dqkv.ptr, self.ld, self.wq.ptr, self.wk.ptr, self.rstd.ptr, self.stash.ptr, self.T, self.H, self.Hkv,
                        p.ptr if p else None, c.ptr if c else None, s.ptr if s else None, dwq.ptr if dwq else None, dwk.ptr if dwk else None,
                        self.ws.ptr if dwq else None) == 0
        return self.get(self.dqkv, (self.T, self.ld))


@pytest.mark.parametrize("T,H,Hkv", SHAPES)
def test_head_norm_bf16_vs_oracle(L, T, H, Hkv):
    """forward y and rstd, the stash, backward dx against the oracle; v columns bit-untouched by both passes; a zero weight element gives finite dx;
    a forward without a stash pointer writes the same y and leaves the stash buffer alone"""
    qkv, dqkv, wq, wk, ld = _inputs(T, H, Hkv, True)
    nqk = (H + Hkv) * 128
    y_ref, rstd_ref, dx_ref, _, _ = _ref(qkv, dqkv, wq, wk, T, H, Hkv, True)
    d = _Dev(L, True, qkv, dqkv, wq, wk, T, H, Hkv)
    got = d.run_fwd(stash=True)
    assert_close(f"head_norm_fwd T{T} H{H} Hkv{Hkv}", got[:, :nqk], y_ref, BF_ULP, 1e-3)
    np.testing.assert_array_equal(got[:, nqk:], qkv[:, nqk:])
    assert_close(f"head_norm_rstd T{T} H{H} Hkv{Hkv}", d.rstd.get(np.float32, (T, H + Hkv)), rstd_ref, 1e-5, 0)
    np.testing.assert_array_equal(d.stash.get_bf16((T, nqk)), qkv[:, :nqk])          # the raw rows, as the projection wrote them
    dx = d.run_bwd()
    assert np.isfinite(dx).all()
    assert_close(f"head_norm_bwd T{T} H{H} Hkv{Hkv}", dx[:, :nqk], dx_ref, BF_ULP, 2e-3)
    np.testing.assert_array_equal(dx[:, nqk:], dqkv[:, nqk:])
    # scoring / stash = false forward: nothing extra is written
    d2 = _Dev(L, True, qkv, dqkv, wq, wk, T, H, Hkv)
    marker = np.full((T, nqk), 3.0, np.float32)
    d2.stash = L.dev_bf16(marker)
    np.testing.assert_array_equal(d2.run_fwd(stash=False), got)
    np.testing.assert_array_equal(d2.stash.get_bf16((T, nqk)), marker)


@pytest.mark.parametrize("T,H,Hkv", SHAPES)
def test_head_norm_f32_vs_oracle(L, T, H, Hkv):
    """the fp32 strict twins at the bounds of the fp32 norm kernels (tests/test_strict_gpu.py test_elementwise_f32_vs_hf_fixtures: 2e-6 / 5e-6 absolute)"""
    qkv, dqkv, wq, wk, ld = _inputs(T, H, Hkv, False)
    nqk = (H + Hkv) * 128
    y_ref, rstd_ref, dx_ref, _, _ = _ref(qkv, dqkv, wq, wk, T, H, Hkv, False)
    d = _Dev(L, False, qkv, dqkv, wq, wk, T, H, Hkv)
    got = d.run_fwd(stash=True)
    e_y = float(np.abs(got[:, :nqk] - y_ref).max())
    np.testing.assert_array_equal(got[:, nqk:], qkv[:, nqk:])
    assert_close(f"head_norm_rstd_f32 T{T} H{H} Hkv{Hkv}", d.rstd.get(np.float32, (T, H + Hkv)), rstd_ref, 1e-5, 0)
    dx = d.run_bwd()
    e_dx = float(np.abs(dx[:, :nqk] - dx_ref).max())
    print(f"head_norm f32 T{T} H{H} Hkv{Hkv}: max|dy|={e_y:.2e} max|d dx|={e_dx:.2e}")
    assert e_y <= 2e-6 and e_dx <= 5e-6, (e_y, e_dx)
    assert np.isfinite(dx).all()
    np.testing.assert_array_equal(dx[:, nqk:], dqkv[:, nqk:])


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("T,H,Hkv", SHAPES)
def test_head_norm_weight_gradients(L, T, H, Hkv, bf16):
    """dwq / dwk (full fine-tune) against fp64 numpy on the same inputs, added ON TOP of what the buffers held, at the bound of test_rmsnorm_bwd_dw
    (1e-4, 1e-4 against fp64; 1e-3, 1e-3 against the fp32 oracle); dx is the dx of the plain backward bit for bit; two calls give identical bits"""
    qkv, dqkv, wq, wk, ld = _inputs(T, H, Hkv, bf16, seed=3)
    nq, nk = H * 128, Hkv * 128
    _, rstd_ref, _, dwq_ref, dwk_ref = _ref(qkv, dqkv, wq, wk, T, H, Hkv, bf16)
    rng = np.random.default_rng(T)
    base_q, base_k = rng.standard_normal(128).astype(np.float32), rng.standard_normal(128).astype(np.float32)
    outs = []
    for _ in range(2):
        d = _Dev(L, bf16, qkv, dqkv, wq, wk, T, H, Hkv)
        d.run_fwd(stash=True)
        dwq_, dwk_ = L.DevBuf(base_q.copy()), L.DevBuf(base_k.copy())
        dx = d.run_bwd(dwq=dwq_, dwk=dwk_)
        outs.append((dx, dwq_.get(np.float32, (128,)), dwk_.get(np.float32, (128,)), d.rstd.get(np.float32, (T, H + Hkv))))
    d0 = _Dev(L, bf16, qkv, dqkv, wq, wk, T, H, Hkv)
    d0.run_fwd(stash=True)
    np.testing.assert_array_equal(outs[0][0], d0.run_bwd())
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)
    rstd = outs[0][3]
    rb = O.rbf if bf16 else (lambda a: a)
    xh_q = rb((qkv[:, :nq].reshape(T, H, 128) * rstd[:, :H, None]).astype(np.float32)).astype(np.float64)
    xh_k = rb((qkv[:, nq:nq + nk].reshape(T, Hkv, 128) * rstd[:, H:, None]).astype(np.float32)).astype(np.float64)
    dwq64 = (dqkv[:, :nq].reshape(T, H, 128).astype(np.float64) * xh_q).sum((0, 1))
    dwk64 = (dqkv[:, nq:nq + nk].reshape(T, Hkv, 128).astype(np.float64) * xh_k).sum((0, 1))
    tag = f"T{T} H{H} Hkv{Hkv} {'bf16' if bf16 else 'f32'}"
    assert_close("head_norm dwq " + tag, outs[0][1] - base_q, dwq64, 1e-4, 1e-4)
    assert_close("head_norm dwk " + tag, outs[0][2] - base_k, dwk64, 1e-4, 1e-4)
    assert_close("head_norm dwq vs oracle " + tag, outs[0][1] - base_q, dwq_ref, 1e-3, 1e-3)
    assert_close("head_norm dwk vs oracle " + tag, outs[0][2] - base_k, dwk_ref, 1e-3, 1e-3)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("tag", ["llama31", "theta1e6"])
@pytest.mark.parametrize("T,H,Hkv", [(300, 4, 2), (1185, 32, 8), (1, 7, 1)])
def test_head_norm_fused_rope_is_bit_equal_to_two_passes(L, T, H, Hkv, tag, bf16):
    """norm + rotation in one traversal == head norm, then tst_k_rope: forward (y, rstd) and backward (dx, dwq, dwk), bit for bit, at positions spread over
    0 .. 8191 on a Llama-3.1-scaled and a plain-theta table"""
    P = 8192
    theta, rs = {c[0]: c[1:] for c in GI.ROPE_SCALING_CASES}.get(tag, (1000000.0, None))
    cos, sin = O.rope_tables(np.arange(P), 128, theta, bf16=bf16, scaling=rs)
    rng = np.random.default_rng(T + P)
    pos = rng.integers(0, P, T).astype(np.int32)
    pos[:4] = (0, 1, P - 2, P - 1)[:min(4, T)]
    qkv, dqkv, wq, wk, ld = _inputs(T, H, Hkv, bf16, seed=7)
    p_, c_, s_ = L.DevBuf(pos), L.dev_f32(cos), L.dev_f32(sin)
    two, one = _Dev(L, bf16, qkv, dqkv, wq, wk, T, H, Hkv), _Dev(L, bf16, qkv, dqkv, wq, wk, T, H, Hkv)
    # two passes
    two.run_fwd(stash=True)
    assert two.rope(two.qkv.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, 128, ld, 0) == 0
    y2 = two.get(two.qkv, (T, ld))
    assert two.rope(two.dqkv.ptr, p_.ptr, c_.ptr, s_.ptr, T, H + Hkv, 128, ld, 1) == 0
    dq2, dk2 = L.DevBuf(np.zeros(128, np.float32)), L.DevBuf(np.zeros(128, np.float32))
    dx2 = two.run_bwd(dwq=dq2, dwk=dk2)
    # one pass
    y1 = one.run_fwd(stash=True, rope=(p_, c_, s_))
    dq1, dk1 = L.DevBuf(np.zeros(128, np.float32)), L.DevBuf(np.zeros(128, np.float32))
    dx1 = one.run_bwd(rope=(p_, c_, s_), dwq=dq1, dwk=dk1)
    np.testing.assert_array_equal(y1, y2)
    np.testing.assert_array_equal(one.rstd.get(np.float32, (T, H + Hkv)), two.rstd.get(np.float32, (T, H + Hkv)))
    np.testing.assert_array_equal(dx1, dx2)
    np.testing.assert_array_equal(dq1.get(np.float32, (128,)), dq2.get(np.float32, (128,)))
    np.testing.assert_array_equal(dk1.get(np.float32, (128,)), dk2.get(np.float32, (128,)))
    # and the rotation really happened: against the oracle's norm -> rope
    nq, nqk = H * 128, (H + Hkv) * 128
    y_ref = _ref(qkv, dqkv, wq, wk, T, H, Hkv, bf16)[0]
    rot = O.rope_apply(y_ref.reshape(T, H + Hkv, 128), cos[pos], sin[pos], bf16=bf16).reshape(T, nqk)
    if bf16:
        assert_close(f"head_norm+rope fwd {tag} T{T}", y1[:, :nqk], rot, 2 * BF_ULP, 2e-3)   # two roundings behind the statistic (test_rmsnorm_rank_fwd: up to two ulps)
    else:
        assert float(np.abs(y1[:, :nqk] - rot).max()) <= 4e-6
    np.testing.assert_array_equal(y1[:, nqk:], qkv[:, nqk:])


def test_head_norm_refuses_bad_arguments(L):
    lab = L.load_lab()
    buf = L.DevBuf(nbytes=4096)
    # ld narrower than (H + 2 Hkv) * 128, missing tables beside pos, dwq without dwk
    assert lab.tst_k_head_norm_fwd(buf.ptr, 128, buf.ptr, buf.ptr, buf.ptr, None, 1, 1, 1, EPS, None, None, None) != 0
    assert lab.tst_k_head_norm_fwd(buf.ptr, 384, buf.ptr, buf.ptr, buf.ptr, None, 1, 1, 1, EPS, buf.ptr, None, None) != 0
    assert lab.tst_k_head_norm_bwd(buf.ptr, 384, buf.ptr, buf.ptr, buf.ptr, buf.ptr, 1, 1, 1, None, None, None, buf.ptr, None, buf.ptr) != 0
    assert lab.tst_k_head_norm_bwd(buf.ptr, 384, buf.ptr, buf.ptr, buf.ptr, buf.ptr, 1, 1, 1, None, None, None, buf.ptr, buf.ptr, None) != 0   # no scratch
