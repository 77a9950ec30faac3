"""The whole hot path on batches whose longest sequence has more than 128 tokens. There the engine leaves the shared-staging attention kernels
(and RoPE inside them) for the general kernels with the stand-alone rope kernel before the attention forward and after its backward
(engine.hip forward / backward, `rope_in`); the fp32 strict mode keeps its single path. Checked against the oracle on the same weights and batch,
as tests/test_edge_cases_gpu.py does for short ragged batches, and at the switch itself:
  * trim_last_token on a batch whose longest sequence has 129 tokens: trimmed it runs 128 (short kernels, RoPE inside), whole 129 (general kernels,
    stand-alone RoPE) -- the two must agree (bf16: the bound of test_compaction_gpu.py's on/off agreements; strict: bit for bit);
  * last-layer compaction with a 300-token sequence in the batch (the same two bounds);
  * stacked folds whose slot 0 holds a 300-token sequence and slot 1 short ones, against one unstacked context per slot (test_stacked_gpu.py's bound);
  * strict mode against the fp32 oracle (test_strict_gpu.py's bounds)."""
import numpy as np
import pytest

import families as FAM
import golden_inputs as GI
from test_compaction_gpu import flat, run
from test_edge_cases_gpu import batch_of, rel_l2
from test_engine_gpu import report   # the engine report of tests/test_engine_gpu.py

pytestmark = pytest.mark.gpu

GPT2_LONG_CFG = dict(GI.GPT2_CFG, max_position=1024)   # wpe sized for GPT-2's own n_positions
FAMILIES = {"tiny": GI.TINY_CFG, "tiny2": GI.TINY2_CFG, "qwen": GI.QWEN_CFG, "gpt2": GPT2_LONG_CFG}
# lengths, labelled tail per sequence (-1: every position)
BATCHES = {
    "700": ((700,), (-1,)),
    "1_300_17_129_64": ((1, 300, 17, 129, 64), (0, 5, -1, 1, 2)),
    "191_192_193": ((191, 192, 193), (3, -1, 1)),
    "129_128_2": ((129, 128, 2), (1, -1, 1)),
}
OPT = [3, 9, 27, 81]


def make_ctx(cfg, precision="bf16", n_stack=1, weights=None, **kw):
    from tst import lib
    ctx = lib.Context(cfg, max_tokens=1024 * n_stack, max_seqs=8 * n_stack, max_labelled=1024 * n_stack, max_position=1024, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, n_stack=n_stack, precision=precision, **kw)
    ctx.load_state_dict(weights if weights is not None else GI.make_weights(cfg))
    return ctx


def long_rows(cu):
    """rows for forward_logits: the last token of every sequence and positions 127 .. 129 and the last 8 of every sequence longer than 128"""
    rows = set()
    for b in range(len(cu) - 1):
        s0, n = int(cu[b]), int(cu[b + 1] - cu[b])
        rows.add(s0 + n - 1)
        if n > 128:
            rows.update(s0 + p for p in (127, 128, 129) if p < n)
            rows.update(range(s0 + n - 8, s0 + n))
    return np.array(sorted(rows), np.int32)


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("case", sorted(BATCHES))
def test_long_batches_match_oracle(fam, case):
    """loss / adapter gradients at the ragged-batch bounds (loss 2e-3 |ref| + 1e-3, rel-L2 4e-2 per tensor); logits of rows past position 128 and s(x)
    ingredients at the bounds test_edge_cases_gpu.py uses for short ragged batches (logits rel-L2 2e-2, |d p| 2e-2, row map exact)"""
    cfg = FAMILIES[fam]
    lengths, labelled = BATCHES[case]
    ids, labels, cu = batch_of(cfg, lengths, labelled, seed=sum(lengths))
    w, lora = GI.make_weights(cfg), GI.make_lora(cfg)
    ctx = make_ctx(cfg, weights=w)
    ctx.set_trainable(lora)
    orc = FAM.oracle(cfg, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True)
    loss = ctx.forward_backward(ids, labels, cu)
    loss_ref, grads_ref = orc.loss_and_grads(ids, labels, cu)
    g = ctx.get_grads()
    worst = max(rel_l2(g[k], grads_ref[k]) for k in grads_ref)
    rows = long_rows(cu)
    got, ref = ctx.forward_logits(ids, cu, rows), orc.forward_logits(ids, cu, rows)
    logp, correct, optl, rseq = ctx.score_rows(ids, labels, cu, OPT)
    lr, cr, olr, rs = orc.score_rows(ids, labels, cu, OPT)
    d_p = float(np.abs(np.exp(logp) - np.exp(lr)).max())
    d_opt = float(np.abs(_softmax(optl) - _softmax(olr)).max())
    report(f"long[{fam}] L{case}: loss hip={loss:.6f} oracle-bf16={loss_ref:.6f} | worst grad rel-L2={worst:.3e} | logits rel-L2={rel_l2(got, ref):.3e} "
           f"| |d p|={d_p:.3e} |d softmax_opt|={d_opt:.3e}")
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref) + 1e-3, (loss, loss_ref)
    assert worst <= 4e-2, worst
    assert np.isfinite(got).all() and rel_l2(got, ref) <= 2e-2
    np.testing.assert_array_equal(rseq, rs)
    assert d_p <= 2e-2 and d_opt <= 2e-2
    ctx.close()


# ------------------------------------------------------------------------------------------------ at the switch
# Across the kernel families the backward of q and k is rounded differently: the short family rotates dq / dk back in fp32 inside the attention
# kernel and rounds once; the general family rounds dq / dk to bf16, and the rope kernel rotates and rounds again (test_kernels_gpu.py
# test_attention_with_rope_inside_the_kernels pins that at 3 bf16 ulps of the largest entry). The q / k adapter gradients inherit that one extra
# rounding, so an agreement that crosses the families is bounded by 3 bf16 ulps of the largest gradient instead of the 2e-3 of a re-tiled fp32 sum
# (measured 4e-3 - 1.1e-2); the forward is the same bits in both families (the loss agrees to 1e-5 all the same).
CROSS_FAMILY_GRAD = 3 * 2.0 ** -7


def _agree_bf16(a, b, what, grad_bound=2e-3):
    """test_compaction_gpu.py's bf16 on/off agreement: loss 1e-5 relative, gradients 2e-3 of the largest entry (grad_bound: CROSS_FAMILY_GRAD when the
    two runs take different attention kernel families)"""
    dl = abs(a["loss0"] - b["loss0"]) / abs(a["loss0"])
    dg = float(np.abs(a["g0"] - b["g0"]).max() / np.abs(a["g0"]).max())
    report(f"long {what} bf16 on/off: loss rel={dl:.3e} grad max|d|/max|g|={dg:.3e} rel-L2={rel_l2(a['g0'], b['g0']):.3e} (bound {grad_bound:.1e})")
    assert dl <= 1e-5 and dg <= grad_bound, (what, dl, dg)
    assert abs(a["loss"][0] - b["loss"][0]) <= 1e-5 * abs(a["loss"][0]) and abs(a["gn"][0] - b["gn"][0]) <= 2e-3 * a["gn"][0]


def _identical(a, b, what):
    assert a["loss0"] == b["loss0"] and (a["g0"] == b["g0"]).all(), f"{what}: first forward / backward"
    assert a["loss"] == b["loss"] and a["gn"] == b["gn"] and (a["w"] == b["w"]).all(), f"{what}: trajectory"


@pytest.mark.parametrize("fam", ["tiny", "tiny2"])
def test_trim_last_token_at_the_128_boundary_bf16(fam):
    """trim on: maxlen 128 (short kernels, RoPE inside attention); trim off: 129 (general kernels, stand-alone RoPE). Same loss, gradients within
    CROSS_FAMILY_GRAD, and both match the oracle"""
    cfg = FAMILIES[fam]
    batches = [GI.make_batch(cfg, (129, 40, 7), (1, 3, 2), seed=31), GI.make_batch(cfg, (100, 129), (2, 1), seed=32)]   # longest 129, its last token labelled
    w, lora = GI.make_weights(cfg), GI.make_lora(cfg)
    loss_ref, grads_ref = FAM.oracle(cfg, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True).loss_and_grads(*batches[0])
    res = []
    for on in (1, 0):
        ctx = make_ctx(cfg, weights=w, weight_decay=0.01)
        ctx.set_trainable(lora)
        r = run(ctx, batches, on, steps=1, option="trim_last_token")
        res.append(r)
        ctx.close()
    for r, on in zip(res, (1, 0)):
        assert abs(r["loss0"] - loss_ref) <= 2e-3 * abs(loss_ref) + 1e-3, (on, r["loss0"], loss_ref)
        gflat = flat(grads_ref)
        assert np.linalg.norm(r["g0"] - gflat) <= 4e-2 * np.linalg.norm(gflat), on
    _agree_bf16(res[0], res[1], f"trim[{fam}] at 129", grad_bound=CROSS_FAMILY_GRAD)


@pytest.mark.parametrize("fam", ["tiny", "gpt2"])
def test_last_layer_compaction_with_a_long_sequence_bf16(fam):
    cfg = FAMILIES[fam]
    batches = [GI.make_batch(cfg, (300, 45, 129), (3, 2, 1), seed=41), GI.make_batch(cfg, (64, 257), (1, 4), seed=42)]
    res = []
    for compact in (0, 1):
        ctx = make_ctx(cfg, weight_decay=0.01)
        ctx.set_trainable(GI.make_lora(cfg))
        res.append(run(ctx, batches, compact, steps=1))
        ctx.close()
    _agree_bf16(res[0], res[1], f"last_compact[{fam}] with 300 tokens")


def _strict_ctx(cfg):
    ctx = make_ctx(cfg, precision="strict", weights=GI.strict_weights(cfg), weight_decay=0.01, max_grad_norm=1.0)
    ctx.set_trainable(GI.make_lora(cfg))
    return ctx


@pytest.mark.parametrize("fam", ["tiny", "tiny2", "gpt2"])
@pytest.mark.parametrize("option", ["trim_last_token", "last_compact"])
def test_strict_mode_is_bit_identical_with_a_long_sequence(fam, option):
    """strict mode: one kernel family at every length, fixed summation order -- trimming the last token / compacting the last layer must not change a bit
    of loss, gradients or the AdamW trajectory on batches holding a 300-token sequence"""
    cfg = FAMILIES[fam]
    batches = [GI.make_batch(cfg, (300, 45, 129), (3, 2, 1), seed=51), GI.make_batch(cfg, (129, 64, 1), (1, 4, 0), seed=52)]
    res = []
    for on in (0, 1):
        ctx = _strict_ctx(cfg)
        res.append(run(ctx, batches, on, steps=2, option=option))
        ctx.close()
    _identical(res[0], res[1], f"strict {option}[{fam}]")


@pytest.mark.parametrize("fam", ["tiny", "qwen", "gpt2"])
def test_stacked_slot_with_a_long_sequence_matches_a_separate_context(fam):
    """n_stack = 2: slot 0 holds a 300-token sequence (the batch's maxlen: general kernels for both slots), slot 1 short ones only. Each slot's loss and
    gradients equal those of an unstacked context on the slot's own batch at test_stacked_gpu.py's bound (loss 2e-4 relative, gradients 2e-3 of the
    largest entry). The unstacked slot-1 context runs the short kernels (its batch has maxlen 70), so slot 1's gradients cross the kernel families:
    CROSS_FAMILY_GRAD there"""
    from test_stacked_gpu import stack_batches
    cfg = FAMILIES[fam]
    parts = [GI.make_batch(cfg, (300, 20), (3, 1), seed=61), GI.make_batch(cfg, (70, 33, 12), (2, 1, 4), seed=62)]
    loras = [GI.make_lora(cfg, seed=99 + s) for s in range(2)]
    one = make_ctx(cfg)
    ref = []
    for s in range(2):
        one.set_trainable(loras[s])
        ref.append((one.forward_backward(*parts[s]), one.get_grads()))
    one.close()
    st = make_ctx(cfg, n_stack=2)
    for s in range(2):
        st.select_slot(s)
        st.set_trainable(loras[s])
    ids, labels, cu, sl = stack_batches([(s, parts[s]) for s in range(2)])
    for s in range(2):
        st.select_slot(s)
        loss = st.forward_backward(ids, labels, cu, seq_slot=sl)
        g = st.get_grads()
        worst = max(float(np.abs(g[k] - ref[s][1][k]).max() / (np.abs(ref[s][1][k]).max() + 1e-30)) for k in g)
        report(f"long stacked[{fam}] slot {s}: loss {loss:.6f} vs {ref[s][0]:.6f}, worst grad max|d|/max|g|={worst:.3e}")
        assert abs(loss - ref[s][0]) < 2e-4 * abs(ref[s][0]), (s, loss, ref[s][0])
        assert worst < (2e-3 if s == 0 else CROSS_FAMILY_GRAD), (s, worst)
    st.close()


@pytest.mark.parametrize("fam", ["tiny", "tiny2", "qwen", "gpt2"])
def test_strict_long_batch_matches_the_fp32_oracle(fam):
    """strict mode on (300, 45, 129) against the fp32 oracle: logits within LOGIT_TOL (1e-4 absolute) on rows past position 128, loss and gradient
    norm of one step within test_strict_gpu.py's step-1 bounds (TRAJ_STEP1 relative + TRAJ_ABS; twice / eight times that on the norm). Per-tensor
    gradients: rel-L2 1e-4 -- there is no per-tensor counterpart in test_strict_gpu.py; two fp32 summation orders differ by ~1e-6 here."""
    from test_strict_gpu import LOGIT_TOL, TRAJ_ABS, TRAJ_STEP1
    cfg = FAMILIES[fam]
    ids, labels, cu = GI.make_batch(cfg, (300, 45, 129), (3, 2, 1), seed=71)
    w, lora = GI.strict_weights(cfg), GI.make_lora(cfg)
    ctx = make_ctx(cfg, precision="strict", weights=w)
    ctx.set_trainable(lora)
    orc = FAM.oracle(cfg, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=False)
    rows = long_rows(cu)
    lg, lg_ref = ctx.forward_logits(ids, cu, rows), orc.forward_logits(ids, cu, rows)
    loss = ctx.forward_backward(ids, labels, cu)
    g = ctx.get_grads()
    loss_ref, g_ref = orc.loss_and_grads(ids, labels, cu)
    d_lg = float(np.abs(lg - lg_ref).max())
    worst = max(rel_l2(g[k], g_ref[k]) for k in g_ref)
    gn, gn_ref = float(np.linalg.norm(flat(g))), float(np.linalg.norm(flat(g_ref)))
    report(f"long strict[{fam}] (300, 45, 129): logits max|d|={d_lg:.3e} loss rel={abs(loss - loss_ref) / abs(loss_ref):.3e} "
           f"gnorm rel={abs(gn - gn_ref) / gn_ref:.3e} worst grad rel-L2={worst:.3e}")
    assert d_lg <= LOGIT_TOL and (lg.argmax(-1) == lg_ref.argmax(-1)).all()
    assert abs(loss - loss_ref) <= TRAJ_STEP1 * abs(loss_ref) + TRAJ_ABS
    assert abs(gn - gn_ref) <= 2 * TRAJ_STEP1 * gn_ref + 8 * TRAJ_ABS
    assert worst <= 1e-4
    ctx.close()
