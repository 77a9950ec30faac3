"""GPU parity of the Qwen3 family (TST_ARCH_QWEN3: per-head q/k RMSNorm between the projection and RoPE, csrc/head_norm.hip) through the whole engine.

References: tests/qwen3_oracle.py (pinned to transformers.Qwen3ForCausalLM by tests/test_qwen3_cpu.py) in bf16-mirror mode, and the HF fp32 fixtures
tests/golden/*qwen3*.npz. Every bound is the one the existing engine tests state for the qwen family, named where it is used:
tests/test_engine_gpu.py (logits, loss, adapter gradients, s(x)), tests/test_strict_gpu.py (LOGIT_TOL, SX_TOL, traj_bound, SX_BF16_FACTOR),
tests/test_long_sequences_gpu.py, tests/test_stacked_gpu.py, tests/test_compaction_gpu.py, tests/test_full_finetune_gpu.py, tests/test_fullsize_gpu.py."""
import json
import os

import numpy as np
import pytest

import golden_inputs as GI
import qwen3_inputs as Q3
from oracle import ops_np as O
from qwen3_oracle import Qwen3Oracle

pytestmark = pytest.mark.gpu

CFG = Q3.QWEN3_CFG
OPT = [3, 9, 27, 81]
LOGIT_TOL, SX_TOL = 1e-4, 1e-3                                                        # tests/test_strict_gpu.py
TRAJ_STEP1, TRAJ_REL, TRAJ_GROWTH, TRAJ_CAP, TRAJ_ABS = 2e-6, 1e-4, 1.5, 5e-3, 2e-6   # tests/test_strict_gpu.py
SX_BF16_FACTOR = 1.25


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def flat(d):
    return np.concatenate([np.asarray(d[k], np.float32).ravel() for k in sorted(d)])


def make_ctx(weights=None, max_tokens=256, max_seqs=8, max_labelled=32, max_position=256, **kw):
    from tst import lib
    ctx = lib.Context(CFG, max_tokens=max_tokens, max_seqs=max_seqs, max_labelled=max_labelled, max_position=max_position, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, **kw)
    ctx.load_state_dict(weights if weights is not None else Q3.make_weights())
    return ctx


def batch():
    return GI.make_batch(CFG, Q3.LENGTHS, Q3.N_ANSWER)


# ------------------------------------------------------------------------------------------------ bf16 path against the oracle and the HF fixtures
def test_forward_logits(golden_dir):
    """tests/test_engine_gpu.py test_forward_logits: no farther from HF fp32 than HF's own bf16 run (1.1 x rel-L2, 1.25 x max), oracle-bf16 within 1.1 x that floor"""
    ids, labels, cu = batch()
    w, lora = Q3.make_weights(), GI.make_lora(CFG)
    ctx = make_ctx(w)
    rows = np.arange(len(ids))[-24:]
    ctx.reset_trainable(seed=1)
    base = ctx.forward_logits(ids, cu, rows)
    g = np.load(os.path.join(golden_dir, "llama_qwen3.npz"))
    e_hf, r_hf = float(np.abs(base - g["logits"][rows]).max()), rel_l2(base, g["logits"][rows])
    e_floor, r_floor = float(np.abs(g["logits_hf_bf16"][rows] - g["logits"][rows]).max()), rel_l2(g["logits_hf_bf16"][rows], g["logits"][rows])
    ref = Qwen3Oracle(CFG, w, None, bf16=True).forward_logits(ids, cu, rows)
    print(f"qwen3 base logits vs HF fp32: max|d|={e_hf:.3e} rel-L2={r_hf:.3e} | HF bf16's own: max|d|={e_floor:.3e} rel-L2={r_floor:.3e} | vs oracle-bf16 {rel_l2(base, ref):.3e}")
    assert r_hf <= 1.1 * r_floor and e_hf <= 1.25 * e_floor
    assert rel_l2(base, ref) <= 1.1 * r_floor
    ctx.set_trainable(lora)
    got = ctx.forward_logits(ids, cu, rows)
    ref32 = Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=False).forward_logits(ids, cu, rows)
    ref16 = Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True).forward_logits(ids, cu, rows)
    print(f"qwen3 lora logits vs oracle-fp32 {rel_l2(got, ref32):.3e} vs oracle-bf16 {rel_l2(got, ref16):.3e} (oracle-bf16 vs fp32 {rel_l2(ref16, ref32):.3e})")
    assert rel_l2(got, ref32) <= 1.25 * max(rel_l2(ref16, ref32), r_floor)
    ctx.close()


def test_loss_and_adapter_grads(golden_dir):
    """tests/test_engine_gpu.py test_loss_and_adapter_grads: loss 2e-3 |ref| + 1e-3 (oracle) / 2e-2 (HF); adapter gradients rel-L2 3e-2 (oracle) / 8e-2 (HF); bit-reproducible"""
    ids, labels, cu = batch()
    lora = GI.make_lora(CFG)
    ctx = make_ctx()
    ctx.set_trainable(lora)
    loss = ctx.forward_backward(ids, labels, cu)
    grads = ctx.get_grads()
    loss_ref, grads_ref = Qwen3Oracle(CFG, Q3.make_weights(), lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True).loss_and_grads(ids, labels, cu)
    g = np.load(os.path.join(golden_dir, "lora_qwen3.npz"))
    worst = max(rel_l2(grads[k], grads_ref[k]) for k in grads_ref)
    worst_hf = max(rel_l2(grads[k], g["g0/" + k]) for k in grads_ref)
    print(f"qwen3 loss hip={loss:.6f} oracle-bf16={loss_ref:.6f} hf-fp32={float(g['loss0']):.6f} | adapter grads worst rel-L2 vs oracle {worst:.3e} vs HF {worst_hf:.3e}")
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref) + 1e-3
    assert abs(loss - float(g["loss0"])) <= 2e-2 * abs(float(g["loss0"]))
    assert sorted(grads) == sorted(grads_ref)
    assert worst <= 3e-2 and worst_hf <= 8e-2
    loss2 = ctx.forward_backward(ids, labels, cu)
    grads2 = ctx.get_grads()
    assert loss2 == loss
    for k in grads:
        np.testing.assert_array_equal(grads[k], grads2[k])
    ctx.close()


def test_score_rows(golden_dir):
    """tests/test_engine_gpu.py test_score_rows: s(x) ingredients vs the fp32 oracle within max(1e-3, 1.25 x HF-bf16's own floor on the same rows)"""
    ids, labels, cu = batch()
    w, lora = Q3.make_weights(), GI.make_lora(CFG)
    ctx = make_ctx(w)
    ctx.set_trainable(lora)
    logp, correct, optl, rseq = ctx.score_rows(ids, labels, cu, OPT)
    logp_r, correct_r, optl_r, rseq_r = Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=False).score_rows(ids, labels, cu, OPT)
    np.testing.assert_array_equal(rseq, rseq_r)
    g = np.load(os.path.join(golden_dir, "llama_qwen3.npz"))
    rows, _, _ = O.shift_labels(labels, cu)
    floor = float(np.abs(_softmax(g["logits_hf_bf16"][rows][:, OPT]) - _softmax(g["logits"][rows][:, OPT])).max())
    d_opt = float(np.abs(_softmax(optl) - _softmax(optl_r)).max())
    d_lp = float(np.abs(np.exp(logp) - np.exp(logp_r)).max())
    print(f"qwen3 score |d softmax_opt|={d_opt:.3e} |d exp(logp)|={d_lp:.3e} floor={floor:.3e}")
    tol = max(1e-3, 1.25 * floor)
    assert d_opt <= tol and d_lp <= tol
    assert (correct == correct_r).mean() >= 0.8
    ctx.close()


def test_bf16_path_scores_inside_the_references_own_bf16_floor(golden_dir):
    """the project's rule (tests/test_strict_gpu.py): the bf16 path's held-out s(x) deviates from HF fp32 by at most 1.25 x what HF's own bf16 run does, worst
    sample and mean, for the base model and for the fold HF's 20 fp32 LoRA steps ended with"""
    g = np.load(os.path.join(golden_dir, "strict_qwen3.npz"))
    hid, hlab, hcu = GI.strict_heldout(CFG)
    ctx = make_ctx(Q3.strict_weights(), max_tokens=1024, max_seqs=32, max_labelled=64)
    for prefix in ("base", "lora"):
        if prefix == "base":
            ctx.reset_trainable(seed=1)
        else:
            ctx.set_trainable({k[len("lora_trained/"):]: g[k] for k in g.files if k.startswith("lora_trained/")})
        optl = ctx.score_rows(hid, hlab, hcu, list(GI.STRICT_OPT_IDS))[2]
        ref = _softmax(g[prefix + "_optl"])
        d = np.abs(_softmax(optl) - ref)
        floor = np.abs(_softmax(g[prefix + "_optl_hf_bf16"]) - ref)
        lg = ctx.forward_logits(hid, hcu, g["heldout_rows"])
        print(f"qwen3 bf16 path {prefix}: |d s(x)| max={d.max():.2e} mean={d.mean():.2e} | HF bf16's own max={floor.max():.2e} mean={floor.mean():.2e} | "
              f"logits max|d| vs HF fp32 {float(np.abs(lg - g[prefix + '_logits']).max()):.2e}")
        assert d.max() <= SX_BF16_FACTOR * floor.max(), (prefix, float(d.max()), float(floor.max()))
        assert d.mean() <= SX_BF16_FACTOR * floor.mean(), (prefix, float(d.mean()), float(floor.mean()))
    ctx.close()


# ------------------------------------------------------------------------------------------------ strict mode against the HF fp32 fixture
def strict_ctx(mode="lora", **kw):
    return make_ctx(Q3.strict_weights(), max_tokens=1024, max_seqs=32, max_labelled=64, train_mode=mode, precision="strict", **kw)


def check_heldout(ctx, g, prefix):
    hid, hlab, hcu = GI.strict_heldout(CFG)
    opt = list(GI.STRICT_OPT_IDS)
    logp, correct, optl, rseq = ctx.score_rows(hid, hlab, hcu, opt)
    assert len(logp) == 32 and (rseq == np.arange(32)).all()
    d_sx = float(np.abs(_softmax(optl) - _softmax(g[prefix + "_optl"])).max())
    d_p = float(np.abs(np.exp(logp) - np.exp(g[prefix + "_logp"])).max())
    lg = ctx.forward_logits(hid, hcu, g["heldout_rows"])
    d_lg = float(np.abs(lg - g[prefix + "_logits"]).max())
    agree = float((lg.argmax(-1) == g[prefix + "_logits"].argmax(-1)).mean())
    same = bool((correct == g[prefix + "_correct"]).all())
    sid, slab, scu = GI.strict_seen(CFG)
    slogp, scorrect, _, _ = ctx.score_rows(sid, slab, scu, opt)
    d_ps = float(np.abs(np.exp(slogp) - np.exp(g[prefix + "_seen_logp"])).max())
    same_seen = bool((scorrect == g[prefix + "_seen_correct"]).all())
    print(f"qwen3 strict {prefix}: |d s(x)|={d_sx:.2e} |d p|={max(d_p, d_ps):.2e} |d logits|={d_lg:.2e} argmax agreement={agree:.3f} correct identical={same and same_seen}")
    return d_sx, max(d_p, d_ps), d_lg, agree, same and same_seen


def test_strict_logits_and_scores_identical_weights(golden_dir):
    g = np.load(os.path.join(golden_dir, "strict_qwen3.npz"))
    ctx = strict_ctx()
    ctx.reset_trainable(seed=1)
    ids, labels, cu = GI.strict_train_batches(CFG)[0]
    lg = ctx.forward_logits(ids, cu, g["logits0_rows"])
    d0 = float(np.abs(lg - g["logits0"]).max())
    print(f"qwen3 strict base logits vs HF fp32: max|d|={d0:.2e}")
    assert d0 <= LOGIT_TOL
    assert (lg.argmax(-1) == g["logits0"].argmax(-1)).all()
    d_sx, d_p, d_lg, agree, same = check_heldout(ctx, g, "base")
    assert d_sx <= SX_TOL and d_p <= SX_TOL and d_lg <= LOGIT_TOL and agree == 1.0 and same
    ctx.close()


def traj_bound(ref, t):
    rel = TRAJ_STEP1 if t == 0 else min(TRAJ_CAP, TRAJ_REL * TRAJ_GROWTH ** t)
    return rel * abs(ref) + TRAJ_ABS


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_strict_twenty_step_trajectory_then_heldout_scores(golden_dir, mode):
    """20 fp32 optimizer steps inside the growing bound stated at the top of tests/test_strict_gpu.py, then held-out s(x) within 1e-3, `correct` identical"""
    g = np.load(os.path.join(golden_dir, "strict_qwen3.npz"))
    ctx = strict_ctx(mode, weight_decay=0.01, max_grad_norm=1.0)
    if mode == "lora":
        ctx.set_trainable(GI.make_lora(CFG))
    batches = GI.strict_train_batches(CFG)
    losses, gnorms = [], []
    for step in range(GI.STRICT_STEPS):
        ids, labels, cu = batches[step % 2]
        l, gn = ctx.train_step(ids, labels, cu, O.linear_lr(step, GI.STRICT_STEPS, GI.STRICT_LR[mode]))
        losses.append(l)
        gnorms.append(gn)
    losses, gnorms = np.array(losses, np.float64), np.array(gnorms, np.float64)
    rl, rg = g[mode + "_losses"], g[mode + "_gnorms"]
    print(f"qwen3 strict {mode} trajectory: loss rel dev " + " ".join(f"{x:.1e}" for x in np.abs(losses - rl) / (np.abs(rl) + 1e-30)))
    print(f"qwen3 strict {mode} trajectory: gnorm rel dev " + " ".join(f"{x:.1e}" for x in np.abs(gnorms - rg) / (np.abs(rg) + 1e-30)))
    for t in range(GI.STRICT_STEPS):
        assert abs(losses[t] - rl[t]) <= traj_bound(rl[t], t), ("loss", t, losses[t], rl[t])
        assert abs(gnorms[t] - rg[t]) <= 2 * traj_bound(rg[t], t) + 8 * TRAJ_ABS, ("gnorm", t, gnorms[t], rg[t])
    d_sx, d_p, d_lg, agree, same = check_heldout(ctx, g, mode)
    assert d_sx <= SX_TOL and d_p <= SX_TOL and agree == 1.0 and same
    ctx.close()


# ------------------------------------------------------------------------------------------------ sequences over 128 tokens: head norm and RoPE in one pass
@pytest.mark.parametrize("lengths,labelled", [((130, 40, 7), (2, 3, 1)), ((300, 17, 129), (5, -1, 1))], ids=["130", "300"])
def test_long_sequences_match_oracle(lengths, labelled):
    """tests/test_long_sequences_gpu.py test_long_batches_match_oracle: loss 2e-3 |ref| + 1e-3, gradients rel-L2 4e-2, logits rel-L2 2e-2, |d p| 2e-2"""
    from test_edge_cases_gpu import batch_of
    ids, labels, cu = batch_of(CFG, lengths, labelled, seed=sum(lengths))
    w, lora = Q3.make_weights(), GI.make_lora(CFG)
    ctx = make_ctx(w, max_tokens=1024, max_labelled=1024, max_position=1024)
    ctx.set_option("trim_last_token", 0)    # the whole sequences run: 130 / 300 tokens, the stand-alone-RoPE route
    ctx.set_trainable(lora)
    orc = Qwen3Oracle(CFG, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True)
    loss = ctx.forward_backward(ids, labels, cu)
    loss_ref, grads_ref = orc.loss_and_grads(ids, labels, cu)
    g = ctx.get_grads()
    worst = max(rel_l2(g[k], grads_ref[k]) for k in grads_ref)
    rows = np.array(sorted({int(cu[b + 1]) - 1 for b in range(len(cu) - 1)} | set(range(int(cu[1]) - 8, int(cu[1]))) | {127, 128, 129}), np.int32)
    got, ref = ctx.forward_logits(ids, cu, rows), orc.forward_logits(ids, cu, rows)
    logp, correct, optl, rseq = ctx.score_rows(ids, labels, cu, OPT)
    lr, cr, olr, rs = orc.score_rows(ids, labels, cu, OPT)
    d_p = float(np.abs(np.exp(logp) - np.exp(lr)).max())
    d_opt = float(np.abs(_softmax(optl) - _softmax(olr)).max())
    print(f"qwen3 long {lengths}: loss hip={loss:.6f} oracle={loss_ref:.6f} worst grad rel-L2={worst:.3e} logits rel-L2={rel_l2(got, ref):.3e} |d p|={d_p:.3e} |d opt|={d_opt:.3e}")
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref) + 1e-3
    assert worst <= 4e-2
    assert np.isfinite(got).all() and rel_l2(got, ref) <= 2e-2
    np.testing.assert_array_equal(rseq, rs)
    assert d_p <= 2e-2 and d_opt <= 2e-2
    ctx.close()


# ------------------------------------------------------------------------------------------------ stacked folds, forks, switches
def test_stacked_slots_match_separate_contexts():
    """tests/test_stacked_gpu.py: three slots equal three single contexts (first-step loss 2e-4, gradients 2e-3 of the largest entry; metrics of later
    steps 1e-2 / 3e-2; scores 0.05)"""
    from test_stacked_gpu import BATCHES, stack_batches, rel
    S = 3
    batches = [GI.make_batch(CFG, L, A, seed=sd) for L, A, sd in BATCHES]
    loras = [GI.make_lora(CFG, seed=99 + s) for s in range(S)]
    lrs = [1e-3, 5e-4, 2e-3]
    plan = [[0, 1, 2], [1, 2, 0], [2, None, 1]]
    one = make_ctx(weight_decay=0.01)
    ref = []
    for s in range(S):
        one.set_trainable(loras[s])
        one.reset_optimizer()
        g0, mets = None, []
        for step in plan:
            if step[s] is None:
                mets.append(None)
                continue
            ids, labels, cu = batches[step[s]]
            if g0 is None:
                one.forward_backward(ids, labels, cu)
                g0 = one.get_grads()
            mets.append(one.train_step(ids, labels, cu, lrs[s]))
        ref.append(dict(mets=mets, g0=g0, score=one.score_rows(*batches[s], OPT)))
    one.close()
    st = make_ctx(max_tokens=256 * S, max_seqs=8 * S, max_labelled=32 * S, n_stack=S, weight_decay=0.01)
    for s in range(S):
        st.select_slot(s)
        st.set_trainable(loras[s])
        st.reset_optimizer()
    ids, labels, cu, sl = stack_batches([(s, batches[plan[0][s]]) for s in range(S)])
    for s in range(S):
        st.select_slot(s)
        loss = st.forward_backward(ids, labels, cu, seq_slot=sl)
        g = st.get_grads()
        assert abs(loss - ref[s]["mets"][0][0]) < 2e-4 * abs(ref[s]["mets"][0][0]), (s, loss, ref[s]["mets"][0])
        worst = max(rel(g[k], ref[s]["g0"][k]) for k in g)
        assert worst < 2e-3, (s, worst)
    got = [[] for _ in range(S)]
    for step in plan:
        parts = [(s, batches[step[s]]) for s in range(S) if step[s] is not None]
        ids, labels, cu, sl = stack_batches(parts)
        st.train_step_stacked_async(ids, labels, cu, sl, lrs)
        loss, gn = st.fetch_metrics_stacked()
        for s in range(S):
            got[s].append((float(loss[s]), float(gn[s])) if step[s] is not None else None)
    for s in range(S):
        for n, (a, b) in enumerate(zip(got[s], ref[s]["mets"])):
            assert (a is None) == (b is None)
            if a is not None:
                tl, tg = (2e-4, 2e-3) if n == 0 else (1e-2, 3e-2)
                assert abs(a[0] - b[0]) < tl * abs(b[0]) and abs(a[1] - b[1]) < tg * abs(b[1]), (s, n, a, b)
    ids, labels, cu, sl = stack_batches([(s, batches[s]) for s in range(S)])
    logp, corr, optl, rseq = st.score_rows(ids, labels, cu, OPT, seq_slot=sl)
    o = 0
    for s in range(S):
        rl, rc, ro, rs = ref[s]["score"]
        n = len(rl)
        assert np.abs(logp[o:o + n] - rl).max() < 0.05 and np.abs(optl[o:o + n] - ro).max() < 0.05
        o += n
    st.close()


def test_fork_shares_the_base():
    """a fork borrows the parent's weights, head-norm vectors included: same loss and gradients bit for bit, no second copy of the base in HBM"""
    ids, labels, cu = batch()
    lora = GI.make_lora(CFG)
    ctx = make_ctx()
    ctx.set_trainable(lora)
    l0, g0 = ctx.forward_backward(ids, labels, cu), ctx.get_grads()
    kid = ctx.fork()
    kid.set_trainable(lora)
    assert kid.forward_backward(ids, labels, cu) == l0
    g1 = kid.get_grads()
    for k in g0:
        np.testing.assert_array_equal(g0[k], g1[k])
    np.testing.assert_array_equal(kid.get_weight("model.layers.1.self_attn.k_norm.weight", (128,)), Q3.make_weights()["model.layers.1.self_attn.k_norm.weight"])
    base_bytes = sum(v.size for v in Q3.make_weights().values()) * 2
    assert ctx.device_bytes() - kid.device_bytes() >= base_bytes      # the child holds no copy of the base
    from tst import lib
    with pytest.raises(lib.TstError, match="borrows"):
        kid.set_weight("model.layers.0.self_attn.q_norm.weight", np.ones(128, np.float32))
    kid.close()
    ctx.close()


@pytest.mark.parametrize("option", ["last_compact", "trim_last_token"])
def test_switches_agree_on_and_off(option):
    """tests/test_compaction_gpu.py: strict mode bit-identical with the switch on and off; bf16 path loss 1e-5 relative, gradients 2e-3 of the largest entry"""
    from test_compaction_gpu import run
    batches = GI.strict_train_batches(CFG)
    res = []
    for on in (0, 1):
        ctx = strict_ctx("lora", weight_decay=0.01, max_grad_norm=1.0)
        ctx.set_trainable(GI.make_lora(CFG))
        res.append(run(ctx, batches, on, option=option))
        ctx.close()
    a, b = res
    assert a["loss0"] == b["loss0"] and (a["g0"] == b["g0"]).all()
    assert a["loss"] == b["loss"] and a["gn"] == b["gn"] and (a["w"] == b["w"]).all()
    bb = [GI.make_batch(CFG, (33, 70, 12, 64), (2, 1, 1, 4), seed=11), GI.make_batch(CFG, (50, 9, 61), (1, 3, 2), seed=12)]
    res = []
    for on in (0, 1):
        ctx = make_ctx(weight_decay=0.01)
        ctx.set_trainable(GI.make_lora(CFG))
        res.append(run(ctx, bb, on, steps=1, option=option))
        ctx.close()
    a, b = res
    print(f"qwen3 {option} on/off bf16: loss rel {abs(a['loss0'] - b['loss0']) / abs(a['loss0']):.2e} grad {np.abs(a['g0'] - b['g0']).max() / np.abs(a['g0']).max():.2e}")
    assert abs(a["loss0"] - b["loss0"]) <= 1e-5 * abs(a["loss0"])
    assert np.abs(a["g0"] - b["g0"]).max() <= 2e-3 * np.abs(a["g0"]).max()
    assert abs(a["loss"][0] - b["loss"][0]) <= 1e-5 * abs(a["loss"][0]) and abs(a["gn"][0] - b["gn"][0]) <= 2e-3 * a["gn"][0]


# ------------------------------------------------------------------------------------------------ full fine-tune
def test_full_finetune_gradients_and_trainable_info(golden_dir):
    """tests/test_full_finetune_gpu.py test_full_gradients: the trainables are HF's state_dict names (q_norm / k_norm among them, in the no-decay tail);
    every gradient rel-L2 4e-2 vs the oracle's bf16 mirror, 0.12 vs the HF digests"""
    ids, labels, cu = batch()
    w = Q3.make_weights()
    ctx = make_ctx(w, train_mode="full")
    layout = ctx.trainable_layout()
    assert set(layout) == set(w)
    from tst import lib
    lay = lib.host_full_layout(lib.make_model_cfg(CFG, train_mode="full"))
    for n in Q3.head_norm_names(CFG):
        off, r, c = layout[n]
        assert (r, c) == (1, 128) and off >= lay["n_decay"]
    assert ctx.trainable_numel() == lay["n_train"]
    t = ctx.get_trainable()
    for k in w:
        np.testing.assert_array_equal(t[k].reshape(w[k].shape), w[k])
    loss = ctx.forward_backward(ids, labels, cu)
    grads = ctx.get_grads()
    loss_ref, grads_ref = Qwen3Oracle(CFG, w, None, bf16=True).loss_and_grads(ids, labels, cu, full=True)
    g = np.load(os.path.join(golden_dir, "llama_qwen3.npz"))
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref) + 1e-3
    worst = worst_hf = 0.0
    for k in sorted(w):
        got = grads[k].reshape(w[k].shape)
        e = rel_l2(got, grads_ref[k])
        n_, head, strided = GI.sample_vec(got)
        e_hf = max(abs(n_ - g["gn/" + k]) / (g["gn/" + k] + 1e-30), rel_l2(strided, g["gs/" + k]))
        worst, worst_hf = max(worst, e), max(worst_hf, e_hf)
        assert e <= 4e-2, (k, e)
        assert e_hf <= 0.12, (k, e_hf)
    print(f"qwen3 full_ft loss hip={loss:.6f} oracle={loss_ref:.6f} grads worst rel-L2 vs oracle {worst:.3e} vs HF digests {worst_hf:.3e}")
    l2, g2 = ctx.forward_backward(ids, labels, cu), ctx.get_grads()      # no atomics: the head-norm weight gradients included
    assert l2 == loss
    for k in grads:
        np.testing.assert_array_equal(grads[k], g2[k])
    ctx.close()


def test_full_finetune_head_norms_take_the_no_decay_update():
    """weight decay 0.1: one step against O.adamw_step on the oracle's clipped gradients, wd = 0 for the head-norm vectors (HF's Trainer excludes "_norm"
    names) and 0.1 for the matrices -- the bounds of test_full_step_trajectory_and_reset; with the wrong group the zero element could not stay put"""
    ids, labels, cu = batch()
    w = Q3.make_weights()
    lr, wd = 1e-3, 0.1
    ctx = make_ctx(w, train_mode="full", weight_decay=wd, max_grad_norm=1.0)
    loss_ref, grads_ref = Qwen3Oracle(CFG, w, None, bf16=True).loss_and_grads(ids, labels, cu, full=True)
    norm_ref, coef = O.clip_coef(np.concatenate([grads_ref[k].ravel() for k in sorted(w)]), 1.0)
    l0, gn = ctx.train_step(ids, labels, cu, lr)
    assert abs(gn - norm_ref) <= 3e-2 * norm_ref
    after = ctx.get_trainable()
    for k in sorted(w):
        p_ref, _, _ = O.adamw_step(w[k], grads_ref[k] * coef, np.zeros_like(w[k]), np.zeros_like(w[k]), 1, lr, wd=0.0 if w[k].ndim == 1 else wd)
        got = after[k].reshape(w[k].shape)
        d = np.abs(got - p_ref)
        assert (d > 2e-4).mean() <= 0.08 and d.max() <= 2.2e-3, (k, float((d > 2e-4).mean()), float(d.max()))
        np.testing.assert_array_equal(ctx.get_weight(k, w[k].shape), O.rbf(got))
    for n in Q3.head_norm_names(CFG):
        # decoupled decay would shrink every element by lr * wd * |w| = 1e-4 |w| on top of Adam's +-lr: the no-decay update keeps |step| <= lr (1 + 1e-3)
        step = np.abs(after[n].reshape(-1) - w[n])
        assert step.max() <= lr * 1.001 and step.max() > 0.5 * lr, (n, float(step.max()))
        with_decay, _, _ = O.adamw_step(w[n], grads_ref[n] * coef, np.zeros_like(w[n]), np.zeros_like(w[n]), 1, lr, wd=wd)
        no_decay, _, _ = O.adamw_step(w[n], grads_ref[n] * coef, np.zeros_like(w[n]), np.zeros_like(w[n]), 1, lr, wd=0.0)
        got = after[n].reshape(-1)
        # (medians: the few elements whose noise-level gradient flips Adam's sign-like first step sit 2 lr away from either reference)
        assert np.median(np.abs(got - no_decay)) < 0.1 * np.median(np.abs(got - with_decay)), n
    ctx.close()


@pytest.mark.parametrize("precision", ["bf16", "strict"])
def test_overlapped_optimizer_is_bit_identical_to_the_serial_step(precision):
    """tests/test_full_finetune_gpu.py: "opt_overlap" / "dw_side" on and off give the same bits (losses, gradient norms, scores, masters, moments, compute copy):
    the per-layer waits of the next forward cover the two head-norm vectors (they are updated with the no-decay tail, the first stage)"""
    ids, labels, cu = batch()
    ids2, labels2, cu2 = GI.make_batch(CFG, (100, 120, 90, 33), (2, 1, 3, 1))
    w = Q3.make_weights()
    runs = []
    for overlap in (1, 0):
        ctx = make_ctx(w, max_tokens=512, train_mode="full", weight_decay=0.05, max_grad_norm=1.0, precision=precision)
        assert ctx.set_option("opt_overlap", overlap) == overlap
        assert ctx.set_option("dw_side", overlap) == overlap
        rec = []
        for i in range(3):
            ctx.train_step_async(ids if i != 1 else ids2, labels if i != 1 else labels2, cu if i != 1 else cu2, 1e-3)
            if i == 1:
                rec.append(np.concatenate([np.asarray(x, np.float64).ravel() for x in ctx.score_rows(ids, labels, cu, OPT)[:3]]))
            rec.append(np.asarray(ctx.fetch_metrics(), np.float64))
        st = ctx.state()
        rec += [st["trainable"], st["m"], st["v"]] + [ctx.get_weight(k, w[k].shape) for k in sorted(w)]
        runs.append(rec)
        ctx.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ front end, full width, refusals
def test_safetensors_checkpoint_loads_through_from_pretrained(tmp_path):
    """a checkpoint written here with model_type "qwen3" (bf16 payload) loads through tst.io.from_pretrained; q_norm / k_norm come back bit-exact and the
    logits equal those of a context loaded tensor by tensor"""
    from safetensors.numpy import save_file
    from tst import io as TIO
    from tst import lib
    w = Q3.make_weights()
    d = tmp_path / "qwen3"
    d.mkdir()
    hf = dict(model_type="qwen3", vocab_size=CFG["vocab_size"], hidden_size=CFG["hidden_size"], num_hidden_layers=CFG["num_layers"],
              num_attention_heads=CFG["num_heads"], num_key_value_heads=CFG["num_kv_heads"], head_dim=CFG["head_dim"], intermediate_size=CFG["intermediate_size"],
              rope_parameters=dict(rope_theta=CFG["rope_theta"], rope_type="default"), rms_norm_eps=CFG["rms_norm_eps"], tie_word_embeddings=False,
              attention_bias=False, use_sliding_window=False, layer_types=["full_attention"] * CFG["num_layers"])
    (d / "config.json").write_text(json.dumps(hf))
    save_file({k: lib.to_bf16_bits(v).reshape(v.shape) for k, v in w.items()}, str(d / "model.safetensors"))
    hdr, base = TIO.read_safetensors_header(str(d / "model.safetensors"))
    raw = open(d / "model.safetensors", "rb").read()[base:]
    for m in hdr.values():
        m["dtype"] = "BF16"
    h = json.dumps(hdr).encode()
    open(d / "model.safetensors", "wb").write(len(h).to_bytes(8, "little") + h + raw)
    kw = dict(max_tokens=256, max_seqs=8, max_labelled=32, max_position=256)
    a = TIO.from_pretrained(str(d), **kw)
    assert a.cfg.get("qk_norm") is True and a.cfg["head_dim"] == 128
    b = lib.Context(CFG, **kw)
    b.load_state_dict(w)
    ids, labels, cu = batch()
    rows = np.arange(len(ids))[-16:]
    for c in (a, b):
        c.reset_trainable(seed=3)
    np.testing.assert_array_equal(a.forward_logits(ids, cu, rows), b.forward_logits(ids, cu, rows))
    for k, v in w.items():
        np.testing.assert_array_equal(a.get_weight(k, v.shape), v)
    a.close()
    b.close()


def test_two_layers_at_qwen3_8b_width_match_the_oracle():
    """tests/test_fullsize_gpu.py "direct": two decoder layers at the Qwen3-8B widths (4096 / 12288) under the full 151936-wide head, T ~ 1185 packed tokens (the
    benchmark's micro-batch of 16 QA pairs), against the oracle's bf16 mirror and its fp32 mode (floor = their distance). The oracle evaluates the head on the
    selected / labelled rows only, so the CPU side stays at the two layers' cost plus the weight draw."""
    from tst import cli, data as D, lib
    cfg = dict(cli.MODEL_SHAPES["qwen3-8b"], num_layers=2)
    assert (cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]) == (4096, 12288, 151936)
    samples = D.synth_vsi(16, cfg["vocab_size"], seed=3)
    ids, labels, cu = D.collate(samples)
    rng = np.random.default_rng(4321)
    w = {}
    names = GI.weight_names_shapes(cfg) + [(n, (128,)) for n in Q3.head_norm_names(cfg)]
    for wname, shape in names:
        a = rng.standard_normal(shape, dtype=np.float32)
        w[wname] = GI.bf16_round((1.0 + 0.1 * a if len(shape) == 1 else 0.02 * a).astype(np.float32))
    lora = GI.make_lora(cfg, seed=17)
    ctx = lib.Context(cfg, max_tokens=2048, max_seqs=16, max_labelled=64, max_position=128, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA)
    try:
        ctx.load_state_dict(w)
        ctx.set_trainable(lora)
        rows = np.flatnonzero(labels >= 0)[:12] - 1
        got = ctx.forward_logits(ids, cu, rows)
        loss = ctx.forward_backward(ids, labels, cu)
        grads = ctx.get_grads()
    finally:
        ctx.close()
    o16 = Qwen3Oracle(cfg, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=True)
    ref16 = o16.forward_logits(ids, cu, rows)
    loss16, g16 = o16.loss_and_grads(ids, labels, cu)
    del o16                                                   # (its bf16-rounded copy of the two 2.5 GB vocabulary matrices)
    o32 = Qwen3Oracle(cfg, w, lora, GI.LORA_R, GI.LORA_ALPHA, bf16=False)
    ref32 = o32.forward_logits(ids, cu, rows)
    loss32, g32 = o32.loss_and_grads(ids, labels, cu)
    floor = rel_l2(ref16, ref32)
    e16, e32 = rel_l2(got, ref16), rel_l2(got, ref32)
    worst16 = max(rel_l2(grads[k], g16[k]) for k in g16)
    worst32 = max(rel_l2(grads[k], g32[k]) for k in g32)
    gfloor = max(rel_l2(g16[k], g32[k]) for k in g32)
    line = (f"qwen3-8b width T={len(ids)}: logits rel-L2 vs oracle-bf16 {e16:.3e} vs fp32 {e32:.3e} (floor {floor:.3e}) | loss hip {loss:.5f} oracle-bf16 {loss16:.5f} "
            f"fp32 {loss32:.5f} | adapter grads worst rel-L2 vs bf16 {worst16:.3e} vs fp32 {worst32:.3e} (floor {gfloor:.3e})")
    print(line)
    assert e16 <= 1.25 * floor and e32 <= 1.5 * floor, line
    assert abs(loss - loss16) <= 2e-3 * abs(loss16) + 1e-3 and abs(loss - loss32) <= 1e-2 * abs(loss32), line
    assert worst16 <= 1.5 * gfloor and worst32 <= 2.0 * gfloor, line


def test_refusals():
    from tst import lib
    with pytest.raises(lib.TstError, match=r"\(-1\).*head_dim"):                      # TST_EINVAL
        lib.Context(dict(CFG, head_dim=64, num_heads=8, num_kv_heads=4), max_tokens=64, max_seqs=2, max_labelled=8, max_position=64)
    ctx = lib.Context(CFG, max_tokens=64, max_seqs=2, max_labelled=8, max_position=64)
    for k, v in Q3.make_weights().items():
        if not k.endswith("layers.1.self_attn.k_norm.weight"):
            ctx.set_weight(k, v)
    with pytest.raises(lib.TstError, match="k_norm"):
        ctx.finalize()
    ctx.set_weight("model.layers.1.self_attn.k_norm.weight", np.ones(128, np.float32))
    ctx.finalize()
    ctx.close()
    rnd = lib.Context(CFG, max_tokens=64, max_seqs=2, max_labelled=8, max_position=64)
    rnd.init_random(seed=1)
    np.testing.assert_array_equal(rnd.get_weight("model.layers.0.self_attn.q_norm.weight", (128,)), np.ones(128, np.float32))
    rnd.close()
    llama = lib.Context({k: v for k, v in CFG.items() if k != "qk_norm"}, max_tokens=64, max_seqs=2, max_labelled=8, max_position=64)
    with pytest.raises(lib.TstError, match="unknown weight"):
        llama.set_weight("model.layers.0.self_attn.q_norm.weight", np.ones(128, np.float32))
    llama.close()
