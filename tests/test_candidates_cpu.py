"""CPU tests of candidate-answer scoring: the host logic of tst_score_candidates_async (csrc/host_logic.h plan_candidates through the CPU library), and the
diagnostic layer around it (tst.score.answer_candidates / candidate_scores, tst.diagnose.fold_records, the run fingerprint). The sanitizer run of plan_candidates
is the stand-alone self-test (csrc/host_selftest.cpp, tests/test_host_logic_sanitized.py)."""
import dataclasses
import json

import numpy as np
import pytest

from tst import data as D
from tst import diagnose as DG
from tst import lib as L
from tst import score as S
from tst.trainer import TrainArgs

CFG = dict(vocab_size=50, hidden_size=64, num_layers=1, num_heads=1, num_kv_heads=1, head_dim=64, intermediate_size=64, rope_theta=10000.0, rms_norm_eps=1e-5)


def model_cfg(max_tokens=64, max_seqs=32, max_labelled=64, max_position=40, n_stack=1):
    return L.make_model_cfg(CFG, max_tokens=max_tokens, max_seqs=max_seqs, max_labelled=max_labelled, max_position=max_position, n_stack=n_stack)


def prompts():
    lens = (3, 1, 7, 4)
    ids = np.arange(sum(lens), dtype=np.int32) % 50
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return ids, cu


# prompt 0: a one-token candidate, a 16-token one, two sharing a first token; prompt 1: none; prompt 2: one of 3; prompt 3: a one-token candidate
CANDS = [[5], list(range(10, 26)), [7, 8], [7, 9, 11], [1, 2, 3], [49]]
SEQ = [0, 0, 0, 0, 2, 3]


def test_plan_candidates_row_map():
    ids, cu = prompts()
    cid, ccu, cseq = L.pack_candidates(CANDS, SEQ)
    p = L.host_plan_candidates(model_cfg(), ids, cu, cid, ccu, cseq)
    T, N = len(ids), len(cid)
    R = N - len(CANDS)
    assert (p["S"], p["T"], p["n_tok"], p["R_e"], p["n_ext"], p["rows_used"]) == (4, T, N, R, 4, T + R)
    assert p["cache_rows"] == 64 + 32 and p["rows_used"] <= p["cache_rows"]
    np.testing.assert_array_equal(p["last_rows"], cu[1:] - 1)
    # tails packed behind the prompts in c-major order: the map is the identity onto T .. T + R_e, so injective and inside the cache; one-token candidates take no row
    np.testing.assert_array_equal(p["ext_rows"], T + np.arange(R))
    want_geo, want_ids, want_pos, want_tgt, want_src, r = [], [], [], [], [], 0
    for c, s in zip(CANDS, SEQ):
        ln = int(cu[s + 1] - cu[s])
        want_src.append((s, c[0]))
        if len(c) >= 2:
            want_geo.append((int(cu[s]), ln, T + r, r, len(c) - 1))
        for q in range(len(c) - 1):
            want_ids.append(c[q])
            want_pos.append(ln + q)
            want_tgt.append(c[q + 1])
            want_src.append((r, -1))
            r += 1
    np.testing.assert_array_equal(p["geo"], np.array(want_geo))
    np.testing.assert_array_equal(p["ext_ids"], want_ids)
    np.testing.assert_array_equal(p["ext_pos"], want_pos)
    np.testing.assert_array_equal(p["ext_tgt"], want_tgt)
    np.testing.assert_array_equal(p["src"], np.array(want_src))
    np.testing.assert_array_equal(p["slot_r_end"], np.full(8, R))
    # the tail of candidate c starts at T + (cu_cand[c] - c)
    for g, c in zip(p["geo"], [i for i, cc in enumerate(CANDS) if len(cc) >= 2]):
        assert g[2] == T + int(ccu[c]) - c
    # a stacked context: the extend rows of the prompts in slots 0 .. q
    ps = L.host_plan_candidates(model_cfg(n_stack=2), ids, cu, cid, ccu, cseq, seq_slot=[0, 0, 1, 1])
    np.testing.assert_array_equal(ps["slot_r_end"], [R - 2] + [R] * 7)
    # a prompt without candidates is legal, and so is a call whose candidates are all single tokens (no extend pass)
    p1 = L.host_plan_candidates(model_cfg(), ids, cu, *L.pack_candidates([[4], [6]], [1, 3]))
    assert (p1["R_e"], p1["n_ext"], p1["n_tok"], p1["rows_used"]) == (0, 0, 2, T)
    np.testing.assert_array_equal(p1["src"], [(1, 4), (3, 6)])


def test_plan_candidates_refusals_carry_their_message():
    ids, cu = prompts()
    cid, ccu, cseq = L.pack_candidates(CANDS, SEQ)
    ok = model_cfg()
    N, R = len(cid), len(cid) - len(CANDS)

    def refused(msg, mc=ok, ids=ids, cu=cu, cid=cid, ccu=ccu, cseq=cseq, **kw):
        with pytest.raises(L.TstError, match=msg):
            L.host_plan_candidates(mc, ids, cu, cid, ccu, cseq, **kw)

    refused("n_cands must be at least 1", cid=cid[:0], ccu=ccu[:1], cseq=cseq[:0])
    refused("cu_cand must start at 0 and increase strictly", ccu=np.concatenate([[1], ccu[1:]]))
    refused("cu_cand must start at 0 and increase strictly", ccu=np.array([0, 1, 1, 3], np.int32), cseq=cseq[:3])
    refused("longer than TST_CAND_MAX_LEN", cid=np.arange(17, dtype=np.int32), ccu=[0, 17], cseq=[0])
    refused("candidate id out of vocabulary", cid=np.where(np.arange(N) == N - 1, 50, cid))
    refused("candidate id out of vocabulary", cid=np.where(np.arange(N) == 0, -1, cid))
    refused("cand_seq out of range", cseq=[0, 0, 0, 0, 2, 4])
    refused("cand_seq out of range", cseq=[-1, 0, 0, 0, 2, 3])
    refused("cand_seq must be non-decreasing", cseq=[0, 0, 2, 0, 2, 3])
    refused("candidate length - 1 exceeds max_position", mc=model_cfg(max_position=17))   # prompt 0: 3 + 16 - 1 = 18
    L.host_plan_candidates(model_cfg(max_position=18), ids, cu, cid, ccu, cseq)
    refused("candidates' tokens exceed max_labelled", mc=model_cfg(max_labelled=N - 1))
    L.host_plan_candidates(model_cfg(max_labelled=N), ids, cu, cid, ccu, cseq)
    for kw in (dict(max_seqs=R - 1), dict(max_tokens=R - 1), dict(max_labelled=R - 1, max_seqs=R + 5)):
        if "max_labelled" in kw:   # (fewer labelled rows than candidate tokens: that refusal comes first)
            refused("exceed max_labelled", mc=model_cfg(**kw))
        else:
            refused(r"extend rows \(sum of length - 1\) exceed min\(max_tokens, max_seqs, max_labelled\)", mc=model_cfg(**kw))
    L.host_plan_candidates(model_cfg(max_seqs=R, max_tokens=R), ids, cu, cid, ccu, cseq)
    refused("more sequences than max_labelled", mc=model_cfg(max_labelled=3), cid=[1], ccu=[0, 1], cseq=[0])
    refused("batch exceeds max_tokens/max_seqs", mc=model_cfg(max_seqs=3))
    refused("sequence length out of range", mc=model_cfg(max_position=6), cid=[1], ccu=[0, 1], cseq=[0])   # a prompt of 7 tokens
    refused("seq_slot must be non-decreasing", mc=model_cfg(n_stack=2), seq_slot=[0, 1, 0, 1])
    refused("cu_seqlens must start at 0", cu=np.concatenate([[1], cu[1:]]))


def _samples():
    """eight samples: "na" answers (3,), (4, 5), (3,), (6,), (4, 5), (7, 7), "mca" answers (9,), (9,)"""
    out = []
    for i, (kind, ans) in enumerate([("na", (3,)), ("na", (4, 5)), ("mca", (9,)), ("na", (3,)), ("na", (6,)), ("na", (4, 5)), ("mca", (9,)), ("na", (7, 7))]):
        prompt = [20 + i, 21, 22]
        out.append(D.Sample(sid=100 + i, ids=np.array(prompt + list(ans), np.int32), n_prompt=len(prompt), kind=kind, gt_option=0 if kind == "mca" else -1))
    return out


def test_answer_candidates_order_ties_and_the_reference_appended():
    smp = _samples()
    # (3,) and (4, 5) occur twice: the tie goes to the first occurrence; then (6,) before (7, 7); "mca" answers never enter
    assert S.answer_candidates(smp, 10) == [(3,), (4, 5), (6,), (7, 7)]
    assert S.answer_candidates(smp, 2) == [(3,), (4, 5)]
    assert S.answer_candidates(smp, 0) == []
    top2 = S.answer_candidates(smp, 2)
    assert S.sample_candidates(smp[0], top2) == [(3,), (4, 5)]            # the reference is on the list
    assert S.sample_candidates(smp[4], top2) == [(3,), (4, 5), (6,)]      # absent: appended
    assert S.sample_candidates(smp[2], top2) == []                        # "mca": none
    long = D.Sample(sid=1, ids=np.arange(3 + 17, dtype=np.int32), n_prompt=3, kind="na", gt_option=-1)
    assert S.answer_candidates([long] + smp, 1) == [(3,)] and S.sample_candidates(long, top2) == [(3,), (4, 5)]   # a 17-token answer cannot be a candidate
    ids, cu, seq = S.pack_candidates(smp[:5], top2)
    np.testing.assert_array_equal(seq, [0, 0, 1, 1, 3, 3, 4, 4, 4])
    np.testing.assert_array_equal(cu, [0, 1, 3, 4, 6, 7, 9, 10, 12, 13])
    np.testing.assert_array_equal(ids, [3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 6])


def test_candidate_scores_against_a_float64_restatement():
    smp = _samples()[:5]
    top2 = [(3,), (4, 5)]
    #        sample 0: ref (3,)   sample 1: ref (4, 5), tied   sample 3: ref (3,)      sample 4: ref (6,) appended
    lp = np.array([-0.5, -2.0,    -1.25, -1.25,                 -3.0, -0.25,            -1.0, -4.0, -2.0], np.float32)
    got = S.candidate_scores(smp, top2, lp)
    assert got[2] is None and [g["n"] for g in got if g] == [2, 2, 2, 3]
    o = 0
    for x, g in zip(smp, got):
        if g is None:
            continue
        z = lp[o:o + g["n"]].astype(np.float64)
        o += g["n"]
        p = np.exp(z) / np.exp(z).sum()
        np.testing.assert_allclose(g["p"], p, rtol=1e-14)
        assert abs(g["p"].sum() - 1.0) < 1e-14 and g["p"].dtype == np.float64
        assert abs(g["mass"] - np.log(np.exp(z).sum())) < 1e-14
        j = g["cands"].index(tuple(int(t) for t in x.ids[x.n_prompt:]))
        assert g["rank"] == 1 + int((z > z[j]).sum()) and abs(g["p_ref"] - p[j]) < 1e-15
    assert [g["rank"] for g in got if g] == [1, 1, 2, 2]      # a tie with the reference does not cost it its rank
    assert got[1]["top"] == [[3], [4, 5]]                      # ... and ties keep the list's order
    assert got[4]["top"] == [[3], [6], [4, 5]] and got[4]["top_p"] == sorted(got[4]["top_p"], reverse=True)
    many = [(i,) for i in range(30, 38)]
    g = S.candidate_scores([smp[0]], many, -np.arange(9, dtype=np.float32))[0]   # eight on the list + the reference (3,)
    assert g["n"] == 9 and len(g["top"]) == len(g["top_p"]) == 5 and g["top"][0] == [30] and g["rank"] == 9
    with pytest.raises(ValueError):
        S.candidate_scores(smp, top2, lp[:-1])


def _decode(ids):
    return " ".join(str(int(t)) for t in ids)


def test_mra_exp_on_a_three_candidate_example_worked_by_hand():
    # reference "10"; candidates "10", "12", "20" with p = 0.5, 0.3, 0.2. MRA over theta = 0.50 .. 0.95 counts the thresholds with relative error < 1 - theta:
    # "10": error 0 -> 10 / 10; "12": error 0.2 < 0.5 .. 0.25 -> theta 0.50 .. 0.75 -> 6 / 10; "20": error 1 -> 0. Expected 0.5 + 0.3 * 0.6 = 0.68
    x = D.Sample(sid=7, ids=np.array([1, 2, 10], np.int32), n_prompt=2, kind="na", gt_option=-1)
    lp = np.log(np.array([0.5, 0.3, 0.2])) - 1.5   # the list covers e^-1.5 of the model's distribution
    cand = S.candidate_scores([x], [(10,), (12,), (20,)], lp)
    [r] = DG.fold_records([x], 0, 0, [0.5], [1], [1], _decode, cand=cand)
    assert abs(r["cand"]["mra_exp"] - 0.68) < 1e-12
    assert r["cand"]["top_text"] == ["10", "12", "20"] and abs(r["cand"]["mass"] + 1.5) < 1e-12 and r["cand"]["rank"] == 1 and abs(r["cand"]["p_ref"] - 0.5) < 1e-12
    [r0] = DG.fold_records([x], 0, 0, [0.5], [1], [1], None, cand=cand)
    assert set(r0["cand"]) == {"n", "rank", "p_ref", "mass", "top", "top_p"}


def test_fold_records_with_and_without_candidates():
    smp = _samples()[:5]
    s, pred, correct = [0.1, 0.2, 0.3, 0.4, 0.5], [1, 0, 1, 0, 1], [1, 0, 1, 0, 1]
    base = DG.fold_records(smp, 2, 0, s, pred, correct)
    assert all("cand" not in r for r in base)
    lp = np.array([-0.5, -2.0, -1.25, -1.25, -3.0, -0.25, -1.0, -4.0, -2.0], np.float32)
    cand = S.candidate_scores(smp, [(3,), (4, 5)], lp)
    recs = DG.fold_records(smp, 2, 0, s, pred, correct, cand=cand)
    for r, b, x in zip(recs, base, smp):
        assert ("cand" in r) == (x.kind == "na")
        assert {k: v for k, v in r.items() if k != "cand"} == b and list(r)[:len(b)] == list(b)   # everything else, and its order, unchanged
        json.dumps(r)
    assert recs[4]["cand"] == dict(n=3, rank=2, p_ref=cand[4]["p_ref"], mass=cand[4]["mass"], top=[[3], [6], [4, 5]], top_p=cand[4]["top_p"])
    # the fingerprint of a run knows the setting only when it is on, and the list itself never enters (it follows from the samples)
    args = TrainArgs()
    fp = DG.run_fingerprint(smp, 2, args)
    on = TrainArgs(candidates=4)
    assert on.candidates == 4 and on.candidate_list is None and args.candidates == 0
    assert dataclasses.asdict(on) == dataclasses.asdict(args)
    assert DG.run_fingerprint(smp, 2, on) != fp and DG.run_fingerprint(smp, 2, TrainArgs(candidates=5)) != DG.run_fingerprint(smp, 2, on)
    DG.set_candidates(smp, on)
    assert on.candidate_list == [(3,), (4, 5), (6,)] and DG.run_fingerprint(smp, 2, on) == DG.run_fingerprint(smp, 2, TrainArgs(candidates=4))
    DG.set_candidates(smp, args)
    assert args.candidate_list is None and DG.run_fingerprint(smp, 2, args) == fp


def test_cli_flag_reaches_the_training_arguments():
    from tst import cli
    ap = cli.build_parser()
    a = ap.parse_args(["diagnose", "--out", "x"])
    assert a.candidates == 0 and cli._args_to_train(a).candidates == 0
    assert cli._args_to_train(ap.parse_args(["diagnose", "--out", "x", "--candidates", "32"])).candidates == 32
    with pytest.raises(SystemExit):
        cli._args_to_train(ap.parse_args(["diagnose", "--out", "x", "--candidates", "-1"]))
