"""GPU tests of candidate-answer scoring (include/tst_hip.h tst_score_candidates_async; csrc/decode.hip attn_extend / cand_logp, engine.hip, host_logic.h
plan_candidates).

Reference = the pinned numpy oracle's forward_logits on the concatenations prompt + candidate, log_softmax in float64 at every candidate token: the definition,
no cache, no device. Inputs: the shared prompts of tests/generate_oracle.py (the five fixture families) and per prompt five candidates -- a one-token one, a
16-token one, two that share their first token (2 and 3 tokens), and the prompt's "reference answer" (4 tokens, what an "na" QA pair carries; the fixture
prompts are random ids, so it is a fixed random draw as well).
  1. strict (fp32) contexts: |logp_tok - reference| <= 2 LOGIT_TOL on EVERY candidate token (LOGIT_TOL = 1e-4 is tests/test_strict_gpu.py's bound on one
     strict logit; two logits may move against each other: the rule of tests/test_generate_gpu.py), every family, base model and LoRA adapters, and one full
     fine-tune context. logp_cand is the double sum of logp_tok in token order, rounded once.
  2. bf16 contexts, against the library's own uncached path: L = forward_logits of the same context on the concatenations, O the oracle's,
     E = max |L - O| measured here; |logp_tok - log_softmax(L)[tok]| <= 4 E. Two runs are bit-identical.
  3. stacked slots, forks, batch independence, side effects, refusals, the mismatched fetch, allocation, device ids, the diagnostic layer."""
import functools

import numpy as np
import pytest

import generate_oracle as G
import golden_inputs as GI

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4   # tests/test_strict_gpu.py
TAGS = list(G.FAMILIES)
ADAPTERS = (None, 99)


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def make_ctx(L, tag, precision, lora_seed=None, mode="lora", n_stack=1, max_seqs=256, max_labelled=512, max_position=256, max_tokens=4096):
    cfg = G.FAMILIES[tag]
    ctx = L.Context(cfg, max_tokens=max_tokens, max_seqs=max_seqs, max_labelled=max_labelled,
                    max_position=cfg["max_position"] if cfg.get("arch") == "gpt2" else max_position, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode,
                    precision=precision, n_stack=n_stack)
    ctx.load_state_dict(G.weights(tag))
    if lora_seed is not None:
        ctx.set_trainable(G.lora(tag, lora_seed))
    return ctx


@functools.lru_cache(maxsize=None)
def candidates_of(tag):
    """per prompt of the family: [one token], [16 tokens], [b, c], [b, d, e], the reference answer [4 tokens]"""
    V = G.FAMILIES[tag]["vocab_size"]
    rng = np.random.default_rng(77)
    out = []
    for _ in G.make_prompts(G.FAMILIES[tag]):
        t = rng.integers(0, V, 1 + 16 + 5 + 4)
        out.append([[int(t[0])], [int(v) for v in t[1:17]], [int(t[17]), int(t[18])], [int(t[17]), int(t[19]), int(t[20])], [int(v) for v in t[22:26]]])
    return out


def flatten(cands, which=None):
    """(list of candidates, prompt index of each) for the prompts `which` (default all), numbered from 0 in that order"""
    which = range(len(cands)) if which is None else which
    flat = [(c, i) for i, s in enumerate(which) for c in cands[s]]
    return [c for c, _ in flat], [i for _, i in flat]


def concat_rows(prompts, flat, seq):
    """the concatenations prompt + candidate packed, and the rows whose logits predict every candidate token (candidate-token order)"""
    seqs = [np.concatenate([prompts[s], np.asarray(c, np.int32)]) for c, s in zip(flat, seq)]
    ids, cu = G.pack(seqs)
    rows = np.concatenate([cu[i] + len(prompts[s]) - 1 + np.arange(len(c)) for i, (c, s) in enumerate(zip(flat, seq))]).astype(np.int32)
    return ids, cu, rows


def logp_at(logits, flat):
    tok = np.array([t for c in flat for t in c])
    return G.log_softmax(logits)[np.arange(len(tok)), tok]


@functools.lru_cache(maxsize=None)
def oracle_logits(tag, lora_seed):
    """the fp32 oracle's logits [n_cand_tokens, V] on the family's prompts + candidates"""
    prompts = G.make_prompts(G.FAMILIES[tag])
    flat, seq = flatten(candidates_of(tag))
    return np.asarray(G.make_oracle(tag, lora_seed).forward_logits(*concat_rows(prompts, flat, seq)), np.float64)


def score(L, ctx, prompts, flat, seq, **kw):
    return ctx.score_candidates(*G.pack(prompts), *L.pack_candidates(flat, seq), **kw)


def check_sums(flat, lt, lc):
    o = 0
    for c, v in zip(flat, lc):
        assert v == np.float32(sum(float(x) for x in lt[o:o + len(c)])), "logp_cand is not the double sum of logp_tok, rounded once"
        o += len(c)


# ------------------------------------------------------------------------------------------------ 1. strict
@pytest.mark.parametrize("lora_seed", ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_strict_logp_of_every_candidate_token_matches_the_oracle(L, tag, lora_seed):
    prompts = G.make_prompts(G.FAMILIES[tag])
    flat, seq = flatten(candidates_of(tag))
    ref = logp_at(oracle_logits(tag, lora_seed), flat)
    ctx = make_ctx(L, tag, "strict", lora_seed)
    lt, lc = score(L, ctx, prompts, flat, seq)
    ctx.close()
    d = float(np.abs(lt - ref).max())
    print(f"strict[{tag}, {lora_seed}]: {len(lt)} candidate tokens of {len(flat)} candidates, |logp_tok - oracle| max = {d:.3e}")
    assert lt.shape == (sum(len(c) for c in flat),) and lc.shape == (len(flat),) and np.isfinite(lt).all()
    assert d <= 2 * LOGIT_TOL
    check_sums(flat, lt, lc)


def test_strict_full_finetune_context_scores_candidates(L):
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    flat, seq = flatten(candidates_of("tiny"))
    ctx = make_ctx(L, "tiny", "strict", mode="full")
    lt, _ = score(L, ctx, prompts, flat, seq)
    ctx.close()
    d = float(np.abs(lt - logp_at(oracle_logits("tiny", None), flat)).max())
    print(f"strict full fine-tune: |logp_tok - oracle| max = {d:.3e}")
    assert d <= 2 * LOGIT_TOL


# ------------------------------------------------------------------------------------------------ 2. bf16
def band_E(ctx, orc_logits, prompts, flat, seq, seq_slot=None):
    """(log_softmax(L) at the candidate tokens, E = max |L - O|) with L the context's own uncached logits on the concatenations"""
    ids, cu, rows = concat_rows(prompts, flat, seq)
    slots = None if seq_slot is None else np.asarray(seq_slot, np.int32)[seq]
    Lg = ctx.forward_logits(ids, cu, rows, seq_slot=slots).astype(np.float64)
    return logp_at(Lg, flat), float(np.abs(Lg - orc_logits).max())


@pytest.mark.parametrize("lora_seed", ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_bf16_logp_stays_inside_the_uncached_paths_error(L, tag, lora_seed):
    prompts = G.make_prompts(G.FAMILIES[tag])
    flat, seq = flatten(candidates_of(tag))
    ctx = make_ctx(L, tag, "bf16", lora_seed)
    lt, lc = score(L, ctx, prompts, flat, seq)
    own, E = band_E(ctx, oracle_logits(tag, lora_seed), prompts, flat, seq)
    lt2, lc2 = score(L, ctx, prompts, flat, seq)
    ctx.close()
    d = float(np.abs(lt - own).max())
    print(f"bf16[{tag}, {lora_seed}]: E = {E:.3e}  |logp_tok - log_softmax(L)[tok]| max = {d:.3e}")
    assert np.isfinite(lt).all() and d <= 4 * E
    check_sums(flat, lt, lc)
    np.testing.assert_array_equal(lt2.view(np.uint32), lt.view(np.uint32))
    np.testing.assert_array_equal(lc2.view(np.uint32), lc.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. stacked
def test_stacked_slots_score_under_their_own_adapters(L):
    tag, adapters = "tiny", (99, 100)
    prompts = G.make_prompts(G.FAMILIES[tag])
    slots = np.array([0] * 5 + [1] * 4, np.int32)
    flat, seq = flatten(candidates_of(tag))
    ctx = make_ctx(L, tag, "bf16", n_stack=2)
    for sl, a in enumerate(adapters):
        ctx.select_slot(sl)
        ctx.set_trainable(G.lora(tag, a))
    lt, _ = score(L, ctx, prompts, flat, seq, seq_slot=slots)
    tok_slot = np.concatenate([np.full(len(c), slots[s]) for c, s in zip(flat, seq)])
    orc = {99: oracle_logits(tag, 99)}
    orc[100] = np.asarray(G.make_oracle(tag, 100).forward_logits(*concat_rows(prompts, flat, seq)), np.float64)
    mixed = np.where((tok_slot == 0)[:, None], orc[99], orc[100])   # every token under its own slot's adapters
    own, E = band_E(ctx, mixed, prompts, flat, seq, seq_slot=slots)
    ctx.close()
    d = np.abs(lt - own)
    print(f"stacked: E = {E:.3e}, own adapters |d logp| max = {d.max():.3e}")
    assert d.max() <= 4 * E
    for sl, other in ((0, 100), (1, 99)):
        wrong = np.abs(lt - logp_at(orc[other], flat))[tok_slot == sl]
        print(f"slot {sl} judged under adapters {other}: |d logp| max = {wrong.max():.3e} ({int((wrong > 4 * E).sum())}/{len(wrong)} tokens outside 4 E)")
        assert wrong.max() > 4 * E + 2 * E, "the other slot's adapters would pass: the inputs do not discriminate"   # (2 E: log_softmax(L) against log_softmax(O))


# ------------------------------------------------------------------------------------------------ forks
def test_forked_contexts_use_their_own_cache(L):
    tag = "tiny"
    prompts = G.make_prompts(G.FAMILIES[tag])
    cands = candidates_of(tag)
    root = make_ctx(L, tag, "strict", 99)
    fork = root.fork()
    fork.set_trainable(G.lora(tag, 100))
    fa, sa = flatten(cands, range(0, 5))
    fb, sb = flatten(cands, range(4, 9))
    pa, pb = prompts[0:5], prompts[4:9]
    alone_a, alone_b = score(L, root, pa, fa, sa), score(L, fork, pb, fb, sb)
    f0 = fork.device_bytes()
    # both pending at once, enqueued back to back on the two contexts' streams: a shared cache would hold the other call's keys
    root.score_candidates_async(*G.pack(pa), *L.pack_candidates(fa, sa))
    fork.score_candidates_async(*G.pack(pb), *L.pack_candidates(fb, sb))
    got_b, got_a = fork.score_candidates_fetch(), root.score_candidates_fetch()
    assert fork.device_bytes() == f0
    fork.close()
    root.close()
    for got, alone in ((got_a, alone_a), (got_b, alone_b)):
        np.testing.assert_array_equal(got[0].view(np.uint32), alone[0].view(np.uint32))
        np.testing.assert_array_equal(got[1].view(np.uint32), alone[1].view(np.uint32))
    # and the fork ran under its own adapters
    orc_b = np.asarray(G.make_oracle(tag, 100).forward_logits(*concat_rows(pb, fb, sb)), np.float64)
    assert float(np.abs(got_b[0] - logp_at(orc_b, fb)).max()) <= 2 * LOGIT_TOL


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("precision", ["strict", "bf16"])
def test_a_prompts_results_do_not_depend_on_its_batch_or_its_other_candidates(L, precision):
    tag, s = "tiny", 6
    prompts = G.make_prompts(G.FAMILIES[tag])
    cands = candidates_of(tag)
    flat, seq = flatten(cands)
    ctx = make_ctx(L, tag, precision, 99)
    lt_all, _ = score(L, ctx, prompts, flat, seq)
    mine = np.flatnonzero(np.concatenate([np.full(len(c), q == s) for c, q in zip(flat, seq)]))
    lt_one, _ = score(L, ctx, [prompts[s]], cands[s], [0] * len(cands[s]))                 # the prompt alone, all of its candidates
    singles = [score(L, ctx, [prompts[s]], [c], [0])[0] for c in cands[s]]                  # ... and every candidate alone
    lt_rev, _ = score(L, ctx, [prompts[s]], cands[s][::-1], [0] * len(cands[s]))           # ... and in another order
    if precision == "bf16":
        _, E = band_E(ctx, oracle_logits(tag, 99), prompts, flat, seq)
        tol = 4 * E
    else:
        tol = 2 * LOGIT_TOL
    ctx.close()
    cut = np.cumsum([len(c) for c in cands[s][::-1]])[:-1]
    rev = np.concatenate(np.split(lt_rev, cut)[::-1])   # back into the list's own order
    for name, got in (("alone", lt_one), ("one candidate per call", np.concatenate(singles)), ("reversed", rev)):
        d = float(np.abs(got - lt_all[mine]).max())
        print(f"{precision}, prompt {s} {name} against in company: |d logp_tok| max = {d:.3e} (bound {tol:.3e})")
        assert d <= tol


# ------------------------------------------------------------------------------------------------ side effects
def test_candidate_scoring_leaves_training_accumulation_and_pending_scores_alone(L):
    cfg = G.FAMILIES["tiny"]
    ids, labels, cu = GI.make_batch(cfg)
    ids2, labels2, cu2 = GI.make_batch(cfg, lengths=(33, 70), n_answer=(4, 1), seed=11)
    prompts = G.make_prompts(cfg)
    pid, pcu = G.pack(prompts)
    flat, seq = flatten(candidates_of("tiny"))

    def trajectory(with_cand):
        ctx = make_ctx(L, "tiny", "bf16", 99)
        packed = L.pack_candidates(flat, seq)
        out = []
        for step in range(4):
            if with_cand and step == 2:
                ctx.score_candidates(pid, pcu, *packed)
            out.append(ctx.train_step(ids if step % 2 == 0 else ids2, labels if step % 2 == 0 else labels2, cu if step % 2 == 0 else cu2, 1e-3))
        ctx.accumulate_async(ids, labels, cu, 11, True)   # an accumulation window with a candidate scoring inside it
        if with_cand:
            ctx.score_candidates_async(pid, pcu, *packed)
        ctx.accumulate_async(ids2, labels2, cu2, 11, False)
        ctx.optimizer_step_async([1e-3])
        out.append(ctx.fetch_metrics())
        if with_cand:
            ctx.score_candidates_fetch()
        ctx.score_rows_async(ids, labels, cu, [3, 9, 27, 81])   # a pending scoring pass fetched after a candidate scoring
        if with_cand:
            ctx.score_candidates(pid, pcu, *packed)
        sc = ctx.score_rows_fetch()
        greedy = ctx.generate(pid, pcu, G.MAX_NEW)            # a generation behind it: the shared cache carries nothing over
        if with_cand:
            ctx.score_candidates(pid, pcu, *packed)
            again = ctx.generate(pid, pcu, G.MAX_NEW)
            for a, b in zip(greedy, again):
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        tr = ctx.get_trainable()
        ctx.close()
        return np.array(out, np.float32), tr, sc, greedy

    m0, t0, s0, g0 = trajectory(False)
    m1, t1, s1, g1 = trajectory(True)
    np.testing.assert_array_equal(m0.view(np.uint32), m1.view(np.uint32))
    assert t0.keys() == t1.keys()
    for k in t0:
        np.testing.assert_array_equal(t0[k].view(np.uint32), t1[k].view(np.uint32), err_msg=k)
    for a, b in zip(s0, s1):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(g0, g1):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ refusals, the pending slot, allocation
def test_refusals_carry_their_message_and_allocate_nothing(L):
    cfg = G.FAMILIES["tiny"]
    prompts = G.make_prompts(cfg)
    ids, cu = G.pack(prompts)
    flat, seq = flatten(candidates_of("tiny"))
    cid, ccu, cseq = L.pack_candidates(flat, seq)
    N, R = len(cid), len(cid) - len(flat)
    ctx = make_ctx(L, "tiny", "bf16", 99, max_seqs=200, max_labelled=N, max_position=145)   # 130 + 16 - 1 = 145 fits exactly
    b0 = ctx.device_bytes()
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending tst_score_candidates_async"):
        ctx.score_candidates_fetch()
    one = np.array([0, 1], np.int32)
    for args, msg in (((cid[:1], np.array([0], np.int32), cseq[:0]), "n_cands must be at least 1"),
                      ((cid, np.concatenate([[1], ccu[1:]]).astype(np.int32), cseq), "cu_cand must start at 0"),
                      ((cid, np.where(np.arange(len(ccu)) == 2, ccu[1], ccu).astype(np.int32), cseq), "cu_cand must start at 0"),
                      ((np.arange(17, dtype=np.int32), np.array([0, 17], np.int32), [0]), "longer than TST_CAND_MAX_LEN"),
                      ((np.where(np.arange(N) == N - 1, 256, cid).astype(np.int32), ccu, cseq), "candidate id out of vocabulary"),
                      ((cid, ccu, np.where(np.arange(len(cseq)) == len(cseq) - 1, 9, cseq)), "cand_seq out of range"),
                      ((cid, ccu, cseq[::-1].copy()), "cand_seq must be non-decreasing")):
        with pytest.raises(L.TstError, match=r"\(-1\).*" + msg):
            ctx.score_candidates(ids, cu, *args)
    with pytest.raises(L.TstError, match=r"\(-1\).*out of vocabulary"):
        ctx.score_candidates(np.where(np.arange(len(ids)) == 3, 256, ids).astype(np.int32), cu, cid[:1], one, [0])
    assert ctx.device_bytes() == b0
    for kw, msg in ((dict(max_position=144), "candidate length - 1 exceeds max_position"), (dict(max_labelled=N - 1), "candidates' tokens exceed max_labelled"),
                    (dict(max_seqs=R - 1), "extend rows"), (dict(max_labelled=8), "more sequences than max_labelled")):
        small = make_ctx(L, "tiny", "bf16", **dict(dict(max_seqs=200, max_labelled=N, max_position=145), **kw))
        s0 = small.device_bytes()
        with pytest.raises(L.TstError, match=r"\(-1\).*" + msg):
            small.score_candidates(ids, cu, cid, ccu, cseq)
        assert small.device_bytes() == s0
        small.close()
    # the three kinds share the one pending slot: a fetch of another kind is refused and leaves the pending call fetchable
    ctx.score_candidates_async(ids, cu, cid, ccu, cseq)
    b1 = ctx.device_bytes()
    assert b1 > b0
    with pytest.raises(L.TstError, match=r"\(-4\).*pending call is a tst_score_candidates_async"):
        ctx.generate_fetch()
    with pytest.raises(L.TstError, match=r"\(-4\).*pending call is a tst_score_candidates_async"):
        ctx.sample_fetch()
    lt, lc = ctx.score_candidates_fetch()
    assert lt.shape == (N,) and lc.shape == (len(flat),) and np.isfinite(lt).all() and (lt < 0).all()
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending"):
        ctx.score_candidates_fetch()
    ctx.generate_async(ids, cu, 1)
    with pytest.raises(L.TstError, match=r"\(-4\).*pending generation is a tst_generate_async"):
        ctx.score_candidates_fetch()
    assert ctx.generate_fetch()[0].shape == (9, 1)
    ctx.sample_async(ids, cu, 1, 2, 1.0, np.arange(9, dtype=np.uint64))
    with pytest.raises(L.TstError, match=r"\(-4\).*pending generation is a tst_sample_async"):
        ctx.score_candidates_fetch()
    assert ctx.sample_fetch()[0].shape == (9, 2, 1)
    # allocation on first use only: the second call, a refused one and a prompt without candidates change nothing
    b2 = ctx.device_bytes()   # (the first sampled generation added its seeds)
    lt2, _ = ctx.score_candidates(ids, cu, cid, ccu, cseq)
    np.testing.assert_array_equal(lt2.view(np.uint32), lt.view(np.uint32))
    with pytest.raises(L.TstError, match=r"\(-1\).*n_cands"):
        ctx.score_candidates(ids, cu, cid[:1], np.array([0], np.int32), cseq[:0])
    lt3, lc3 = ctx.score_candidates(ids, cu, [flat[0][0], flat[-1][0]], [0, 1, 2], [0, 8])   # seven prompts without candidates, no extend pass
    assert ctx.device_bytes() == b2
    np.testing.assert_array_equal(lt3.view(np.uint32), np.array([lt[0], lt[ccu[-2]]]).view(np.uint32))
    np.testing.assert_array_equal(lc3.view(np.uint32), lt3.view(np.uint32))
    bids, blab, bcu = GI.make_batch(cfg)
    loss, gn = ctx.train_step(bids, blab, bcu, 1e-3)
    assert np.isfinite(loss) and np.isfinite(gn) and loss > 0
    ctx.close()


def test_device_resident_prompt_ids_give_the_same_numbers(L):
    L.load_lab()
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ids, cu = G.pack(prompts)
    flat, seq = flatten(candidates_of("tiny"))
    packed = L.pack_candidates(flat, seq)
    ctx = make_ctx(L, "tiny", "strict", 99)
    want = ctx.score_candidates(ids, cu, *packed)
    good = L.DevBuf(ids)
    got = ctx.score_candidates(L.DeviceIds(good.ptr.value, len(ids)), cu, *packed)
    ctx.close()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the diagnostic layer
def test_fold_records_carry_cand_with_the_flag_and_not_without(L, tmp_path):
    """diagnose on the tiny model in the plain layout (one context) and the concurrent-forks layout, strict precision, adapters trained at learning rate 0 (both
    layouts hold the same model). candidates = 0 writes byte for byte what a run without the setting writes; candidates = 4 writes those shards plus `cand` on the
    "na" records only, and the two layouts agree on it: equal n, rank and top, p_ref / mass / top_p within what 2 LOGIT_TOL per candidate token moves them."""
    import dataclasses
    import json
    from tst import data as D
    from tst import diagnose as DG
    from tst import score as S
    from tst.trainer import TrainArgs
    cfg = G.FAMILIES["tiny"]
    samples = D.synth_vsi(24, cfg["vocab_size"], seed=3)
    args = TrainArgs(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=0.0, logging_steps=0,
                     lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA)
    fields = dataclasses.asdict(args)
    assert DG.run_fingerprint(samples, 2, args) == DG.run_fingerprint(samples, 2, TrainArgs(**fields, candidates=0))
    assert DG.run_fingerprint(samples, 2, args) != DG.run_fingerprint(samples, 2, TrainArgs(**fields, candidates=4))
    n_na = sum(x.kind == "na" for x in samples)
    assert 4 <= n_na < len(samples)
    cands = S.answer_candidates(samples, 4)

    def make():
        c = L.Context(cfg, max_tokens=8 * 160, max_seqs=256, max_labelled=256, max_position=160, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, precision="strict")
        c.load_state_dict(G.weights("tiny"))
        return c

    by_layout = {}
    for layout, forks, k in (("one", 0, 2), ("concurrent", 1, 4)):
        shards = {}
        for name, a in (("off", args), ("zero", TrainArgs(**fields, candidates=0)), ("on", TrainArgs(**fields, candidates=4))):
            root = make()
            ctxs = [root] + [root.fork() for _ in range(forks)]
            out = str(tmp_path / f"{layout}_{name}")
            recs, _ = DG.diagnose(ctxs if forks else root, samples, k, a, 0, 1, 0, out)
            shards[name] = [open(DG.fold_path(out, 0, f)).read() for f in range(k)]
            for c in ctxs[1:]:
                c.close()
            root.close()
            assert len(recs) == len(samples)
            if name == "on":
                by_id = {s.sid: s for s in samples}
                for r in recs:
                    assert ("cand" in r) == (by_id[r["id"]].kind == "na")
                    if "cand" in r:
                        c = r["cand"]
                        mine = S.sample_candidates(by_id[r["id"]], cands)
                        assert set(c) == {"n", "rank", "p_ref", "mass", "top", "top_p"} and c["n"] == len(mine) and 1 <= c["rank"] <= c["n"]
                        assert c["mass"] < 0 and 0 < c["p_ref"] <= 1 and len(c["top"]) == min(5, c["n"]) and all(tuple(t) in mine for t in c["top"])
                        assert c["top_p"] == sorted(c["top_p"], reverse=True) and (c["rank"] == 1) == (c["p_ref"] == c["top_p"][0])
                by_layout[layout] = {r["id"]: r["cand"] for r in recs if "cand" in r}
            else:
                assert all("cand" not in r for r in recs)
        assert shards["zero"] == shards["off"]
        for off, on in zip(shards["off"], shards["on"]):
            stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk != "cand"}) + "\n" for line in on.splitlines())
            assert stripped == off
    assert by_layout["one"].keys() == by_layout["concurrent"].keys() and len(by_layout["one"]) == n_na
    tol = 4 * 2 * LOGIT_TOL * 2   # a candidate has at most 4 tokens, each inside rule 1's bound; a softmax over such sums moves by at most twice that
    for sid, c in by_layout["one"].items():
        o = by_layout["concurrent"][sid]
        assert (c["n"], c["rank"], c["top"]) == (o["n"], o["rank"], o["top"]), f"QA pair {sid}: cand depends on the fold layout"
        np.testing.assert_allclose([c["p_ref"], c["mass"]] + c["top_p"], [o["p_ref"], o["mass"]] + o["top_p"], atol=tol, rtol=0)
