"""GPU tests of greedy generation with the per-context KV cache (include/tst_hip.h tst_generate_async; csrc/decode.hip, engine.hip, host_logic.h).

Reference = tests/generate_oracle.py: the pinned numpy oracle's forward_logits re-run on the growing sequences, arg-max taken -- the definition, no cache.
  1. strict (fp32) contexts are TOKEN-EXACT against it on every row and step, all five families, base model and LoRA adapters, and
     |logp - oracle log-softmax at the token| <= 2 LOGIT_TOL (LOGIT_TOL = 1e-4 is tests/test_strict_gpu.py's bound on one strict logit; the oracle's smallest
     top-1 / top-2 gap over these cases is 6.0e-4 (tiny, LoRA-99), against the 2e-4 two strict logits may move).
  2. bf16 contexts are held against the library's OWN uncached path: the generated sequences are replayed through forward_logits of the same context (L) and
     through the fp32 oracle (O); E = max |L - O| is the existing path's error, measured here, and at every step L[tok] >= max(L) - 2 E and
     |logp - log_softmax(L)[tok]| <= 4 E. Two runs give bit-identical tokens and logp.
  3. stacked contexts: every sequence obeys rule 2 under its own slot's adapters, and the inputs discriminate (the other slot's adapters break the band).
  4. EOS cut, 5. no side effects on training / accumulation / a pending scoring pass, 6. refusals, 7. the diagnostic layer."""
import numpy as np
import pytest

import generate_oracle as G
import golden_inputs as GI

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4   # tests/test_strict_gpu.py
TAGS = list(G.FAMILIES)
ADAPTERS = [None, 99]


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def make_ctx(L, tag, precision, lora_seed=None, mode="lora", n_stack=1, max_labelled=128, max_position=256):
    cfg = G.FAMILIES[tag]
    ctx = L.Context(cfg, max_tokens=1024, max_seqs=16, max_labelled=max_labelled, max_position=cfg["max_position"] if cfg.get("arch") == "gpt2" else max_position,
                    lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode, precision=precision, n_stack=n_stack)
    ctx.load_state_dict(G.weights(tag))
    if lora_seed is not None:
        ctx.set_trainable(G.lora(tag, lora_seed))
    return ctx


def check_band(name, ctx, orc, prompts, tokens, logp, seq_slot=None):
    """rule 2 of the module docstring for the sequences `prompts` + `tokens`; returns E"""
    ids, cu, rows = G.replay_rows(prompts, tokens)
    Lg = ctx.forward_logits(ids, cu, rows, seq_slot=seq_slot).astype(np.float64)
    Og = np.asarray(orc.forward_logits(ids, cu, rows), np.float64)
    E = float(np.abs(Lg - Og).max())
    tok = tokens.reshape(-1)
    at_tok = Lg[np.arange(len(tok)), tok]
    short = float((Lg.max(-1) - at_tok).max())
    d_logp = float(np.abs(logp.reshape(-1) - G.log_softmax(Lg)[np.arange(len(tok)), tok]).max())
    n_not_argmax = int((Lg.argmax(-1) != tok).sum())
    print(f"{name}: E = {E:.3e}  max(L) - L[tok] <= {short:.3e}  |d logp| <= {d_logp:.3e}  tokens that are not the replay's arg-max: {n_not_argmax}/{len(tok)}")
    assert (at_tok >= Lg.max(-1) - 2 * E).all(), f"{name}: a generated token lies {short:.3e} under the replay's maximum, E = {E:.3e}"
    assert d_logp <= 4 * E, f"{name}: logp off the replay's by {d_logp:.3e}, E = {E:.3e}"
    return E


# ------------------------------------------------------------------------------------------------ 1. strict: token-exact
@pytest.mark.parametrize("lora_seed", ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_strict_generation_is_token_exact(L, tag, lora_seed):
    prompts = G.make_prompts(G.FAMILIES[tag])
    ref_tok, ref_logp, _ = G.greedy_reference(tag, lora_seed)
    ctx = make_ctx(L, tag, "strict", lora_seed)
    tok, logp, n_new = ctx.generate(*G.pack(prompts), G.MAX_NEW)
    ctx.close()
    d = float(np.abs(logp - ref_logp).max())
    print(f"strict[{tag}, {lora_seed}]: tokens equal {int((tok == ref_tok).sum())}/{tok.size}  |d logp| max = {d:.3e}")
    np.testing.assert_array_equal(tok, ref_tok)
    assert d <= 2 * LOGIT_TOL
    assert (n_new == G.MAX_NEW).all()


def test_strict_full_finetune_context_generates(L):
    """a full fine-tune context (every weight trainable, no adapters) continues like the base model"""
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ref_tok, ref_logp, _ = G.greedy_reference("tiny", None)
    ctx = make_ctx(L, "tiny", "strict", mode="full")
    tok, logp, _ = ctx.generate(*G.pack(prompts), G.MAX_NEW)
    ctx.close()
    np.testing.assert_array_equal(tok, ref_tok)
    assert float(np.abs(logp - ref_logp).max()) <= 2 * LOGIT_TOL


# ------------------------------------------------------------------------------------------------ 2. bf16: against the library's own uncached path
@pytest.mark.parametrize("lora_seed", ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_bf16_generation_stays_inside_the_uncached_paths_error(L, tag, lora_seed):
    prompts = G.make_prompts(G.FAMILIES[tag])
    ctx = make_ctx(L, tag, "bf16", lora_seed)
    ids, cu = G.pack(prompts)
    tok, logp, n_new = ctx.generate(ids, cu, G.MAX_NEW)
    assert tok.min() >= 0 and tok.max() < G.FAMILIES[tag]["vocab_size"] and (n_new == G.MAX_NEW).all() and np.isfinite(logp).all()
    check_band(f"bf16[{tag}, {lora_seed}]", ctx, G.make_oracle(tag, lora_seed), prompts, tok, logp)
    tok2, logp2, _ = ctx.generate(ids, cu, G.MAX_NEW)
    ctx.close()
    np.testing.assert_array_equal(tok2, tok)
    np.testing.assert_array_equal(logp2.view(np.uint32), logp.view(np.uint32))


def test_forked_context_generates_with_its_own_cache(L):
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    root = make_ctx(L, "tiny", "bf16", 99)
    child = root.fork()
    child.set_trainable(G.lora("tiny", 100))
    ids, cu = G.pack(prompts)
    b0 = child.device_bytes()
    child.generate_async(ids, cu, G.MAX_NEW)
    root.generate_async(ids, cu, G.MAX_NEW)
    tok_c, logp_c, _ = child.generate_fetch()
    tok_r, logp_r, _ = root.generate_fetch()
    assert child.device_bytes() > b0
    check_band("fork lora100", child, G.make_oracle("tiny", 100), prompts, tok_c, logp_c)
    check_band("root lora99", root, G.make_oracle("tiny", 99), prompts, tok_r, logp_r)
    child.close()
    root.close()


# ------------------------------------------------------------------------------------------------ 3. stacked
def test_stacked_slots_generate_under_their_own_adapters(L):
    tag, seeds = "tiny", (99, 100)
    prompts = G.make_prompts(G.FAMILIES[tag])
    slots = np.array([0] * 5 + [1] * 4, np.int32)
    ctx = make_ctx(L, tag, "bf16", n_stack=2)
    for sl, seed in enumerate(seeds):
        ctx.select_slot(sl)
        ctx.set_trainable(G.lora(tag, seed))
    ids, cu = G.pack(prompts)
    tok, logp, _ = ctx.generate(ids, cu, G.MAX_NEW, seq_slot=slots)
    E = 0.0
    for sl, seed in enumerate(seeds):
        mine = np.flatnonzero(slots == sl)
        E = max(E, check_band(f"stacked slot {sl}", ctx, G.make_oracle(tag, seed), [prompts[i] for i in mine], tok[mine], logp[mine],
                              seq_slot=np.full(len(mine), sl, np.int32)))
    ctx.close()
    # the inputs discriminate, from the oracle alone: every one of the 9 oracle continuations under one adapter set leaves the band of the OTHER set by more
    # than the measured error could hide (a GPU logit is within E of the oracle's, so 4 E under the oracle's maximum is more than 2 E under the GPU's)
    for a, b in ((99, 100), (100, 99)):
        ref_tok, _, _ = G.greedy_reference(tag, a)
        rid, rcu, rows = G.replay_rows(prompts, ref_tok)
        Ob = np.asarray(G.make_oracle(tag, b).forward_logits(rid, rcu, rows), np.float64).reshape(len(prompts), G.MAX_NEW, -1)
        under = Ob.max(-1) - np.take_along_axis(Ob, ref_tok[..., None].astype(np.int64), -1)[..., 0]
        broke = (under > 4 * E).any(-1)
        print(f"adapters {a} judged under {b}: {int(broke.sum())}/9 sequences break the band (E = {E:.3e}); smallest worst-step deficit {float(under.max(-1).min()):.3e}")
        assert broke.all()
    assert int((G.greedy_reference(tag, 99)[0] == G.greedy_reference(tag, 100)[0]).sum()) <= 1


# ------------------------------------------------------------------------------------------------ 4. EOS
def test_eos_cuts_a_row_and_leaves_the_others_alone(L):
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ref_tok, _, _ = G.greedy_reference("tiny", None)
    assert [tuple(x) for x in np.argwhere(ref_tok == 99)] == [(3, 2)]   # the oracle emits 99 as the third new token of the fourth prompt and nowhere else
    ctx = make_ctx(L, "tiny", "strict")
    ids, cu = G.pack(prompts)
    tok0, logp0, n0 = ctx.generate(ids, cu, G.MAX_NEW)
    tok, logp, n_new = ctx.generate(ids, cu, G.MAX_NEW, eos_ids=(99,))
    ctx.close()
    assert n_new[3] == 3 and (tok[3, 3:] == -1).all() and (logp[3, 3:] == 0).all()
    np.testing.assert_array_equal(tok[3, :3], ref_tok[3, :3])
    keep = np.arange(len(prompts)) != 3
    np.testing.assert_array_equal(tok[keep], tok0[keep])
    np.testing.assert_array_equal(logp[keep].view(np.uint32), logp0[keep].view(np.uint32))
    np.testing.assert_array_equal(logp[3, :3].view(np.uint32), logp0[3, :3].view(np.uint32))
    assert (n_new[keep] == G.MAX_NEW).all() and (n0 == G.MAX_NEW).all()


# ------------------------------------------------------------------------------------------------ 5. no side effects
def test_generation_leaves_training_accumulation_and_pending_scores_alone(L):
    cfg = G.FAMILIES["tiny"]
    ids, labels, cu = GI.make_batch(cfg)
    ids2, labels2, cu2 = GI.make_batch(cfg, lengths=(33, 70), n_answer=(4, 1), seed=11)
    pid, pcu = G.pack(G.make_prompts(cfg))

    def trajectory(with_generate):
        ctx = make_ctx(L, "tiny", "bf16", 99)
        out = []
        for step in range(4):
            if with_generate and step == 2:
                ctx.generate(pid, pcu, G.MAX_NEW)
            out.append(ctx.train_step(ids if step % 2 == 0 else ids2, labels if step % 2 == 0 else labels2, cu if step % 2 == 0 else cu2, 1e-3))
        # an accumulation window with a generation inside it
        ctx.accumulate_async(ids, labels, cu, 11, True)
        if with_generate:
            ctx.generate_async(pid, pcu, 3)
        ctx.accumulate_async(ids2, labels2, cu2, 11, False)
        ctx.optimizer_step_async([1e-3])
        out.append(ctx.fetch_metrics())
        if with_generate:
            ctx.generate_fetch()
        # a pending scoring pass fetched after a generation
        ctx.score_rows_async(ids, labels, cu, [3, 9, 27, 81])
        if with_generate:
            ctx.generate(pid, pcu, G.MAX_NEW)
        score = ctx.score_rows_fetch()
        tr = ctx.get_trainable()
        ctx.close()
        return np.array(out, np.float32), tr, score

    m0, t0, s0 = trajectory(False)
    m1, t1, s1 = trajectory(True)
    np.testing.assert_array_equal(m0.view(np.uint32), m1.view(np.uint32))
    assert t0.keys() == t1.keys()
    for k in t0:
        np.testing.assert_array_equal(t0[k].view(np.uint32), t1[k].view(np.uint32), err_msg=k)
    for a, b in zip(s0, s1):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. refusals, allocation
def test_refusals_carry_their_message_and_the_context_still_trains(L):
    cfg = G.FAMILIES["tiny"]
    prompts = G.make_prompts(cfg)
    ids, cu = G.pack(prompts)
    ctx = make_ctx(L, "tiny", "bf16", 99, max_labelled=8, max_position=136)
    b0 = ctx.device_bytes()
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending tst_generate_async"):
        ctx.generate_fetch()
    for kw, msg in ((dict(max_new_tokens=0), "max_new_tokens out of range"), (dict(max_new_tokens=257), "max_new_tokens out of range"),
                    (dict(max_new_tokens=4), "more sequences than max_labelled"),                                   # 9 prompts, the head has 8 rows
                    (dict(max_new_tokens=4, eos_ids=(256,)), "eos id out of vocabulary"), (dict(max_new_tokens=4, eos_ids=(-1,)), "eos id out of vocabulary"),
                    (dict(max_new_tokens=4, eos_ids=tuple(range(17))), "more than 16 eos ids")):
        with pytest.raises(L.TstError, match=r"\(-1\).*" + msg):
            ctx.generate(ids, cu, **kw)
    ids8, cu8 = G.pack(prompts[:8])
    with pytest.raises(L.TstError, match=r"\(-1\).*out of vocabulary"):
        ctx.generate(np.where(np.arange(len(ids8)) == 3, 256, ids8).astype(np.int32), cu8, 2)
    assert ctx.device_bytes() == b0                                      # nothing refused so far has allocated the cache
    ctx.generate(ids8, cu8, 8)                                           # 125 + 8 <= 136
    ids9, cu9 = G.pack(prompts[1:])
    with pytest.raises(L.TstError, match=r"\(-1\).*exceeds max_position"):
        ctx.generate(ids9, cu9, 8)                                       # 130 + 8 > 136
    with pytest.raises(L.TstError, match=r"\(-1\).*out of vocabulary"):
        ctx.generate(np.where(np.arange(len(ids8)) == 3, 256, ids8).astype(np.int32), cu8, 2)
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending"):
        ctx.generate_fetch()                                             # a refused generation leaves nothing pending
    assert ctx.device_bytes() > b0
    bids, blab, bcu = GI.make_batch(cfg)
    loss, gn = ctx.train_step(bids, blab, bcu, 1e-3)
    assert np.isfinite(loss) and np.isfinite(gn) and loss > 0
    ctx.close()


def test_cache_is_allocated_on_first_use_and_grows_with_max_new(L):
    cfg = G.FAMILIES["tiny"]
    prompts = G.make_prompts(cfg)
    ids, cu = G.pack(prompts)
    ref_tok, _, _ = G.greedy_reference("tiny", 99)
    ctx = make_ctx(L, "tiny", "strict", 99)
    b0 = ctx.device_bytes()
    bids, blab, bcu = GI.make_batch(cfg)
    ctx.score_rows(bids, blab, bcu)
    assert ctx.device_bytes() == b0                                      # a context that never generates allocates nothing
    tok3, _, _ = ctx.generate(ids, cu, 3)
    b1 = ctx.device_bytes()
    # all layers, K and V, (max_tokens + max_seqs * max_new) rows of Hkv * dh fp32 elements, + the small row-map and output arrays
    kv = cfg["num_layers"] * 2 * (1024 + 16 * 3) * cfg["num_kv_heads"] * cfg["head_dim"] * 4
    assert kv <= b1 - b0 <= kv + (1 << 16)
    np.testing.assert_array_equal(tok3, ref_tok[:, :3])
    tok1, _, _ = ctx.generate(ids, cu, 1)
    assert ctx.device_bytes() == b1                                      # a smaller request reuses the cache
    np.testing.assert_array_equal(tok1, ref_tok[:, :1])
    tok8, _, _ = ctx.generate(ids, cu, 8)
    assert ctx.device_bytes() - b0 >= cfg["num_layers"] * 2 * (1024 + 16 * 8) * cfg["num_kv_heads"] * cfg["head_dim"] * 4
    np.testing.assert_array_equal(tok8, ref_tok)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. the diagnostic layer
def test_scoring_correct_and_gen_correct_equal_the_construction(L):
    """strict tiny, "na" samples: the answer is the oracle's own greedy continuation for the even samples, and that continuation with its SECOND token
    changed for the odd ones. Teacher-forced `correct` (every answer token is the arg-max given the reference prefix) and gen_correct (the generated
    ids start with the answer) are then both 1 on the even and 0 on the odd samples."""
    from tst import data as D
    from tst.trainer import TrainArgs, generate_heldout, score_heldout
    cfg = G.FAMILIES["tiny"]
    prompts = G.make_prompts(cfg)
    ref_tok, _, _ = G.greedy_reference("tiny", None)
    samples = []
    for i, p in enumerate(prompts):
        ans = ref_tok[i, :3].copy()
        if i % 2:
            ans[1] = (ans[1] + 1) % cfg["vocab_size"]
        samples.append(D.Sample(i, np.concatenate([p, ans]).astype(np.int32), len(p), "na", -1))
    want = [1 - i % 2 for i in range(len(samples))]
    args = TrainArgs(per_device_eval_batch_size=4, generate=True, max_new_tokens=5)
    ctx = make_ctx(L, "tiny", "strict")
    _, pred, correct = score_heldout(ctx, samples, args)
    gen = generate_heldout(ctx, samples, args)
    ctx.close()
    assert list(correct) == want and (pred == -1).all()
    assert [gc for _, gc in gen] == want
    assert [g for g, _ in gen] == [list(map(int, ref_tok[i, :5])) for i in range(len(samples))]


def test_fold_records_carry_gen_with_the_flag_and_not_without(L, tmp_path):
    """run_fold (one context) and run_fold_group (stacked contexts, the default layout): with TrainArgs.generate every record gains gen / gen_correct and
    nothing else changes -- the shards without the flag are, byte for byte, what the run with it writes minus the two keys"""
    import dataclasses
    import json
    from tst import data as D
    from tst import diagnose as DG
    from tst.trainer import TrainArgs
    cfg = G.FAMILIES["tiny"]
    samples = D.synth_vsi(40, cfg["vocab_size"], seed=3)
    args = TrainArgs(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=1e-3, logging_steps=0,
                     lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA)
    gargs = dataclasses.replace(args, generate=True, max_new_tokens=4, eos_ids=(17,))

    def make(n_stack):
        c = L.Context(cfg, max_tokens=8 * 136 * n_stack, max_seqs=8 * n_stack, max_labelled=32 * n_stack, max_position=136, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, n_stack=n_stack)
        c.load_state_dict(G.weights("tiny"))
        return c

    for n_stack, k in ((1, 2), (2, 4)):
        shards = {}
        for name, a in (("off", args), ("on", gargs)):
            root = make(n_stack)
            ctxs = [root, root.fork()] if n_stack > 1 else root
            out = str(tmp_path / f"s{n_stack}_{name}")
            recs, _ = DG.diagnose(ctxs, samples, k, a, 0, 1, 0, out)
            shards[name] = [open(DG.fold_path(out, 0, f)).read() for f in range(k)]
            if n_stack > 1:
                ctxs[1].close()
            root.close()
            assert len(recs) == len(samples)
            if name == "off":
                assert all("gen" not in r and "gen_correct" not in r for r in recs)
            else:
                by_id = {s.sid: s for s in samples}
                for r in recs:
                    assert isinstance(r["gen"], list) and len(r["gen"]) <= 4 and 17 not in r["gen"] and r["gen_correct"] in (0, 1)
                    ans = [int(t) for t in by_id[r["id"]].ids[by_id[r["id"]].n_prompt:]]
                    assert r["gen_correct"] == int(r["gen"][:len(ans)] == ans)
        for off, on in zip(shards["off"], shards["on"]):
            stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk not in ("gen", "gen_correct")}) + "\n" for line in on.splitlines())
            assert stripped == off


def test_device_resident_prompts_generate_the_same_tokens(L):
    """TST_BATCH_DEVICE_IDS: the prompt ids are read from device memory; same tokens, and an id outside the vocabulary is caught by the device-side check"""
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ids, cu = G.pack(prompts)
    ref_tok, _, _ = G.greedy_reference("tiny", 99)
    ctx = make_ctx(L, "tiny", "strict", 99)
    good = L.DevBuf(ids)
    tok, _, _ = ctx.generate(L.DeviceIds(good.ptr.value, len(ids)), cu, G.MAX_NEW)
    np.testing.assert_array_equal(tok, ref_tok)
    bad = L.DevBuf(np.where(np.arange(len(ids)) == 7, 256, ids).astype(np.int32))
    ctx.generate(L.DeviceIds(bad.ptr.value, len(ids)), cu, 2)          # asynchronous: the flag travels back behind the batch ...
    with pytest.raises(L.TstError, match="out of vocabulary"):
        ctx.sync()                                                      # ... and the next host wait reports it
    tok, _, _ = ctx.generate(ids, cu, G.MAX_NEW)
    np.testing.assert_array_equal(tok, ref_tok)
    ctx.close()
