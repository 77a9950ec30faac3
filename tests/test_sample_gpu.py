"""GPU tests of sampled generation (include/tst_hip.h tst_sample_async; csrc/decode.hip sample_rows / attn_decode_shared, engine.hip, host_logic.h plan_sample).

Reference = tests/sample_oracle.py: the pinned numpy oracle's forward_logits re-run on the growing sequences, argmax(logits / temperature + g) with the same
Philox words and float64 noise -- the definition, no cache, no device.
  1. strict (fp32) contexts are TOKEN-EXACT against it on every row, sample and step, all five families, base model and LoRA adapters, temperature 1 and 0.5,
     and |logp - oracle| <= 2 LOGIT_TOL / temperature + 1e-5. The per-case sample seeds (sample_oracle.SAMPLE_SEED) leave every draw's top-1 / top-2 gap above
     2 band = 2 (2 LOGIT_TOL / temperature + 2e-5), which tests/test_sample_cpu.py pins on the CPU.
  2. bf16 contexts are held against the library's OWN uncached path (rule 2 of tests/test_generate_gpu.py carried over): the sampled sequences are replayed
     through forward_logits of the same context (L) and through the fp32 oracle (O), E = max |L - O| is measured, and every draw satisfies
     L[tok] / t + g[tok] >= max(L / t + g) - 2 E / t - 2e-5 and |logp - log_softmax(L / t)[tok]| <= 4 E / t. Two runs give bit-identical tokens and logp.
  3. stacked contexts: every row obeys rule 2 under its own slot's adapters, and the other slot's adapters break the band.
  4. coverage: the samples of a prompt differ; the first-token frequencies of 512 draws of one prompt follow softmax(O / t) (chi-square).
  5. the eos cut per (s, i), 6. no side effects, 7. refusals, 8. the diagnostic layer."""
import numpy as np
import pytest

import generate_oracle as G
import golden_inputs as GI
import sample_oracle as SO

pytestmark = pytest.mark.gpu

LOGIT_TOL = SO.LOGIT_TOL
TAGS = list(G.FAMILIES)
N = SO.N_SAMPLES


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def make_ctx(L, tag, precision, lora_seed=None, mode="lora", n_stack=1, max_seqs=64, max_labelled=512, max_position=256, max_tokens=4096):
    cfg = G.FAMILIES[tag]
    ctx = L.Context(cfg, max_tokens=max_tokens, max_seqs=max_seqs, max_labelled=max_labelled,
                    max_position=cfg["max_position"] if cfg.get("arch") == "gpt2" else max_position, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode,
                    precision=precision, n_stack=n_stack)
    ctx.load_state_dict(G.weights(tag))
    if lora_seed is not None:
        ctx.set_trainable(G.lora(tag, lora_seed))
    return ctx


def noise_of(seeds, n, max_new, V):
    """g [S, n, max_new, V] float64"""
    return np.stack([np.stack([np.stack([SO.gumbel(seed, V, j, i) for j in range(max_new)]) for i in range(n)]) for seed in seeds])


def check_band(name, ctx, orc, prompts, tokens, logp, seeds, temperature, seq_slot=None):
    """rule 2 of the module docstring for the draws `tokens` [S, n, max_new] of `prompts`; returns E"""
    S, n, m = tokens.shape
    ids, cu, rows = SO.replay_rows(prompts, tokens)
    slots = None if seq_slot is None else np.repeat(seq_slot, n).astype(np.int32)
    Lg = ctx.forward_logits(ids, cu, rows, seq_slot=slots).astype(np.float64)
    Og = np.asarray(orc.forward_logits(ids, cu, rows), np.float64)
    E = float(np.abs(Lg - Og).max())
    V = Lg.shape[-1]
    sc = Lg / temperature + noise_of(seeds, n, m, V).reshape(-1, V)
    tok = tokens.reshape(-1)
    at_tok = sc[np.arange(len(tok)), tok]
    short = float((sc.max(-1) - at_tok).max())
    d_logp = float(np.abs(logp.reshape(-1) - G.log_softmax(Lg / temperature)[np.arange(len(tok)), tok]).max())
    print(f"{name}: E = {E:.3e}  max(score) - score[tok] <= {short:.3e}  |d logp| <= {d_logp:.3e}  draws that are not the replay's arg-max: "
          f"{int((sc.argmax(-1) != tok).sum())}/{len(tok)}")
    assert (at_tok >= sc.max(-1) - 2 * E / temperature - 2e-5).all(), f"{name}: a draw lies {short:.3e} under the replay's best score, E = {E:.3e}"
    assert d_logp <= 4 * E / temperature, f"{name}: logp off the replay's by {d_logp:.3e}, E = {E:.3e}"
    return E


# ------------------------------------------------------------------------------------------------ 1. strict: token-exact
@pytest.mark.parametrize("temperature", SO.TEMPERATURES)
@pytest.mark.parametrize("lora_seed", SO.ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_strict_sampling_is_token_exact(L, tag, lora_seed, temperature):
    prompts = G.make_prompts(G.FAMILIES[tag])
    ref_tok, ref_logp, gap, seeds = SO.sampled_reference(tag, lora_seed, temperature)
    ctx = make_ctx(L, tag, "strict", lora_seed)
    tok, logp, n_new = ctx.sample(*G.pack(prompts), G.MAX_NEW, N, temperature, seeds)
    ctx.close()
    d = float(np.abs(logp - ref_logp).max())
    print(f"strict[{tag}, {lora_seed}, T={temperature}]: draws equal {int((tok == ref_tok).sum())}/{tok.size}  |d logp| max = {d:.3e}  smallest gap {gap.min():.3e}")
    assert tok.shape == (len(prompts), N, G.MAX_NEW)
    np.testing.assert_array_equal(tok, ref_tok)
    assert d <= 2 * LOGIT_TOL / temperature + 1e-5
    assert (n_new == G.MAX_NEW).all()


def test_strict_full_finetune_context_samples(L):
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ref_tok, ref_logp, _, seeds = SO.sampled_reference("tiny", None, 1.0)
    ctx = make_ctx(L, "tiny", "strict", mode="full")
    tok, logp, _ = ctx.sample(*G.pack(prompts), G.MAX_NEW, N, 1.0, seeds)
    ctx.close()
    np.testing.assert_array_equal(tok, ref_tok)
    assert float(np.abs(logp - ref_logp).max()) <= 2 * LOGIT_TOL + 1e-5


def test_a_prompts_draws_do_not_depend_on_its_batch(L):
    """a prompt's draws are a function of its logits, its seed, the step and the sample index: alone, reversed in the batch, or with fewer samples -- the same
    draws (strict: the oracle's, whose gaps are far above what a change of batch geometry moves)"""
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ref_tok, _, _, seeds = SO.sampled_reference("tiny", 99, 1.0)
    ctx = make_ctx(L, "tiny", "strict", 99)
    tok_rev, _, _ = ctx.sample(*G.pack(prompts[::-1]), G.MAX_NEW, N, 1.0, seeds[::-1])
    tok_one, _, _ = ctx.sample(*G.pack(prompts[4:5]), G.MAX_NEW, N, 1.0, seeds[4:5])
    tok_two, _, _ = ctx.sample(*G.pack(prompts), G.MAX_NEW, 2, 1.0, seeds)
    ctx.close()
    np.testing.assert_array_equal(tok_rev[::-1], ref_tok)
    np.testing.assert_array_equal(tok_one[0], ref_tok[4])
    np.testing.assert_array_equal(tok_two, ref_tok[:, :2])


# ------------------------------------------------------------------------------------------------ 2. bf16: against the library's own uncached path
@pytest.mark.parametrize("temperature", SO.TEMPERATURES)
@pytest.mark.parametrize("lora_seed", SO.ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", TAGS)
def test_bf16_sampling_stays_inside_the_uncached_paths_error(L, tag, lora_seed, temperature):
    prompts = G.make_prompts(G.FAMILIES[tag])
    seeds = SO.prompt_seeds(SO.case_seed(tag, lora_seed, temperature), len(prompts))
    ctx = make_ctx(L, tag, "bf16", lora_seed)
    ids, cu = G.pack(prompts)
    tok, logp, n_new = ctx.sample(ids, cu, G.MAX_NEW, N, temperature, seeds)
    assert tok.min() >= 0 and tok.max() < G.FAMILIES[tag]["vocab_size"] and (n_new == G.MAX_NEW).all() and np.isfinite(logp).all()
    if temperature == 1.0:   # the draws of one prompt differ somewhere in the batch
        assert any(len({tuple(tok[s, i]) for i in range(N)}) > 1 for s in range(len(prompts)))
    check_band(f"bf16[{tag}, {lora_seed}, T={temperature}]", ctx, G.make_oracle(tag, lora_seed), prompts, tok, logp, seeds, temperature)
    tok2, logp2, _ = ctx.sample(ids, cu, G.MAX_NEW, N, temperature, seeds)
    ctx.close()
    np.testing.assert_array_equal(tok2, tok)
    np.testing.assert_array_equal(logp2.view(np.uint32), logp.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. stacked
def test_stacked_slots_sample_under_their_own_adapters(L):
    tag, adapters, temperature = "tiny", (99, 100), 1.0
    prompts = G.make_prompts(G.FAMILIES[tag])
    slots = np.array([0] * 5 + [1] * 4, np.int32)
    seeds = SO.prompt_seeds(3, len(prompts))
    ctx = make_ctx(L, tag, "bf16", n_stack=2)
    for sl, a in enumerate(adapters):
        ctx.select_slot(sl)
        ctx.set_trainable(G.lora(tag, a))
    tok, logp, _ = ctx.sample(*G.pack(prompts), G.MAX_NEW, N, temperature, seeds, seq_slot=slots)
    E = 0.0
    for sl, a in enumerate(adapters):
        mine = np.flatnonzero(slots == sl)
        E = max(E, check_band(f"stacked slot {sl}", ctx, G.make_oracle(tag, a), [prompts[i] for i in mine], tok[mine], logp[mine], seeds[mine], temperature,
                              seq_slot=np.full(len(mine), sl, np.int32)))
    ctx.close()
    # the inputs discriminate, from the oracle alone: the oracle's draws under one adapter set, judged with the logits of the OTHER set, leave the band on every
    # prompt by more than the measured error could hide (a GPU score is within E / t of the oracle's: 4 E / t under the oracle's best is more than 2 E / t under
    # the GPU's)
    g = noise_of(seeds, N, G.MAX_NEW, G.FAMILIES[tag]["vocab_size"])
    for a, b in ((99, 100), (100, 99)):
        ref_tok, _, _ = SO.sampled(G.make_oracle(tag, a), prompts, N, temperature, seeds)
        rid, rcu, rows = SO.replay_rows(prompts, ref_tok)
        sc = np.asarray(G.make_oracle(tag, b).forward_logits(rid, rcu, rows), np.float64).reshape(len(prompts), N, G.MAX_NEW, -1) / temperature + g
        under = sc.max(-1) - np.take_along_axis(sc, ref_tok[..., None].astype(np.int64), -1)[..., 0]
        broke = (under > 4 * E / temperature + 2e-5).any((-1, -2))
        print(f"adapters {a} judged under {b}: {int(broke.sum())}/9 prompts break the band (E = {E:.3e}); smallest worst-draw deficit {float(under.max((-1, -2)).min()):.3e}")
        assert broke.all()


# ------------------------------------------------------------------------------------------------ 4. coverage
def test_samples_differ_and_first_tokens_follow_the_models_distribution(L):
    tag, temperature = "tiny", 1.0
    prompts = G.make_prompts(G.FAMILIES[tag])
    ref_tok, _, _, seeds = SO.sampled_reference(tag, None, temperature)
    assert any(len({tuple(ref_tok[s, i]) for i in range(N)}) > 1 for s in range(len(prompts)))   # (token-exact on the GPU: test 1)
    # 512 first tokens of ONE prompt in one call: the prompt 8 times under 8 seeds, 64 samples each
    p = prompts[SO.COVER_PROMPT]
    seeds8 = SO.cover_seeds()
    ctx = make_ctx(L, tag, "strict", max_seqs=512, max_labelled=512)
    tok, _, _ = ctx.sample(*G.pack([p] * SO.COVER_SEEDS), 1, 64, temperature, seeds8)
    ctx.close()
    ids, cu = G.pack([p])
    O = np.asarray(G.make_oracle(tag).forward_logits(ids, cu, cu[1:] - 1), np.float64)[0]
    probs = np.exp(G.log_softmax(O / temperature))
    counts = np.bincount(tok.reshape(-1), minlength=len(probs))
    chi2 = SO.first_token_chi2(counts, probs, tok.size)
    print(f"first-token chi-square of {tok.size} draws over the oracle's 8 likeliest tokens + rest: {chi2:.2f} (8 degrees of freedom; 43.3 is p = 1e-6)")
    assert tok.size == 512 and len(set(map(int, tok.reshape(-1)))) > 8
    assert chi2 < 43.3


# ------------------------------------------------------------------------------------------------ 5. EOS
def test_eos_cuts_a_draw_and_leaves_its_neighbours_alone(L):
    prompts = G.make_prompts(G.FAMILIES["tiny"])
    ref_tok, _, _, seeds = SO.sampled_reference("tiny", None, 1.0)
    eos = int(ref_tok[3, 1, 2])                      # the third token of draw 1 of prompt 3: that draw ends there (or earlier), most others run on
    ctx = make_ctx(L, "tiny", "strict")
    ids, cu = G.pack(prompts)
    tok0, logp0, n0 = ctx.sample(ids, cu, G.MAX_NEW, N, 1.0, seeds)
    tok, logp, n_new = ctx.sample(ids, cu, G.MAX_NEW, N, 1.0, seeds, eos_ids=(eos,))
    ctx.close()
    assert (n0 == G.MAX_NEW).all()
    S = len(prompts)
    want_tok, want_logp, want_n = L.host_cut_at_eos(tok0.reshape(S * N, -1), logp0.reshape(S * N, -1), (eos,))
    assert n_new[3, 1] <= 3 and (tok[3, 1, n_new[3, 1]:] == -1).all() and (logp[3, 1, n_new[3, 1]:] == 0).all() and tok[3, 1, n_new[3, 1] - 1] == eos
    assert (n_new == G.MAX_NEW).sum() >= S * N // 2, "the eos id cuts most draws: the neighbours are not tested"
    np.testing.assert_array_equal(tok.reshape(S * N, -1), want_tok)
    np.testing.assert_array_equal(logp.reshape(S * N, -1).view(np.uint32), want_logp.view(np.uint32))
    np.testing.assert_array_equal(n_new.reshape(-1), want_n)


# ------------------------------------------------------------------------------------------------ 6. no side effects
def test_sampling_leaves_training_accumulation_pending_scores_and_greedy_generation_alone(L):
    cfg = G.FAMILIES["tiny"]
    ids, labels, cu = GI.make_batch(cfg)
    ids2, labels2, cu2 = GI.make_batch(cfg, lengths=(33, 70), n_answer=(4, 1), seed=11)
    prompts = G.make_prompts(cfg)
    pid, pcu = G.pack(prompts)
    seeds = SO.prompt_seeds(0, len(prompts))

    def trajectory(with_sample):
        ctx = make_ctx(L, "tiny", "bf16", 99)
        out = []
        for step in range(4):
            if with_sample and step == 2:
                ctx.sample(pid, pcu, G.MAX_NEW, N, 1.0, seeds)
            out.append(ctx.train_step(ids if step % 2 == 0 else ids2, labels if step % 2 == 0 else labels2, cu if step % 2 == 0 else cu2, 1e-3))
        ctx.accumulate_async(ids, labels, cu, 11, True)   # an accumulation window with a sampled generation inside it
        if with_sample:
            ctx.sample_async(pid, pcu, 3, 2, 0.5, seeds)
        ctx.accumulate_async(ids2, labels2, cu2, 11, False)
        ctx.optimizer_step_async([1e-3])
        out.append(ctx.fetch_metrics())
        if with_sample:
            ctx.sample_fetch()
        ctx.score_rows_async(ids, labels, cu, [3, 9, 27, 81])   # a pending scoring pass fetched after a sampled generation
        if with_sample:
            ctx.sample(pid, pcu, G.MAX_NEW, N, 1.0, seeds)
        score = ctx.score_rows_fetch()
        greedy = ctx.generate(pid, pcu, G.MAX_NEW)           # greedy generation behind a sampled one: the shared cache and buffers carry nothing over
        if with_sample:
            ctx.sample(pid, pcu, 5, N, 1.0, seeds)
            again = ctx.generate(pid, pcu, G.MAX_NEW)
            for a, b in zip(greedy, again):
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        tr = ctx.get_trainable()
        ctx.close()
        return np.array(out, np.float32), tr, score, greedy

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


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_carry_their_message_and_allocate_nothing(L):
    cfg = G.FAMILIES["tiny"]
    prompts = G.make_prompts(cfg)
    ids, cu = G.pack(prompts)
    seeds = SO.prompt_seeds(0, len(prompts))
    ctx = make_ctx(L, "tiny", "bf16", 99, max_seqs=40, max_labelled=36, max_position=136)
    b0 = ctx.device_bytes()
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending tst_sample_async"):
        ctx.sample_fetch()
    ok = dict(max_new_tokens=4, n_samples=4, temperature=1.0)
    for kw, msg in ((dict(ok, max_new_tokens=0), "max_new_tokens out of range"), (dict(ok, max_new_tokens=257), "max_new_tokens out of range"),
                    (dict(ok, n_samples=0), "n_samples out of range"), (dict(ok, n_samples=65), "n_samples out of range"),
                    (dict(ok, n_samples=5), "n_seqs \\* n_samples exceeds"),                                         # 45 rows: over max_seqs and max_labelled
                    (dict(ok, temperature=0.0), "temperature must be finite"), (dict(ok, temperature=0.009), "temperature must be finite"),
                    (dict(ok, temperature=101.0), "temperature must be finite"), (dict(ok, temperature=float("nan")), "temperature must be finite"),
                    (dict(ok, temperature=float("inf")), "temperature must be finite"),
                    (dict(ok, eos_ids=(256,)), "eos id out of vocabulary"), (dict(ok, eos_ids=tuple(range(17))), "more than 16 eos ids")):
        with pytest.raises(L.TstError, match=r"\(-1\).*" + msg):
            ctx.sample(ids, cu, seq_seeds=seeds, **kw)
    with pytest.raises(L.TstError, match=r"\(-1\).*exceeds max_position"):
        ctx.sample(ids, cu, seq_seeds=seeds, **dict(ok, max_new_tokens=8))                                          # 130 + 8 > 136
    with pytest.raises(L.TstError, match=r"\(-1\).*out of vocabulary"):
        ctx.sample(np.where(np.arange(len(ids)) == 3, 256, ids).astype(np.int32), cu, seq_seeds=seeds, **ok)
    import ctypes as C
    b, _keep = ctx._batch(ids, None, cu)
    assert ctx.lib.tst_sample_async(ctx.h, C.byref(b), 4, 4, 1.0, None, None, 0) == -1                              # seq_seeds NULL
    assert b"seq_seeds" in ctx.lib.tst_last_error(ctx.h)
    # a context whose max_seqs and max_labelled exceed its max_tokens: the draws fit both, but a decode step would run more token rows than the activations hold
    wide = make_ctx(L, "tiny", "bf16", max_tokens=64, max_seqs=128, max_labelled=128, max_position=136)
    w0 = wide.device_bytes()
    sid, scu = G.pack([prompts[1][:4], prompts[2][:4]])
    with pytest.raises(L.TstError, match=r"\(-1\).*n_seqs \* n_samples exceeds max_tokens"):
        wide.sample(sid, scu, 4, 64, 1.0, seeds[:2])
    with pytest.raises(L.TstError, match=r"\(-1\).*n_seqs \* n_samples exceeds max_tokens"):
        wide.sample(sid, scu, 4, 33, 1.0, seeds[:2])
    assert wide.device_bytes() == w0
    wtok, _, _ = wide.sample(sid, scu, 4, 32, 1.0, seeds[:2])             # 64 rows = max_tokens: the largest call this context runs
    assert wtok.shape == (2, 32, 4) and wtok.min() >= 0 and wtok.max() < cfg["vocab_size"]
    wide.close()
    assert ctx.device_bytes() == b0                                      # nothing refused so far has allocated the cache
    # the two kinds share the one pending slot: a fetch of the other kind is refused and leaves the pending call fetchable
    ctx.sample_async(ids, cu, seq_seeds=seeds, **ok)
    with pytest.raises(L.TstError, match=r"\(-4\).*pending generation is a tst_sample_async"):
        ctx.generate_fetch()
    tok, logp, n_new = ctx.sample_fetch()
    assert tok.shape == (9, 4, 4) and tok.min() >= 0 and np.isfinite(logp).all()
    ctx.generate_async(ids, cu, 4)
    with pytest.raises(L.TstError, match=r"\(-4\).*pending generation is a tst_generate_async"):
        ctx.sample_fetch()
    gtok, _, _ = ctx.generate_fetch()
    assert gtok.shape == (9, 4)
    with pytest.raises(L.TstError, match=r"\(-4\).*without a pending"):
        ctx.sample_fetch()
    b1 = ctx.device_bytes()
    assert b1 > b0
    with pytest.raises(L.TstError, match=r"\(-1\).*n_samples out of range"):
        ctx.sample(ids, cu, seq_seeds=seeds, **dict(ok, n_samples=65))
    assert ctx.device_bytes() == b1
    bids, blab, bcu = GI.make_batch(cfg)
    loss, gn = ctx.train_step(bids, blab, bcu, 1e-3)
    assert np.isfinite(loss) and np.isfinite(gn) and loss > 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. the diagnostic layer
def test_fold_records_carry_samples_with_the_flag_and_not_without(L, tmp_path):
    """diagnose on the tiny model in its three single-GPU layouts: one context (run_fold), two forked contexts at once (run_fold_group, concurrent) and a
    2-slot stacked context with a fork (run_fold_group, stacked). With TrainArgs.sample_n every record gains `samples` and nothing else changes -- the shards
    without the flag are, byte for byte, what the run with it writes minus that key, and the fingerprint of a run without it does not know the three settings.
    The adapters are trained at learning rate 0 (they stay at their initial values, B = 0), so every layout holds the same model, and the same sample seed must
    give every QA pair the same draws in the one-context and the concurrent layout, which run in strict precision. (The library refuses a stacked context in
    strict precision -- stacked folds are a bf16-path feature -- so the stacked layout runs in bf16, where a near-tie may fall either way: it is held to the
    record format and the byte-for-byte rule, and the draws' independence of stacking is test 3's.)"""
    import dataclasses
    import json
    from tst import data as D
    from tst import diagnose as DG
    from tst.trainer import TrainArgs
    cfg = G.FAMILIES["tiny"]
    samples = D.synth_vsi(24, cfg["vocab_size"], seed=3)
    args = TrainArgs(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=0.0, logging_steps=0,
                     lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, max_new_tokens=4, eos_ids=(17,))
    fields = dataclasses.asdict(args)
    sargs = TrainArgs(**fields, sample_n=4, temperature=0.8, sample_seed=5)
    assert DG.run_fingerprint(samples, 2, args) == DG.run_fingerprint(samples, 2, TrainArgs(**fields, temperature=0.3, sample_seed=9))
    assert DG.run_fingerprint(samples, 2, args) == DG.run_fingerprint(samples, 2, dataclasses.replace(args, max_new_tokens=8, eos_ids=()))
    assert len({DG.run_fingerprint(samples, 2, a) for a in (args, sargs, TrainArgs(**fields, sample_n=4, temperature=0.8, sample_seed=6),
                                                            TrainArgs(**dict(fields, max_new_tokens=5), sample_n=4, temperature=0.8, sample_seed=5))}) == 4

    def make(n_stack, precision):
        c = L.Context(cfg, max_tokens=8 * 136 * n_stack, max_seqs=32 * n_stack, max_labelled=32 * n_stack, max_position=136, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, n_stack=n_stack, precision=precision)
        c.load_state_dict(G.weights("tiny"))
        return c

    by_layout = {}
    for layout, n_stack, forks, k, precision in (("one", 1, 0, 2, "strict"), ("concurrent", 1, 1, 4, "strict"), ("stacked", 2, 1, 4, "bf16")):
        shards = {}
        for name, a in (("off", args), ("on", sargs)):
            root = make(n_stack, precision)
            ctxs = [root] + [root.fork() for _ in range(forks)]
            out = str(tmp_path / f"{layout}_{name}")
            recs, _ = DG.diagnose(ctxs if forks else root, samples, k, a, 0, 1, 0, out)
            shards[name] = [open(DG.fold_path(out, 0, f)).read() for f in range(k)]
            for c in ctxs[1:]:
                c.close()
            root.close()
            assert len(recs) == len(samples)
            if name == "off":
                assert all("samples" not in r for r in recs)
            else:
                by_id = {s.sid: s for s in samples}
                for r in recs:
                    sm = r["samples"]
                    assert set(sm) == {"ids", "logp", "match"} and len(sm["ids"]) == len(sm["logp"]) == 4
                    assert all(len(g) <= 4 and 17 not in g for g in sm["ids"]) and all(v <= 0 for v in sm["logp"])
                    ans = [int(t) for t in by_id[r["id"]].ids[by_id[r["id"]].n_prompt:]]
                    assert sm["match"] == sum(g[:len(ans)] == ans for g in sm["ids"]) / 4
                by_layout[layout] = {r["id"]: r["samples"] for r in recs}
        for off, on in zip(shards["off"], shards["on"]):
            stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk != "samples"}) + "\n" for line in on.splitlines())
            assert stripped == off
    assert by_layout["one"].keys() == by_layout["concurrent"].keys() == by_layout["stacked"].keys()
    for sid, sm in by_layout["one"].items():
        assert sm["ids"] == by_layout["concurrent"][sid]["ids"], f"QA pair {sid}: the draws depend on the fold layout"
        np.testing.assert_allclose(sm["logp"], by_layout["concurrent"][sid]["logp"], atol=4 * (2 * LOGIT_TOL / 0.8 + 1e-5), rtol=0)   # four tokens, each inside test 1's bound
    assert len({tuple(map(tuple, sm["ids"])) for sm in by_layout["one"].values()}) > len(samples) // 2
