"""GPU tests of token attribution (include/tst_hip.h tst_attribute_async; csrc/attribute.hip, engine.hip, host_logic.h).

Reference = tests/golden/attr_<tag>.npz (tools/make_golden.py attr): gradient x input and gradient norm of J = sum_i log s(x_i) with respect to the
embedding-layer output, from the HF model fed inputs_embeds with requires_grad, in fp64 (`ref`), fp32 and bf16 (`floor32` / `floor16` = the distance of HF's own
fp32 / bf16 runs from `ref`, per output the max over sequences of max_t |x - ref| / max_t |ref|).
  1. the two kernels on their own, through the lab hooks, against float64 numpy.
  2. strict (fp32) contexts: per sequence, both outputs, both fixture sets, max_t |x - ref| / max_t |ref| <= SX_TOL = 1e-3 (the project's bound on s(x), of which
     the attribution is the derivative; a missing term is an O(1) error), and |logs - log s(x)| <= 2 LOGIT_TOL with s(x) from Context.score_rows + bias_scores.
  3. bf16 contexts: per tag and output the same deviation is <= 2 x floor16 of the tag (two independent bf16 roundings of the same path can at worst add).
     floor16 of a tag = the largest of the fixture's floor16 entries of that output (two sets x three adapter sets): gradient x input cancels under bf16, which
     hits single sequences haphazardly (tiny2: 0.11 ... 0.49 over the six entries), so one entry is one draw of the noise and the tag's floor is the worst draw.
     Also with last_compact, trim_last_token, norm_rank and swiglu_rank each switched off in turn, and two runs are bit-identical.
     Measured on an MI355X (worst deviation / tag floor16, gxi | gnorm): tiny 2.20 | 0.33, tiny2 0.21 | 0.40, qwen 0.56 | 0.68, qwen3 0.84 | 0.78,
     gpt2 0.25 | 1.18. tiny exceeds 2 x on ONE figure: gxi of the 7-token sequence, open form, base model, 0.192 against a floor of 0.088. Chased: on that
     sequence max_t sum_d |g e| / max_t |gxi| = 339, i.e. gradient x input cancels 339-fold and one bf16 rounding (2^-8) of the products is 1.3 x the
     result's scale; HF's OWN bf16 model lands 0.077 from `ref` with its eager attention (the stored floor) and 0.181 with its sdpa attention -- a second
     draw of the same noise, as far out as this library's 0.192. No term is missing (the strict context agrees with `ref` to 1e-5 on the same sequence).
     So tiny takes the factor 3 the feature's specification allows for such a tag, BF16_FACTOR below, with the per-tag table in DESIGN.md section 13;
     every other tag keeps 2.
  4. stacked context: every sequence meets rule 3 against the fixture of its own slot's adapters and misses it against the other slot's. Output used: gnorm, on
     all four sequences -- the fixtures of adapters 99 and 7 differ there by 0.10 ... 0.90 on every sequence of every tag, more than 4 x floor16 (<= 0.25), so a
     result within 2 x floor16 of one cannot be within 2 x floor16 of the other (test_attribution_cpu.py asserts that from the fixtures).
  5. batch independence, 6. no side effects, 7. refusals, 8. the diagnostic layer."""
import types

import numpy as np
import pytest

import attribution_inputs as AI
import golden_inputs as GI

pytestmark = pytest.mark.gpu

SX_TOL = 1e-3      # tests/test_strict_gpu.py: the project's bound on s(x)
LOGIT_TOL = 1e-4   # tests/test_strict_gpu.py: one strict logit
TAGS = list(AI.TAGS)
BF16_FACTOR = dict(tiny=3.0)   # rule 3 of the module docstring: 2 unless a tag is listed here with its measurement
TST_EINVAL, TST_ESTATE = -1, -4


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


_GOLD = {}


def gold(golden_dir, tag):
    if tag not in _GOLD:
        _GOLD[tag] = dict(np.load(f"{golden_dir}/attr_{tag}.npz"))
    return _GOLD[tag]


def tag_floor16(g):
    """per output, the tag's floor16 (module docstring, rule 3)"""
    return np.max([g[f"{s}/{a}/floor16"] for s in AI.SETS for a in AI.ADAPTERS], axis=0)


def make_ctx(L, tag, precision, adapter="base", mode="lora", n_stack=1, max_tokens=1024):
    cfg = AI.TAGS[tag][0]
    ctx = L.Context(cfg, max_tokens=max_tokens, max_seqs=16, max_labelled=64, max_position=cfg["max_position"] if cfg.get("arch") == "gpt2" else 256,
                    lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode, precision=precision, n_stack=n_stack)
    ctx.load_state_dict(AI.TAGS[tag][1](cfg))
    if mode == "lora" and n_stack == 1:
        ctx.set_trainable(AI.zero_lora(tag) if AI.ADAPTERS[adapter] is None else AI.lora(tag, AI.ADAPTERS[adapter]))
    return ctx


def attribute(ctx, tag, sname, **kw):
    ids, labels, cu = AI.batch(tag)
    return ctx.attribute(ids, labels, cu, seq_kind=AI.SETS[sname], option_ids=AI.option_ids(tag), **kw)


def deviations(got, g, key, cu):
    """[output][sequence] max_t |x - ref| / max_t |ref|"""
    return np.stack([AI.seq_dev(got[i], g[f"{key}ref_{o}"], cu) for i, o in enumerate(AI.OUTPUTS)])


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [128, 256, 4096])
@pytest.mark.parametrize("T", [1, 3, 64, 257])
def test_token_attr_kernel(L, T, d, f32):
    lab = L.load_lab()
    rng = np.random.default_rng(T * 10007 + d)
    g, e = rng.standard_normal((T, d)).astype(np.float32), rng.standard_normal((T, d)).astype(np.float32)
    if not f32:
        g, e = GI.bf16_round(g), GI.bf16_round(e)
    g_, e_ = (L.dev_f32(g), L.dev_f32(e)) if f32 else (L.dev_bf16(g), L.dev_bf16(e))
    fn = lab.tst_k_token_attr_f32 if f32 else lab.tst_k_token_attr
    outs = []
    for _ in range(2):
        x_, n_ = L.DevBuf(nbytes=4 * T), L.DevBuf(nbytes=4 * T)
        assert fn(g_.ptr, e_.ptr, T, d, x_.ptr, n_.ptr) == 0
        outs.append((x_.get(np.float32, (T,)), n_.get(np.float32, (T,))))
    g64, e64 = g.astype(np.float64), e.astype(np.float64)
    ref_x, ref_n2 = (g64 * e64).sum(-1), (g64 * g64).sum(-1)
    bound = d * 2.0 ** -23
    err_x = np.abs(outs[0][0] - ref_x) / np.abs(g64 * e64).sum(-1)
    err_n = np.abs(outs[0][1].astype(np.float64) ** 2 - ref_n2) / ref_n2
    print(f"token_attr T={T} d={d} f32={f32}: gxi err / sum|g e| <= {err_x.max():.3e}, gnorm^2 rel err <= {err_n.max():.3e}, bound {bound:.3e}")
    assert (err_x <= bound).all() and (err_n <= bound).all()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert lab.tst_k_token_attr(g_.ptr, e_.ptr, T, d + 4, x_.ptr, n_.ptr) == TST_EINVAL   # d must be a multiple of 8


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,Vp", [(256, 256), (1001, 1024), (128256, 128256)])
@pytest.mark.parametrize("R", [1, 5])
def test_attr_seed_kernel(L, R, V, Vp, f32):
    lab = L.load_lab()
    rng = np.random.default_rng(R * 7919 + V)
    z = np.zeros((R, Vp), np.float32)
    z[:, :V] = (3.0 * rng.standard_normal((R, V))).astype(np.float32)
    z[:, V:] = 1e30   # the padding of the logits must never be read as a logit
    opt = rng.choice(V, 6, replace=False).astype(np.int32)
    opt[5] = opt[1]   # an id listed twice counts twice
    kind = (np.arange(R) % 2 == 0).astype(np.int32)   # option and open rows mixed (R = 1: one option row)
    tgt = np.where(kind == 1, opt[rng.integers(0, 6, R)], rng.integers(0, V, R)).astype(np.int32)
    w = (1.0 / rng.integers(1, 5, R)).astype(np.float32)
    z64, ref = z[:, :V].astype(np.float64), np.zeros((R, Vp))
    lse = np.log(np.exp(z64 - z64.max(-1, keepdims=True)).sum(-1)) + z64.max(-1)
    olse = np.zeros(R)
    for r in range(R):
        if kind[r]:
            zo = z64[r, opt]
            olse[r] = np.log(np.exp(zo - zo.max()).sum()) + zo.max()
            np.add.at(ref[r], opt, -np.exp(zo - olse[r]))
        else:
            ref[r, :V] = -np.exp(z64[r] - lse[r])
        ref[r, tgt[r]] += 1.0
        ref[r] *= w[r]
    z_, t_, w_, k_, o_ = L.dev_f32(z), L.DevBuf(tgt), L.dev_f32(w), L.DevBuf(kind), L.DevBuf(opt)
    st_ = L.DevBuf(nbytes=16 * R)
    garbage = np.full((R, Vp), 7.0, np.float32)   # every element of the padded row must be written
    dl_ = L.dev_f32(garbage) if f32 else L.dev_bf16(garbage)
    fn = lab.tst_k_attr_seed_f32 if f32 else lab.tst_k_attr_seed
    assert fn(z_.ptr, Vp, t_.ptr, w_.ptr, k_.ptr, o_.ptr, 6, R, V, Vp, st_.ptr, dl_.ptr, Vp) == 0
    got = (dl_.get(np.float32, (R, Vp)) if f32 else dl_.get_bf16((R, Vp))).astype(np.float64)
    st = st_.get(np.float32, (R, 4))
    err = np.abs(got - ref)
    print(f"attr_seed R={R} V={V}/{Vp} f32={f32}: max |dlogits - ref| = {err.max():.3e}")
    if f32:
        assert err.max() <= 1e-6
    else:
        assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-7).all()
    assert (got[:, V:] == 0).all()
    for r in np.flatnonzero(kind):
        other = np.ones(Vp, bool)
        other[opt] = False
        assert (got[r, other] == 0).all()
        assert abs(st[r, 2] - olse[r]) <= 1e-5
    assert np.abs(st[:, 0] - lse).max() <= 1e-5 and (st[:, 1] == z[np.arange(R), tgt]).all()


# ------------------------------------------------------------------------------------------------ 2. strict contexts vs ref
STRICT_CASES = [(t, a, "lora") for t in TAGS for a in ("base", "l99")] + [("tiny", "base", "full")]


@pytest.mark.parametrize("tag,adapter,mode", STRICT_CASES, ids=[f"{t}-{a}-{m}" for t, a, m in STRICT_CASES])
def test_strict_attribution_matches_the_reference(L, golden_dir, tag, adapter, mode):
    from tst import score as S
    g = gold(golden_dir, tag)
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    ctx = make_ctx(L, tag, "strict", adapter, mode)
    for sname, kinds in AI.SETS.items():
        key = f"{sname}/{adapter}/"
        gxi, gnorm, logs = attribute(ctx, tag, sname)
        dev = deviations((gxi, gnorm), g, key, cu)
        print(f"strict[{tag}, {adapter}, {mode}, {sname}]: gxi dev per sequence {dev[0]}, gnorm {dev[1]}; floor32 {g[key + 'floor32']}")
        assert dev.max() <= SX_TOL
        # log s(x) from the scoring pass on the same batch
        samples = []
        for s in range(len(cu) - 1):
            lab = labels[cu[s]:cu[s + 1]]
            n_ans = int((lab != -100).sum())
            samples.append(types.SimpleNamespace(sid=s, kind="mca" if kinds[s] else "open", n_answer=n_ans,
                                                 gt_option=int(np.flatnonzero(opt == lab[-1])[0]) if kinds[s] else -1))
        sx, _, _ = S.bias_scores(samples, *ctx.score_rows(ids, labels, cu, opt))
        d_logs = np.abs(logs - np.log(sx.astype(np.float64)))
        print(f"  logs {logs}  |logs - log s(x)| <= {d_logs.max():.3e}  |logs - ref| <= {np.abs(logs - g[key + 'ref_logs']).max():.3e}")
        assert d_logs.max() <= 2 * LOGIT_TOL
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. bf16 contexts vs ref
@pytest.mark.parametrize("adapter", ["base", "l99"])
@pytest.mark.parametrize("tag", TAGS)
def test_bf16_attribution_stays_within_twice_the_bf16_floor(L, golden_dir, tag, adapter):
    g = gold(golden_dir, tag)
    cu = AI.batch(tag)[2]
    floor = tag_floor16(g)
    ctx = make_ctx(L, tag, "bf16", adapter)
    worst = np.zeros(2)
    for sname in AI.SETS:
        got = attribute(ctx, tag, sname)
        dev = deviations(got, g, f"{sname}/{adapter}/", cu)
        worst = np.maximum(worst, dev.max(1))
        print(f"bf16[{tag}, {adapter}, {sname}]: gxi dev per sequence {dev[0]}, gnorm {dev[1]}; this entry's floor16 {g[f'{sname}/{adapter}/floor16']}")
        again = attribute(ctx, tag, sname)
        for a, b in zip(got, again):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    ctx.close()
    print(f"bf16[{tag}, {adapter}]: worst deviation gxi {worst[0]:.4f} gnorm {worst[1]:.4f}; tag floor16 {floor}; ratio {worst / floor}")
    assert (worst <= BF16_FACTOR.get(tag, 2.0) * floor).all()


@pytest.mark.parametrize("tag", TAGS)
def test_bf16_attribution_with_each_engine_option_off(L, golden_dir, tag):
    g = gold(golden_dir, tag)
    cu = AI.batch(tag)[2]
    floor = tag_floor16(g)
    ctx = make_ctx(L, tag, "bf16", "l99")
    for name in ("last_compact", "trim_last_token", "norm_rank", "swiglu_rank"):
        try:
            before = ctx.set_option(name, -1)
        except RuntimeError:
            continue   # (the switch does not exist for this family)
        ctx.set_option(name, 0)
        dev = deviations(attribute(ctx, tag, "mix"), g, "mix/l99/", cu)
        ctx.set_option(name, int(before))
        print(f"bf16[{tag}] {name} off: gxi dev {dev[0].max():.4f} gnorm dev {dev[1].max():.4f}; 2 x floor16 {2 * floor}")
        assert (dev.max(1) <= 2 * floor).all(), name
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. stacked context
@pytest.mark.parametrize("tag", TAGS)
def test_stacked_slots_are_attributed_under_their_own_adapters(L, golden_dir, tag):
    g = gold(golden_dir, tag)
    ids, labels, cu = AI.batch(tag)
    floor = tag_floor16(g)[1]   # gnorm
    ctx = make_ctx(L, tag, "bf16", n_stack=2)
    for sl, a in enumerate(("l99", "l7")):
        ctx.select_slot(sl)
        ctx.set_trainable(AI.lora(tag, AI.ADAPTERS[a]))
    slots = np.array([0, 0, 1, 1], np.int32)
    _, gnorm, _ = attribute(ctx, tag, "mix", seq_slot=slots)
    ctx.close()
    own = AI.seq_dev(gnorm, np.where(np.repeat(slots, np.diff(cu)) == 0, g["mix/l99/ref_gnorm"], g["mix/l7/ref_gnorm"]), cu)
    other = AI.seq_dev(gnorm, np.where(np.repeat(slots, np.diff(cu)) == 0, g["mix/l7/ref_gnorm"], g["mix/l99/ref_gnorm"]), cu)
    print(f"stacked[{tag}]: gnorm deviation from the own slot's fixture {own}, from the other slot's {other}; 2 x floor16 = {2 * floor:.4f}")
    assert (own <= 2 * floor).all() and (other > 2 * floor).all()


# ------------------------------------------------------------------------------------------------ 5. batch independence
def test_each_sequence_alone_agrees_with_its_in_batch_values(L, golden_dir):
    tag = "tiny"
    g = gold(golden_dir, tag)
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, "strict", "l99")
    gxi, gnorm, logs = attribute(ctx, tag, "mix")
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        one = ctx.attribute(ids[a:b], labels[a:b], np.array([0, b - a], np.int32), seq_kind=AI.SETS["mix"][s:s + 1], option_ids=AI.option_ids(tag))
        for o, (alone, batch, ref) in enumerate(((one[0], gxi[a:b], g["mix/l99/ref_gxi"][a:b]), (one[1], gnorm[a:b], g["mix/l99/ref_gnorm"][a:b]))):
            scale = np.abs(ref).max()
            print(f"sequence {s} {AI.OUTPUTS[o]}: alone vs ref {np.abs(alone - ref).max() / scale:.3e}, alone vs in-batch {np.abs(alone - batch).max() / scale:.3e}")
            assert np.abs(alone - ref).max() / scale <= SX_TOL and np.abs(alone - batch).max() / scale <= SX_TOL
        assert abs(one[2][0] - logs[s]) <= 2 * LOGIT_TOL
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. no side effects
def _bits(d):
    return {k: np.ascontiguousarray(v).view(np.uint32).copy() for k, v in d.items()}


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_attribution_leaves_training_state_alone(L, mode):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    runs = []
    for with_attr in (False, True):
        ctx = make_ctx(L, tag, "bf16", "l99", mode)
        log = []
        for step in range(3):
            log.append(ctx.train_step(ids, labels, cu, 1e-3))
            if with_attr:
                before = ctx.state()
                attribute(ctx, tag, "mix")
                after = ctx.state()
                assert before["step"] == after["step"]
                for k in ("trainable", "m", "v"):
                    np.testing.assert_array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
        runs.append((np.array(log, np.float32).view(np.uint32), _bits(ctx.get_trainable())))
        ctx.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k])


def test_pending_score_and_generation_survive_an_attribution(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    ctx = make_ctx(L, tag, "bf16", "l99")
    want_score = ctx.score_rows(ids, labels, cu, opt)
    want_gen = ctx.generate(ids, cu, 4)
    want_attr = attribute(ctx, tag, "mix")
    ctx.score_rows_async(ids, labels, cu, opt)
    ctx.generate_async(ids, cu, 4)
    ctx.attribute_async(ids, labels, cu, seq_kind=AI.SETS["mix"], option_ids=opt)
    got_attr = ctx.attribute_fetch()
    got_gen = ctx.generate_fetch()
    got_score = ctx.score_rows_fetch()
    ctx.close()
    for a, b in zip(want_score + want_gen + want_attr, got_score + got_gen + got_attr):
        np.testing.assert_array_equal(a, b)


def test_optimizer_step_refuses_a_gradient_an_attribution_overwrote(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, "bf16", "l99")
    ctx.forward_backward(ids, labels, cu)
    attribute(ctx, tag, "mix")
    gn = L.C.c_float()
    assert ctx.lib.tst_optimizer_step(ctx.h, 1e-3, L.C.byref(gn)) == TST_ESTATE
    before = _bits(ctx.get_trainable())
    ctx.forward_backward(ids, labels, cu)   # a fresh gradient: the step goes through
    ctx.optimizer_step(1e-3)
    after = _bits(ctx.get_trainable())
    assert any((before[k] != after[k]).any() for k in before)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_as_it_was(L):
    tag = "tiny"
    cfg = AI.TAGS[tag][0]
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    mix = np.array(AI.SETS["mix"], np.int32)
    ctx = make_ctx(L, tag, "bf16", "l99")
    want = attribute(ctx, tag, "mix")
    nbytes = ctx.device_bytes()

    def rc_of(ids=ids, labels=labels, cu=cu, kind=mix, opt=opt, n_opt=None):
        b, keep = ctx._batch(ids, labels, cu)
        o = np.ascontiguousarray(opt, np.int32)
        k = None if kind is None else np.ascontiguousarray(kind, np.int32)
        return ctx.lib.tst_attribute_async(ctx.h, L.C.byref(b), None if k is None else L._ptr(k), L._ptr(o), len(o) if n_opt is None else n_opt)

    def unchanged(what):
        assert ctx.device_bytes() == nbytes, what
        for a, b in zip(want, attribute(ctx, tag, "mix")):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)

    bad_id = ids.copy()
    bad_id[3] = cfg["vocab_size"]
    no_lab = np.full_like(labels, -100)
    two = labels.copy()
    two[cu[1] - 2] = ids[cu[1] - 2]   # a second labelled token on the first (kind-1) sequence
    cases = {
        "the batch's own checks (id outside the vocabulary)": dict(ids=bad_id),
        "the batch's own checks (cu_seqlens)": dict(cu=np.array([0, 7, 5, 155, 285], np.int32)),
        "no labelled token": dict(labels=no_lab, kind=None),
        "n_opt > 256": dict(opt=np.arange(257) % cfg["vocab_size"]),
        "n_opt < 0": dict(n_opt=-1),
        "option id outside the vocabulary": dict(opt=np.array([opt[0], opt[1], cfg["vocab_size"]], np.int32)),
        "kind-1 sequence with two labelled rows": dict(labels=two),
        "kind 1 on a sequence that has two labelled rows": dict(kind=np.array([1, 1, 0, 1], np.int32)),
        "kind-1 target not among the options": dict(opt=np.array([o for o in (3, 9, 27, 81, 5, 6) if o not in labels[[cu[1] - 1, cu[4] - 1]]][:4], np.int32)),
        "kind-1 sequence with n_opt == 0": dict(n_opt=0),
        "seq_kind outside 0 / 1": dict(kind=np.array([1, 0, 2, 1], np.int32)),
    }
    for what, kw in cases.items():
        assert rc_of(**kw) == TST_EINVAL, what
        assert ctx.lib.tst_attribute_fetch(ctx.h, None, None, None) == TST_ESTATE, what   # nothing became pending
        unchanged(what)
    # TST_ESTATE: an open accumulation window
    ctx.accumulate_async(ids, labels, cu, int((labels != -100).sum()), first=True)
    assert rc_of() == TST_ESTATE
    ctx.forward_backward(ids, labels, cu)   # a plain forward / backward drops the window (and leaves the trainables alone)
    assert ctx.device_bytes() > nbytes   # (the window's own buffer)
    nbytes = ctx.device_bytes()
    unchanged("after the accumulation window")
    ctx.close()
    # TST_ESTATE: weights not finalised; a context that has joined a data-parallel group
    raw = L.Context(cfg, max_tokens=1024, max_seqs=16, max_labelled=64, max_position=256, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA)
    b, keep = raw._batch(ids, labels, cu)
    n0 = raw.device_bytes()
    assert raw.lib.tst_attribute_async(raw.h, L.C.byref(b), None, None, 0) == TST_ESTATE and raw.device_bytes() == n0
    raw.close()
    dp = make_ctx(L, tag, "bf16", "l99")
    dp.dp_init(L.Context.dp_unique_id(), 1, 0)
    b, keep = dp._batch(ids, labels, cu)
    n0 = dp.device_bytes()
    assert dp.lib.tst_attribute_async(dp.h, L.C.byref(b), None, None, 0) == TST_ESTATE and dp.device_bytes() == n0
    assert dp.lib.tst_attribute_fetch(dp.h, None, None, None) == TST_ESTATE
    dp.close()


def test_first_attribution_allocates_its_small_buffers_once(L):
    tag = "tiny"
    ctx = make_ctx(L, tag, "bf16", "l99")
    n0 = ctx.device_bytes()
    attribute(ctx, tag, "mix")
    n1 = ctx.device_bytes()
    attribute(ctx, tag, "open")
    assert 0 < n1 - n0 <= 8 * 1024 + 8 * 64 + 1024 and ctx.device_bytes() == n1
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. the diagnostic layer
def test_diagnose_records_carry_attr_with_the_flag_and_not_without(L, tmp_path):
    """tiny model, k = 2, one context and the stacked layout: with TrainArgs.attribute every record gains attr = {gxi, gnorm} over its prompt tokens (and
    attr_top with a decode function) and nothing else changes -- the shards without the flag are, byte for byte, what the run with it writes minus those keys,
    and their keys and the run's fingerprint are what they were before the option existed"""
    import json
    from tst import data as D
    from tst import diagnose as DG
    from tst.trainer import TrainArgs
    cfg = AI.TAGS["tiny"][0]
    samples = D.synth_vsi(40, cfg["vocab_size"], seed=3)
    kw = dict(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=1e-3, logging_steps=0, lora_r=GI.LORA_R,
              lora_alpha=GI.LORA_ALPHA)
    args, aargs = TrainArgs(**kw), TrainArgs(**kw, attribute=True, attribute_top=3)
    assert DG.run_fingerprint(samples, 2, args) != DG.run_fingerprint(samples, 2, aargs)

    def make(n_stack):
        c = L.Context(cfg, max_tokens=8 * 136 * n_stack, max_seqs=8 * n_stack, max_labelled=32 * n_stack, max_position=136, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, n_stack=n_stack)
        c.load_state_dict(AI.TAGS["tiny"][1](cfg))
        return c

    by_id = {s.sid: s for s in samples}
    for n_stack, k in ((1, 2), (2, 2)):
        shards = {}
        for name, a in (("off", args), ("on", aargs)):
            ctx = make(n_stack)
            out = str(tmp_path / f"s{n_stack}_{name}")
            recs, _ = DG.diagnose(ctx, samples, k, a, 0, 1, 0, out, decode=(lambda ids: "<" + ",".join(map(str, ids)) + ">") if name == "on" else None)
            ctx.close()
            shards[name] = [open(DG.fold_path(out, 0, f)).read() for f in range(k)]
            assert len(recs) == len(samples)
            if name == "off":
                assert all(list(r) == ["id", "fold", "round", "s", "pred", "correct", "kind"] for r in recs)
                continue
            for r in recs:
                smp = by_id[r["id"]]
                gxi, gnorm = np.array(r["attr"]["gxi"]), np.array(r["attr"]["gnorm"])
                assert len(gxi) == len(gnorm) == smp.n_prompt and np.isfinite(gxi).all() and np.isfinite(gnorm).all() and (gnorm >= 0).all() and gnorm.max() > 0
                top = np.argsort(-gnorm, kind="stable")[:3]
                assert r["attr_top"] == [f"<{int(smp.ids[t])}>" for t in top]
        for off, on in zip(shards["off"], shards["on"]):
            stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk not in ("attr", "attr_top")}) + "\n" for line in on.splitlines())
            assert stripped == off
