"""GPU tests of integrated gradients (include/tst_hip.h tst_attribute_ig_async; csrc/attribute.hip embed_interp / token_ig, engine.hip, host_logic.h).

Reference = tests/golden/ig_<tag>.npz (tools/make_golden.py ig): the midpoint-rule integrated gradients of J = sum_i log s(x_i) from a baseline prompt to the real
one at m = 16 steps, from the HF model in fp64 (`ref`), fp32 and bf16 (`floor32` / `floor16` = the distance of HF's own fp32 / bf16 runs from `ref`, the max over
sequences of max_t |ig - ref| / max_t |ref|, AI.seq_dev), for two baseline patterns (IG.PATTERNS) x the fixture sets and adapter sets of the attribution fixtures.
  1. the two kernels on their own, through the lab hooks: embed_interp bit for bit against numpy's fp32 arithmetic with one rounding (and against the embedding
     kernels at alpha = 1), token_ig against float64 numpy within the fp32 accumulation bound of the token_attr test.
  2. strict (fp32) contexts against `ref` at the fixtures' m: seq_dev <= SX_TOL = 1e-3 per sequence (the project's strict criterion; the reference's own fp32 floor
     is <= 2.2e-6), both log s within 2 LOGIT_TOL of the reference's.
  3. completeness as shipped, strict, m = 64: per sequence |delta_lib - delta_ref| <= SX_TOL sum_t |ref_ig64[t]| + 4 LOGIT_TOL -- the parity bound summed over
     the tokens plus the tolerances of the two log s; delta = sum_t ig[t] - (logs - logs_base).
  4. bf16 contexts: seq_dev <= 2 x the tag's floor16 (DESIGN.md section 13's rule: two independent bf16 roundings of the same path can at worst add; the tag's
     floor16 = the largest of its stored entries), also with last_compact, trim_last_token, norm_rank and swiglu_rank each switched off.
  5. the limits of the definition, 6. stacked slots, 7. batch independence, 8. repeatability, 9. state, 10. the diagnostic layer.
Measured on an MI355X: strict seq_dev <= 5.4e-6 and both log s within 4.5e-6 of the reference's; |delta - delta_ref64| about 2e-6; bf16 worst deviation / tag
floor16: tiny 0.27, tiny2 0.72, qwen 0.45, qwen3 0.40, gpt2 0.44 -- no tag near the factor 2, so none is raised (DESIGN.md section 14 has the table)."""
import numpy as np
import pytest

import attribution_inputs as AI
import golden_inputs as GI
import ig_inputs as IG

pytestmark = pytest.mark.gpu

SX_TOL = 1e-3      # tests/test_strict_gpu.py: the project's bound on s(x)
LOGIT_TOL = 1e-4   # tests/test_strict_gpu.py: one strict logit
TAGS = list(AI.TAGS)
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
        _GOLD[tag] = dict(np.load(f"{golden_dir}/ig_{tag}.npz"))
    return _GOLD[tag]


def tag_floor16(g):
    return max(float(g[IG.key(s, p, a) + "floor16"]) for s in AI.SETS for p in IG.PATTERNS for a in AI.ADAPTERS)


def make_ctx(L, tag, precision, adapter="base", mode="lora", n_stack=1, max_tokens=1024):
    cfg = AI.TAGS[tag][0]
    ctx = L.Context(cfg, max_tokens=max_tokens, max_seqs=16, max_labelled=64, max_position=cfg["max_position"] if cfg.get("arch") == "gpt2" else 256,
                    lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA, train_mode=mode, precision=precision, n_stack=n_stack)
    ctx.load_state_dict(AI.TAGS[tag][1](cfg))
    if mode == "lora" and n_stack == 1:
        ctx.set_trainable(AI.zero_lora(tag) if AI.ADAPTERS[adapter] is None else AI.lora(tag, AI.ADAPTERS[adapter]))
    return ctx


def run_ig(ctx, tag, sname, pname, steps=IG.STEPS, **kw):
    ids, labels, cu = AI.batch(tag)
    return ctx.attribute_ig(ids, labels, cu, IG.baseline_ids(tag, pname), steps, seq_kind=AI.SETS[sname], option_ids=AI.option_ids(tag), **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. kernels
def _table(rng, rows, d, f32):
    x = rng.standard_normal((rows, d)).astype(np.float32)
    x[0, :4] = (-0.0, 0.0, 1e-30, -3e4)   # a -0 must stay a -0 where the kernel only copies; a wide range of binades where it interpolates
    return x if f32 else GI.bf16_round(x)


def _round_to(x, f32):
    return np.ascontiguousarray(x, np.float32) if f32 else GI.bf16_round(x)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [128, 4096])
@pytest.mark.parametrize("T", [1, 3, 257])
def test_embed_interp_kernel(L, T, d, f32):
    lab = L.load_lab()
    rng = np.random.default_rng(T * 10007 + d)
    V, npos = 37, 300
    E, P = _table(rng, V, d, f32), _table(rng, npos, d, f32)
    ids, bids = rng.integers(0, V, T).astype(np.int32), rng.integers(0, V, T).astype(np.int32)
    ids[0] = 0                       # (the row with the -0)
    bids[::3] = ids[::3]             # tokens that are their own baseline (T = 1: the only one, checked again below with a different baseline)
    pos = rng.integers(0, npos, T).astype(np.int32)
    up = L.dev_f32 if f32 else L.dev_bf16
    E_, P_, i_, p_ = up(E), up(P), L.DevBuf(ids), L.DevBuf(pos)
    fn = lab.tst_k_embed_interp_f32 if f32 else lab.tst_k_embed_interp
    esz = 4 if f32 else 2

    def run(b, alpha, with_pos):
        out = L.DevBuf(to_garbage(T, d, f32))
        b_ = L.DevBuf(b)
        assert fn(i_.ptr, b_.ptr, p_.ptr if with_pos else None, E_.ptr, P_.ptr if with_pos else None, out.ptr, T, d, V, npos, alpha) == 0
        return out.get(np.float32, (T, d)) if f32 else out.get_bf16((T, d))

    def to_garbage(T, d, f32):
        return np.full((T, d), 7.0, np.float32) if f32 else np.full((T, d), 0x40E0, np.uint16)

    other = ((ids + 1 + rng.integers(0, V - 1, T)) % V).astype(np.int32)   # a baseline that differs from the id on every token
    for b in (bids, other):
        same = (ids == b)[:, None]
        e, bb = E[ids], E[b]
        for alpha in (0.0, 0.46875, 1.0):
            mix = e if alpha == 1.0 else bb if alpha == 0.0 else (bb + np.float32(alpha) * (e - bb)).astype(np.float32)   # b + alpha (e - b): every step an fp32 value
            x = np.where(same, e, mix)
            for with_pos in (False, True):
                want = _round_to(x + P[pos], f32) if with_pos else x   # without the position term the result is one fp32 value, rounded once (or a table row)
                if not with_pos and alpha not in (0.0, 1.0):
                    want = np.where(same, e, _round_to(mix, f32))
                got = run(b, alpha, with_pos)
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"alpha={alpha} pos={with_pos}")
                if same.any():   # an id equal to its baseline id: the table row (plus the position row, rounded once) at every alpha
                    rows = np.flatnonzero(same[:, 0])
                    np.testing.assert_array_equal(_bits(got[rows]), _bits(_round_to(e[rows] + P[pos[rows]], f32) if with_pos else e[rows]))
    if not f32:   # alpha = 1 is the embedding kernels' output bit for bit (their lab hooks are the bf16 instances)
        out = L.DevBuf(nbytes=esz * T * d)
        assert lab.tst_k_embed(i_.ptr, E_.ptr, out.ptr, T, d, V) == 0
        np.testing.assert_array_equal(_bits(run(other, 1.0, False)), _bits(out.get_bf16((T, d))))
        assert lab.tst_k_embed_pos(i_.ptr, p_.ptr, E_.ptr, P_.ptr, out.ptr, T, d, V, npos) == 0
        np.testing.assert_array_equal(_bits(run(other, 1.0, True)), _bits(out.get_bf16((T, d))))
    out = L.DevBuf(nbytes=esz * T * (d + 8))
    o_ = L.DevBuf(other)
    assert fn(i_.ptr, o_.ptr, None, E_.ptr, None, out.ptr, T, d + 4, V, npos, 0.5) == TST_EINVAL   # d must be a multiple of 8
    assert fn(i_.ptr, o_.ptr, None, E_.ptr, None, out.ptr, T, d, V, npos, 1.5) == TST_EINVAL       # alpha lies in [0, 1]
    assert fn(i_.ptr, None, None, E_.ptr, None, out.ptr, T, d, V, npos, 0.5) == TST_EINVAL


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [128, 4096])
@pytest.mark.parametrize("T", [1, 3, 257])
def test_token_ig_kernel(L, T, d, f32):
    lab = L.load_lab()
    rng = np.random.default_rng(T * 7919 + d)
    V = 37
    E = _table(rng, V, d, f32)
    g = _round_to(rng.standard_normal((T, d)).astype(np.float32), f32)
    ids = rng.integers(0, V, T).astype(np.int32)
    bids = ((ids + 1 + rng.integers(0, V - 1, T)) % V).astype(np.int32)
    if T > 1:
        bids[1::3] = ids[1::3]   # tokens that are their own baseline: exactly 0
    up = L.dev_f32 if f32 else L.dev_bf16
    g_, E_, i_, b_ = up(g), up(E), L.DevBuf(ids), L.DevBuf(bids)
    fn = lab.tst_k_token_ig_f32 if f32 else lab.tst_k_token_ig
    w1, w2 = 1.0 / 16.0, 1.0 / 3.0
    garbage = np.full(T, 1e30, np.float32)

    def first(w):
        acc = L.DevBuf(garbage)
        assert fn(g_.ptr, E_.ptr, i_.ptr, b_.ptr, T, d, V, w, 1, acc.ptr) == 0
        return acc, acc.get(np.float32, (T,))

    acc_a, a1 = first(w1)
    _, a1_again = first(w1)
    _, b1 = first(w2)
    np.testing.assert_array_equal(_bits(a1), _bits(a1_again))   # bit-identical across two runs
    diff = E[ids].astype(np.float64) - E[bids].astype(np.float64)
    ref = (g.astype(np.float64) * diff).sum(-1)
    mass = np.abs(g.astype(np.float64) * diff).sum(-1)
    moved = ids != bids
    bound = d * 2.0 ** -23
    err = np.abs(a1[moved] / np.float32(w1) - ref[moved]) / mass[moved]
    print(f"token_ig T={T} d={d} f32={f32}: |ig / w - ref| / sum|g (e - b)| <= {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound + 2.0 ** -23).all()   # (+ one fp32 rounding of the product with w)
    assert (a1[~moved] == 0).all() and (b1[~moved] == 0).all()
    # a second call adds: exactly the fp32 sum of the two single results
    assert fn(g_.ptr, E_.ptr, i_.ptr, b_.ptr, T, d, V, w2, 0, acc_a.ptr) == 0
    np.testing.assert_array_equal(_bits(acc_a.get(np.float32, (T,))), _bits((a1 + b1).astype(np.float32)))
    assert fn(g_.ptr, E_.ptr, i_.ptr, b_.ptr, T, d + 4, V, w1, 1, acc_a.ptr) == TST_EINVAL   # d must be a multiple of 8


# ------------------------------------------------------------------------------------------------ 2. strict contexts vs ref
STRICT_CASES = [(t, a, "lora") for t in TAGS for a in ("base", "l99")] + [("tiny", "base", "full")]


@pytest.mark.parametrize("tag,adapter,mode", STRICT_CASES, ids=[f"{t}-{a}-{m}" for t, a, m in STRICT_CASES])
def test_strict_ig_matches_the_reference(L, golden_dir, tag, adapter, mode):
    g = gold(golden_dir, tag)
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, "strict", adapter, mode)
    for sname in AI.SETS:
        for pname in IG.PATTERNS:
            key = IG.key(sname, pname, adapter)
            ig, logs, logs_base = run_ig(ctx, tag, sname, pname)
            dev = AI.seq_dev(ig, g[key + "ref_ig"], cu)
            d_logs, d_base = np.abs(logs - g[key + "ref_logs"]), np.abs(logs_base - g[key + "ref_logs_base"])
            print(f"strict[{tag}, {adapter}, {mode}, {sname}, {pname}]: ig dev per sequence {dev}; floor32 {g[key + 'floor32']:.2e}; "
                  f"|logs - ref| <= {d_logs.max():.2e}, |logs_base - ref| <= {d_base.max():.2e}")
            assert dev.max() <= SX_TOL
            assert d_logs.max() <= 2 * LOGIT_TOL and d_base.max() <= 2 * LOGIT_TOL
            if pname == "prompt":   # uninterpolated tokens carry exactly 0
                assert (ig[labels != -100] == 0).all()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. completeness as shipped
@pytest.mark.parametrize("adapter", ["base", "l99"])
@pytest.mark.parametrize("tag", ["tiny", "gpt2"])
def test_strict_completeness_gap_is_the_reference_s(L, golden_dir, tag, adapter):
    g = gold(golden_dir, tag)
    cu = AI.batch(tag)[2]
    ctx = make_ctx(L, tag, "strict", adapter)
    for pname in IG.PATTERNS:
        key = IG.key("mix", pname, adapter)
        ig, logs, logs_base = run_ig(ctx, tag, "mix", pname, steps=IG.STEPS_FINE)
        ig64 = ig.astype(np.float64)
        delta = np.array([ig64[cu[s]:cu[s + 1]].sum() for s in range(len(cu) - 1)]) - (logs.astype(np.float64) - logs_base.astype(np.float64))
        bound = SX_TOL * np.array([np.abs(g[key + "ref_ig64"][cu[s]:cu[s + 1]]).sum() for s in range(len(cu) - 1)]) + 4 * LOGIT_TOL
        print(f"completeness[{tag}, {adapter}, {pname}] m = {IG.STEPS_FINE}: delta {delta}, reference's {g[key + 'delta_ref64']}, bound on the difference {bound}; "
              f"dJ {logs - logs_base}")
        assert (np.abs(delta - g[key + "delta_ref64"]) <= bound).all()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. bf16 contexts vs ref
@pytest.mark.parametrize("adapter", ["base", "l99"])
@pytest.mark.parametrize("tag", TAGS)
def test_bf16_ig_stays_within_twice_the_bf16_floor(L, golden_dir, tag, adapter):
    g = gold(golden_dir, tag)
    cu = AI.batch(tag)[2]
    floor = tag_floor16(g)
    ctx = make_ctx(L, tag, "bf16", adapter)
    worst = 0.0
    for sname in AI.SETS:
        for pname in IG.PATTERNS:
            key = IG.key(sname, pname, adapter)
            got = run_ig(ctx, tag, sname, pname)
            dev = AI.seq_dev(got[0], g[key + "ref_ig"], cu)
            worst = max(worst, dev.max())
            print(f"bf16[{tag}, {adapter}, {sname}, {pname}]: ig dev per sequence {dev}; this entry's floor16 {g[key + 'floor16']:.4f}")
    ctx.close()
    print(f"bf16[{tag}, {adapter}]: worst deviation {worst:.4f}; tag floor16 {floor:.4f}; ratio {worst / floor:.3f}")
    assert worst <= 2.0 * floor


@pytest.mark.parametrize("tag", TAGS)
def test_bf16_ig_with_each_engine_option_off(L, golden_dir, tag):
    g = gold(golden_dir, tag)
    cu = AI.batch(tag)[2]
    floor = tag_floor16(g)
    ctx = make_ctx(L, tag, "bf16", "l99")
    for name in ("last_compact", "trim_last_token", "norm_rank", "swiglu_rank"):
        before = ctx.set_option(name, -1)   # (every family has all four on a bf16 LoRA context: a switch that is missing is a failure, not a skipped case)
        ctx.set_option(name, 0)
        dev = AI.seq_dev(run_ig(ctx, tag, "mix", "all")[0], g[IG.key("mix", "all", "l99") + "ref_ig"], cu)
        ctx.set_option(name, int(before))
        print(f"bf16[{tag}] {name} off: ig dev {dev}; 2 x floor16 {2 * floor:.4f}")
        assert dev.max() <= 2 * floor, name
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. limits of the definition
@pytest.mark.parametrize("precision", ["bf16", "strict"])
def test_a_baseline_equal_to_the_input_gives_zero_and_equal_log_s(L, precision):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, precision, "l99")
    ig, logs, logs_base = ctx.attribute_ig(ids, labels, cu, ids.copy(), 1, seq_kind=AI.SETS["mix"], option_ids=AI.option_ids(tag))
    assert (ig == 0).all()
    np.testing.assert_array_equal(_bits(logs), _bits(logs_base))
    _, _, want = ctx.attribute(ids, labels, cu, seq_kind=AI.SETS["mix"], option_ids=AI.option_ids(tag))
    print(f"logs of attribute_ig {logs}, of attribute {want}")
    assert np.abs(logs - want).max() <= 2 * LOGIT_TOL
    # and with a real baseline logs is still the real prompt's
    _, logs2, base2 = run_ig(ctx, tag, "mix", "all", steps=2)
    assert np.abs(logs2 - want).max() <= 2 * LOGIT_TOL and np.abs(base2 - want).max() > 100 * LOGIT_TOL
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. stacked context
@pytest.mark.parametrize("tag", TAGS)
def test_stacked_slots_are_attributed_under_their_own_adapters(L, golden_dir, tag):
    g = gold(golden_dir, tag)
    ids, labels, cu = AI.batch(tag)
    floor = tag_floor16(g)
    apart = g["mix/all/l99_vs_l7"]
    use = apart > 4 * floor   # only there can a result within 2 x floor16 of one fixture not be within 2 x floor16 of the other
    assert use.any(), "no sequence tells the two adapter sets apart"
    ctx = make_ctx(L, tag, "bf16", n_stack=2)
    for sl, a in enumerate(("l99", "l7")):
        ctx.select_slot(sl)
        ctx.set_trainable(AI.lora(tag, AI.ADAPTERS[a]))
    slots = np.array([0, 0, 1, 1], np.int32)
    ig, _, _ = run_ig(ctx, tag, "mix", "all", seq_slot=slots)
    ctx.close()
    tok_slot = np.repeat(slots, np.diff(cu))
    own = AI.seq_dev(ig, np.where(tok_slot == 0, g["mix/all/l99/ref_ig"], g["mix/all/l7/ref_ig"]), cu)
    other = AI.seq_dev(ig, np.where(tok_slot == 0, g["mix/all/l7/ref_ig"], g["mix/all/l99/ref_ig"]), cu)
    print(f"stacked[{tag}]: ig deviation from the own slot's fixture {own}, from the other slot's {other}; l99 vs l7 {apart}; 2 x floor16 = {2 * floor:.4f}; used {use}")
    assert (own <= 2 * floor).all() and (other[use] > 2 * floor).all()


# ------------------------------------------------------------------------------------------------ 7. batch independence
def test_each_sequence_alone_equals_its_in_batch_values(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    base = IG.baseline_ids(tag, "all")
    ctx = make_ctx(L, tag, "strict", "l99")
    ig, logs, logs_base = run_ig(ctx, tag, "mix", "all", steps=4)
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        one = ctx.attribute_ig(ids[a:b], labels[a:b], np.array([0, b - a], np.int32), base[a:b], 4, seq_kind=AI.SETS["mix"][s:s + 1], option_ids=AI.option_ids(tag))
        np.testing.assert_array_equal(_bits(one[0]), _bits(ig[a:b]), err_msg=f"sequence {s}")
        assert one[1][0] == logs[s] and one[2][0] == logs_base[s]
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. repeatability
@pytest.mark.parametrize("precision", ["bf16", "strict"])
def test_two_identical_calls_are_bit_identical(L, precision):
    tag = "qwen3"
    ctx = make_ctx(L, tag, precision, "l99")
    a = run_ig(ctx, tag, "mix", "all", steps=4)
    b = run_ig(ctx, tag, "mix", "all", steps=4)
    ctx.close()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    assert np.abs(a[0]).max() > 0


# ------------------------------------------------------------------------------------------------ 9. state
def _dbits(d):
    return {k: np.ascontiguousarray(v).view(np.uint32).copy() for k, v in d.items()}


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_ig_leaves_training_state_alone(L, mode):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    runs = []
    for with_ig in (False, True):
        ctx = make_ctx(L, tag, "bf16", "l99", mode)
        log = []
        for step in range(3):
            log.append(ctx.train_step(ids, labels, cu, 1e-3))
            if with_ig:
                before = ctx.state()
                run_ig(ctx, tag, "mix", "all", steps=2)
                after = ctx.state()
                assert before["step"] == after["step"]
                for k in ("trainable", "m", "v"):
                    np.testing.assert_array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
        runs.append((np.array(log, np.float32).view(np.uint32), _dbits(ctx.get_trainable())))
        ctx.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k])


def test_pending_score_generation_and_kv_cache_survive_an_ig_call(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    base = IG.baseline_ids(tag, "all")
    ctx = make_ctx(L, tag, "bf16", "l99")
    want_score = ctx.score_rows(ids, labels, cu, opt)
    want_gen = ctx.generate(ids, cu, 4)
    want_ig = run_ig(ctx, tag, "mix", "all", steps=2)
    ctx.score_rows_async(ids, labels, cu, opt)
    ctx.generate_async(ids, cu, 4)
    ctx.attribute_ig_async(ids, labels, cu, base, 2, seq_kind=AI.SETS["mix"], option_ids=opt)
    got_ig = ctx.attribute_ig_fetch()
    got_gen = ctx.generate_fetch()
    got_score = ctx.score_rows_fetch()
    again_gen = ctx.generate(ids, cu, 4)   # (the KV cache of a generation is the context's: the next one finds it usable)
    ctx.close()
    for a, b in zip(want_score + want_gen + want_ig + want_gen, got_score + got_gen + got_ig + again_gen):
        np.testing.assert_array_equal(a, b)


def test_optimizer_step_refuses_a_gradient_an_ig_call_overwrote(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, "bf16", "l99")
    ctx.forward_backward(ids, labels, cu)
    run_ig(ctx, tag, "mix", "all", steps=1)
    gn = L.C.c_float()
    assert ctx.lib.tst_optimizer_step(ctx.h, 1e-3, L.C.byref(gn)) == TST_ESTATE
    before = _dbits(ctx.get_trainable())
    ctx.forward_backward(ids, labels, cu)   # a fresh gradient: the step goes through
    ctx.optimizer_step(1e-3)
    after = _dbits(ctx.get_trainable())
    assert any((before[k] != after[k]).any() for k in before)
    ctx.close()


def test_a_fetch_of_the_wrong_kind_is_refused_and_keeps_the_pending_one(L):
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    base = IG.baseline_ids(tag, "all")
    ctx = make_ctx(L, tag, "bf16", "l99")
    want_ig = run_ig(ctx, tag, "mix", "all", steps=2)
    want_attr = ctx.attribute(ids, labels, cu, seq_kind=AI.SETS["mix"], option_ids=opt)
    assert ctx.lib.tst_attribute_ig_fetch(ctx.h, None, None, None) == TST_ESTATE   # nothing pending
    ctx.attribute_ig_async(ids, labels, cu, base, 2, seq_kind=AI.SETS["mix"], option_ids=opt)
    assert ctx.lib.tst_attribute_fetch(ctx.h, None, None, None) == TST_ESTATE
    for a, b in zip(want_ig, ctx.attribute_ig_fetch()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert ctx.lib.tst_attribute_ig_fetch(ctx.h, None, None, None) == TST_ESTATE
    ctx.attribute_async(ids, labels, cu, seq_kind=AI.SETS["mix"], option_ids=opt)
    assert ctx.lib.tst_attribute_ig_fetch(ctx.h, None, None, None) == TST_ESTATE
    for a, b in zip(want_attr, ctx.attribute_fetch()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    ctx.close()


def test_refusals_leave_the_context_as_it_was(L):
    tag = "tiny"
    cfg = AI.TAGS[tag][0]
    ids, labels, cu = AI.batch(tag)
    opt = AI.option_ids(tag)
    mix = np.array(AI.SETS["mix"], np.int32)
    base = IG.baseline_ids(tag, "all")
    ctx = make_ctx(L, tag, "bf16", "l99")
    n_before_first = ctx.device_bytes()

    def rc_of(ctx=ctx, ids=ids, labels=labels, cu=cu, kind=mix, opt=opt, base=base, steps=4):
        b, keep = ctx._batch(ids, labels, cu)
        o = np.ascontiguousarray(opt, np.int32)
        k = None if kind is None else np.ascontiguousarray(kind, np.int32)
        bb = None if base is None else np.ascontiguousarray(base, np.int32)
        return ctx.lib.tst_attribute_ig_async(ctx.h, L.C.byref(b), None if k is None else L._ptr(k), L._ptr(o), len(o), None if bb is None else L._ptr(bb), steps)

    bad_base = base.copy()
    bad_base[5] = cfg["vocab_size"]
    neg_base = base.copy()
    neg_base[-1] = -1
    bad_id = ids.copy()
    bad_id[3] = cfg["vocab_size"]
    cases = {
        "null baseline_ids": dict(base=None),
        "baseline id outside the vocabulary": dict(base=bad_base),
        "negative baseline id": dict(base=neg_base),
        "n_steps == 0": dict(steps=0),
        "n_steps > TST_IG_MAX_STEPS": dict(steps=L.IG_MAX_STEPS + 1),
        "the batch's own checks (id outside the vocabulary)": dict(ids=bad_id),
        "tst_attribute_async's checks (seq_kind outside 0 / 1)": dict(kind=np.array([1, 0, 2, 1], np.int32)),
        "tst_attribute_async's checks (no labelled token)": dict(labels=np.full_like(labels, -100), kind=None),
    }
    # a refusal before the first call allocates nothing
    for what, kw in cases.items():
        assert rc_of(**kw) == TST_EINVAL, what
        assert ctx.device_bytes() == n_before_first, what
    want = run_ig(ctx, tag, "mix", "all", steps=4)
    nbytes = ctx.device_bytes()

    def unchanged(what):
        assert ctx.device_bytes() == nbytes, what
        for a, b in zip(want, run_ig(ctx, tag, "mix", "all", steps=4)):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)

    for what, kw in cases.items():
        assert rc_of(**kw) == TST_EINVAL, what
        assert ctx.lib.tst_attribute_ig_fetch(ctx.h, None, None, None) == TST_ESTATE, what   # nothing became pending
        unchanged(what)
    assert "n_steps" in _err_of(ctx, lambda: rc_of(steps=0)) and "baseline" in _err_of(ctx, lambda: rc_of(base=bad_base))
    # TST_ESTATE: an open accumulation window
    ctx.accumulate_async(ids, labels, cu, int((labels != -100).sum()), first=True)
    assert rc_of() == TST_ESTATE
    ctx.forward_backward(ids, labels, cu)   # a plain forward / backward drops the window (and leaves the trainables alone)
    nbytes = ctx.device_bytes()
    unchanged("after the accumulation window")
    ctx.close()
    # TST_ESTATE: weights not finalised; a context that has joined a data-parallel group
    raw = L.Context(cfg, max_tokens=1024, max_seqs=16, max_labelled=64, max_position=256, lora_r=GI.LORA_R, lora_alpha=GI.LORA_ALPHA)
    n0 = raw.device_bytes()
    assert rc_of(ctx=raw) == TST_ESTATE and raw.device_bytes() == n0
    raw.close()
    dp = make_ctx(L, tag, "bf16", "l99")
    dp.dp_init(L.Context.dp_unique_id(), 1, 0)
    n0 = dp.device_bytes()
    assert rc_of(ctx=dp) == TST_ESTATE and dp.device_bytes() == n0
    assert dp.lib.tst_attribute_ig_fetch(dp.h, None, None, None) == TST_ESTATE
    dp.close()


def _err_of(ctx, call):
    assert call() != 0
    return ctx.lib.tst_last_error(ctx.h).decode()


def test_first_ig_call_allocates_its_small_buffers_once(L):
    tag = "tiny"
    ctx = make_ctx(L, tag, "bf16", "l99")
    n0 = ctx.device_bytes()
    run_ig(ctx, tag, "mix", "all", steps=1)
    n1 = ctx.device_bytes()
    run_ig(ctx, tag, "open", "prompt", steps=2)
    ids, labels, cu = AI.batch(tag)
    ctx.attribute(ids, labels, cu)   # (its buffers came with the first integrated-gradients call)
    # the attribution's own buffers (8 bytes per max_tokens + 8 per max_labelled + 1 KB) plus 8 bytes per max_tokens, each rounded up by the pool
    assert 8 * 1024 < n1 - n0 <= 16 * 1024 + 8 * 64 + 1024 + 2 * 512 and ctx.device_bytes() == n1
    ctx.close()


def test_device_ids_and_trimmed_tokens(L):
    """a TST_BATCH_DEVICE_IDS batch gives what the host-id batch gives (baseline_ids stay in host memory), and the last token of every sequence, which
    trim_last_token keeps off the device, gets 0"""
    tag = "tiny"
    ids, labels, cu = AI.batch(tag)
    ctx = make_ctx(L, tag, "bf16", "l99")
    want = run_ig(ctx, tag, "mix", "all", steps=2)
    assert (want[0][cu[1:] - 1] == 0).all() and np.abs(want[0]).max() > 0
    buf = L.DevBuf(ids)
    got = ctx.attribute_ig(L.DeviceIds(buf.ptr.value, len(ids)), labels, cu, IG.baseline_ids(tag, "all"), 2, seq_kind=AI.SETS["mix"], option_ids=AI.option_ids(tag))
    for a, b in zip(want, got):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    ctx.set_option("trim_last_token", 0)
    untrimmed = run_ig(ctx, tag, "mix", "all", steps=2)
    assert (untrimmed[0][cu[1:] - 1] == 0).all()   # nothing reads the last token under the causal mask: its gradient is exactly 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 10. the diagnostic layer
def test_diagnose_records_carry_attr_ig_with_the_flag_and_not_without(L, tmp_path):
    """tiny model, k = 2, one context and the stacked layout: with TrainArgs.attribute_ig every record gains attr_ig = {ig, log_s_base, delta}, ig over its prompt
    tokens (and attr_ig_top with a decode function), and nothing else changes -- the shards without the flag are, byte for byte, what the run with it writes minus
    those keys, and their keys are what they were before the option existed"""
    import json
    from tst import data as D
    from tst import diagnose as DG
    from tst.trainer import TrainArgs
    cfg = AI.TAGS["tiny"][0]
    samples = D.synth_vsi(40, cfg["vocab_size"], seed=3)
    kw = dict(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=1e-3, logging_steps=0, lora_r=GI.LORA_R,
              lora_alpha=GI.LORA_ALPHA)
    args, iargs = TrainArgs(**kw), TrainArgs(**kw, attribute_ig=8, attribute_baseline_id=2, attribute_top=3)
    assert DG.run_fingerprint(samples, 2, args) != DG.run_fingerprint(samples, 2, iargs)

    def make(n_stack):
        c = L.Context(cfg, max_tokens=8 * 136 * n_stack, max_seqs=8 * n_stack, max_labelled=32 * n_stack, max_position=136, lora_r=GI.LORA_R,
                      lora_alpha=GI.LORA_ALPHA, n_stack=n_stack)
        c.load_state_dict(AI.TAGS["tiny"][1](cfg))
        return c

    by_id = {s.sid: s for s in samples}
    for n_stack, k in ((1, 2), (2, 2)):
        shards = {}
        for name, a in (("off", args), ("on", iargs)):
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
                ig = np.array(r["attr_ig"]["ig"])
                assert list(r["attr_ig"]) == ["ig", "log_s_base", "delta"] and len(ig) == smp.n_prompt and np.isfinite(ig).all() and np.abs(ig).max() > 0
                assert (ig[np.asarray(smp.ids[:smp.n_prompt]) == 2] == 0).all()   # a prompt token that IS the baseline token does not move
                # the record's own arithmetic: delta = sum(ig) - (log s - log s_base), with s the record's score (the answer tokens carry exactly 0)
                want = ig.sum() - (np.log(r["s"]) - r["attr_ig"]["log_s_base"])
                # (the score comes from the scoring pass, log s inside delta from the attribution's own pass: two bf16 forwards of the same prompt, which agree
                # to a bf16 rounding, 2^-8, of logits that are O(1) on this model -- 2e-2 covers both log-sum-exps)
                assert abs(r["attr_ig"]["delta"] - want) <= 2e-2, (r["attr_ig"]["delta"], want)
                top = np.argsort(-np.abs(ig), kind="stable")[:3]
                assert r["attr_ig_top"] == [[f"<{int(smp.ids[t])}>", float(ig[t])] for t in top]
        for off, on in zip(shards["off"], shards["on"]):
            stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk not in ("attr_ig", "attr_ig_top")}) + "\n" for line in on.splitlines())
            assert stripped == off
