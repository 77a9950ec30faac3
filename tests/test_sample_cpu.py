"""CPU tests of sampled generation: the reference's own pieces (tests/sample_oracle.py: Philox4x32-10 known answers, the u mapping), tsthost::plan_sample
through libtst_host.so (csrc/host_logic.h, what tst_sample_async runs before any launch), tst.score.sample_seeds / sampled_answers, tst.benchmarks'
mean relative accuracy, and the conditions the GPU tests rest on, asserted on the oracle alone: every draw of every strict case keeps its top-1 / top-2 gap above
2 band under the pinned per-case seeds, and the oracle's own 512 first tokens pass the coverage chi-square."""
import types

import numpy as np
import pytest

import generate_oracle as G
import golden_inputs as GI
import sample_oracle as SO
from tst import lib
from tst.benchmarks import mean_relative_accuracy, parse_number
from tst.score import sample_seeds, sampled_answers


# ------------------------------------------------------------------------------------------------ Philox4x32-10, the noise
def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32_10 (key words in the order k0, k1)"""
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        assert [int(x) for x in SO.philox4x32_10(ctr, key)] == want
    # vectorised over counters, and the word of vocabulary entry v is word v & 3 of counter (v >> 2, step, sample, 0) under (low, high) of the seed
    seed = 0x299f31d0a4093822
    w = SO.noise_words(seed, 11, 0x85a308d3, 0x13198a2e)
    one = SO.philox4x32_10([2, 0x85a308d3, 0x13198a2e, 0], [0xa4093822, 0x299f31d0])
    assert len(w) == 11 and [int(x) for x in w[8:11]] == [int(x) for x in one[:3]]


def test_u_is_exact_in_fp32_and_never_0_or_1():
    x = np.array([0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], np.uint32)
    u = SO.uniform_of(x)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    u32 = ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)   # the device's arithmetic
    assert (u32.astype(np.float64) == u).all()
    g = -np.log(-np.log(u))
    assert np.isfinite(g).all() and np.abs(g).max() <= 16.7


# ------------------------------------------------------------------------------------------------ plan_sample
def _prompts():
    lens = (3, 1, 40, 17)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return np.arange(cu[-1], dtype=np.int32) % 200, cu, lens


def test_plan_sample_row_map_and_capacity():
    ids, cu, lens = _prompts()
    S, T, max_new, n = len(lens), int(cu[-1]), 5, 3
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=64, max_seqs=13, max_labelled=12, max_position=64)
    seeds = np.array([1, 2 ** 63 + 5, 2 ** 32, 2 ** 64 - 1], np.uint64)
    p = lib.host_plan_sample(mc, ids, cu, max_new, n, 0.7, seeds, eos_ids=(2,))
    R = S * n
    assert (p["S"], p["T"], p["R"]) == (S, T, R) and p["rows_used"] == T + R * max_new <= p["cache_rows"] == 64 + 13 * max_new
    assert p["dev_ints"] == p["dev_ints_alloc"] == 3 + 2 * 13 + 64 + 13 * max_new   # the image fills a greedy generation's, which keeps its size
    assert list(p["geo"][:3]) == [R, max_new, n]
    geo = p["geo"][3:].reshape(R, 3)
    np.testing.assert_array_equal(geo[:, 0], np.repeat(cu[:-1], n))
    np.testing.assert_array_equal(geo[:, 1], np.repeat(lens, n))
    np.testing.assert_array_equal(geo[:, 2], T + np.arange(R) * max_new)
    np.testing.assert_array_equal(p["prefill_rows"], np.arange(T))
    np.testing.assert_array_equal(p["last_rows"], cu[1:] - 1)
    np.testing.assert_array_equal(p["decode_rows"], geo[None, :, 2] + np.arange(max_new - 1)[:, None])
    # tails: disjoint from each other and from the prompts, inside the cache
    tails = (geo[:, 2, None] + np.arange(max_new)[None]).reshape(-1)
    assert len(set(tails)) == len(tails) and tails.min() >= T and tails.max() < p["rows_used"]
    np.testing.assert_array_equal(p["seeds"].view(np.uint32), np.stack([seeds & np.uint64(0xffffffff), seeds >> np.uint64(32)], 1).astype(np.uint32))
    assert (p["slot_r_end"] == R).all()
    # stacked: the slot boundaries of plan_generate times n_samples (rows are s-major)
    mc3 = lib.make_model_cfg(GI.TINY_CFG, max_tokens=64, max_seqs=13, max_labelled=12, max_position=64, n_stack=3)
    p3 = lib.host_plan_sample(mc3, ids, cu, max_new, n, 1.0, seeds, seq_slot=[0, 2, 2, 2])
    pg = lib.host_plan_generate(mc3, ids, cu, max_new, seq_slot=[0, 2, 2, 2])
    np.testing.assert_array_equal(p3["slot_r_end"], pg["slot_s_end"] * n)
    assert list(p3["slot_r_end"][:3]) == [3, 3, 12]
    p1 = lib.host_plan_sample(mc, ids, cu, 1, n, 1.0, seeds)
    assert p1["decode_rows"].size == 0 and p1["rows_used"] == T + R


def test_plan_sample_refusals():
    ids, cu, lens = _prompts()
    seeds = np.arange(4, dtype=np.uint64)
    mk = lambda **kw: lib.make_model_cfg(GI.TINY_CFG, **dict(dict(max_tokens=64, max_seqs=12, max_labelled=12, max_position=48), **kw))  # noqa: E731
    mc = mk()
    ok = dict(max_new=8, n_samples=3, temperature=1.0, seq_seeds=seeds)
    lib.host_plan_sample(mc, ids, cu, **ok)                                         # 40 + 8 <= 48, 12 rows
    for kw, msg in ((dict(max_new=0), "max_new_tokens out of range"), (dict(max_new=257), "max_new_tokens out of range"), (dict(max_new=9), "exceeds max_position"),
                    (dict(eos_ids=(256,)), "eos id out of vocabulary"), (dict(eos_ids=tuple(range(17))), "more than 16 eos ids"),
                    (dict(n_samples=0), r"n_samples out of range \(1..64\)"), (dict(n_samples=65), r"n_samples out of range \(1..64\)"),
                    (dict(n_samples=4), r"n_seqs \* n_samples exceeds max_seqs or max_labelled"),
                    (dict(temperature=0.0), "temperature must be finite and in"), (dict(temperature=0.00999), "temperature must be finite and in"),
                    (dict(temperature=100.01), "temperature must be finite and in"), (dict(temperature=float("nan")), "temperature must be finite and in"),
                    (dict(temperature=float("inf")), "temperature must be finite and in"), (dict(temperature=-1.0), "temperature must be finite and in"),
                    (dict(seq_seeds=None), "null seq_seeds")):
        with pytest.raises(lib.TstError, match=msg):
            lib.host_plan_sample(mc, ids, cu, **dict(ok, **kw))
    lib.host_plan_sample(mc, ids, cu, **dict(ok, temperature=0.01))
    lib.host_plan_sample(mc, ids, cu, **dict(ok, temperature=100.0))
    lib.host_plan_sample(mc, ids, cu, **dict(ok, eos_ids=tuple(range(16))))
    with pytest.raises(lib.TstError, match=r"n_seqs \* n_samples exceeds"):
        lib.host_plan_sample(mk(max_labelled=11), ids, cu, **ok)
    with pytest.raises(lib.TstError, match=r"n_seqs \* n_samples exceeds"):
        lib.host_plan_sample(mk(max_seqs=11), ids, cu, **ok)
    # the rows fit max_seqs and max_labelled, not max_tokens: a decode step runs the model over n_seqs * n_samples token rows (prompts shorter than n_samples)
    short_ids, short_cu = np.arange(8, dtype=np.int32), np.array([0, 4, 8], np.int32)
    big = mk(max_tokens=64, max_seqs=128, max_labelled=128)
    lib.host_plan_sample(big, short_ids, short_cu, 8, 32, 1.0, seeds[:2])          # 64 rows <= max_tokens
    with pytest.raises(lib.TstError, match=r"n_seqs \* n_samples exceeds max_tokens"):
        lib.host_plan_sample(big, short_ids, short_cu, 8, 33, 1.0, seeds[:2])      # 66 rows > 64
    with pytest.raises(lib.TstError, match=r"n_seqs \* n_samples exceeds max_tokens"):
        lib.host_plan_sample(big, short_ids, short_cu, 8, 64, 1.0, seeds[:2])
    with pytest.raises(lib.TstError, match="more sequences than max_labelled"):
        lib.host_plan_sample(mk(max_labelled=3), ids, cu, **ok)
    with pytest.raises(lib.TstError, match="cu_seqlens must be non-decreasing"):
        lib.host_plan_sample(mc, ids, np.array([0, 3, 2, 44, 61], np.int32), **ok)
    with pytest.raises(lib.TstError, match="seq_slot must be non-decreasing"):
        lib.host_plan_sample(mc, ids, cu, seq_slot=[0, 0, 1, 1], **ok)


# ------------------------------------------------------------------------------------------------ seeds, answers, MRA
def test_sample_seeds_depend_on_the_run_seed_and_the_pair_index_only():
    idx = np.arange(10_000)
    a = sample_seeds(7, idx)
    assert a.dtype == np.uint64 and len(set(map(int, a))) == len(idx)
    np.testing.assert_array_equal(sample_seeds(7, idx), a)
    perm = np.random.default_rng(0).permutation(len(idx))
    np.testing.assert_array_equal(sample_seeds(7, idx[perm]), a[perm])
    np.testing.assert_array_equal(sample_seeds(7, [5, 5, 9999]), a[[5, 5, 9999]])
    assert not (sample_seeds(8, idx[:100]) == a[:100]).any()
    assert int(sample_seeds(0, [0])[0]) == 0xE220A8397B1DCDAF   # splitmix64's first output for seed 0
    assert int(sample_seeds(2 ** 64 - 1, [3])[0]) == int(sample_seeds(-1, [3])[0])


def test_mean_relative_accuracy():
    assert mean_relative_accuracy(2, 2) == 1.0 and mean_relative_accuracy("2.0", " 2") == 1.0
    assert mean_relative_accuracy(1.5, 1) == 0.0 and mean_relative_accuracy(0.5, 1) == 0.0      # relative error 0.5 is not < 0.5
    assert mean_relative_accuracy(1.49, 1) == 0.1
    # the ten thresholds 0.50, 0.45, ..., 0.05: an error exactly ON a threshold does not pass it
    for k in range(10):
        edge = (50 - 5 * k) / 100
        assert mean_relative_accuracy(round(1 + edge, 2), 1) == k / 10
        assert mean_relative_accuracy(round(1 - edge, 2), 1) == k / 10
        assert mean_relative_accuracy(round(1 + edge - 0.01, 2), 1) == (k + 1) / 10
    assert mean_relative_accuracy(0.96, 1) == 1.0 and mean_relative_accuracy(0.95, 1) == 0.9
    assert mean_relative_accuracy(-3, -2.9) == 1.0 and mean_relative_accuracy(3, -3) == 0.0
    assert mean_relative_accuracy("about 19 chairs", "20") == 0.9
    for bad in ("", "none", "n/a", None, "."):
        assert mean_relative_accuracy(bad, 3) == 0.0
    assert mean_relative_accuracy(0, 0) == 1.0 and mean_relative_accuracy(0.1, 0) == 0.0
    with pytest.raises(ValueError):
        mean_relative_accuracy(1, "many")
    assert parse_number(" 2") == 2.0 and parse_number("-.5e1x") == -5.0 and parse_number("x3.25m") == 3.25 and parse_number("1,200") == 1.0
    assert parse_number("e5") == 5.0 and parse_number("--") is None and parse_number(float("nan")) is None and parse_number(7) == 7.0


def test_sampled_answers_cut_the_eos_and_count_matches():
    smp = [types.SimpleNamespace(ids=np.array([9, 9, 9, 4, 5], np.int32), n_prompt=3), types.SimpleNamespace(ids=np.array([1, 7], np.int32), n_prompt=1),
           types.SimpleNamespace(ids=np.array([1, 2], np.int32), n_prompt=2)]
    tok = np.array([[[4, 5, 2, -1], [4, 5, 6, 7], [4, 2, -1, -1], [2, -1, -1, -1]],
                    [[7, 7, 7, 7], [7, 2, -1, -1], [8, 7, 2, -1], [2, -1, -1, -1]],
                    [[1, 2, -1, -1]] * 4], np.int32)
    n_new = np.array([[3, 4, 2, 1], [4, 2, 3, 1], [2, 2, 2, 2]], np.int32)
    logp = np.where(tok >= 0, -0.5, 0.0).astype(np.float32)
    out = sampled_answers(smp, tok, logp, n_new, eos_ids=(2,))
    assert out[0]["ids"] == [[4, 5], [4, 5, 6, 7], [4], []] and out[0]["match"] == 0.5
    assert out[0]["logp"] == [-1.5, -2.0, -1.0, -0.5]
    assert out[1]["ids"] == [[7, 7, 7, 7], [7], [8, 7], []] and out[1]["match"] == 0.5
    assert out[2]["match"] == 0.0 and out[2]["ids"] == [[1]] * 4           # a sample without a reference answer matches nothing
    out = sampled_answers(smp[:1], tok[:1], logp[:1], n_new[:1])            # no eos ids: nothing is stripped
    assert out[0]["ids"][0] == [4, 5, 2] and out[0]["ids"][3] == [2] and out[0]["match"] == 0.5


def test_records_with_a_tokenizer_carry_texts_and_mra():
    """fold_records with a decode function (CPU only: no context): texts for every draw, mra for the numeric references only"""
    from tst import diagnose as DG
    held = [types.SimpleNamespace(sid=0, kind="na", ids=np.array([9, 9, 20], np.int32), n_prompt=2),
            types.SimpleNamespace(sid=1, kind="mca", ids=np.array([9, 65], np.int32), n_prompt=1)]
    decode = lambda ids: " ".join("A" if t == 65 else str(t) for t in ids)   # noqa: E731
    smp = [dict(ids=[[20], [19, 3], [30], []], logp=[-1.0, -2.0, -3.0, -0.5], match=0.25), dict(ids=[[65], [66], [65], [65]], logp=[-1.0] * 4, match=0.75)]
    recs = DG.fold_records(held, 0, 0, [0.5, 0.5], [-1, 0], [1, 1], decode, samples=smp)
    assert recs[0]["samples"]["texts"] == ["20", "19 3", "30", ""]
    assert recs[0]["samples"]["mra"] == pytest.approx((1.0 + 0.9 + 0.0 + 0.0) / 4)
    assert recs[1]["samples"]["texts"] == ["A", "66", "A", "A"] and "mra" not in recs[1]["samples"]
    assert "texts" not in DG.fold_records(held, 0, 0, [0.5, 0.5], [-1, 0], [1, 1], samples=smp)[0]["samples"]


# ------------------------------------------------------------------------------------------------ what the GPU tests rest on, from the oracle alone
@pytest.mark.parametrize("temperature", SO.TEMPERATURES)
@pytest.mark.parametrize("lora_seed", SO.ADAPTERS, ids=["base", "lora99"])
@pytest.mark.parametrize("tag", list(G.FAMILIES))
def test_every_draw_of_the_strict_cases_is_decidable_twice_over(tag, lora_seed, temperature):
    """no draw of the oracle's trajectory has a top-1 / top-2 gap under 2 band under the case's pinned sample seed, and that seed is the first that passes"""
    tok, logp, gap, seeds = SO.sampled_reference(tag, lora_seed, temperature)
    S = len(G.make_prompts(G.FAMILIES[tag]))
    assert tok.shape == gap.shape == (S, SO.N_SAMPLES, G.MAX_NEW) and tok.size == 288 - 32 * (S == 8)
    print(f"{tag} {lora_seed} T={temperature}: smallest gap {gap.min():.3e}, 2 band = {2 * SO.band(temperature):.3e}")
    assert gap.min() >= 2 * SO.band(temperature)
    assert np.isfinite(logp).all() and (logp <= 0).all()
    for earlier in range(SO.case_seed(tag, lora_seed, temperature)):
        assert SO.sampled_reference(tag, lora_seed, temperature, earlier)[2].min() < 2 * SO.band(temperature)


def test_the_oracles_first_tokens_pass_the_coverage_chi_square():
    tag, temperature = "tiny", 1.0
    p = G.make_prompts(G.FAMILIES[tag])[SO.COVER_PROMPT]
    ids, cu = G.pack([p])
    O = np.asarray(G.make_oracle(tag).forward_logits(ids, cu, cu[1:] - 1), np.float64)[0]
    probs = np.exp(G.log_softmax(O / temperature))
    toks = np.array([SO.draw(O, temperature, SO.gumbel(seed, len(O), 0, i))[0] for seed in SO.cover_seeds() for i in range(SO.COVER_N)])
    chi2 = SO.first_token_chi2(np.bincount(toks, minlength=len(O)), probs, len(toks))
    print(f"chi-square of the oracle's {len(toks)} first tokens: {chi2:.2f}")
    assert len(toks) == 512 and chi2 < 43.3
    # the test has power: the same draws against the distribution at temperature 0.5 fail it
    assert SO.first_token_chi2(np.bincount(toks, minlength=len(O)), np.exp(G.log_softmax(O / 0.5)), len(toks)) > 43.3
