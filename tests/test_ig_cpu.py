"""CPU tests of integrated gradients: the fixtures' own invariants, the host side (csrc/host_logic.h plan_ig / trim_tokens_i32 through libtst_host.so),
tst.score.token_ig, the held-out loops on a fake context, the records, the command line and the run fingerprint. The GPU side is tests/test_ig_gpu.py."""
import dataclasses
import hashlib
import json
import types

import numpy as np
import pytest

import attribution_inputs as AI
import golden_inputs as GI
import ig_inputs as IG
from tst import data as D
from tst import lib


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("tag", list(AI.TAGS))
def test_fixture_invariants(golden_dir, tag):
    g = dict(np.load(f"{golden_dir}/ig_{tag}.npz"))
    ids, labels, cu = AI.batch(tag)
    T, S = len(ids), len(cu) - 1
    np.testing.assert_array_equal(g["option_ids"], AI.option_ids(tag))
    for sname in AI.SETS:
        for pname in IG.PATTERNS:
            base = IG.baseline_ids(tag, pname)
            assert base.dtype == np.int32 and (base[labels == -100] == IG.BASELINE_ID).all() and ((base == IG.BASELINE_ID).all() if pname == "all" else (base == ids)[labels != -100].all())
            for aname in AI.ADAPTERS:
                key = IG.key(sname, pname, aname)
                for pre in ("ref", "hf32", "hf_bf16"):
                    assert g[key + pre + "_ig"].shape == (T,) and g[key + pre + "_logs"].shape == (S,) and g[key + pre + "_logs_base"].shape == (S,)
                assert g[key + "ref_ig"].dtype == np.float64 and np.isfinite(g[key + "ref_ig"]).all() and g[key + "ref_ig64"].shape == (T,)
                # the generator's self-check: completeness of the fp64 reference within 2 % of |dJ| wherever |dJ| >= 0.05, at m = 64 -- or, for a case whose
                # quadrature has not converged by then, at m = 128 (DESIGN.md section 14 lists those cases); the bound is the same
                gap = g[key + "ref_gap128"] if key + "ref_gap128" in g else g[key + "ref_gap64"]
                dJ = g[key + "ref_logs"] - g[key + "ref_logs_base"]
                assert gap.shape == (S,) and (np.isnan(gap) == (np.abs(dJ) < 0.05)).all()
                assert np.nanmax(gap) <= 0.02, (key, gap)
                if key + "ref_gap128" in g:
                    assert np.nanmax(g[key + "ref_gap64"]) > 0.02
                delta = np.array([g[key + "ref_ig64"][cu[s]:cu[s + 1]].sum() for s in range(S)]) - dJ
                np.testing.assert_allclose(g[key + "delta_ref64"], delta, rtol=0, atol=1e-12)
                assert g[key + "floor32"] <= 1e-4 and g[key + "floor16"] > g[key + "floor32"]
                assert AI.seq_dev(g[key + "hf32_ig"], g[key + "ref_ig"], cu).max() == g[key + "floor32"]
                assert AI.seq_dev(g[key + "hf_bf16_ig"], g[key + "ref_ig"], cu).max() == g[key + "floor16"]
                # a token that is its own baseline is not interpolated: exactly 0 (the `prompt` pattern: every labelled position), in every precision
                for pre in ("ref", "hf32", "hf_bf16"):
                    assert (g[key + pre + "_ig"][base == ids] == 0).all()
                if pname == "prompt":
                    assert (base == ids)[labels != -100].all() and (g[key + "ref_ig"][labels != -100] == 0).all()
                # the last token of a sequence is read by nothing: its gradient, and so its share, is exactly 0
                assert (g[key + "ref_ig"][cu[1:] - 1] == 0).all()
                # log s of the real prompt does not depend on the baseline
                np.testing.assert_array_equal(g[key + "ref_logs"], g[IG.key(sname, "all", aname) + "ref_logs"])
            np.testing.assert_allclose(g[f"{sname}/{pname}/l99_vs_l7"], AI.seq_dev(g[IG.key(sname, pname, "l7") + "ref_ig"], g[IG.key(sname, pname, "l99") + "ref_ig"], cu))


# ------------------------------------------------------------------------------------------------ host logic through libtst_host
def test_plan_ig_through_the_host_library():
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=64, max_seqs=4, max_labelled=8, max_position=32)
    V = GI.TINY_CFG["vocab_size"]
    ids = np.arange(8, dtype=np.int32)
    cu = [0, 1, 3, 8]
    base = np.ones(8, np.int32)
    for m in (1, 16, lib.IG_MAX_STEPS):
        alpha = lib.host_plan_ig(mc, ids, cu, base, m)
        assert alpha.dtype == np.float32 and len(alpha) == m
        np.testing.assert_array_equal(alpha, [IG.alpha(k, m) for k in range(1, m + 1)])
        assert (np.diff(alpha) > 0).all() and 0 < alpha[0] and alpha[-1] < 1
    hi, lo = base.copy(), base.copy()
    hi[7], lo[0] = V, -1
    for kw, msg in ((dict(baseline_ids=None, n_steps=4), "null baseline_ids"), (dict(baseline_ids=hi, n_steps=4), "baseline id out of vocabulary"),
                    (dict(baseline_ids=lo, n_steps=4), "baseline id out of vocabulary"), (dict(baseline_ids=base, n_steps=0), "n_steps out of range"),
                    (dict(baseline_ids=base, n_steps=-3), "n_steps out of range"), (dict(baseline_ids=base, n_steps=lib.IG_MAX_STEPS + 1), "n_steps out of range")):
        with pytest.raises(lib.TstError, match=msg):
            lib.host_plan_ig(mc, ids, cu, **kw)
    with pytest.raises(lib.TstError, match="one entry per token"):
        lib.host_plan_ig(mc, ids, cu, base[:-1], 4)
    hi[7] = V - 1
    lib.host_plan_ig(mc, ids, cu, hi, 4)   # the last id of the vocabulary is one


def test_trim_through_the_host_library():
    tr = lib.host_trim_tokens
    np.testing.assert_array_equal(tr([5], [0, 1], [0, 1]), [5])                                     # length 1 is never trimmed
    np.testing.assert_array_equal(tr([5, 6], [0, 1], [0, 2]), [5])                                  # length 2, trimmed
    src = np.arange(1, 9, dtype=np.int32)
    np.testing.assert_array_equal(tr(src, [0, 1, 2, 6], [0, 1, 3, 8]), [1, 2, 4, 5, 6, 7])          # lengths 1, 2, 5, trimmed
    np.testing.assert_array_equal(tr(src, [0, 1, 3, 8], [0, 1, 3, 8]), src)                         # ... untrimmed
    # the round trip with the fetch side: a per-token value comes back where it was, 0 where the device did not run the token
    back = lib.host_untrim_tokens(tr(src, [0, 1, 2, 6], [0, 1, 3, 8]).astype(np.float32), [0, 1, 2, 6], [0, 1, 3, 8])
    np.testing.assert_array_equal(back, [1, 2, 0, 4, 5, 6, 7, 0])
    with pytest.raises(lib.TstError):
        tr([1, 2], [0, 2], [0, 1])    # longer on the device than in the caller's batch
    with pytest.raises(lib.TstError):
        tr([1], [0, 2], [0, 2])       # fewer values than the caller's map covers


def test_every_new_symbol_is_declared_in_its_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for header, table, names in (("tst_hip.h", lib.SIGNATURES, ("tst_attribute_ig_async", "tst_attribute_ig_fetch", "tst_attribute_ig")),
                                 ("tst_hip_lab.h", lib.LAB_SIGNATURES, ("tst_k_embed_interp", "tst_k_embed_interp_f32", "tst_k_token_ig", "tst_k_token_ig_f32")),
                                 ("tst_host.h", lib.HOST_SIGNATURES, ("tst_host_plan_ig", "tst_host_trim_tokens"))):
        text = open(os.path.join(root, "include", header)).read()
        for n in names:
            assert n in table and f"int {n}(" in text, n
    assert f"#define TST_IG_MAX_STEPS {lib.IG_MAX_STEPS}\n" in open(os.path.join(root, "include", "tst_hip.h")).read()


# ------------------------------------------------------------------------------------------------ tst.score.token_ig, the held-out loops
def _sample(sid, prompt, answer, kind="na"):
    return types.SimpleNamespace(sid=sid, ids=np.array(list(prompt) + list(answer), np.int32), n_prompt=len(prompt), n_answer=len(answer), kind=kind, gt_option=0)


def test_token_ig_on_hand_made_arrays():
    from tst.score import ig_baseline_ids, token_ig
    smp = [_sample(0, [5, 6, 7], [8]), _sample(1, [9], [10, 11], kind="mca")]
    ig = np.array([1, -2, 3, 0.5, 4, 0, 0], np.float32)
    out = token_ig(smp, ig, np.array([-0.5, -2.0], np.float32), np.array([-3.5, -5.0], np.float32))
    np.testing.assert_array_equal(out[0]["ig"], [1, -2, 3])    # the prompt slice
    np.testing.assert_array_equal(out[1]["ig"], [4])
    assert (out[0]["log_s"], out[0]["log_s_base"], out[1]["log_s"], out[1]["log_s_base"]) == (-0.5, -3.5, -2.0, -5.0)
    assert out[0]["delta"] == pytest.approx(2.5 - 3.0) and out[1]["delta"] == pytest.approx(4.0 - 3.0)   # the sum runs over ALL tokens of the sample
    np.testing.assert_array_equal(ig_baseline_ids(smp, 2), [2, 2, 2, 8, 2, 10, 11])   # prompt tokens move, answer tokens are their own baseline
    assert ig_baseline_ids(smp, 2).dtype == np.int32
    with pytest.raises(ValueError):
        token_ig(smp, ig[:-1], [0, 0], [0, 0])
    with pytest.raises(ValueError):
        token_ig(smp, ig, [0, 0], [0])


class FakeCtx:
    """ig[t] = the token's id + 1000 slot where the token moves, 0 where it is its own baseline; logs[i] = -(sequence index), logs_base = logs - steps"""

    def __init__(self, n_stack=1):
        self.n_stack, self.calls, self._pending = n_stack, [], None

    def attribute_ig_async(self, ids, labels, cu, baseline_ids, n_steps, seq_kind=None, option_ids=(), seq_slot=None):
        assert self._pending is None, "one attribution may be pending per context"
        n = len(cu) - 1
        slots = np.zeros(n, np.int32) if seq_slot is None else np.asarray(seq_slot)
        assert (np.diff(slots) >= 0).all() and slots.max() < self.n_stack and len(labels) == len(ids) == len(baseline_ids) and len(seq_kind) == n
        self.calls.append((n, tuple(int(s) for s in slots), tuple(int(k) for k in seq_kind), tuple(option_ids), int(n_steps), tuple(int(b) for b in baseline_ids)))
        moved = np.asarray(ids) != np.asarray(baseline_ids)
        logs = -np.arange(n, dtype=np.float32)
        self._pending = (np.where(moved, np.asarray(ids, np.float32) + 1000 * np.repeat(slots, np.diff(cu)), 0).astype(np.float32), logs, logs - n_steps)

    def attribute_ig_fetch(self):
        out, self._pending = self._pending, None
        return out


def test_attribute_ig_heldout_loops_keep_order_batches_kinds_slots_and_baselines():
    from tst.trainer import TrainArgs, IG, attribute_ig_heldout, run_heldout_concurrent, run_heldout_stacked
    args = TrainArgs(per_device_eval_batch_size=4, attribute_ig=8, attribute_baseline_id=7, option_ids=(3, 4))
    assert (args.attribute_ig, args.attribute_baseline_id, args.attribute) == (8, 7, False)
    sets = [[_sample(100 * f + i, [100 * f + 10 * i, 100 * f + 10 * i + 1], [3], kind="mca" if i % 2 else "na") for i in range(n)] for f, n in enumerate((10, 3, 6))]
    c = FakeCtx()
    got = attribute_ig_heldout(c, sets[0], args)
    assert [call[0] for call in c.calls] == [4, 4, 2] and c.calls[0][2:5] == ((0, 1, 0, 1), (3, 4), 8)
    assert c.calls[0][5] == (7, 7, 3) * 4                                                # the prompt of baseline tokens, the answer token itself
    assert [list(g["ig"]) for g in got] == [[10 * i, 10 * i + 1] for i in range(10)]     # the prompt tokens of every sample, in input order
    assert [g["log_s"] for g in got] == [0, -1, -2, -3, 0, -1, -2, -3, 0, -1] and all(g["log_s_base"] == g["log_s"] - 8 for g in got)
    assert all(g["delta"] == pytest.approx(float(np.sum(g["ig"])) - 8) for g in got)
    cs = [FakeCtx() for _ in sets]
    outs = run_heldout_concurrent(IG, cs, sets, args)
    assert [[call[0] for call in c.calls] for c in cs] == [[4, 4, 2], [3], [4, 2]]
    for smp, out in zip(sets, outs):
        assert [list(g["ig"]) for g in out] == [[float(t) for t in x.ids[:2]] for x in smp]
    cs = [FakeCtx(2), FakeCtx(2)]
    outs = run_heldout_stacked(IG, cs, sets, args)
    assert [call[:2] for call in cs[0].calls] == [(7, (0, 0, 0, 0, 1, 1, 1)), (4, (0, 0, 0, 0)), (2, (0, 0))]
    assert [len(o) for o in outs] == [10, 3, 6]
    assert [list(g["ig"]) for g in outs[1]] == [[float(t) + 1000 for t in x.ids[:2]] for x in sets[1]]      # fold 1 ran in slot 1
    assert [list(g["ig"]) for g in outs[0] + outs[2]] == [[float(t) for t in x.ids[:2]] for x in sets[0] + sets[2]]


# ------------------------------------------------------------------------------------------------ records, command line, fingerprint
def test_fold_records_carry_attr_ig_only_when_asked():
    from tst.diagnose import fold_records
    held = [_sample(4, [20, 21, 22], [30]), _sample(9, [23], [31, 32])]
    plain = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1])
    assert list(plain[0]) == ["id", "fold", "round", "s", "pred", "correct", "kind"]        # key order is part of the shard's bytes
    ig = [dict(ig=np.array([1, -5, 3], np.float32), log_s=-1.0, log_s_base=-2.5, delta=0.125), dict(ig=np.array([0.5], np.float32), log_s=-2.0, log_s_base=-2.0, delta=0.0)]
    recs = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], ig=ig)
    assert recs[0]["attr_ig"] == dict(ig=[1.0, -5.0, 3.0], log_s_base=-2.5, delta=0.125) and recs[1]["attr_ig"] == dict(ig=[0.5], log_s_base=-2.0, delta=0.0)
    assert "attr_ig_top" not in recs[0] and "attr" not in recs[0] and list(recs[0])[:7] == list(plain[0])
    recs = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], decode=lambda ids: "|".join(map(str, ids)), ig=ig, attr_top=2)
    assert recs[0]["attr_ig_top"] == [["21", -5.0], ["22", 3.0]] and recs[1]["attr_ig_top"] == [["23", 0.5]]   # largest |ig| first, with sign
    json.dumps(recs)


def test_cli_flags(tmp_path):
    from tst import cli
    a = cli.build_parser().parse_args(["diagnose", "--out", "x"])
    t = cli._args_to_train(a)
    assert (a.attribute_ig, a.attribute_baseline_id) == (0, None) and (t.attribute_ig, t.attribute_baseline_id, t.attribute) == (0, 0, False)
    a = cli.build_parser().parse_args(["prune", "--out", "x", "--attribute-ig", "16", "--attribute-baseline-id", "3", "--attribute-top", "2"])
    t = cli._args_to_train(a)
    assert (t.attribute_ig, t.attribute_baseline_id, t.attribute_top, t.attribute, t.generate) == (16, 3, 2, False, False)
    assert a.attribute_baseline_source == "--attribute-baseline-id"
    # the default baseline id: pad, else eos, else 0 -- and where it came from
    a = cli.build_parser().parse_args(["diagnose", "--out", "x", "--attribute-ig", "8"])
    assert cli._args_to_train(a).attribute_baseline_id == 0 and a.attribute_baseline_source == "default"
    d = tmp_path / "m"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(eos_token_id=[11, 12])))
    a = cli.build_parser().parse_args(["diagnose", "--out", "x", "--attribute-ig", "8", "--model-dir", str(d)])
    assert cli._args_to_train(a).attribute_baseline_id == 11 and a.attribute_baseline_source == "eos id"
    (d / "config.json").write_text(json.dumps(dict(eos_token_id=[11, 12], pad_token_id=5)))
    a = cli.build_parser().parse_args(["diagnose", "--out", "x", "--attribute-ig", "8", "--model-dir", str(d)])
    assert cli._args_to_train(a).attribute_baseline_id == 5 and a.attribute_baseline_source.startswith("pad_token_id")
    for bad in (["--attribute-ig", "8", "--dp", "2"], ["--attribute-ig", "8", "--layout", "dp-stacked"], ["--attribute-ig", "257"], ["--attribute-ig", "-1"],
                ["--attribute-ig", "8", "--attribute-top", "-1"], ["--attribute-ig", "8", "--attribute-baseline-id", "-2"], ["--attribute-baseline-id", "3"]):
        with pytest.raises(SystemExit):
            cli._args_to_train(cli.build_parser().parse_args(["diagnose", "--out", "x"] + bad))
    # both attributions may run in one sweep
    t = cli._args_to_train(cli.build_parser().parse_args(["diagnose", "--out", "x", "--attribute", "--attribute-ig", "4"]))
    assert t.attribute and t.attribute_ig == 4


def test_diagnose_refuses_the_data_parallel_layouts():
    from tst import diagnose as DG
    from tst.trainer import TrainArgs
    samples = D.synth_vsi(6, vocab=256, seed=4)
    with pytest.raises(ValueError, match="data-parallel"):
        DG.diagnose_dp(None, samples, 2, TrainArgs(attribute_ig=4), 0, 1, 1)
    with pytest.raises(ValueError, match="data-parallel"):
        DG.diagnose_dp_stacked([None], samples, 2, TrainArgs(attribute_ig=4), 0, 1)


def test_run_fingerprint_is_the_parents_without_the_flag_and_differs_with_it():
    from tst.diagnose import run_fingerprint
    from tst.trainer import TrainArgs
    samples = D.synth_vsi(9, vocab=256, seed=4)
    ident = dict(model="tiny", weights_seed=0)
    # the fields TrainArgs had before any attribution existed, with their values: what a run directory written then was fingerprinted with
    parent_fields = dict(learning_rate=1e-3, num_train_epochs=1, per_device_train_batch_size=16, per_device_eval_batch_size=16, warmup_steps=0, weight_decay=0.0,
                         adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, max_grad_norm=1.0, seed=42, lora_r=16, lora_alpha=32.0,
                         lora_targets=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"], logging_steps=50,
                         gradient_accumulation_steps=1, option_ids=list(D.OPTION_IDS))
    h = hashlib.sha256()
    h.update(json.dumps(dict(args=dict(sorted(parent_fields.items())), k=5, n=len(samples), extra=ident), sort_keys=True).encode())
    for x in samples:
        h.update(np.int64(x.sid).tobytes())
        h.update(np.ascontiguousarray(x.ids, dtype=np.int32).tobytes())
        h.update(np.int32(x.n_prompt).tobytes())
    kw = dict(num_train_epochs=1, learning_rate=1e-3)
    args = TrainArgs(**kw)
    off = run_fingerprint(samples, 5, args, ident)
    assert off == h.hexdigest()
    assert set(dataclasses.asdict(args)) == set(parent_fields) | {"generate", "max_new_tokens", "eos_ids"}   # the settings are no dataclass fields
    assert run_fingerprint(samples, 5, TrainArgs(**kw, attribute_baseline_id=9, attribute_top=2), ident) == off   # dormant while the flag is off
    attr = run_fingerprint(samples, 5, TrainArgs(**kw, attribute=True), ident)
    assert attr == run_fingerprint(samples, 5, TrainArgs(**kw, attribute=True, attribute_baseline_id=9), ident)   # --attribute alone is what it was
    on = [run_fingerprint(samples, 5, TrainArgs(**kw, **more), ident) for more in
          (dict(attribute_ig=16), dict(attribute_ig=32), dict(attribute_ig=16, attribute_baseline_id=9), dict(attribute_ig=16, attribute_top=2),
           dict(attribute_ig=16, attribute=True))]
    assert len({off, attr, *on}) == 7
