"""CPU tests of token attribution: the fixtures' integrity, the host side of the fetch (csrc/host_logic.h through libtst_host.so), tst.score.token_attribution,
the held-out loops on a fake context, the command line and the run fingerprint. The GPU side is tests/test_attribution_gpu.py."""
import dataclasses
import hashlib
import json
import types

import numpy as np
import pytest

import attribution_inputs as AI
import golden_inputs as GI
from tst import data as D
from tst import lib


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("tag", list(AI.TAGS))
def test_fixture_integrity(golden_dir, tag):
    g = dict(np.load(f"{golden_dir}/attr_{tag}.npz"))
    ids, labels, cu = AI.batch(tag)
    T, S = len(ids), len(cu) - 1
    np.testing.assert_array_equal(g["option_ids"], AI.option_ids(tag))
    opt = AI.option_ids(tag)
    assert len(opt) == 4 and len(set(opt.tolist())) == 4 and all(labels[cu[s + 1] - 1] in opt for s in (0, 3))
    for sname in AI.SETS:
        for aname in AI.ADAPTERS:
            key = f"{sname}/{aname}/"
            for pre in ("ref", "hf32", "hf_bf16"):
                assert g[key + pre + "_gxi"].shape == (T,) and g[key + pre + "_gnorm"].shape == (T,) and g[key + pre + "_logs"].shape == (S,)
            assert g[key + "ref_gxi"].dtype == np.float64 and np.isfinite(g[key + "ref_gxi"]).all() and (g[key + "ref_gnorm"] >= 0).all()
            assert g[key + "floor32"].shape == (2,) and (g[key + "floor32"] <= 1e-4).all() and (g[key + "floor16"] > g[key + "floor32"]).all()
            assert g[key + "fd_check"] <= 1e-6   # the reference against a central difference of J, checked when the fixture was written
            assert (g[key + "ref_logs"] < 0).all()
            # the last token of a sequence is read by nothing: its gradient is exactly 0 (what the engine reports for a trimmed token)
            assert (g[key + "ref_gnorm"][cu[1:] - 1] == 0).all() and (g[key + "ref_gxi"][cu[1:] - 1] == 0).all()
            for pre in ("hf32", "hf_bf16"):
                for i, o in enumerate(AI.OUTPUTS):
                    assert AI.seq_dev(g[key + f"{pre}_{o}"], g[key + f"ref_{o}"], cu).max() == g[key + ("floor32" if pre == "hf32" else "floor16")][i]
        # the open sequences of the two sets are the same computation
        for o in AI.OUTPUTS:
            a, b = g[f"mix/l99/ref_{o}"], g[f"open/l99/ref_{o}"]
            np.testing.assert_array_equal(a[cu[1]:cu[3]], b[cu[1]:cu[3]])
            assert not np.array_equal(a[:cu[1]], b[:cu[1]])


@pytest.mark.parametrize("tag", list(AI.TAGS))
def test_fixtures_of_the_two_adapter_sets_can_be_told_apart_by_gnorm(golden_dir, tag):
    """what tests/test_attribution_gpu.py's stacked test relies on: on every sequence the gnorm references of adapters 99 and 7 differ by more than
    4 x floor16 of the tag, so a result within 2 x floor16 of one lies more than 2 x floor16 from the other"""
    g = dict(np.load(f"{golden_dir}/attr_{tag}.npz"))
    floor = np.max([g[f"{s}/{a}/floor16"] for s in AI.SETS for a in AI.ADAPTERS], axis=0)[1]
    cu = AI.batch(tag)[2]
    for sname in AI.SETS:
        d = np.minimum(AI.seq_dev(g[f"{sname}/l7/ref_gnorm"], g[f"{sname}/l99/ref_gnorm"], cu), AI.seq_dev(g[f"{sname}/l99/ref_gnorm"], g[f"{sname}/l7/ref_gnorm"], cu))
        np.testing.assert_allclose(g[f"{sname}/l99_vs_l7"][1], AI.seq_dev(g[f"{sname}/l7/ref_gnorm"], g[f"{sname}/l99/ref_gnorm"], cu))
        assert (d > 4 * floor).all(), (tag, sname, d, floor)


# ------------------------------------------------------------------------------------------------ host logic through libtst_host
def test_untrim_through_the_host_library():
    un = lib.host_untrim_tokens
    np.testing.assert_array_equal(un([1.5], [0, 1], [0, 1]), [1.5])                                  # length 1 is never trimmed
    np.testing.assert_array_equal(un([1.5], [0, 1], [0, 2]), [1.5, 0.0])                             # length 2, trimmed
    np.testing.assert_array_equal(un([1.5, 2.5], [0, 2], [0, 2]), [1.5, 2.5])                        # length 2, untrimmed
    src = np.arange(1, 7, dtype=np.float32)
    np.testing.assert_array_equal(un(src, [0, 1, 2, 6], [0, 1, 3, 8]), [1, 2, 0, 3, 4, 5, 6, 0])     # several sequences, lengths 1, 2, 5, trimmed
    np.testing.assert_array_equal(un(np.arange(8.0), [0, 1, 3, 8], [0, 1, 3, 8]), np.arange(8.0))    # ... untrimmed
    with pytest.raises(lib.TstError):
        un([1.0, 2.0], [0, 2], [0, 1])    # longer on the device than in the caller's batch
    with pytest.raises(lib.TstError):
        un([1.0], [0, 2], [0, 2])         # fewer values than the device map covers


def test_plan_attribute_through_the_host_library():
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=64, max_seqs=4, max_labelled=8, max_position=32)
    ids = np.arange(8, dtype=np.int32)
    labels = np.array([9, -100, 7, -100, -100, 3, 4, 5], np.int32)
    cu = [0, 1, 3, 8]
    w, k, q = lib.host_plan_attribute(mc, ids, labels, cu, [0, 1, 0], [2, 7, 11])
    np.testing.assert_array_equal(k, [1, 0, 0, 0])
    np.testing.assert_array_equal(q, [1, 2, 2, 2])
    np.testing.assert_allclose(w, [1, 1 / 3, 1 / 3, 1 / 3], rtol=1e-7)
    plan = lib.host_plan_batch(mc, ids, labels, cu)
    np.testing.assert_array_equal(plan["row_seq"], q)   # the same rows in the same order as the batch plan's
    for kw, msg in ((dict(seq_kind=[0, 1, 0], option_ids=[2, 11]), "not one of the option ids"), (dict(seq_kind=[0, 0, 1], option_ids=[2, 7]), "exactly one"),
                    (dict(seq_kind=[0, 1, 0]), "n_opt == 0"), (dict(seq_kind=[0, 3, 0], option_ids=[7]), "seq_kind"),
                    (dict(option_ids=[256]), "option id"), (dict(option_ids=list(range(257))), "n_opt")):
        with pytest.raises(lib.TstError, match=msg):
            lib.host_plan_attribute(mc, ids, labels, cu, **kw)
    with pytest.raises(lib.TstError, match="no labelled"):
        lib.host_plan_attribute(mc, ids, np.full(8, -100, np.int32), cu)


def test_every_new_symbol_is_declared_in_its_header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for header, table, names in (("tst_hip.h", lib.SIGNATURES, ("tst_attribute_async", "tst_attribute_fetch", "tst_attribute")),
                                 ("tst_hip_lab.h", lib.LAB_SIGNATURES, ("tst_k_attr_seed", "tst_k_attr_seed_f32", "tst_k_token_attr", "tst_k_token_attr_f32")),
                                 ("tst_host.h", lib.HOST_SIGNATURES, ("tst_host_plan_attribute", "tst_host_untrim_tokens"))):
        text = open(os.path.join(root, "include", header)).read()
        for n in names:
            assert n in table and f"int {n}(" in text, n


# ------------------------------------------------------------------------------------------------ tst.score.token_attribution, the held-out loops
def _sample(sid, prompt, answer, kind="na"):
    return types.SimpleNamespace(sid=sid, ids=np.array(list(prompt) + list(answer), np.int32), n_prompt=len(prompt), n_answer=len(answer), kind=kind, gt_option=0)


def test_token_attribution_on_hand_made_arrays():
    from tst.score import attribution_kinds, token_attribution
    smp = [_sample(0, [5, 6, 7], [8]), _sample(1, [9], [10, 11], kind="mca")]
    gxi = np.array([1, -2, 3, 0, 4, 5, 0], np.float32)
    gnorm = np.array([1, 2, 1, 0, 0, 6, 0], np.float32)
    out = token_attribution(smp, gxi, gnorm, np.array([-0.5, -2.0], np.float32))
    np.testing.assert_array_equal(out[0]["gxi"], [1, -2, 3])
    np.testing.assert_array_equal(out[0]["gnorm"], [1, 2, 1])
    np.testing.assert_allclose(out[0]["share"], [0.25, 0.5, 0.25])
    assert out[0]["log_s"] == -0.5 and out[1]["log_s"] == -2.0
    np.testing.assert_array_equal(out[1]["gxi"], [4])
    np.testing.assert_array_equal(out[1]["share"], [0])   # a prompt whose gradient is exactly zero gets no share, not a NaN
    np.testing.assert_array_equal(attribution_kinds(smp), [0, 1])
    with pytest.raises(ValueError):
        token_attribution(smp, gxi[:-1], gnorm[:-1], [0, 0])


class FakeCtx:
    """gxi[t] = the token's id + 1000 slot, gnorm[t] = its position in the batch, logs[i] = -(sequence index); records every call"""

    def __init__(self, n_stack=1):
        self.n_stack, self.calls, self._pending = n_stack, [], None

    def attribute_async(self, ids, labels, cu, seq_kind=None, option_ids=(), seq_slot=None):
        assert self._pending is None, "one attribution may be pending per context"
        n = len(cu) - 1
        slots = np.zeros(n, np.int32) if seq_slot is None else np.asarray(seq_slot)
        assert (np.diff(slots) >= 0).all() and slots.max() < self.n_stack and len(labels) == len(ids) and len(seq_kind) == n
        self.calls.append((n, tuple(int(s) for s in slots), tuple(int(k) for k in seq_kind), tuple(option_ids)))
        self._pending = (np.asarray(ids, np.float32) + 1000 * np.repeat(slots, np.diff(cu)), np.arange(len(ids), dtype=np.float32), -np.arange(n, dtype=np.float32))

    def attribute_fetch(self):
        out, self._pending = self._pending, None
        return out


def test_attribute_heldout_loops_keep_order_batches_kinds_and_slots():
    from tst.trainer import TrainArgs, ATTRIBUTE, attribute_heldout, run_heldout_concurrent, run_heldout_stacked
    args = TrainArgs(per_device_eval_batch_size=4, attribute=True, option_ids=(3, 4))
    sets = [[_sample(100 * f + i, [100 * f + 10 * i, 100 * f + 10 * i + 1], [3], kind="mca" if i % 2 else "na") for i in range(n)] for f, n in enumerate((10, 3, 6))]
    c = FakeCtx()
    got = attribute_heldout(c, sets[0], args)
    assert [call[0] for call in c.calls] == [4, 4, 2] and c.calls[0][2:] == ((0, 1, 0, 1), (3, 4))
    assert [list(g["gxi"]) for g in got] == [[10 * i, 10 * i + 1] for i in range(10)]     # the prompt tokens of every sample, in input order
    assert [g["log_s"] for g in got] == [0, -1, -2, -3, 0, -1, -2, -3, 0, -1]
    cs = [FakeCtx() for _ in sets]
    outs = run_heldout_concurrent(ATTRIBUTE, cs, sets, args)
    assert [[call[0] for call in c.calls] for c in cs] == [[4, 4, 2], [3], [4, 2]]
    for smp, out in zip(sets, outs):
        assert [list(g["gxi"]) for g in out] == [[float(t) for t in x.ids[:2]] for x in smp]
    cs = [FakeCtx(2), FakeCtx(2)]
    outs = run_heldout_stacked(ATTRIBUTE, cs, sets, args)
    assert [call[:2] for call in cs[0].calls] == [(7, (0, 0, 0, 0, 1, 1, 1)), (4, (0, 0, 0, 0)), (2, (0, 0))]
    assert [len(o) for o in outs] == [10, 3, 6]
    assert [list(g["gxi"]) for g in outs[1]] == [[float(t) + 1000 for t in x.ids[:2]] for x in sets[1]]      # fold 1 ran in slot 1
    assert [list(g["gxi"]) for g in outs[0] + outs[2]] == [[float(t) for t in x.ids[:2]] for x in sets[0] + sets[2]]


# ------------------------------------------------------------------------------------------------ records, command line, fingerprint
def test_fold_records_carry_attr_only_when_asked():
    from tst.diagnose import fold_records
    held = [_sample(4, [20, 21, 22], [30]), _sample(9, [23], [31, 32])]
    plain = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1])
    assert list(plain[0]) == ["id", "fold", "round", "s", "pred", "correct", "kind"]        # key order is part of the shard's bytes
    attr = [dict(gxi=np.array([1, -2, 3], np.float32), gnorm=np.array([1, 5, 3], np.float32), share=None, log_s=-1.0),
            dict(gxi=np.array([0.5], np.float32), gnorm=np.array([2], np.float32), share=None, log_s=-2.0)]
    recs = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], attr=attr)
    assert recs[0]["attr"] == dict(gxi=[1.0, -2.0, 3.0], gnorm=[1.0, 5.0, 3.0]) and recs[1]["attr"] == dict(gxi=[0.5], gnorm=[2.0]) and "attr_top" not in recs[0]
    recs = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], decode=lambda ids: "|".join(map(str, ids)), attr=attr, attr_top=2)
    assert recs[0]["attr_top"] == ["21", "22"] and recs[1]["attr_top"] == ["23"]
    json.dumps(recs)


def test_cli_flags():
    from tst import cli
    a = cli.build_parser().parse_args(["diagnose", "--out", "x"])
    t = cli._args_to_train(a)
    assert (a.attribute, a.attribute_top) == (False, 5) and (t.attribute, t.attribute_top) == (False, 5)
    a = cli.build_parser().parse_args(["prune", "--out", "x", "--attribute", "--attribute-top", "3"])
    t = cli._args_to_train(a)
    assert (t.attribute, t.attribute_top, t.generate) == (True, 3, False)
    for bad in (["--dp", "2"], ["--layout", "dp-stacked"], ["--attribute-top", "-1"]):
        with pytest.raises(SystemExit):
            cli._args_to_train(cli.build_parser().parse_args(["diagnose", "--out", "x", "--attribute"] + bad))


def test_run_fingerprint_is_the_parents_without_the_flag_and_differs_with_it():
    from tst.diagnose import run_fingerprint
    from tst.trainer import TrainArgs
    samples = D.synth_vsi(9, vocab=256, seed=4)
    ident = dict(model="tiny", weights_seed=0)
    # the fields TrainArgs had before attribution existed, with their values: what a run directory written then was fingerprinted with
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
    args = TrainArgs(num_train_epochs=1, learning_rate=1e-3)
    off = run_fingerprint(samples, 5, args, ident)
    assert off == h.hexdigest()
    assert set(dataclasses.asdict(args)) == set(parent_fields) | {"generate", "max_new_tokens", "eos_ids"}
    assert run_fingerprint(samples, 5, TrainArgs(num_train_epochs=1, learning_rate=1e-3, attribute_top=9), ident) == off   # dormant while the flag is off
    on = run_fingerprint(samples, 5, TrainArgs(num_train_epochs=1, learning_rate=1e-3, attribute=True), ident)
    on9 = run_fingerprint(samples, 5, TrainArgs(num_train_epochs=1, learning_rate=1e-3, attribute=True, attribute_top=9), ident)
    assert len({off, on, on9}) == 3
