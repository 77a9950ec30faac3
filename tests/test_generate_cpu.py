"""CPU tests of greedy answer generation: everything of it that needs no GPU.
  * tsthost::plan_generate (csrc/host_logic.h, what tst_generate_async runs before any launch) through libtst_host.so: the KV-cache row map, its capacity,
    every refusal with its message; csrc/host_selftest.cpp runs the same function under AddressSanitizer / UBSan (tests/test_host_logic_sanitized.py);
  * tst.score.generated_answers: eos truncation and gen_correct;
  * the three generate_heldout* loops of tst.trainer against a fake context: order, batching, slots;
  * the command line: flags, YAML keys, the default eos ids; the run fingerprint with the flag off (unchanged) and on;
  * tst.hf_compat.TstModel.generate: the HF-shaped padded result, on a fake context."""
import dataclasses
import hashlib
import json

import numpy as np
import pytest

import golden_inputs as GI
from tst import data as D
from tst import lib


# ------------------------------------------------------------------------------------------------ plan_generate
def _prompts(lens, vocab=256, seed=31):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, vocab, n).astype(np.int32) for n in lens]
    return np.concatenate(seqs), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def test_plan_generate_row_map_and_capacity():
    lens, max_new = (1, 5, 17, 63, 64, 65, 100, 125, 130), 8
    ids, cu = _prompts(lens)
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=1024, max_seqs=16, max_labelled=64, max_position=256)
    p = lib.host_plan_generate(mc, ids, cu, max_new, eos_ids=(2, 255))
    S, T = len(lens), int(cu[-1])
    assert (p["S"], p["T"]) == (S, T) and p["rows_used"] == T + S * max_new and p["cache_rows"] == 1024 + 16 * max_new
    np.testing.assert_array_equal(p["meta"], np.concatenate([[S, max_new], cu, lens]))
    np.testing.assert_array_equal(p["last_rows"], cu[1:] - 1)
    # row of (sequence s, position p) = cu[s] + s max_new + p: prompts first, then the decode steps' rows; no row is used twice
    want = np.concatenate([cu[s] + s * max_new + np.arange(lens[s]) for s in range(S)])
    np.testing.assert_array_equal(p["prefill_rows"], want)
    for j in range(1, max_new):
        np.testing.assert_array_equal(p["decode_rows"][j - 1], cu[:-1] + np.arange(S) * max_new + np.array(lens) + j - 1)
    rows = np.concatenate([p["prefill_rows"], p["decode_rows"].reshape(-1)])
    assert len(set(rows.tolist())) == len(rows) and rows.min() == 0 and rows.max() == p["rows_used"] - 2   # (the last new token is never fed back)
    assert list(p["slot_s_end"]) == [S] * 8
    # stacked: the slot boundaries of a decode step are sequence counts
    mc3 = lib.make_model_cfg(GI.TINY_CFG, max_tokens=1024, max_seqs=16, max_labelled=64, max_position=256, n_stack=3)
    p3 = lib.host_plan_generate(mc3, ids, cu, max_new, seq_slot=[0, 0, 0, 0, 2, 2, 2, 2, 2])
    assert list(p3["slot_s_end"]) == [4, 4, 9, 9, 9, 9, 9, 9]
    # max_new = 1: the prefill alone
    p1 = lib.host_plan_generate(mc, ids, cu, 1)
    assert p1["decode_rows"].shape == (0, S) and p1["rows_used"] == T + S


def test_plan_generate_refusals():
    ids, cu = _prompts((1, 5, 17, 100))
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=128, max_seqs=4, max_labelled=4, max_position=108)
    lib.host_plan_generate(mc, ids, cu, 8)                                         # 100 + 8 <= 108
    for kw, msg in ((dict(max_new=0), "max_new_tokens out of range"), (dict(max_new=257), "max_new_tokens out of range"), (dict(max_new=-3), "max_new_tokens out of range"),
                    (dict(max_new=9), "exceeds max_position"), (dict(max_new=8, eos_ids=(256,)), "eos id out of vocabulary"),
                    (dict(max_new=8, eos_ids=(3, -1)), "eos id out of vocabulary"), (dict(max_new=8, eos_ids=tuple(range(17))), "more than 16 eos ids")):
        with pytest.raises(lib.TstError, match=msg):
            lib.host_plan_generate(mc, ids, cu, **kw)
    lib.host_plan_generate(mc, ids, cu, 8, eos_ids=tuple(range(16)))
    with pytest.raises(lib.TstError, match="more sequences than max_labelled"):
        lib.host_plan_generate(lib.make_model_cfg(GI.TINY_CFG, max_tokens=128, max_seqs=4, max_labelled=3, max_position=108), ids, cu, 8)
    with pytest.raises(lib.TstError, match="exceeds max_tokens/max_seqs"):
        lib.host_plan_generate(lib.make_model_cfg(GI.TINY_CFG, max_tokens=122, max_seqs=4, max_labelled=4, max_position=108), ids, cu, 8)
    with pytest.raises(lib.TstError, match="cu_seqlens"):
        lib.host_plan_generate(mc, ids, np.array([0, 1, 6, 5, 123], np.int32), 8)
    with pytest.raises(lib.TstError, match="sequence length"):
        lib.host_plan_generate(mc, ids, np.array([0, 1, 1, 23, 123], np.int32), 8)
    with pytest.raises(lib.TstError, match="seq_slot"):
        lib.host_plan_generate(mc, ids, cu, 8, seq_slot=[0, 0, 1, 1])              # an unstacked context has slot 0 only


def test_cut_at_eos_is_the_fetch_sides_rule():
    tok = np.array([[5, 6, 7, 8], [9, 2, 9, 2], [1, 1, 1, 3], [4, 4, 4, 4]], np.int32)
    logp = -np.ones((4, 4), np.float32)
    t, lp, n = lib.host_cut_at_eos(tok, logp, (2, 3))
    assert list(n) == [4, 2, 4, 4]                                                  # n_new counts the eos token
    np.testing.assert_array_equal(t, [[5, 6, 7, 8], [9, 2, -1, -1], [1, 1, 1, 3], [4, 4, 4, 4]])
    np.testing.assert_array_equal(lp[1], [-1, -1, 0, 0])
    t, _, n = lib.host_cut_at_eos(tok, logp, ())
    assert list(n) == [4] * 4 and (t == tok).all()


# ------------------------------------------------------------------------------------------------ generated_answers
def _sample(sid, prompt, answer, kind="na"):
    return D.Sample(sid, np.array(list(prompt) + list(answer), np.int32), len(prompt), kind, -1)


def test_generated_answers_truncation_and_gen_correct():
    from tst.score import generated_answers
    smp = [_sample(0, [20, 21], [30, 31]), _sample(1, [20], [30, 31]), _sample(2, [22, 23, 24], [40]), _sample(3, [25], [50, 51, 52]), _sample(4, [26], [7])]
    tok = np.array([[30, 31, 99, -1], [30, 32, 33, 34], [40, 99, -1, -1], [50, 51, 60, 61], [99, -1, -1, -1]], np.int32)
    n_new = np.array([3, 4, 2, 4, 1], np.int32)
    got = generated_answers(smp, tok, n_new, eos_ids=(99,))
    assert got == [([30, 31], 1), ([30, 32, 33, 34], 0), ([40], 1), ([50, 51, 60, 61], 0), ([], 0)]
    # without eos ids nothing is stripped; a continuation that goes on behind the answer still counts
    got = generated_answers(smp[:1], np.array([[30, 31, 99, 5]], np.int32), np.array([4], np.int32))
    assert got == [([30, 31, 99, 5], 1)]


# ------------------------------------------------------------------------------------------------ generate_heldout* on a fake context
class FakeCtx:
    """continues every prompt with (its first id + slot) + 1, + 2, ...; records every call"""

    def __init__(self, n_stack=1):
        self.n_stack, self.calls, self._pending = n_stack, [], None

    def generate_async(self, ids, cu, max_new_tokens, eos_ids=(), seq_slot=None):
        assert self._pending is None, "one generation may be pending per context"
        n = len(cu) - 1
        slots = np.zeros(n, np.int32) if seq_slot is None else np.asarray(seq_slot)
        assert (np.diff(slots) >= 0).all() and slots.max() < self.n_stack
        self.calls.append((n, tuple(int(s) for s in slots), int(max_new_tokens), tuple(eos_ids)))
        tok = np.array([[int(ids[cu[s]]) + int(slots[s]) + j + 1 for j in range(max_new_tokens)] for s in range(n)], np.int32)
        self._pending = lib.host_cut_at_eos(tok, np.zeros(tok.shape, np.float32), eos_ids)

    def generate_fetch(self):
        out, self._pending = self._pending, None
        return out

    def generate(self, ids, cu, max_new_tokens, eos_ids=(), seq_slot=None):
        self.generate_async(ids, cu, max_new_tokens, eos_ids, seq_slot)
        return self.generate_fetch()


def test_generate_heldout_loops_keep_order_batches_and_slots():
    from tst.trainer import TrainArgs, GENERATE, generate_heldout, run_heldout_concurrent, run_heldout_stacked
    args = TrainArgs(per_device_eval_batch_size=4, generate=True, max_new_tokens=3, eos_ids=(1000,))
    # sample i: prompt starts with 100 + 10 i, the reference answer is what FakeCtx says in slot 0
    sets = [[_sample(100 * f + i, [100 + 10 * i + 100 * f, 7], [101 + 10 * i + 100 * f, 102 + 10 * i + 100 * f]) for i in range(n)] for f, n in enumerate((10, 3, 6))]
    c = FakeCtx()
    got = generate_heldout(c, sets[0], args)
    assert [n for n, _, _, _ in c.calls] == [4, 4, 2] and all(call[2:] == (3, (1000,)) for call in c.calls)
    assert [g for g, _ in got] == [[101 + 10 * i, 102 + 10 * i, 103 + 10 * i] for i in range(10)] and all(ok == 1 for _, ok in got)
    # concurrent: one context per fold, every fold's batches in its own order
    cs = [FakeCtx() for _ in sets]
    outs = run_heldout_concurrent(GENERATE, cs, sets, args)
    assert [[n for n, _, _, _ in c.calls] for c in cs] == [[4, 4, 2], [3], [4, 2]]
    for smp, out in zip(sets, outs):
        assert [g[0] for g, _ in out] == [int(x.ids[0]) + 1 for x in smp] and all(ok == 1 for _, ok in out)
    # stacked: folds 0, 1 in the slots of context 0, fold 2 in context 1 (place_folds); the slot shifts FakeCtx's tokens, so slot 1's answers are wrong
    cs = [FakeCtx(2), FakeCtx(2)]
    outs = run_heldout_stacked(GENERATE, cs, sets, args)
    assert [call[:2] for call in cs[0].calls] == [(7, (0, 0, 0, 0, 1, 1, 1)), (4, (0, 0, 0, 0)), (2, (0, 0))]
    assert [call[:2] for call in cs[1].calls] == [(4, (0, 0, 0, 0)), (2, (0, 0))]
    assert [len(o) for o in outs] == [10, 3, 6]
    assert [g[0] for g, _ in outs[1]] == [int(x.ids[0]) + 2 for x in sets[1]] and all(ok == 0 for _, ok in outs[1])
    assert all(ok == 1 for _, ok in outs[0] + outs[2])
    # an eos id inside the continuation cuts it
    args2 = TrainArgs(per_device_eval_batch_size=4, generate=True, max_new_tokens=3, eos_ids=(102,))
    assert generate_heldout(FakeCtx(), sets[0][:1], args2) == [([101], 0)]


# ------------------------------------------------------------------------------------------------ command line, fingerprint
def test_cli_flags_yaml_keys_and_default_eos(tmp_path):
    from tst import cli
    a = cli.build_parser().parse_args(["diagnose", "--out", "x"])
    t = cli._args_to_train(a)
    assert (a.generate, a.max_new_tokens, a.eos_ids) == (False, 8, None) and (t.generate, t.max_new_tokens, t.eos_ids) == (False, 8, ())
    a = cli.build_parser().parse_args(["prune", "--out", "x", "--generate", "--max-new-tokens", "5", "--eos-ids", "2,32000"])
    t = cli._args_to_train(a)
    assert (t.generate, t.max_new_tokens, t.eos_ids) == (True, 5, (2, 32000))
    (tmp_path / "c.yaml").write_text("generate: true\nmax_new_tokens: 12\neos_ids: '7 9'\nk: 3\n")
    argv = ["diagnose", "--out", "x", "--config", str(tmp_path / "c.yaml"), "--max-new-tokens", "4"]
    a = cli.apply_config(cli.build_parser().parse_args(argv), argv)
    t = cli._args_to_train(a)
    assert (t.generate, t.max_new_tokens, t.eos_ids, a.k) == (True, 4, (7, 9), 3)     # the flag given on the command line wins over the file
    # the checkpoint's own eos: generation_config.json first, then config.json; an int or a list
    md = tmp_path / "ckpt"
    md.mkdir()
    assert cli.default_eos_ids(str(md)) == () and cli.default_eos_ids(None) == ()
    (md / "config.json").write_text(json.dumps(dict(eos_token_id=2)))
    assert cli.default_eos_ids(str(md)) == (2,)
    (md / "generation_config.json").write_text(json.dumps(dict(eos_token_id=[128001, 128009])))
    assert cli.default_eos_ids(str(md)) == (128001, 128009)
    a = cli.build_parser().parse_args(["diagnose", "--out", "x", "--generate", "--model-dir", str(md)])
    assert cli._args_to_train(a).eos_ids == (128001, 128009)


def test_run_fingerprint_is_the_parents_without_the_flag_and_differs_with_it():
    from tst.diagnose import run_fingerprint
    from tst.trainer import TrainArgs
    samples = D.synth_vsi(9, vocab=256, seed=4)
    args = TrainArgs(num_train_epochs=1, learning_rate=1e-3)
    ident = dict(model="tiny", weights_seed=0)

    def parent_form(a):
        """run_fingerprint as it was before generation existed: every TrainArgs field of that time, nothing else"""
        d = {k: v for k, v in dataclasses.asdict(a).items() if k not in ("generate", "max_new_tokens", "eos_ids")}
        h = hashlib.sha256()
        h.update(json.dumps(dict(args={kk: (list(v) if isinstance(v, tuple) else v) for kk, v in sorted(d.items())}, k=5, n=len(samples), extra=ident),
                            sort_keys=True).encode())
        for x in samples:
            h.update(np.int64(x.sid).tobytes())
            h.update(np.ascontiguousarray(x.ids, dtype=np.int32).tobytes())
            h.update(np.int32(x.n_prompt).tobytes())
        return h.hexdigest()

    off = run_fingerprint(samples, 5, args, ident)
    assert off == parent_form(args)
    # the two dormant settings do not matter while the flag is off
    assert run_fingerprint(samples, 5, dataclasses.replace(args, max_new_tokens=3, eos_ids=(2,)), ident) == off
    on = run_fingerprint(samples, 5, dataclasses.replace(args, generate=True), ident)
    assert on != off
    assert len({on, run_fingerprint(samples, 5, dataclasses.replace(args, generate=True, max_new_tokens=3), ident),
                run_fingerprint(samples, 5, dataclasses.replace(args, generate=True, eos_ids=(2,)), ident)}) == 3


def test_fold_records_carry_gen_only_when_asked():
    from tst.diagnose import fold_records
    held = [_sample(4, [20, 21], [30]), _sample(9, [22], [31, 32], kind="na")]
    plain = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1])
    assert plain == [dict(id=4, fold=2, round=0, s=0.25, pred=-1, correct=0, kind="na"), dict(id=9, fold=2, round=0, s=0.5, pred=-1, correct=1, kind="na")]
    assert list(plain[0]) == ["id", "fold", "round", "s", "pred", "correct", "kind"]        # key order is part of the shard's bytes
    gen = fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], gen=[([30, 5], 1), ([], 0)], decode=lambda ids: "|".join(map(str, ids)))
    assert [{k: r[k] for k in ("gen", "gen_correct", "gen_text")} for r in gen] == [dict(gen=[30, 5], gen_correct=1, gen_text="30|5"), dict(gen=[], gen_correct=0, gen_text="")]
    assert "gen_text" not in fold_records(held, 2, 0, [0.25, 0.5], [-1, -1], [0, 1], gen=[([30], 1), ([], 0)])[0]
    json.dumps(gen)


# ------------------------------------------------------------------------------------------------ hf_compat
def test_tstmodel_generate_pads_behind_each_rows_end():
    from tst.hf_compat import TstModel
    c = FakeCtx()
    m = TstModel(c)
    ids = np.array([[50, 51, 52, 0], [60, 0, 0, 0], [70, 71, 72, 73]])
    mask = np.array([[1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1]])
    out = m.generate(ids, mask, max_new_tokens=3, eos_token_id=62)
    assert out.shape == (3, 7) and out.dtype == np.int64 and c.calls == [(3, (0, 0, 0), 3, (62,))]
    np.testing.assert_array_equal(out, [[50, 51, 52, 51, 52, 53, 62], [60, 61, 62, 62, 62, 62, 62], [70, 71, 72, 73, 71, 72, 73]])
    out = m.generate(ids, mask, max_new_tokens=2, pad_token_id=-7)
    np.testing.assert_array_equal(out, [[50, 51, 52, 51, 52, -7], [60, 61, 62, -7, -7, -7], [70, 71, 72, 73, 71, 72]])
    with pytest.raises(ValueError, match="right-padded"):
        m.generate(ids, np.array([[0, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 1]]), max_new_tokens=2)
