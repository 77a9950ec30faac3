"""The held-out drivers of tst.trainer (one context, a context per fold, stacked contexts) against a fake context, no GPU: the scoring pass keeps order,
batches and slots in all three layouts, an empty fold gives empty arrays, and the four passes (score, generate, attribute, ig) run one after the other through
the stacked driver on the same contexts without leaving anything pending. The generate / attribute / ig loops have their own order tests in
test_generate_cpu.py, test_attribution_cpu.py and test_ig_cpu.py."""
import numpy as np

from tst import data as D

FOLDS = (10, 3, 6)   # with an eval batch of 4 the folds run out of batches at different times
OPTS = (8, 9, 10, 11)


def _sample(sid, first, kind):
    """prompt [first, first + 1], one answer token; a multiple-choice sample's right option is sid % 4"""
    mca = kind == "mca"
    return D.Sample(sid, np.array([first, first + 1, OPTS[sid % 4] if mca else 3], np.int32), 2, kind, sid % 4 if mca else -1)


def _sets():
    return [[_sample(100 * f + i, 100 * f + 10 * i, "mca" if i % 2 else "na") for i in range(n)] for f, n in enumerate(FOLDS)]


class FakeCtx:
    """every pass answers from key = the sequence's first id + its slot, so a result says which sample it belongs to and which slot ran it; the context
    holds ONE pending slot for all passes and refuses a second enqueue before the fetch. Records (pass, sequences, slots) of every call."""

    def __init__(self, n_stack=1):
        self.n_stack, self.calls, self._pending = n_stack, [], None

    def _enqueue(self, what, ids, cu, seq_slot, result):
        assert self._pending is None, "at most one pass may be pending per context"
        n = len(cu) - 1
        slots = np.zeros(n, np.int32) if seq_slot is None else np.asarray(seq_slot)
        assert len(slots) == n and (np.diff(slots) >= 0).all() and slots.max() < self.n_stack
        self.calls.append((what, n, tuple(int(s) for s in slots)))
        keys = np.array([int(ids[cu[b]]) + int(slots[b]) for b in range(n)])
        self._pending = (what, result(keys, slots))

    def _fetch(self, what):
        assert self._pending is not None and self._pending[0] == what, f"{what} fetch, pending: {self._pending and self._pending[0]}"
        out, self._pending = self._pending[1], None
        return out

    def score_rows_async(self, ids, labels, cu, option_ids=(), seq_slot=None):
        rows = [(p, b) for b in range(len(cu) - 1) for p in range(cu[b], cu[b + 1] - 1) if labels[p + 1] != -100]
        rseq = np.array([b for _, b in rows], np.int32)
        self._enqueue("score", ids, cu, seq_slot, lambda keys, slots: (
            (-keys[rseq] / 1024.0).astype(np.float32), (keys[rseq] % 2).astype(np.int32),
            np.array([[1.0 if j == k % len(option_ids) else 0.0 for j in range(len(option_ids))] for k in keys[rseq]], np.float32), rseq))

    def score_rows_fetch(self):
        return self._fetch("score")

    def score_rows(self, ids, labels, cu, option_ids=(), seq_slot=None):
        self.score_rows_async(ids, labels, cu, option_ids, seq_slot)
        return self.score_rows_fetch()

    def generate_async(self, ids, cu, max_new_tokens, eos_ids=(), seq_slot=None):
        self._enqueue("generate", ids, cu, seq_slot, lambda keys, slots: (
            np.array([[k + j + 1 for j in range(max_new_tokens)] for k in keys], np.int32), None, np.full(len(keys), max_new_tokens, np.int32)))

    def generate_fetch(self):
        return self._fetch("generate")

    def attribute_async(self, ids, labels, cu, seq_kind=None, option_ids=(), seq_slot=None):
        self._enqueue("attribute", ids, cu, seq_slot, lambda keys, slots: (
            np.asarray(ids, np.float32) + 1000 * np.repeat(slots, np.diff(cu)), np.arange(len(ids), dtype=np.float32), -keys.astype(np.float32)))

    def attribute_fetch(self):
        return self._fetch("attribute")

    def attribute_ig_async(self, ids, labels, cu, baseline_ids, n_steps, seq_kind=None, option_ids=(), seq_slot=None):
        assert len(baseline_ids) == len(ids)
        self._enqueue("ig", ids, cu, seq_slot, lambda keys, slots: (
            np.asarray(ids, np.float32) + 1000 * np.repeat(slots, np.diff(cu)), -keys.astype(np.float32), -keys.astype(np.float32) - n_steps))

    def attribute_ig_fetch(self):
        return self._fetch("ig")


def _want_scores(samples, slot=0):
    """what tst.score.bias_scores makes of FakeCtx's rows for these samples, run in `slot`"""
    s, pred, correct = np.zeros(len(samples), np.float32), np.full(len(samples), -1, np.int32), np.zeros(len(samples), np.int32)
    for i, x in enumerate(samples):
        key = int(x.ids[0]) + slot
        if x.kind == "mca":
            z = np.array([1.0 if j == key % 4 else 0.0 for j in range(4)], np.float32).astype(np.float64)
            p = np.exp(z - z.max())
            p /= p.sum()
            s[i], pred[i], correct[i] = p[x.gt_option], key % 4, int(key % 4 == x.gt_option)
        else:
            s[i], correct[i] = np.exp(np.mean(np.array([-key / 1024.0], np.float32).astype(np.float64))), key % 2
    return s, pred, correct


def _check_fold(got, samples, slot=0):
    want = _want_scores(samples, slot)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == (len(samples),)
        np.testing.assert_array_equal(g, w)


STACKED_CALLS = ([(7, (0, 0, 0, 0, 1, 1, 1)), (4, (0, 0, 0, 0)), (2, (0, 0))], [(4, (0, 0, 0, 0)), (2, (0, 0))])


def test_score_heldout_loops_keep_order_batches_and_slots():
    from tst.trainer import SCORE, TrainArgs, run_heldout_concurrent, run_heldout_stacked, score_heldout
    args = TrainArgs(per_device_eval_batch_size=4, option_ids=OPTS)
    sets = _sets()
    assert {x.kind for x in sets[0]} == {"mca", "na"}
    # one context
    c = FakeCtx()
    _check_fold(score_heldout(c, sets[0], args), sets[0])
    assert c.calls == [("score", 4, (0,) * 4), ("score", 4, (0,) * 4), ("score", 2, (0,) * 2)] and c._pending is None
    # a context per fold: every fold's batches in its own order
    cs = [FakeCtx() for _ in sets]
    outs = run_heldout_concurrent(SCORE, cs, sets, args)
    assert [[n for _, n, _ in c.calls] for c in cs] == [[4, 4, 2], [3], [4, 2]] and all(c._pending is None for c in cs)
    assert len(outs) == 3
    for smp, out in zip(sets, outs):
        _check_fold(out, smp)
    # stacked: folds 0, 1 in the slots of context 0, fold 2 in context 1 (place_folds); the slot shifts FakeCtx's key, so fold 1's scores say "slot 1"
    cs = [FakeCtx(2), FakeCtx(2)]
    outs = run_heldout_stacked(SCORE, cs, sets, args)
    assert [[call[1:] for call in c.calls] for c in cs] == list(STACKED_CALLS) and all(c._pending is None for c in cs)
    assert [len(o[0]) for o in outs] == list(FOLDS)
    for smp, out, slot in zip(sets, outs, (0, 1, 0)):
        _check_fold(out, smp, slot)
    assert not np.array_equal(outs[1][0], _want_scores(sets[1], 0)[0])   # (the slot does show in the scores)


def test_an_empty_fold_scores_to_empty_arrays():
    from tst.trainer import SCORE, TrainArgs, run_heldout_concurrent, run_heldout_stacked
    args = TrainArgs(per_device_eval_batch_size=4, option_ids=OPTS)
    sets = _sets()
    sets[1] = []
    for run, cs in ((run_heldout_concurrent, [FakeCtx() for _ in sets]), (run_heldout_stacked, [FakeCtx(2), FakeCtx(2)])):
        outs = run(SCORE, cs, sets, args)
        assert run is run_heldout_stacked or cs[1].calls == []   # (nothing is enqueued for an empty fold)
        assert [(a.dtype, a.shape) for a in outs[1]] == [(np.float32, (0,)), (np.int32, (0,)), (np.int32, (0,))]
        for smp, out, slot in zip(sets, outs, (0, 1, 0)):
            _check_fold(out, smp, slot if run is run_heldout_stacked else 0)
    assert run_heldout_concurrent(SCORE, [], [], args) == [] and run_heldout_stacked(SCORE, [FakeCtx(2)], [], args) == []


def test_the_four_passes_run_in_turn_on_the_same_stacked_contexts():
    """score, generate, attribute, ig through the stacked driver on the SAME fakes, which hold one pending slot for all passes: every pass fetches what it
    enqueued, so the next one finds nothing pending; every pass sees the same batches and slots"""
    from tst.trainer import ATTRIBUTE, GENERATE, IG, SCORE, TrainArgs, run_heldout_stacked
    args = TrainArgs(per_device_eval_batch_size=4, option_ids=OPTS, generate=True, max_new_tokens=2, attribute=True, attribute_ig=8, attribute_baseline_id=7)
    sets = _sets()
    cs = [FakeCtx(2), FakeCtx(2)]
    scored, gen, attr, ig = (run_heldout_stacked(p, cs, sets, args) for p in (SCORE, GENERATE, ATTRIBUTE, IG))
    assert all(c._pending is None for c in cs)
    for c, want in zip(cs, STACKED_CALLS):
        assert c.calls == [(what,) + call for what in ("score", "generate", "attribute", "ig") for call in want]
    for smp, slot, sc, g, a, i in zip(sets, (0, 1, 0), scored, gen, attr, ig):
        _check_fold(sc, smp, slot)
        assert [t for t, _ in g] == [[int(x.ids[0]) + slot + 1, int(x.ids[0]) + slot + 2] for x in smp]
        assert [list(r["gxi"]) for r in a] == [[float(t) + 1000 * slot for t in x.ids[:2]] for x in smp]
        assert [r["log_s"] for r in a] == [-float(int(x.ids[0]) + slot) for x in smp]
        assert [list(r["ig"]) for r in i] == [[float(t) + 1000 * slot for t in x.ids[:2]] for x in smp]
        assert all(r["log_s_base"] == r["log_s"] - 8 for r in i)
