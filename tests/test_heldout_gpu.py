"""The held-out passes of the diagnostic (score, generate, attribute, ig) do not disturb one another, in every layout: tiny model, k = 2, through tst.diagnose
on one context, on root + one fork (both folds at once) and on one stacked context (n_stack = 2).
  (a) the shards of a run with all passes on, stripped of the gen* / attr* keys, are byte for byte the shards of a run with all of them off;
  (b) every extra key of that run equals, exactly, the same key of a run with only its own pass on;
  (c) the forked layout writes the records of the one-context layout (compared like tests/test_diagnostic_gpu.py test_resident_folds_sweep_equals_sequential_sweep).
Every run takes a fresh context; the runs of a layout are made once and shared by the tests."""
import json

import numpy as np
import pytest

import attribution_inputs as AI
import golden_inputs as GI

pytestmark = pytest.mark.gpu

K = 2
BASE_KEYS = ["id", "fold", "round", "s", "pred", "correct", "kind"]
PASSES = dict(gen=dict(generate=True, max_new_tokens=3), attr=dict(attribute=True), ig=dict(attribute_ig=4, attribute_baseline_id=2, attribute_top=3))
OWNER = dict(gen="gen", gen_correct="gen", gen_text="gen", attr="attr", attr_top="attr", attr_ig="ig", attr_ig_top="ig")   # record key -> the pass that writes it
LAYOUTS = ("one", "forked", "stacked")
_RUNS = {}


def _decode(ids):
    return "<" + ",".join(map(str, ids)) + ">"


def runs(layout, tmp_root):
    """{"off" | "on" | "gen" | "attr" | "ig": (shard texts per fold, records sorted by id)} of one layout"""
    if layout in _RUNS:
        return _RUNS[layout]
    from tst import data as D
    from tst import diagnose as DG
    from tst import lib as L
    from tst.trainer import TrainArgs
    assert L.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    cfg = AI.TAGS["tiny"][0]
    samples = D.synth_vsi(24, cfg["vocab_size"], seed=3)
    kw = dict(num_train_epochs=1, per_device_train_batch_size=8, per_device_eval_batch_size=8, learning_rate=1e-3, logging_steps=0, lora_r=GI.LORA_R,
              lora_alpha=GI.LORA_ALPHA)
    n_stack = 2 if layout == "stacked" else 1
    variants = dict(off={}, on={k: v for p in PASSES.values() for k, v in p.items()}, **{name: dict(p, attribute_top=3) for name, p in PASSES.items()})
    out = {}
    for name, extra in variants.items():
        root = L.Context(cfg, max_tokens=8 * 136 * n_stack, max_seqs=8 * n_stack, max_labelled=32 * n_stack, max_position=136, lora_r=GI.LORA_R,
                         lora_alpha=GI.LORA_ALPHA, n_stack=n_stack)
        root.load_state_dict(AI.TAGS["tiny"][1](cfg))
        ctxs = [root, root.fork()] if layout == "forked" else root
        d = str(tmp_root / f"{layout}_{name}")
        try:
            recs, stats = DG.diagnose(ctxs, samples, K, TrainArgs(**kw, **extra), 0, 1, 0, d, decode=_decode)
        finally:
            if layout == "forked":
                ctxs[1].close()
            root.close()
        assert len(recs) == len(samples)
        if layout != "one":
            assert [st["resident_folds"] for st in stats] == [K] * K   # both folds at once
        out[name] = ([open(DG.fold_path(d, 0, f)).read() for f in range(K)], DG.gather_round(d, 0, K, len(samples)))
    _RUNS[layout] = out
    return out


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("heldout")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_all_passes_on_leaves_the_scores_as_they_are(layout, tmp_root):
    r = runs(layout, tmp_root)
    assert all(list(rec) == BASE_KEYS for rec in r["off"][1])
    assert all(list(rec) == BASE_KEYS + list(OWNER) for rec in r["on"][1])
    for off, on in zip(r["off"][0], r["on"][0]):
        stripped = "".join(json.dumps({kk: v for kk, v in json.loads(line).items() if kk not in OWNER}) + "\n" for line in on.splitlines())
        assert stripped == off


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_pass_gives_what_it_gives_alone(layout, tmp_root):
    r = runs(layout, tmp_root)
    for name in PASSES:
        assert all(list(rec) == BASE_KEYS + [kk for kk in OWNER if OWNER[kk] == name] for rec in r[name][1])
    n = 0
    for i, on in enumerate(r["on"][1]):
        for key, name in OWNER.items():
            alone = r[name][1][i]
            assert alone["id"] == on["id"] and on[key] == alone[key], (layout, on["id"], key, on[key], alone[key])
            n += 1
    assert n == 24 * len(OWNER)
    ig = np.array([v for rec in r["on"][1] for v in rec["attr_ig"]["ig"]])
    assert np.isfinite(ig).all() and np.abs(ig).max() > 0 and any(rec["gen"] for rec in r["on"][1])   # (the passes did run)


def test_forked_folds_write_the_records_of_one_context(tmp_root):
    assert runs("forked", tmp_root)["on"][1] == runs("one", tmp_root)["on"][1]
