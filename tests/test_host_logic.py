"""CPU tests of the host side: k-fold assignment vs sklearn fixtures, collation, s(x) aggregation, LR schedule,
the C-ABI export list, and the "no CPU fallback" behaviour."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kfold_matches_sklearn_fixtures(golden_dir):
    from tst import kfold
    g = np.load(os.path.join(golden_dir, "kfold.npz"))
    for key in g.files:
        parts = key.split("_")
        n, k = int(parts[1]), int(parts[2])
        if parts[3] == "noshuffle":
            got = kfold.kfold_assign(n, k, shuffle=False)
        else:
            got = kfold.kfold_assign(n, k, shuffle=True, seed=int(parts[3]))
        np.testing.assert_array_equal(got, g[key], err_msg=key)
    # SURVEY §4 known answer: KFold(5, shuffle=True, random_state=42) on n=12
    a = kfold.kfold_assign(12, 5, True, 42)
    assert [list(np.flatnonzero(a == f)) for f in range(5)] == [[0, 9, 10], [2, 5, 8], [1, 11], [4, 7], [3, 6]]
    tr, te = kfold.fold_indices(a, 1)
    assert list(te) == [2, 5, 8] and len(tr) == 9 and not set(tr) & set(te)
    with pytest.raises(ValueError):
        kfold.kfold_assign(3, 5)


def test_planned_maxlen_around_the_128_token_kernel_switch():
    """plan_batch's maxlen picks the attention kernel family (<= 128: shared-staging kernels and RoPE inside them; above: the general kernels and
    the stand-alone rope kernel). With trim_last the last token of EVERY sequence is dropped -- it predicts nothing and, under the causal mask, nothing
    attends to it -- so a 129-token sequence plans 128 whether or not it carries labels, and 129 with trim off. Caller-chosen rows
    (tst_forward_logits) may read any position: the sequence is kept whole, as is a one-token sequence."""
    import golden_inputs as GI
    from tst import lib
    rng = np.random.default_rng(129)
    mc = lib.make_model_cfg(GI.TINY_CFG, max_tokens=512, max_seqs=8, max_labelled=64, max_position=256)
    lengths = (129, 40, 1, 7)
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ids = rng.integers(0, GI.TINY_CFG["vocab_size"], int(cu[-1])).astype(np.int32)
    for labelled_129 in (True, False):
        labels = np.full(len(ids), -100, np.int32)
        labels[cu[2] - 3:cu[2]] = ids[cu[2] - 3:cu[2]]            # the 40-token sequence is labelled in both cases
        if labelled_129:
            labels[cu[1] - 1] = ids[cu[1] - 1]                    # the 129-token sequence: its last token
        whole = lib.host_plan_batch(mc, ids, labels, cu, trim_last=False)
        assert whole["maxlen"] == 129 and list(np.diff(whole["cu"])) == list(lengths)
        trimmed = lib.host_plan_batch(mc, ids, labels, cu, trim_last=True)
        assert trimmed["maxlen"] == 128, (labelled_129, trimmed["maxlen"])
        assert list(np.diff(trimmed["cu"])) == [128, 39, 1, 6]
        assert trimmed["R"] == whole["R"] == 3 + int(labelled_129)
        # the labelled rows point at the same source positions either way (trimming only drops the tail of each sequence)
        src = lambda p: np.searchsorted(p["cu"], p["lab_idx"], side="right") - 1
        np.testing.assert_array_equal(src(trimmed), src(whole))
        np.testing.assert_array_equal(trimmed["targets"], whole["targets"])
        rows = lib.host_plan_batch(mc, ids, labels, cu, trim_last=True, rows=[int(cu[1]) - 1, 0])
        assert rows["maxlen"] == 129


def test_fold_placement():
    from tst import kfold
    assert [kfold.folds_for_rank(5, r, 8) for r in range(8)] == [[0], [1], [2], [3], [4], [], [], []]
    assert [kfold.folds_for_rank(5, r, 2) for r in range(2)] == [[0, 2, 4], [1, 3]]
    assert sorted(sum((kfold.folds_for_rank(8, r, 4) for r in range(4)), [])) == list(range(8))


def test_synth_and_collate():
    from tst import data as D
    s = D.synth_vsi(200, vocab=5000, seed=1)
    assert len(s) == 200 and all(33 <= len(x.ids) <= 128 for x in s)
    assert all((x.kind == "mca") == (x.n_answer == 1) for x in s)
    assert all(x.ids[-1] in D.OPTION_IDS for x in s if x.kind == "mca")
    frac1 = np.mean([x.n_answer == 1 for x in s])
    assert 0.4 < frac1 < 0.7
    s2 = D.synth_vsi(200, vocab=5000, seed=1)
    assert all((a.ids == b.ids).all() for a, b in zip(s, s2))  # deterministic
    ids, labels, cu = D.collate(s[:5])
    assert cu[0] == 0 and cu[-1] == len(ids) and len(cu) == 6
    for i, x in enumerate(s[:5]):
        seg = labels[cu[i]:cu[i + 1]]
        assert (seg[:x.n_prompt] == -100).all() and (seg[x.n_prompt:] == x.ids[x.n_prompt:]).all()
    # padded HF-style batch -> packed
    B, S = 5, 128
    pid, plab, mask = np.zeros((B, S), np.int64), np.full((B, S), -100), np.zeros((B, S), np.int64)
    for i, x in enumerate(s[:5]):
        pid[i, :len(x.ids)] = x.ids
        plab[i, x.n_prompt:len(x.ids)] = x.ids[x.n_prompt:]
        mask[i, :len(x.ids)] = 1
    ids2, lab2, cu2 = D.from_padded(pid, mask, plab)
    np.testing.assert_array_equal(ids, ids2)
    np.testing.assert_array_equal(labels, lab2)
    np.testing.assert_array_equal(cu, cu2)


def test_bias_scores():
    from tst import data as D
    from tst import score as S
    mca = D.Sample(0, np.array([20, 21, 22, D.OPTION_IDS[2]], np.int32), 3, "mca", 2)
    na = D.Sample(1, np.array([30, 31, 40, 41, 42], np.int32), 2, "na", -1)
    logp = np.log(np.array([0.9, 0.5, 0.25, 0.125], np.float32))
    correct = np.array([1, 1, 0, 1], np.int32)
    optl = np.array([[0.0, 1.0, 3.0, -1.0]] * 4, np.float32)
    s, pred, corr = S.bias_scores([mca, na], logp, correct, optl, np.array([0, 1, 1, 1]))
    z = np.exp(optl[0] - 3.0)
    assert abs(s[0] - z[2] / z.sum()) < 1e-6 and pred[0] == 2 and corr[0] == 1
    assert abs(s[1] - (0.5 * 0.25 * 0.125) ** (1 / 3)) < 1e-6 and pred[1] == -1 and corr[1] == 0
    with pytest.raises(ValueError):
        S.bias_scores([mca, na], logp, correct, optl, np.array([0, 1, 1, 0]))


def test_linear_lr_matches_hf_formula():
    from tst.trainer import linear_lr
    assert linear_lr(0, 10, 1.0) == 1.0 and linear_lr(5, 10, 1.0) == 0.5 and linear_lr(10, 10, 1.0) == 0.0
    assert linear_lr(1, 10, 1.0, warmup=4) == 0.25 and linear_lr(4, 10, 1.0, warmup=4) == 1.0 and linear_lr(7, 10, 1.0, warmup=4) == 0.5


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(tst_[a-z0-9_]+)\s*\(", hdr)) - {"tst_ctx"}


def _exported(path):
    """EVERY symbol the shared object defines in its dynamic table (functions, weak template instantiations, vtables, data): the libraries are built with
    -fvisibility=hidden and export through the headers' visibility pragma only, so anything beyond the declared entry points is a leak"""
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_cabi_exports_every_declared_symbol():
    """both shared libraries load on a CPU-only box. The product library exports exactly the entry points include/tst_hip.h declares
    (no test hook, no experimental tile family leaks into the ABI a maintainer binds); the lab library adds exactly those of
    include/tst_hip_lab.h."""
    from tst import lib
    L, LAB = lib.load(), lib.load_lab()
    declared, declared_lab = _declared("tst_hip.h"), _declared("tst_hip_lab.h")
    assert declared and declared_lab, "no declarations parsed"
    assert declared == set(lib.SIGNATURES), declared ^ set(lib.SIGNATURES)
    assert declared_lab == set(lib.LAB_SIGNATURES), declared_lab ^ set(lib.LAB_SIGNATURES)
    for name in declared:
        assert hasattr(L, name) and hasattr(LAB, name), name
    for name in declared_lab:
        assert hasattr(LAB, name), name
    assert _exported(lib.LIB_PATH) == declared
    assert _exported(lib.LAB_PATH) == declared | declared_lab


def test_no_cpu_fallback_without_gpu():
    from tst import lib
    if lib.device_count() > 0:
        pytest.skip("GPU present")
    import golden_inputs as GI
    with pytest.raises(lib.TstError, match="no HIP device|no CPU fallback"):
        lib.Context(GI.TINY_CFG)


def test_cli_yaml_config_fills_unset_options(tmp_path):
    """--config: TrainingArguments-style keys; flags given on the command line win over the file."""
    from tst import cli
    (tmp_path / "c.yaml").write_text("learning_rate: 1.0e-4\nnum_train_epochs: 1\nk: 8\nlora_r: 32\nmodel: tiny\n")
    argv = ["diagnose", "--out", str(tmp_path), "--config", str(tmp_path / "c.yaml"), "--k", "4", "--lora-r=8"]
    a = cli.apply_config(cli.build_parser().parse_args(argv), argv)
    assert (a.learning_rate, a.num_train_epochs, a.k, a.lora_r, a.model) == (1e-4, 1, 4, 8, "tiny")
    t = cli._args_to_train(a)
    assert t.learning_rate == 1e-4 and t.num_train_epochs == 1 and t.lora_r == 8 and t.logging_steps == 50
    (tmp_path / "bad.yaml").write_text("learning_rat: 1\n")
    import pytest
    with pytest.raises(SystemExit):
        cli.apply_config(cli.build_parser().parse_args(["diagnose", "--out", "x", "--config", str(tmp_path / "bad.yaml")]), [])


def test_place_folds_and_collate_stacked():
    """stacked folds, host side: folds go to contexts as evenly as the slots allow, consecutive folds share a context, and the
    concatenated micro-batch keeps each fold's sequences together in slot order"""
    from tst import data as D
    from tst.trainer import collate_stacked, place_folds

    class C:
        def __init__(self, n):
            self.n_stack = n

    assert place_folds(5, [C(3), C(3)]) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    assert place_folds(4, [C(3), C(3)]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert place_folds(3, [C(1), C(1), C(1)]) == [(0, 0), (1, 0), (2, 0)]
    assert place_folds(7, [C(8)]) == [(0, i) for i in range(7)]
    assert place_folds(4, [C(1), C(3)]) == [(0, 0), (1, 0), (1, 1), (1, 2)]
    with pytest.raises(ValueError):
        place_folds(7, [C(3), C(3)])
    samples = D.synth_vsi(10, vocab=500, seed=1)
    ids, labels, cu, slot = collate_stacked([(0, samples[:3]), (2, samples[3:4]), (3, samples[4:9])])
    ids2, labels2, cu2 = D.collate(samples[:9])
    assert (ids == ids2).all() and (labels == labels2).all() and (cu == cu2).all()
    assert slot.tolist() == [0, 0, 0, 2, 3, 3, 3, 3, 3] and slot.dtype == np.int32


def test_cli_fold_layout():
    """which folds are resident and how they are stacked (tst.cli.fold_layout): the defaults DESIGN.md measured, and the overrides"""
    from tst.cli import MODEL_SHAPES, fold_layout
    big, small = MODEL_SHAPES["llama3-8b"], MODEL_SHAPES["gpt2-small"]
    assert fold_layout(big, "lora", 5, 0, 1) == (5, 3, 2)            # k = 5 on one GPU: two contexts of 3 + 2 folds
    assert fold_layout(big, "lora", 8, 0, 1) == (6, 3, 2)            # six of the eight resident at a time, 3 + 3
    assert fold_layout(big, "lora", 5, 0, 2) == (3, 3, 1)            # rank 0 of two runs folds 0, 2, 4: one stacked context
    assert fold_layout(big, "lora", 5, 1, 2) == (2, 2, 1)
    assert fold_layout(big, "lora", 8, 3, 8) == (1, 1, 1)            # one fold per GPU
    assert fold_layout(big, "full", 8, 0, 1) == (1, 1, 1)            # a full fine-tune owns its weights
    assert fold_layout(big, "lora", 5, 0, 1, folds_per_gpu=3, stack=1) == (3, 1, 3)   # three streams, not stacked
    assert fold_layout(big, "lora", 5, 0, 1, folds_per_gpu=4) == (4, 3, 2)
    assert fold_layout(small, "lora", 2, 0, 1) == (2, 2, 1)          # config 1: k = 2 on GPT-2-small
    assert fold_layout(small, "lora", 20, 0, 1) == (16, 8, 2)        # small bases: deeper stacks
    assert fold_layout(big, "lora", 5, 0, 1, stack=64) == (5, 5, 1)  # never more slots than folds / TST_MAX_STACK


def test_cli_export_filters_the_benchmark_file(tmp_path):
    """tst.cli export --data-file QA.jsonl --to-data OUT.jsonl: the debiased benchmark is the surviving records, unchanged and in order"""
    import json
    from tst import cli
    run = tmp_path / "run"
    run.mkdir()
    recs = [dict(id=i, question=f"q {i} ?", answer=str(i)) for i in (5, 3, 9, 1, 7)]
    qa = tmp_path / "qa.jsonl"
    qa.write_text("\n".join(json.dumps(r) for r in recs) + "\n\n")
    (run / "ibp_final.json").write_text(json.dumps(dict(surviving=[9, 5, 1], history=[dict(round=0, n_before=5, n_pruned=2)], meta=dict(k=5))))
    assert cli.main(["export", "--run", str(run), "--to", str(tmp_path / "d.json"), "--data-file", str(qa), "--to-data", str(tmp_path / "deb.jsonl")]) == 0
    assert json.load(open(tmp_path / "d.json"))["keep_ids"] == [1, 5, 9]
    out = [json.loads(x) for x in open(tmp_path / "deb.jsonl")]
    assert out == [recs[0], recs[2], recs[3]]


def test_integration_stub_matches_the_abi_structs():
    """INTEGRATION.md prints the ctypes stub a maintainer would copy: its two structures must have the fields and sizes of the ones the
    library is bound with (tst/lib.py = include/tst_hip.h), or a copied stub hands the library a short struct"""
    import ctypes as C
    from tst import lib
    src = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = src[src.index("class ModelCfg(C.Structure):"):src.index("def make_ctx(")]
    ns = {"C": C}
    exec(code, ns)
    for name in ("ModelCfg", "Batch"):
        doc, real = ns[name], getattr(lib, name)
        assert [f[0] for f in doc._fields_] == [f[0] for f in real._fields_], name
        assert C.sizeof(doc) == C.sizeof(real), name
    hdr = open(os.path.join(ROOT, "include", "tst_hip.h")).read()
    assert "int32_t n_stack;" in hdr and "const int32_t* seq_slot;" in hdr and "int32_t precision;" in hdr and "int32_t zero_ranks, zero_rank;" in hdr


def test_agreement_metrics_on_known_inputs():
    """tst.agreement: Spearman rho with ties, accuracy gap, Jaccard of the IBP-pruned sets (the distributional-agreement protocol)"""
    from tst import agreement as AG
    a = [dict(id=i, s=s, correct=int(s > 0.5)) for i, s in enumerate([0.1, 0.9, 0.8, 0.3, 0.7, 0.2])]
    b = [dict(id=i, s=s, correct=int(s > 0.5)) for i, s in enumerate([0.15, 0.85, 0.9, 0.25, 0.6, 0.1])]
    m = AG.compare_runs(a, b, tau=0.5, prune_frac=0.34)
    assert m["n"] == 6 and m["accuracy_gap_pp"] == 0.0 and m["pred_agreement"] == 1.0 and m["pruned_jaccard"] == 1.0
    assert abs(m["spearman"] - (1 - 6 * 4 / (6 * 35))) < 1e-12
    assert AG.spearman([1, 2, 3, 4], [4, 3, 2, 1]) == -1.0 and AG.spearman([1, 1, 2, 2], [1, 1, 2, 2]) == 1.0
    import pytest
    with pytest.raises(ValueError):
        AG.compare_runs(a, b[:-1])
    assert AG.auroc([0.9, 0.8, 0.1, 0.2], [1, 1, 0, 0]) == 1.0 and AG.auroc([0.1, 0.2, 0.9, 0.8], [1, 1, 0, 0]) == 0.0
    assert AG.auroc([0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0]) == 0.5 and abs(AG.auroc([0.9, 0.4, 0.6, 0.1], [1, 1, 0, 0]) - 0.75) < 1e-12


def test_train_plan_with_accumulation_and_ranks_and_the_micro_batch_slices():
    """an update consumes gradient_accumulation_steps x world micro-batches (HF: trainer.py:1722-1758); the last update of an epoch takes what is
    left; micro_batches() deals micro-batch i of rank r = run (i * world + r) of the update; every sample is used exactly once per epoch."""
    from tst import data as D
    from tst.trainer import TrainArgs, micro_batches, train_plan
    samples = D.synth_vsi(103, vocab=2000, seed=1)
    args = TrainArgs(num_train_epochs=2, per_device_train_batch_size=4, gradient_accumulation_steps=3, learning_rate=1e-3)
    for world in (1, 2):
        plan = list(train_plan(samples, args, fold_seed=7, world=world))
        per = 4 * 3 * world
        assert len(plan) == 2 * -(-103 // per) and plan[-1][1] == len(plan)
        assert [p[0] for p in plan] == list(range(1, len(plan) + 1))
        assert plan[0][2] == 1e-3 and plan[-1][2] == pytest.approx(1e-3 / len(plan))           # linear decay over the UPDATES (optimization.py:101-104)
        first_epoch = plan[:len(plan) // 2]
        seen = []
        for _, _, _, upd in first_epoch:
            parts = [micro_batches(upd, args, r, world) for r in range(world)]
            assert all(len(mb) <= 4 for ps in parts for mb in ps) and all(len(ps) <= 3 for ps in parts)
            got = [x.sid for i in range(3) for r in range(world) if i < len(parts[r]) for x in parts[r][i]]
            assert got == [x.sid for x in upd]                                                  # the slices tile the update in order
            seen += got
        assert sorted(seen) == list(range(103))
        assert len(first_epoch[-1][3]) == 103 - per * (len(first_epoch) - 1)                    # the ragged last update
    # one rank, no accumulation: the update IS the micro-batch (what every existing caller relies on)
    plain = TrainArgs(num_train_epochs=1, per_device_train_batch_size=4)
    assert [len(u) for _, _, _, u in train_plan(samples, plain)] == [4] * 25 + [3]
    assert D.count_labelled(samples[:5]) == sum(len(s.ids) - s.n_prompt for s in samples[:5])


def test_fold_placement_and_the_dp_stacked_layout():
    from tst import kfold
    assert [kfold.folds_for_rank(3, r, 5) for r in range(5)] == [[0], [1], [2], [], []]          # ranks beyond k idle
    import bench
    for world in (1, 2, 8):
        for rank in range(world):
            mine, F, S, nctx = bench.sweep_layout(5, rank, world, "lora", 3, "dp-stacked")
            assert (mine, F, S, nctx) == ([0, 1, 2, 3, 4], 5, 3, 2)                              # every rank: all five folds as 3 + 2
    assert bench.sweep_layout(5, 1, 2, "lora", 3, "folds")[0] == [1, 3] and bench.sweep_layout(5, 7, 8, "lora", 3, "folds")[0] == []
