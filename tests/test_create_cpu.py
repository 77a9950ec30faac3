"""What tst_create / tst_fork answer to a configuration before they allocate anything, on the CPU box: tsthost::check_cfg and tsthost::lora_layout
(test-set-training_amd/csrc/host_logic.h, the code the engine's build_ctx runs first) through libtst_host.so. The configurations, the expected messages and the
expected trainable tables are written out in tests/create_cases.py; tests/test_create_gpu.py holds tst_create itself to the same tables."""
import os

import numpy as np
import pytest

import create_cases as CC
import golden_inputs as GI


@pytest.fixture(scope="module")
def lib():
    from tst import lib
    lib.load_host()
    return lib


@pytest.mark.parametrize("tag,cfg,kw,forkable", CC.accepted(), ids=[a[0] for a in CC.accepted()])
def test_accepted_configurations(lib, tag, cfg, kw, forkable):
    mc = CC.model_cfg(cfg, **kw)
    assert lib.host_check_cfg(mc) == (0, "")
    if kw.get("train_mode") != "full":
        assert lib.host_check_cfg(mc, is_fork=True) == (0, "")


def test_golden_configurations_are_accepted_at_the_suites_workspaces(lib):
    for cfg in CC.GOLDEN.values():
        for kw in (dict(), dict(train_mode="full"), dict(precision="strict"), dict(max_tokens=2048, max_seqs=16, max_labelled=64, max_position=512)):
            assert lib.host_check_cfg(CC.model_cfg(cfg, **kw)) == (0, ""), (cfg, kw)


@pytest.mark.parametrize("base,field,value,msg", CC.REFUSALS, ids=[f"{r[0]}-{r[1]}={r[2]}" for r in CC.REFUSALS])
def test_refused_configurations(lib, base, field, value, msg):
    ok = CC.bases()[base]
    assert lib.host_check_cfg(ok) == (0, "")
    assert lib.host_check_cfg(CC.variant(ok, field, value)) == (CC.EINVAL, msg)


@pytest.mark.parametrize("base,field,value", CC.ZERO_SIZE, ids=[f"{r[0]}-{r[1]}={r[2]}" for r in CC.ZERO_SIZE])
def test_zero_sizes_are_refused_not_divided_by(lib, base, field, value):
    assert lib.host_check_cfg(CC.variant(CC.bases()[base], field, value)) == (CC.EINVAL, CC.POSITIVE)


def test_full_fine_tune_is_not_forkable_and_the_first_fault_is_reported(lib):
    b = CC.bases()
    assert lib.host_check_cfg(b["full"], is_fork=True) == (CC.EINVAL, CC.FORK)
    assert lib.host_check_cfg(b["lora"], is_fork=True) == (0, "")
    # several faults: the engine's order decides
    assert lib.host_check_cfg(CC.variant(CC.variant(b["lora"], "arch", 9), "precision", 9))[1] == "precision must be TST_PRECISION_BF16 or TST_PRECISION_STRICT"
    assert lib.host_check_cfg(CC.variant(CC.variant(b["lora"], "head_dim", 0), "train_mode", 9))[1] == CC.POSITIVE
    assert lib.host_check_cfg(CC.variant(CC.variant(b["lora"], "lora_targets", 0), "n_stack", 9))[1] == "n_stack must be <= 8"
    assert lib.host_check_cfg(CC.variant(CC.variant(b["full"], "n_stack", 2), "head_dim", 64), is_fork=True)[1] == CC.FORK
    # what a family does not use is not looked at: RoPE scaling of a GPT-2 context, rank and targets of a full fine-tune
    assert lib.host_check_cfg(CC.variant(b["gpt2"], "rope_scaling", 3)) == (0, "")
    assert lib.host_check_cfg(CC.variant(CC.variant(b["full"], "lora_r", 0), "lora_targets", 0)) == (0, "")


def test_lora_layout_of_tiny_matches_the_hf_fixture(lib, golden_dir):
    """names and shapes of tests/golden/lora_tiny.npz (peft's own parameters of TINY_CFG at r = 16, all seven modules), in the fixture's order"""
    g = np.load(os.path.join(golden_dir, "lora_tiny.npz"))
    want = [(k[3:], g[k].shape) for k in g.files if k.startswith("g0/")]
    lay = lib.host_lora_layout(CC.model_cfg(GI.TINY_CFG))
    assert len(want) == 28 and [(n, (r, c)) for n, _, r, c in lay["entries"]] == want
    at = 0
    for _, off, r, c in lay["entries"]:
        assert off == at
        at += r * c
    assert lay["n1"] == lay["n_train"] == at


@pytest.mark.parametrize("fam", list(CC.GOLDEN))
def test_lora_layout_against_the_written_out_module_list(lib, fam):
    cfg = CC.GOLDEN[fam]
    mods = GI.GPT2_MODS if cfg.get("arch") == "gpt2" else GI.MODS
    subsets = [None, mods[:1], mods[-1:], (mods[0], mods[-2])] + [(m,) for m in mods]
    for targets in subsets:
        for r, ns in ((16, 1), (8, 3)):
            kw = dict(lora_r=r, n_stack=ns)
            if targets is not None:
                kw["lora_targets"] = tuple(targets)
            want, n1 = CC.lora_table(cfg, r, targets)
            lay = lib.host_lora_layout(CC.model_cfg(cfg, **kw))
            assert lay["entries"] == want and lay["n1"] == n1 and lay["n_train"] == n1 * ns
    # GPT-2: any of Q / K / V enables c_attn, GATE or UP enables c_fc
    if cfg.get("arch") == "gpt2":
        for bits, mod in ((1, "attn.c_attn"), (2, "attn.c_attn"), (4, "attn.c_attn"), (8, "attn.c_proj"), (16, "mlp.c_fc"), (32, "mlp.c_fc"), (64, "mlp.c_proj")):
            lay = lib.host_lora_layout(CC.variant(CC.model_cfg(cfg), "lora_targets", bits))
            assert lay["entries"] == CC.lora_table(cfg, 16, (mod,))[0]


@pytest.mark.parametrize("fam", list(CC.GOLDEN))
def test_written_out_full_table_agrees_with_host_full_layout(lib, fam):
    """the table test_create_gpu.py holds tst_trainable_info of a full fine-tune to, anchored on tsthost::full_layout's offsets"""
    cfg = CC.GOLDEN[fam]
    table, n = CC.full_table(cfg)
    fl = lib.host_full_layout(CC.model_cfg(cfg, train_mode="full"))
    at = {name: off for name, off, _, _ in table}
    gpt2 = cfg.get("arch") == "gpt2"
    assert n == fl["n_train"] and table[0][1] == fl["embed"] == 0
    assert at["transformer.h.0.attn.c_attn.weight" if gpt2 else "model.layers.0.self_attn.q_proj.weight"] == fl["layer0"]
    assert at["transformer.h.0.ln_1.weight" if gpt2 else "model.layers.0.input_layernorm.weight"] == fl["tail"] == fl["n_decay"]
    if gpt2:
        assert at["transformer.wpe.weight"] == fl["wpe"] and fl["lm_head"] == fl["embed"]
    else:
        assert at["lm_head.weight"] == fl["lm_head"]
    assert at["transformer.h.1.attn.c_attn.weight" if gpt2 else "model.layers.1.self_attn.q_proj.weight"] == fl["layer0"] + fl["per_layer"]
