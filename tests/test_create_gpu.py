"""tst_create / tst_fork on the device, held to the tables of tests/create_cases.py: every accepted configuration gets the trainable table, the K-major bits and
the last-layer compaction it must get; every refused one is refused with the return code and the message tsthost::check_cfg gives on the CPU, and leaves nothing
behind. Creation and queries only (a fork needs finalised weights: tst_init_random): no training step."""
import ctypes as C

import pytest

import create_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tst import lib
    lib.load()
    lib.load_host()
    return lib


def table_of(ctx):
    return [(name, off, rows, cols) for name, (off, rows, cols) in ctx.trainable_layout().items()]


def raw_create(lib, mc):
    """(rc, message, handle) of tst_create itself"""
    h = C.c_void_p()
    rc = lib.load().tst_create(C.byref(mc), 0, C.byref(h))
    return int(rc), lib.load().tst_last_error(None).decode(), h


@pytest.mark.parametrize("tag,cfg,kw,forkable", CC.accepted(), ids=[a[0] for a in CC.accepted()])
def test_accepted_configuration(lib, tag, cfg, kw, forkable):
    mc = CC.model_cfg(cfg, **kw)
    assert lib.host_check_cfg(mc) == (0, "")
    full, strict, ns = kw.get("train_mode") == "full", kw.get("precision") == "strict", kw.get("n_stack", 1)
    ctx = lib.Context(cfg, **dict(CC.WORKSPACE, **kw))
    kid = None
    try:
        if full:
            want, n1 = CC.full_table(cfg)
            assert n1 == lib.host_full_layout(mc)["n_train"]
        else:
            want, n1 = CC.lora_table(cfg, kw.get("lora_r", 16), kw.get("lora_targets"))
            lay = lib.host_lora_layout(mc)
            assert lay["entries"] == want and lay["n1"] == n1 and lay["n_train"] == n1 * ns
        assert table_of(ctx) == want
        assert ctx.trainable_numel() == n1 and int(ctx.lib.tst_stack_size(ctx.h)) == ns
        assert int(ctx.lib.tst_set_option(ctx.h, b"kmajor", -1)) == (3 if full and not strict else 0)
        assert int(ctx.lib.tst_set_option(ctx.h, b"last_compact", -1)) == (CC.EINVAL if full else 1)
        assert ctx.device_bytes() > 0
        print(f"[create] {tag} device_bytes={ctx.device_bytes()} n_train={n1 * ns} entries={len(want)}")
        if forkable:
            ctx.init_random(seed=1, std=0.02)
            kid = ctx.fork()
            assert table_of(kid) == want and kid.trainable_numel() == n1
            assert int(kid.lib.tst_set_option(kid.h, b"last_compact", -1)) == 1
            assert 0 < kid.device_bytes() < ctx.device_bytes()   # (the frozen weights and the RoPE tables are the parent's)
            print(f"[create] {tag}/fork device_bytes={kid.device_bytes()}")
    finally:
        if kid is not None:
            kid.close()
        ctx.close()


def _refused(lib, cases):
    b = CC.bases()
    probe = lambda: lib.Context(CC.FAMILIES["llama"], **CC.WORKSPACE)
    first = probe()
    before = first.device_bytes()
    first.close()
    for base, field, value, msg in cases:
        mc = CC.variant(b[base], field, value)
        rc, err, h = raw_create(lib, mc)
        assert (rc, err) == (CC.EINVAL, msg) == lib.host_check_cfg(mc) and not h.value, (base, field, value, rc, err)
    after = probe()
    try:
        assert after.device_bytes() == before
    finally:
        after.close()


def test_refused_configurations_give_check_cfgs_answer(lib):
    _refused(lib, CC.REFUSALS)


def test_zero_sizes_are_refused_by_tst_create(lib):
    _refused(lib, [(base, field, value, CC.POSITIVE) for base, field, value in CC.ZERO_SIZE])


def test_a_full_fine_tune_refuses_to_fork(lib):
    ctx = lib.Context(CC.FAMILIES["llama"], **dict(CC.WORKSPACE, train_mode="full"))
    try:
        ctx.init_random(seed=1, std=0.02)
        before = ctx.device_bytes()
        h = C.c_void_p()
        assert int(ctx.lib.tst_fork(ctx.h, C.byref(h))) == CC.EINVAL and not h.value
        assert ctx.lib.tst_last_error(ctx.h).decode() == CC.FORK == lib.host_check_cfg(CC.model_cfg(CC.FAMILIES["llama"], train_mode="full"), is_fork=True)[1]
        assert ctx.device_bytes() == before
    finally:
        ctx.close()
