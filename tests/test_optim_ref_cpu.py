"""The references of tests/test_optim_kernels_gpu.py checked on their own, so that they cannot be wrong unnoticed: the float64 AdamW / clip evaluation
(oracle/ops_np.py adamw_step64, clip_coef64) against the torch-fused record of tests/golden/ops.npz and against the fp32 numpy oracle, the LoRA pack / unpack
restatement (lora_pack_ref, lora_unpack_ref) against the dense definition of a LoRA module group and against each other."""
import os

import numpy as np

from oracle import ops_np as O

HP = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)


def _close(name, a, b, rtol=2e-6, atol_rms=1e-6):
    """the tolerance of test_adamw_clip: |a - b| <= rtol |b| + atol_rms rms(b) per element"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rms = float(np.sqrt(np.mean(b * b))) + 1e-30
    bad = np.abs(a - b) > rtol * np.abs(b) + atol_rms * rms
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.size} out of tolerance, max|d|={np.abs(a - b).max():.3e} rms(ref)={rms:.3e}"


def test_adamw64_and_clip64_follow_the_torch_fused_record(golden_dir):
    g = np.load(os.path.join(golden_dir, "ops.npz"))
    n = g["ad_p0"].size
    p, m, v = g["ad_p0"].astype(np.float64), np.zeros(n), np.zeros(n)
    p32, m32, v32 = g["ad_p0"].astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for s in range(3):
        norm, coef = O.clip_coef64(g["ad_g"][s], 1.0)
        assert abs(norm - g["ad_norm"][s]) <= 1e-5 * g["ad_norm"][s]
        norm32, coef32 = O.clip_coef(g["ad_g"][s], 1.0)
        assert abs(norm - norm32) <= 1e-6 * norm and abs(coef - coef32) <= 1e-6 * coef
        p, m, v = O.adamw_step64(p, g["ad_g"][s], m, v, s + 1, coef=coef, **HP)
        _close(f"adamw64 step {s + 1} p vs torch fused", p, g["ad_p"][s])
        p32, m32, v32 = O.adamw_step(p32, g["ad_g"][s] * coef32, m32, v32, s + 1, **HP)
        for name, a, b in (("p", p32, p), ("m", m32, m), ("v", v32, v)):
            _close(f"adamw_step fp32 vs adamw64 step {s + 1} {name}", a, b)


def test_adamw64_single_step_from_given_states_follows_the_fp32_oracle():
    """the recipe of the GPU cases (ops_np.optim_recipe: uploaded states, every seventh gradient element 0; a coefficient below 1), where no torch record exists"""
    n = 4099
    p, g, m, v = O.optim_recipe(n, 5)
    assert not g[6::7].any() and np.count_nonzero(g) == n - n // 7
    coef = np.float32(0.4)
    for step in (1, 7):
        ref = O.adamw_step64(p, g, m, v, step, coef=coef, **HP)
        got = O.adamw_step(p, g * coef, m, v, step, **HP)
        for name, a, b in zip("pmv", got, ref):
            _close(f"step {step} {name}", a, b)


def _tiny_group(rng, nslot=1, scale=1.0):
    din, dout, r, rows = 64, 192, 4, [(0, 64), (128, 192)]   # rows 64 .. 127 belong to no enabled module
    (off,), n1, end = O.lora_offsets([(din, r, rows)], nslot, base=12)
    gd = O.lora_group(din, dout, r, rows, nslot, off[0], off[1], scale)
    return gd, rng.standard_normal(end + 5).astype(np.float32), n1


def test_pack_reference_is_the_dense_lora_product():
    """Bg . Ag == sum over the modules of B_seg . A_seg placed at the module's rows (one slot), and AgT / BgT are the scaled resp. plain transposes"""
    rng = np.random.default_rng(0)
    gd, master, _ = _tiny_group(rng, scale=0.5)
    Ag, AgT, Bg, BgT = O.lora_pack_ref(gd, master)
    dense = np.zeros((gd["dout"], gd["din"]))
    for mod, (r0, r1) in enumerate(gd["rows"]):
        A = master[gd["a_off"][mod]:][:gd["r"] * gd["din"]].reshape(gd["r"], gd["din"]).astype(np.float64)
        B = master[gd["b_off"][mod]:][:(r1 - r0) * gd["r"]].reshape(r1 - r0, gd["r"]).astype(np.float64)
        dense[r0:r1] += B @ A
    np.testing.assert_allclose(Bg.astype(np.float64) @ Ag.astype(np.float64), dense, rtol=1e-13, atol=1e-15)   # four float64 products per element either way
    assert not dense[64:128].any() and dense[:64].any() and dense[128:].any()
    assert Ag.shape == (64, 64) and not Ag[8:].any() and not Bg[:, 8:].any()   # nseg r = 8 of RP = 64 columns are live
    np.testing.assert_array_equal(AgT, (np.float32(0.5) * Ag).T)
    np.testing.assert_array_equal(BgT, Bg.T)


def test_unpack_reference_inverts_the_pack_reference():
    rng = np.random.default_rng(1)
    gd, master, n1 = _tiny_group(rng, nslot=3)
    assert gd["nseg"] == 6 and gd["a_off"][2] == gd["a_off"][0] + n1 and gd["b_off"][5] == gd["b_off"][1] + 2 * n1
    Ag, AgT, Bg, BgT = O.lora_pack_ref(gd, master)
    np.testing.assert_array_equal(AgT, Ag.T)
    grad = O.lora_unpack_ref(gd, Ag, Bg, np.full_like(master, np.nan))
    lo, hi = 12, 12 + 3 * n1   # one group: its segments tile [base, base + nslot n1)
    np.testing.assert_array_equal(grad[lo:hi], master[lo:hi])
    assert np.isnan(grad[:lo]).all() and np.isnan(grad[hi:]).all()
