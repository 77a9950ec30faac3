"""GPU tests of the optimizer kernels of csrc/optim.hip one by one, through the lab hooks (tst_k_clip_coef .. tst_k_lora_unpack_grad): global-norm clip
stages, flat and tiled AdamW, gradient accumulation, LoRA pack / unpack -- at the sizes where their code takes another path (unaligned pointers, tails, the
partly live second piece, several workgroups, the second trip of a capped grid-stride loop, idle workgroups, rank chunks, stacked slots, groups of unequal
size in one launch).

References (oracle/ops_np.py, checked on their own in tests/test_optim_ref_cpu.py): AdamW = the header formula of optim.hip in float64 (adamw_step64), at the
tolerance of test_adamw_clip, |d| <= 2e-6 |ref| + 1e-6 rms(ref), for p, m AND v; norms against the float64 sum at 1e-5 relative; everything else bit for bit.
Every device array sits behind a guard of GUARD sentinel elements (and, where stated, behind an offset that breaks its 16-byte alignment); the guard and the
offset are checked bit for bit after each call, so a tail or a padding write beyond the array fails the test.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ops_np as O
from test_kernels_gpu import assert_close, report

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = {4: 0xFFC5A5A5, 2: 0xFFC5}   # a NaN of the element type: read by mistake it poisons a sum, overwritten it shows
UINT = {4: np.uint32, 2: np.uint16}
EINVAL = -1   # TST_EINVAL of include/tst_hip.h
HP = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)


@pytest.fixture(scope="module")
def L():
    from tst import lib
    lib.load_lab()
    assert lib.device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    return lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def sentinel(n, dtype=np.float32):
    dt = np.dtype(dtype)
    return np.full(n, SENT[dt.itemsize], UINT[dt.itemsize]).view(dt)


class G:
    """n elements on the device at `off` elements into a larger allocation (off = 1 breaks the 16-byte alignment of an fp32 array, the 8-byte alignment of a bf16
    one) with GUARD sentinel elements behind them; get() returns the n elements after checking that the offset and the guard still hold the sentinel"""

    def __init__(self, L, host, off=0):
        host = np.ascontiguousarray(host).reshape(-1)
        self.n, self.off, self.dtype = host.size, off, host.dtype
        full = sentinel(off + self.n + GUARD, host.dtype)
        full[off:off + self.n] = host
        self.dev = L.DevBuf(full)
        self.ptr = C.c_void_p(self.dev.ptr.value + off * host.dtype.itemsize)

    def get(self, shape=None):
        full = self.dev.get(self.dtype, (self.off + self.n + GUARD,))
        out = full[self.off:self.off + self.n]
        full = bits(full)
        assert (full[:self.off] == SENT[self.dtype.itemsize]).all(), "write in front of the array"
        assert (full[self.off + self.n:] == SENT[self.dtype.itemsize]).all(), "write behind the array's last element"
        return out.copy().reshape(shape if shape is not None else (self.n,))


def same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ------------------------------------------------------------------------------------------------------------------ inputs
recipe_g, adam_inputs = O.optim_recipe_g, O.optim_recipe   # shared with tests/test_optim_ref_cpu.py, which checks the references on this very recipe


COEF = np.float32(0.4)   # the device {norm, coef} pair of the clipped cases: the kernel must read element 1


def run_flat(L, inp, step, wd, coef, offs=(0, 0, 0, 0), shadow=None, shadow_off=0, at=None):
    """one tst_k_adamw_flat call; returns (p, m, v, shadow bits or None). g must come back unchanged. at: the element type of the compute copy, which picks the
    kernel's instance also where shadow is NULL (default: that of `shadow`, bf16 without one)"""
    p, g, m, v = inp
    n = p.size
    P, Gr, M, V = (G(L, a, o) for a, o in zip((p, g, m, v), offs))
    clip = G(L, np.array([2.5, coef], np.float32)) if coef is not None else None
    sdt = {None: None, "bf16": np.uint16, "f32": np.float32}[shadow]
    S = G(L, sentinel(n, sdt), shadow_off) if shadow else None
    rc = L.load_lab().tst_k_adamw_flat(P.ptr, Gr.ptr, M.ptr, V.ptr, n, clip.ptr if clip else None, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, step,
                                       S.ptr if S else None, 1 if (at or shadow) == "f32" else 0)
    assert rc == 0, f"tst_k_adamw_flat rc={rc}"
    same_bits(Gr.get(), g, "g after the step")
    if clip:
        same_bits(clip.get(), np.array([2.5, coef], np.float32), "clip pair after the step")
    return P.get(), M.get(), V.get(), (S.get() if S else None)


_REF = {}


def flat_ref(n, seed, step, wd, coef):
    key = (n, seed, step, wd, None if coef is None else float(coef))
    if key not in _REF:
        p, g, m, v = adam_inputs(n, seed)
        _REF[key] = O.adamw_step64(p, g, m, v, step, wd=wd, coef=1.0 if coef is None else coef, **HP)
    return _REF[key]


def check_pmv(name, got, ref):
    for what, a, b in zip("pmv", got[:3], ref):
        assert_close(f"{name} {what}", a, b, 2e-6, 1e-6)


def check_shadow(p_out, s, shadow):
    if shadow == "bf16":
        same_bits(s, O.to_bf16_bits(p_out), "bf16 compute copy vs rounded p")
    else:
        same_bits(s, p_out, "fp32 compute copy vs p")


SMALL_N = [1, 3, 4, 1027, 1028, 2051, 6149]   # tails 1 / 3 / 0; 1028: n4 = 257, one piece past a full stride; 2051: two full pieces + tail; 6149: four workgroups
LARGE_N = 16_779_267                          # n4 = 4 194 816 > 8192 workgroups x 256 lanes x 2 pieces: the smallest size with a second trip of the loop; tail 3


# ------------------------------------------------------------------------------------------------------------------ flat AdamW
@pytest.mark.parametrize("step,wd,clipped", [(7, 0.05, True), (1, 0.0, False), (1, 0.05, False), (7, 0.0, True)])
@pytest.mark.parametrize("n", SMALL_N)
def test_adamw_flat_plain_instance(L, n, step, wd, clipped):
    """shadow == NULL: the default-policy instance; clip from a device {norm, coef} pair with coef < 1, and clip == NULL"""
    coef = COEF if clipped else None
    got = run_flat(L, adam_inputs(n, n), step, wd, coef)
    check_pmv(f"adamw_flat n{n} step{step} wd{wd} clip{int(clipped)}", got, flat_ref(n, n, step, wd, coef))


@pytest.mark.parametrize("shadow", ["bf16", "f32"])
@pytest.mark.parametrize("n", SMALL_N)
def test_adamw_flat_compute_copy_and_nontemporal_instance(L, n, shadow):
    """shadow != NULL selects the non-temporal instance: the compute copy is the rounded / the very p, and p, m, v are bit-identical to the plain instance's
    (the claim of the comment in adamw_step). The claim holds per element type: the bf16 and the fp32 instance differ from EACH OTHER in the last bit of m on
    a few per cent of the second in-flight piece's elements and of p on far fewer (counts and the presumed cause, another FMA contraction of the m update, in
    profiles/optim_kernel_parity.txt; both forms far inside the tolerance), so the plain run takes the compute copy's type."""
    inp = adam_inputs(n, n)
    nt = run_flat(L, inp, 7, 0.05, COEF, shadow=shadow)
    check_pmv(f"adamw_flat_nt {shadow} n{n}", nt, flat_ref(n, n, 7, 0.05, COEF))
    check_shadow(nt[0], nt[3], shadow)
    plain = run_flat(L, inp, 7, 0.05, COEF, at=shadow)   # the plain instance of the same element type
    for what, a, b in zip("pmv", nt[:3], plain[:3]):
        same_bits(a, b, f"{what}: non-temporal vs plain instance")


@pytest.mark.parametrize("shadow", [None, "bf16", "f32"])
def test_adamw_flat_unaligned_arrays_take_the_scalar_path(L, shadow):
    """p, g, m, v each one float past a 16-byte boundary (n4 = 0: every element through the scalar loop, several workgroups)"""
    n = 2051
    got = run_flat(L, adam_inputs(n, n), 7, 0.05, COEF, offs=(1, 1, 1, 1), shadow=shadow)
    check_pmv(f"adamw_flat unaligned n{n} shadow {shadow}", got, flat_ref(n, n, 7, 0.05, COEF))
    if shadow:
        check_shadow(got[0], got[3], shadow)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_adamw_flat_one_unaligned_array_is_enough(L, which):
    n = 2051
    offs = tuple(1 if i == which else 0 for i in range(4))
    got = run_flat(L, adam_inputs(n, n), 7, 0.05, COEF, offs=offs, shadow="bf16")
    check_pmv(f"adamw_flat unaligned array {which}", got, flat_ref(n, n, 7, 0.05, COEF))
    check_shadow(got[0], got[3], "bf16")


@pytest.mark.parametrize("shadow", ["bf16", "f32"])
def test_adamw_flat_only_the_compute_copy_unaligned(L, shadow):
    """the alignment test of shadow is 4 sizeof(AT): one element off sends the whole call down the scalar path, 8-byte / 16-byte stores must not happen"""
    n = 2051
    got = run_flat(L, adam_inputs(n, n), 7, 0.05, COEF, shadow=shadow, shadow_off=1)
    check_pmv(f"adamw_flat unaligned {shadow} copy", got, flat_ref(n, n, 7, 0.05, COEF))
    check_shadow(got[0], got[3], shadow)


def test_adamw_flat_second_trip_of_the_grid_stride_loop(L):
    """the one large case: 8192 workgroups (the cap), pieces 0 .. 4 194 303 in the first trip, 512 pieces in the second, a tail of 3; both instances"""
    n = LARGE_N
    inp = adam_inputs(n, 99)
    ref = O.adamw_step64(*inp, 7, wd=0.05, coef=COEF, **HP)
    nt = run_flat(L, inp, 7, 0.05, COEF, shadow="bf16")
    check_pmv(f"adamw_flat_nt n{n}", nt, ref)
    check_shadow(nt[0], nt[3], "bf16")
    del ref
    plain = run_flat(L, inp, 7, 0.05, COEF, at="bf16")
    for what, a, b in zip("pmv", nt[:3], plain[:3]):
        same_bits(a, b, f"{what}: non-temporal vs plain instance")


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_adamw_flat_zero_gradient_with_zero_state_only_decays(L, wd):
    """g = m = v = 0 at every seventh element: denom = eps, m / denom = 0 -- p only decays (is untouched at wd = 0), m and v stay 0, nothing is non-finite"""
    n = 2051
    p, g, m, v = adam_inputs(n, 7)
    z = g == 0
    assert z.sum() == n // 7
    m[z] = 0
    v[z] = 0
    got = run_flat(L, (p, g, m, v), 1, wd, None)
    check_pmv(f"adamw_flat zero-g wd{wd}", got, O.adamw_step64(p, g, m, v, 1, wd=wd, **HP))
    assert all(np.isfinite(a).all() for a in got[:3])
    assert not got[1][z].any() and not got[2][z].any()
    decay = 1.0 - float(np.float32(HP["lr"])) * float(np.float32(wd))
    assert np.abs(got[0][z] - p[z].astype(np.float64) * decay).max() <= 2e-6 * np.abs(p[z]).max()
    if wd == 0.0:
        same_bits(got[0][z], p[z], "p where g = m = v = 0, no decay")


def test_adamw_flat_three_steps_with_clip_stage(L):
    """three steps from zero states, the coefficient of each from tst_k_clip_coef on that step's gradient (norm about 17 against max_norm 1); p, m and v after
    every step against the float64 trajectory. The clip stage has its own, wider bound (1e-5 on the norm), so the float64 AdamW reference is handed the
    kernel's coefficient, which is checked where it is made: norm against the float64 sum, coefficient against the fp32 formula on that norm."""
    n = 1000
    lab = L.load_lab()
    rng = np.random.default_rng(3)
    p0 = np.float32(0.05) * rng.standard_normal(n, dtype=np.float32)
    P, M, V = G(L, p0), G(L, np.zeros(n, np.float32)), G(L, np.zeros(n, np.float32))
    ws, nc = G(L, sentinel(256)), G(L, sentinel(2))
    ref = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    for s in range(1, 4):
        g = recipe_g(rng, n)
        Gr = G(L, g)
        assert lab.tst_k_clip_coef(Gr.ptr, n, 1.0, ws.ptr, 256, nc.ptr) == 0
        norm, coef = nc.get()
        norm64, coef64 = O.clip_coef64(g, 1.0)
        assert abs(norm - norm64) <= 1e-5 * norm64 and coef64 < 0.2
        assert ulps(coef, np.float32(1.0) / (np.float32(norm) + np.float32(1e-6))) <= 1
        assert lab.tst_k_adamw_flat(P.ptr, Gr.ptr, M.ptr, V.ptr, n, nc.ptr, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 0.05, s, None, 0) == 0
        ref = O.adamw_step64(*ref[:1], g, *ref[1:], s, wd=0.05, coef=coef, **HP)
        check_pmv(f"adamw_flat trajectory step{s}", (P.get(), M.get(), V.get()), ref)


# ------------------------------------------------------------------------------------------------------------------ tiled AdamW
@pytest.mark.parametrize("at", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", [(64, 64), (64, 192), (192, 64), (128, 320)])
def test_adamw_matrix(L, rows, cols, at):
    """64 x 64 tiles of a row-major matrix: p, m, v against the reference, the compute copy == rounded p, its transpose == the copy transposed, bit for bit;
    the non-square shapes tell rows from cols in the tile index and in the pitch of the transposed copy"""
    n = rows * cols
    inp = adam_inputs(n, rows * 1000 + cols)
    sdt = np.uint16 if at == "bf16" else np.float32
    P, Gr, M, V = (G(L, a) for a in inp)
    clip = G(L, np.array([2.5, COEF], np.float32))
    S, ST = G(L, sentinel(n, sdt)), G(L, sentinel(n, sdt))
    rc = L.load_lab().tst_k_adamw_matrix(P.ptr, Gr.ptr, M.ptr, V.ptr, rows, cols, clip.ptr, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 0.05, 7, S.ptr, ST.ptr,
                                         1 if at == "f32" else 0)
    assert rc == 0, f"tst_k_adamw_matrix rc={rc}"
    got = (P.get(), M.get(), V.get())
    check_pmv(f"adamw_matrix {at} {rows}x{cols}", got, O.adamw_step64(*inp, 7, wd=0.05, coef=COEF, **HP))
    same_bits(Gr.get(), inp[1], "g after the step")
    s, sT = S.get((rows, cols)), ST.get((cols, rows))
    check_shadow(got[0].reshape(rows, cols), s, at)
    same_bits(sT, np.ascontiguousarray(s.T), "transposed compute copy vs the copy")


def test_adamw_matrix_refuses_partial_tiles_and_missing_copies(L):
    n = 96 * 96
    inp = adam_inputs(n, 1)
    P, Gr, M, V = (G(L, a) for a in inp)
    S, ST = G(L, sentinel(n, np.uint16)), G(L, sentinel(n, np.uint16))
    call = lambda rows, cols, s, st: L.load_lab().tst_k_adamw_matrix(P.ptr, Gr.ptr, M.ptr, V.ptr, rows, cols, None, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                                                                      0.0, 1, s, st, 0)
    assert call(96, 64, S.ptr, ST.ptr) == EINVAL
    assert call(64, 96, S.ptr, ST.ptr) == EINVAL
    assert call(64, 64, S.ptr, None) == EINVAL
    assert call(64, 64, None, ST.ptr) == EINVAL
    for buf, a in zip((P, Gr, M, V), inp):   # nothing ran
        same_bits(buf.get(), a, "array after a refused call")
    S.get(), ST.get()


# ------------------------------------------------------------------------------------------------------------------ clip
def clip_coef_run(L, g, max_norm, nparts, goff=0):
    Gr, ws, out = G(L, g, goff), G(L, sentinel(max(nparts, 1))), G(L, sentinel(2))
    rc = L.load_lab().tst_k_clip_coef(Gr.ptr, g.size, max_norm, ws.ptr, nparts, out.ptr)
    same_bits(Gr.get(), g, "g after the clip pass")
    ws.get()
    return rc, out.get()


def check_norm_coef(name, norm, coef, norm64, max_norm):
    report(name, norm=float(norm), rel_err=abs(float(norm) - norm64) / norm64)
    assert abs(float(norm) - norm64) <= 1e-5 * norm64, f"{name}: norm {norm} vs {norm64}"
    if max_norm > 0 and float(norm) > max_norm:
        want = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))   # the fp32 formula on the kernel's own norm: only the division's rounding may differ
        assert want < 1 and ulps(coef, want) <= 1, f"{name}: coef {coef} vs {want}"
    else:
        assert np.float32(coef) == np.float32(1.0), f"{name}: coef {coef}"


@pytest.mark.parametrize("n,nparts", [(1, 256), (3, 256), (5, 256), (1023, 256), (1025, 256), (262_147, 256), (1_048_583, 256), (262_147, 1), (262_147, 4096)])
def test_clip_coef(L, n, nparts):
    """nparts is clamped to the work (n <= 1025: one or two workgroups of the 256 asked for; 4096 asked at 262 147: 256); 1 048 583 gives every lane a second
    piece (a workgroup stride); nparts = 1 walks the whole array with one workgroup. max_norm below the norm: coef < 1"""
    g = recipe_g(np.random.default_rng(n + nparts), n)
    norm64 = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    max_norm = float(np.float32(0.37 * norm64))
    rc, (norm, coef) = clip_coef_run(L, g, max_norm, nparts)
    assert rc == 0
    check_norm_coef(f"clip_coef n{n} parts{nparts}", norm, coef, norm64, max_norm)
    assert coef < 1


def test_clip_coef_arguments(L):
    g = recipe_g(np.random.default_rng(0), 1025)
    for nparts in (0, 4097):
        rc, out = clip_coef_run(L, g, 1.0, nparts)
        assert rc == EINVAL
        same_bits(out, sentinel(2), "out2 after a refused call")


def test_clip_refuses_an_unaligned_gradient(L):
    """sumsq_partial_kernel reads 16-byte pieces and has no scalar form: the host refuses a pointer that is not 16-byte aligned, nothing is launched"""
    g = recipe_g(np.random.default_rng(0), 1025)
    for off in (1, 2, 3):
        rc, out = clip_coef_run(L, g, 1.0, 256, goff=off)
        assert rc == EINVAL
        same_bits(out, sentinel(2), "out2 after a refused call")
        Gr, part = G(L, g, off), G(L, sentinel(8))
        assert L.load_lab().tst_k_sumsq_partial(Gr.ptr, g.size, part.ptr, 8) == EINVAL
        same_bits(part.get(), sentinel(8), "partials after a refused call")
    rc, out = clip_coef_run(L, g, 1.0, 256, goff=4)   # 16 bytes in: aligned again
    assert rc == 0 and np.isfinite(out).all()


@pytest.mark.parametrize("max_norm", [0.0, -1.0])
def test_clip_coef_disabled_gives_exactly_one(L, max_norm):
    g = recipe_g(np.random.default_rng(1), 1025)
    rc, (norm, coef) = clip_coef_run(L, g, max_norm, 256)
    assert rc == 0
    check_norm_coef(f"clip_coef max_norm{max_norm}", norm, coef, float(np.sqrt(np.sum(g.astype(np.float64) ** 2))), max_norm)
    assert bits(np.float32(coef)) == bits(np.float32(1.0))


def test_clip_coef_norm_below_max_norm_gives_exactly_one(L):
    g = recipe_g(np.random.default_rng(2), 1025)
    g = (g * (0.5 / np.sqrt(np.sum(g.astype(np.float64) ** 2)))).astype(np.float32)
    norm64 = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    assert abs(norm64 - 0.5) < 1e-6
    rc, (norm, coef) = clip_coef_run(L, g, 1.0, 256)
    assert rc == 0
    check_norm_coef("clip_coef norm 0.5 max_norm 1", norm, coef, norm64, 1.0)
    assert bits(np.float32(coef)) == bits(np.float32(1.0))


def test_sumsq_partial_idle_workgroups_write_zero(L):
    """the engine adds ALL partials of a 1024 / 2048-workgroup launch, also on ranges of fewer than 256 nparts 4 elements: n = 1000 is work for workgroup 0 only, and
    the other 1023 must overwrite whatever the buffer held (here NaN) with an exact 0"""
    n, nparts = 1000, 1024
    g = recipe_g(np.random.default_rng(4), n)
    Gr, part = G(L, g), G(L, np.full(nparts, np.nan, np.float32))
    assert L.load_lab().tst_k_sumsq_partial(Gr.ptr, n, part.ptr, nparts) == 0
    got = part.get()
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} partials were not written"
    assert not bits(got[1:]).any(), "idle workgroups must write +0"
    ref = float(np.sum(g.astype(np.float64) ** 2))
    report("sumsq_partial n1000 parts1024", sum=float(got.sum(dtype=np.float64)), rel_err=abs(float(got.sum(dtype=np.float64)) - ref) / ref)
    assert abs(np.sqrt(got.sum(dtype=np.float64)) - np.sqrt(ref)) <= 1e-5 * np.sqrt(ref)


@pytest.mark.parametrize("nparts,off", [(1, 0), (3, 0), (4, 0), (1023, 0), (4099, 0), (330_001, 0), (4099, 1)])
def test_clip_finalize(L, nparts, off):
    """16 bytes per lane on an aligned buffer (tails 1 / 3 / 0 / 3 / 3 / 1), one float per lane on an unaligned one; 330 001 = a full fine-tune's tile partials"""
    part = np.abs(np.random.default_rng(nparts).standard_normal(nparts, dtype=np.float32)) * np.float32(3e-3)
    norm64 = float(np.sqrt(np.sum(part.astype(np.float64))))
    max_norm = float(np.float32(0.5 * norm64))
    Pt, out = G(L, part, off), G(L, sentinel(2))
    assert L.load_lab().tst_k_clip_finalize(Pt.ptr, nparts, max_norm, out.ptr) == 0
    same_bits(Pt.get(), part, "partials after the pass")
    norm, coef = out.get()
    check_norm_coef(f"clip_finalize parts{nparts} off{off}", norm, coef, norm64, max_norm)
    assert coef < 1


@pytest.mark.parametrize("nparts", [1, 256, 300])
def test_sum_partials_then_clip_from_sumsq(L, nparts):
    """the sharded optimizer's pair: the shard's sum of squares, then {norm, coef} from the (all-reduced) sum"""
    lab = L.load_lab()
    part = np.abs(np.random.default_rng(nparts).standard_normal(nparts, dtype=np.float32)) * np.float32(0.7)
    sum64 = float(np.sum(part.astype(np.float64)))
    Pt, one, out = G(L, part), G(L, sentinel(1)), G(L, sentinel(2))
    assert lab.tst_k_sum_partials(Pt.ptr, nparts, one.ptr) == 0
    s = one.get()
    assert abs(np.sqrt(float(s[0])) - np.sqrt(sum64)) <= 1e-5 * np.sqrt(sum64)
    for max_norm in (float(np.float32(0.5 * np.sqrt(sum64))), float(np.float32(2 * np.sqrt(sum64))), 0.0):
        assert lab.tst_k_clip_from_sumsq(one.ptr, max_norm, out.ptr) == 0
        norm, coef = out.get()
        check_norm_coef(f"clip_from_sumsq parts{nparts} max_norm{max_norm:.3g}", norm, coef, np.sqrt(sum64), max_norm)
    same_bits(one.get(), s, "the sum after clip_from_sumsq")
    same_bits(Pt.get(), part, "partials after the pass")


# ------------------------------------------------------------------------------------------------------------------ gradient accumulation
@pytest.mark.parametrize("n,aoff,goff", [(1, 0, 0), (8, 0, 0), (1027, 0, 0), (4_195_333, 0, 0), (1027, 1, 0), (1027, 0, 1)])
def test_grad_accumulate(L, n, aoff, goff):
    """first = 1 must not read acc (the engine hands it fresh pool memory: here NaN); first = 0 is one fp32 add per element. 4 195 333 = past the 4096-workgroup
    cap (a second trip for 772 pieces) with a tail of 1; an offset on either array takes the scalar path"""
    lab = L.load_lab()
    rng = np.random.default_rng(n)
    g1, g2 = recipe_g(rng, n), recipe_g(rng, n)
    A, G1 = G(L, np.full(n, np.nan, np.float32), aoff), G(L, g1, goff)
    assert lab.tst_k_grad_accumulate(A.ptr, G1.ptr, n, 1) == 0
    same_bits(A.get(), g1, "acc after first = 1")
    G2 = G(L, g2, goff)
    assert lab.tst_k_grad_accumulate(A.ptr, G2.ptr, n, 0) == 0
    same_bits(A.get(), g1 + g2, "acc after first = 0")
    same_bits(G2.get(), g2, "g after the pass")


# ------------------------------------------------------------------------------------------------------------------ LoRA pack / unpack
QKV = [(0, 128), (128, 192), (192, 256)]   # the q | k | v rows of a fused projection with two kv heads' worth of k and v
# name -> (nslot, [(din, dout, r, rows of the ENABLED modules)])
LORA_CASES = {
    "a_qkv_r16": (1, [(128, 256, 16, QKV)]),
    "b_q_v_only_r8": (1, [(128, 256, 8, [QKV[0], QKV[2]])]),          # rows 128 .. 191 belong to no enabled module: zero in Bg / BgT
    "c_qkv_r1": (1, [(128, 256, 1, QKV)]),                             # r % 8 != 0: the per-element path
    "c_qkv_r2": (1, [(128, 256, 2, QKV)]),
    "c_qkv_r4": (1, [(128, 256, 4, QKV)]),
    "d_8slots_3mod_r8": (8, [(128, 256, 8, QKV)]),                     # RP = 192: three rank chunks
    "d_5slots_2mod_r16": (5, [(128, 256, 16, [(0, 128), (128, 256)])]),   # nseg r = 160 of RP = 192: columns 160 .. 191 are padding
    "d_2slots_1mod_r64": (2, [(128, 256, 64, [(0, 256)])]),            # a segment fills a whole chunk
    "d_3slots_3mod_r32": (3, [(128, 256, 32, QKV)]),                   # RP = 320: five chunks
    "e_two_groups": (1, [(64, 192, 16, [(0, 64), (64, 128), (128, 192)]), (256, 64, 16, [(0, 64)])]),   # grid sized by 256: workgroups of the short axes leave early
    "e_two_groups_2slots_r4": (2, [(64, 192, 4, [(0, 64), (128, 192)]), (256, 64, 4, [(0, 64)])]),
}
FILL = {4: 0x5A5A5A5A, 2: 0x5A5A}   # what the outputs hold beforehand: finite and non-zero, so that every padding zero is a write


def lora_setup(L, case, at, rng):
    nslot, groups = LORA_CASES[case]
    base = 4 * int(rng.integers(1, 16))   # a prefix in front of the first tensor (a multiple of 4 floats: the A master is read 16 bytes at a time)
    offs, n1, end = O.lora_offsets([(din, r, rows) for din, dout, r, rows in groups], nslot, base)
    gds = [O.lora_group(din, dout, r, rows, nslot, a, b, 32.0 / r / 3) for (din, dout, r, rows), (a, b) in zip(groups, offs)]
    odt = np.uint16 if at == "bf16" else np.float32
    bufs = []
    for gd in gds:
        na, nb = gd["RP"] * gd["din"], gd["dout"] * gd["RP"]
        fill = lambda k: np.full(k, FILL[np.dtype(odt).itemsize], UINT[np.dtype(odt).itemsize]).view(odt)
        bufs.append([G(L, fill(na)), G(L, fill(na)), G(L, fill(nb)), G(L, fill(nb)),
                     G(L, rng.standard_normal(na, dtype=np.float32)), G(L, rng.standard_normal(nb, dtype=np.float32))])
    ng = len(gds)
    dims = (C.c_int32 * (5 * ng))(*[x for gd in gds for x in (gd["din"], gd["dout"], gd["r"], gd["nmod"], gd["nslot"])])
    row0, row1 = (C.c_int32 * (4 * ng))(), (C.c_int32 * (4 * ng))()
    a_off, b_off = (C.c_int64 * (32 * ng))(), (C.c_int64 * (32 * ng))()
    for i, gd in enumerate(gds):
        for m_, (r0, r1) in enumerate(gd["rows"]):
            row0[4 * i + m_], row1[4 * i + m_] = r0, r1
        for s in range(gd["nseg"]):
            a_off[32 * i + s], b_off[32 * i + s] = gd["a_off"][s], gd["b_off"][s]
    scale = (C.c_float * ng)(*[gd["scale"] for gd in gds])
    ptrs = (C.c_void_p * (6 * ng))(*[b.ptr.value for gb in bufs for b in gb])
    return gds, bufs, end, (ng, dims, row0, row1, a_off, b_off, scale, ptrs)


@pytest.mark.parametrize("at", ["bf16", "f32"])
@pytest.mark.parametrize("case", list(LORA_CASES))
def test_lora_pack(L, case, at):
    rng = np.random.default_rng(sorted(LORA_CASES).index(case))
    gds, bufs, end, args = lora_setup(L, case, at, rng)
    master = rng.standard_normal(end + 7, dtype=np.float32)
    Mst = G(L, master)
    assert L.load_lab().tst_k_lora_pack(*args, Mst.ptr, 1 if at == "f32" else 0) == 0
    same_bits(Mst.get(), master, "master after the pack")
    rnd = O.to_bf16_bits if at == "bf16" else (lambda x: x)
    for i, (gd, gb) in enumerate(zip(gds, bufs)):
        ref = O.lora_pack_ref(gd, master)
        shapes = [(gd["RP"], gd["din"]), (gd["din"], gd["RP"]), (gd["dout"], gd["RP"]), (gd["RP"], gd["dout"])]
        for name, buf, r, shp in zip(("Ag", "AgT", "Bg", "BgT"), gb, ref, shapes):
            same_bits(buf.get(shp), rnd(r), f"{case} {at} group {i} {name}")
        gb[4].get(), gb[5].get()


@pytest.mark.parametrize("at", ["bf16", "f32"])
@pytest.mark.parametrize("case", list(LORA_CASES))
def test_lora_unpack_grad(L, case, at):
    """dAg / dBg random everywhere, also in the blocks unpack must not read (rows >= nseg r of dAg; other modules' column blocks, rows of no module and padding
    columns of dBg); grad pre-filled with the sentinel: every logical element equals its source, everything else keeps the sentinel"""
    rng = np.random.default_rng(100 + sorted(LORA_CASES).index(case))
    gds, bufs, end, args = lora_setup(L, case, at, rng)
    Gd = G(L, sentinel(end + 7))
    assert L.load_lab().tst_k_lora_unpack_grad(*args, Gd.ptr, 1 if at == "f32" else 0) == 0
    want = sentinel(end + 7)
    for gd, gb in zip(gds, bufs):
        O.lora_unpack_ref(gd, gb[4].get((gd["RP"], gd["din"])), gb[5].get((gd["dout"], gd["RP"])), want)
        for b in gb[:4]:
            b.get()
    got = Gd.get()
    same_bits(got, want, f"{case} {at} grad")
    assert (bits(got[:args[4][0]]) == SENT[4]).all() and (bits(got[end:]) == SENT[4]).all()


def test_lora_hooks_refuse_what_the_kernels_cannot_take(L):
    rng = np.random.default_rng(0)
    gds, bufs, end, args = lora_setup(L, "a_qkv_r16", "bf16", rng)
    Mst = G(L, rng.standard_normal(end + 7, dtype=np.float32))
    lab = L.load_lab()
    assert lab.tst_k_lora_pack(0, *args[1:], Mst.ptr, 0) == EINVAL
    bad = (C.c_int32 * 5)(96, 256, 16, 3, 1)   # din not a multiple of the 64-wide tile
    assert lab.tst_k_lora_pack(1, bad, *args[2:], Mst.ptr, 0) == EINVAL
    assert lab.tst_k_lora_pack(*args, None, 0) == EINVAL
