#!/usr/bin/env python3
"""HBM-bound kernels alone on the benchmark's stacked micro-batch shape (T = 3555 tokens, d = 4096, F = 14336), for rocprofv3:
    rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/ew_prof -- python3 tools/ew_bench.py
(algorithmic bytes per launch are printed; divide by the CSV's average duration)

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/ew_bench.py --head-norm PLAN.json
    python3 tools/ew_bench.py --head-norm-report DIR PLAN.json [out.txt]
the Qwen3 head-norm kernels (csrc/head_norm.hip) instead, at T = 3555 and 1185, H = 32, Hkv = 8, next to the stand-alone rope kernel over the same q|k columns
in the same run. The first command launches the forms interleaved over 6 rounds of 40 calls (the first round is warm-up) and writes the launch plan; the second
reads the kernel trace, walks its head-norm / rope dispatches in start order along the plan and prints, per form, the median (min, max) KERNEL time per call
-- the sum of its kernels' durations for the forms of two launches -- and the achieved GB/s of the algorithmic bytes. Every call works on the next of a ring of
buffer sets larger than the 256 MiB Infinity Cache, so the rates are HBM rates. In-place kernels are re-applied to their own output, so the data has unit RMS
and unit norm weights: every pass maps O(1) values to O(1) values."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "test-set-training_amd"))
from tst import lib  # noqa: E402

HN_ROUNDS, HN_CALLS = 6, 40   # round 0 is warm-up


def head_norm_bench(plan_path):
    L = lib.load_lab()
    H, Hkv, dh, P = 32, 8, 128, 128
    ld, nqk = (H + 2 * Hkv) * dh, (H + Hkv) * dh
    rng = np.random.default_rng(0)
    ang = np.arange(P, dtype=np.float32)[:, None] * (1.0 / (1000000.0 ** (np.arange(0, dh, 2, dtype=np.float32) / dh)))[None, :]
    bf = lambda a: lib.from_bf16_bits(lib.to_bf16_bits(a))
    cosT, sinT = lib.dev_f32(bf(np.cos(ang))), lib.dev_f32(bf(np.sin(ang)))
    ones = lib.dev_bf16(np.ones(dh, np.float32))
    ws = lib.DevBuf(nbytes=lib.HEAD_NORM_WS_FLOATS * 4)
    plan = []
    for T in (3555, 1185):
        nbuf = int(400e6 // (T * ld * 2)) + 1          # ring of buffer sets: > 256 MiB of qkv alone
        host = rng.standard_normal((T, ld)).astype(np.float32)
        sets = [dict(qkv=lib.dev_bf16(host), dqkv=lib.dev_bf16(host[::-1]), stash=lib.dev_bf16(host[:, :nqk])) for _ in range(nbuf)]
        rstd = lib.dev_f32(np.ones((T, H + Hkv), np.float32))
        pos = lib.DevBuf((np.arange(T) % 74).astype(np.int32))
        dwq, dwk = lib.dev_f32(np.zeros(dh, np.float32)), lib.dev_f32(np.zeros(dh, np.float32))
        qk = 2.0 * T * nqk   # bytes of one pass over the bf16 q|k columns
        fwd = lambda b, st, rope: L.tst_k_head_norm_fwd(b["qkv"].ptr, ld, ones.ptr, ones.ptr, rstd.ptr, b["stash"].ptr if st else None, T, H, Hkv, 1e-6,
                                                        pos.ptr if rope else None, cosT.ptr if rope else None, sinT.ptr if rope else None)
        bwd = lambda b, rope, dw=False: L.tst_k_head_norm_bwd(b["dqkv"].ptr, ld, ones.ptr, ones.ptr, rstd.ptr, b["stash"].ptr, T, H, Hkv, pos.ptr if rope else None,
                                                              cosT.ptr if rope else None, sinT.ptr if rope else None, dwq.ptr if dw else None,
                                                              dwk.ptr if dw else None, ws.ptr if dw else None)
        rope = lambda buf, back: L.tst_k_rope(buf.ptr, pos.ptr, cosT.ptr, sinT.ptr, T, H + Hkv, dh, ld, back)
        # (name, algorithmic bytes, kernel-name fragments of one call in launch order, call)
        forms = [("rope_kernel fwd (yardstick)", 2 * qk, ["rope_kernel"], lambda b: rope(b["qkv"], 0)),
                 ("head_norm fwd, no stash", 2 * qk, ["head_norm_fwd"], lambda b: fwd(b, False, False)),
                 ("head_norm fwd, stash", 3 * qk, ["head_norm_fwd"], lambda b: fwd(b, True, False)),
                 ("head_norm bwd", 3 * qk, ["head_norm_bwd"], lambda b: bwd(b, False)),
                 ("head_norm bwd + dw (bwd, finish)", 3 * qk, ["head_norm_bwd", "head_norm_dw_finish"], lambda b: bwd(b, False, True)),
                 ("head_norm+rope fwd, stash (one pass)", 3 * qk, ["head_norm_fwd"], lambda b: fwd(b, True, True)),
                 ("head_norm fwd, stash; rope (two passes)", 5 * qk, ["head_norm_fwd", "rope_kernel"], lambda b: fwd(b, True, False) or rope(b["qkv"], 0)),
                 ("head_norm+rope bwd (one pass)", 3 * qk, ["head_norm_bwd"], lambda b: bwd(b, True)),
                 ("head_norm+rope bwd + dw (bwd, finish)", 3 * qk, ["head_norm_bwd", "head_norm_dw_finish"], lambda b: bwd(b, True, True)),
                 ("rope bwd; head_norm bwd (two passes)", 5 * qk, ["rope_kernel", "head_norm_bwd"], lambda b: rope(b["dqkv"], 1) or bwd(b, False))]
        n = 0
        for rnd in range(HN_ROUNDS):
            for name, nbytes, kernels, fn in forms:
                for _ in range(HN_CALLS):
                    assert fn(sets[n % nbuf]) == 0
                    n += 1
                plan.append(dict(T=T, form=name, bytes=nbytes, kernels=kernels, calls=HN_CALLS, timed=rnd > 0))
            assert L.tst_dev_sync() == 0
    with open(plan_path, "w") as f:
        json.dump(plan, f)
    print(f"head-norm plan: {len(plan)} entries -> {plan_path}")


def head_norm_report(trace_dir, plan_path, out_path=None):
    import csv
    import glob
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    marks = ("head_norm_fwd", "head_norm_bwd", "head_norm_dw_finish", "rope_kernel")
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])) if any(m in r["Kernel_Name"] for m in marks)]
    rows.sort()
    plan = json.load(open(plan_path))
    assert len(rows) == sum(e["calls"] * len(e["kernels"]) for e in plan), (len(rows), "dispatches in the trace do not match the plan")
    at, times, order = 0, {}, []
    for e in plan:
        key = (e["T"], e["form"], e["bytes"])
        if key not in times:
            times[key] = []
            order.append(key)
        for _ in range(e["calls"]):
            dur = 0
            for frag in e["kernels"]:
                s, t, name = rows[at]
                assert frag in name, (frag, name, at)
                dur += t - s
                at += 1
            if e["timed"]:
                times[key].append(dur / 1e3)
    lines = []
    for key in order:
        T, form, nbytes = key
        t = np.array(times[key])
        lines.append(f"T={T:5d} {form:42s} {np.median(t):7.2f} us (min {t.min():7.2f} max {t.max():7.2f}; {len(t)} calls)  {nbytes / np.median(t) / 1e3:7.1f} GB/s  [{nbytes / 1e6:.1f} MB]")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if "--head-norm" in sys.argv:
    head_norm_bench(sys.argv[sys.argv.index("--head-norm") + 1])
    sys.exit(0)
if "--head-norm-report" in sys.argv:
    i = sys.argv.index("--head-norm-report")
    head_norm_report(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3] if len(sys.argv) > i + 3 else None)
    sys.exit(0)

L = lib.load_lab()
T, d, F = 3555, 4096, 14336
rng = np.random.default_rng(0)
x = lib.dev_bf16(rng.standard_normal((T, d)).astype(np.float32))
dy = lib.dev_bf16(rng.standard_normal((T, d)).astype(np.float32))
dres = lib.dev_bf16(rng.standard_normal((T, d)).astype(np.float32))
w = lib.dev_bf16((1 + 0.1 * rng.standard_normal(d)).astype(np.float32))
y, dx = lib.DevBuf(nbytes=T * d * 2), lib.DevBuf(nbytes=T * d * 2)
rstd = lib.DevBuf(nbytes=T * 4)
gu = lib.dev_bf16(rng.standard_normal((T, 2 * F)).astype(np.float32))
dact = lib.dev_bf16(rng.standard_normal((T, F)).astype(np.float32))
act, dgu = lib.DevBuf(nbytes=T * F * 2), lib.DevBuf(nbytes=T * 2 * F * 2)
H, Hkv, dh = 32, 8, 128
ld = (H + 2 * Hkv) * dh
qkv = lib.dev_bf16(rng.standard_normal((T, ld)).astype(np.float32))
pos = lib.DevBuf(np.concatenate([np.arange(n) for n in ([74] * 48 + [3])])[:T].astype(np.int32))
ang = np.arange(128, dtype=np.float32)[:, None] * (1.0 / (500000.0 ** (np.arange(0, dh, 2, dtype=np.float32) / dh)))[None, :]
cosT, sinT = lib.dev_f32(np.cos(ang).astype(np.float32)), lib.dev_f32(np.sin(ang).astype(np.float32))
print("rope MB", 2 * T * (H + Hkv) * dh * 2 / 1e6)
print("rmsnorm_fwd MB", 2 * T * d * 2 / 1e6, "rmsnorm_bwd MB", 4 * T * d * 2 / 1e6, "swiglu_fwd MB", 3 * T * F * 2 / 1e6, "swiglu_bwd MB", 5 * T * F * 2 / 1e6)
Ag = lib.dev_bf16((rng.standard_normal((192, d)) * 0.05).astype(np.float32))
us = lib.DevBuf(nbytes=T * 192 * 2)
import ctypes as C
ends = (C.c_int32 * 8)(1190, 2371, 3555, 3555, 3555, 3555, 3555, 3555)
for _ in range(30):
    assert L.tst_k_rmsnorm_fwd(x.ptr, w.ptr, y.ptr, rstd.ptr, T, d, 1e-5) == 0
    assert L.tst_k_rmsnorm_rank_fwd(x.ptr, w.ptr, y.ptr, rstd.ptr, T, d, 1e-5, Ag.ptr, d, us.ptr, 192, 2.0, 48, 3, ends) == 0     # + us of the q|k|v group (three slots)
    assert L.tst_k_rmsnorm_rank_fwd(x.ptr, w.ptr, y.ptr, rstd.ptr, T, d, 1e-5, Ag.ptr, d, us.ptr, 128, 2.0, 32, 3, ends) == 0     # + us of the gate|up group
    assert L.tst_k_rmsnorm_bwd(dy.ptr, x.ptr, rstd.ptr, w.ptr, dres.ptr, dx.ptr, T, d) == 0
    assert L.tst_k_swiglu_fwd(gu.ptr, act.ptr, T, F) == 0
    assert L.tst_k_swiglu_bwd(dact.ptr, gu.ptr, dgu.ptr, T, F) == 0
    assert L.tst_k_rope(qkv.ptr, pos.ptr, cosT.ptr, sinT.ptr, T, H + Hkv, dh, ld, 0) == 0
