"""fp8 (e4m3) weight-only linear layers against the fp16 GEMMs (FFMI_MODEL_W8).

GEMMs: time per call of ffmi_linear_w8 and of ffmi_linear_ws (the fp16 path, in
the form the model calls it: packed activation tiles in, FFMI_W_STREAM) at the
LLaMA-7B shapes of SURVEY.md section 8 a1 -- qkv, o, gate/up with the fused
SiLU-mul, down, lm_head -- at T = 8 and T = 32, and at T = 168 to record what
the fp8 kernel's one-pass-per-64-rows costs.  Every call of a leg reads the
next of several weight copies (together > 768 MB, three Infinity Caches), as a
model's step reads each weight cold.  The two legs alternate within each
round; a leg's figure is the median of its rounds with the spread (max - min)
/ median; a timed block is as many calls as fill --window-ms at the warm-up
rate, at least 20.  Weights are random finite values (fp16) / bytes (e4m3).

Serving: incremental-decoding tokens/s of the bench's LLaMA-7B workload (8
requests, 128 prompt + 128 decoded tokens, synthetic weights) with
weight_dtype "fp16" and "fp8", alternating, after a warm-up generate each.
--layers n shortens the model (rehearsals); --serve 0 skips this part.

    python scripts/linear_w8_bench.py [--out profiles/linear_w8_bench.json]

--mid: the M-split fp8 kernel (65 .. 256 rows in one weight pass) instead.  The
same five shapes at T = 72, 128, 168, 256, same method, three legs: "onepass"
(ffmi_linear_w8 with ffmi_linear_w8_onepass_workspace_bytes), "multipass" (the
same call under FFMI_W8_MULTIPASS=1: one skinny pass per 64 rows) and "fp16".
The switch is read once per process, so the legs run in two worker processes
(one with the switch set) that hold their own weight copies and time blocks of
calls when the parent tells them to, in turn within each round.  No serving
part: SpecInfer would need a third and fourth model-holding process.

    python scripts/linear_w8_bench.py --mid [--out profiles/linear_w8_mid_bench.json]

--a8: W8A8 (fp8 activations with per-token scales on the fp8 matrix
instruction).  The same five shapes, cold-weight protocol and method at T = 8
and 168, three legs alternating in one process: "a8" (ffmi_linear_w8a8; for
o_proj and down, whose input no norm produces, the ffmi_quantize_rows_fp8 launch
ahead of it is inside the timed call), "w8a16" (ffmi_linear_w8 with its one-pass
workspace: the M-split kernel at T = 168, as --mid's "onepass") and "fp16".
Then the quantising norm against the plain one (ffmi_rmsnorm_fp8 /
ffmi_rmsnorm, H = 4096), and the serving part with weight_dtype "fp8" against
"fp8" + activation_dtype "fp8".

    python scripts/linear_w8_bench.py --a8 [--out profiles/linear_w8a8_bench.json]

--w4: OCP MXFP4 weights (ffmi_linear_w4).  The same five shapes, cold-weight
protocol and method at T = 8, 32 and 168, three legs alternating in one
process: "mxfp4" (with its one-pass workspace: the M-split kernel at T = 168;
profiles/linear_w4_bench.json predates that kernel and holds three passes of 64
rows there; each weight copy has its own scale bytes), "fp8" (ffmi_linear_w8 with its one-pass workspace) and
"fp16".  Then the serving part with weight_dtype "fp16", "fp8" and "mxfp4".

    python scripts/linear_w8_bench.py --w4 [--out profiles/linear_w4_bench.json]

--w4 --mid: the M-split MXFP4 kernel, as --mid: T = 72, 128, 168, 256, two worker
processes, four legs: "onepass" (ffmi_linear_w4 with
ffmi_linear_w4_onepass_workspace_bytes), "multipass" (the same call under
FFMI_W4_MULTIPASS=1), "fp8" (ffmi_linear_w8, one-pass) and "fp16".

    python scripts/linear_w8_bench.py --w4 --mid [--out profiles/linear_w4_mid_bench.json]

--w4 --a8: W4A8 (MXFP4 weights against fp8 rows on the block-scaled matrix
instruction).  The five shapes, cold-weight protocol and method at T = 8, 32,
168 and 256, four legs alternating in one process: "w4a8" (ffmi_linear_w4a8; for
o_proj and down the ffmi_quantize_rows_fp8 launch ahead of it is inside the
timed call), "w4a16" (ffmi_linear_w4 with its one-pass workspace: the skinny
kernel up to 64 rows, the M-split one above), "w8a8" (ffmi_linear_w8a8, with
the same quantise launch) and "fp16".  Then the serving part with weight_dtype
"mxfp4" against "mxfp4" + activation_dtype "fp8".

    python scripts/linear_w8_bench.py --w4 --a8 [--out profiles/linear_w4a8_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flexflow_amd as fa  # noqa: E402
import flexflow_amd.ffmi as F  # noqa: E402
from bench import LLAMA_7B, make_prompts  # noqa: E402
from hip_util import Buf, Timer, f16, hip  # noqa: E402

H, FF, V = LLAMA_7B["hidden"], LLAMA_7B["intermediate"], LLAMA_7B["vocab_size"]
SHAPES = [("qkv", 3 * H, H, F.EPI_NONE), ("o_proj", H, H, F.EPI_NONE),
          ("gate_up_silu", FF, H, F.EPI_SILU_MUL), ("down", H, FF, F.EPI_NONE),
          ("lm_head", V, H, F.EPI_NONE)]
COLD_BYTES = 768 << 20


def copies(nbytes, block):
    """a device buffer of n >= 2 copies of `nbytes` weight bytes, filled from block"""
    n = max(2, -(-COLD_BYTES // nbytes))
    buf = Buf.empty((n * nbytes,), np.uint8)
    for off in range(0, n * nbytes, block.nbytes):
        m = min(block.nbytes, n * nbytes - off)
        assert hip().hipMemcpy(ctypes.c_void_p(buf.ptr.value + off), block.ctypes.data, m, 1) == 0
    return buf, n


def gemm_rows(args):
    L, rng, rows = F.lib(), np.random.default_rng(0), []
    block16 = f16(rng.standard_normal(8 << 20) * 0.02)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    for name, N, K, epi in SHAPES:
        g = 2 if epi == F.EPI_SILU_MUL else 1
        b16, b8 = g * L.ffmi_linear_packed_bytes(N, K), g * L.ffmi_linear_w8_packed_bytes(N, K)
        w16, n16 = copies(b16, block16)
        w8, n8 = copies(b8, block8)
        sc = Buf(np.full(g * L.ffmi_linear_w8_scale_count(N), 2.0**-6, np.float32))
        for T in [int(t) for t in args.T.split(",")]:
            X = Buf(f16(rng.standard_normal((T, K))))
            Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K),), np.uint8)
            F.check(L.ffmi_pack_activations(X.ptr, T, K, Xp.ptr, None))
            Y = Buf.empty((T, N), np.float16)
            nws = max(L.ffmi_linear_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w8_workspace_bytes(T, N, K, epi), 16)
            ws = Buf.empty((nws,), np.uint8)
            it = {"fp8": 0, "fp16": 0}

            def calls(leg, n):
                for _ in range(n):
                    i = it[leg] = it[leg] + 1
                    if leg == "fp8":
                        F.check(L.ffmi_linear_w8(X.ptr, ctypes.c_void_p(w8.ptr.value + (i % n8) * b8),
                                                 sc.ptr, Y.ptr, T, N, K, epi | F.W_STREAM, ws.ptr, nws, None))
                    else:
                        F.check(L.ffmi_linear_ws(Xp.ptr, ctypes.c_void_p(w16.ptr.value + (i % n16) * b16),
                                                 Y.ptr, T, N, K, epi | F.X_PACKED | F.W_STREAM, ws.ptr,
                                                 nws, None))
            us, block, tm = {"fp8": [], "fp16": []}, {}, Timer()
            for leg in us:  # warm-up (code objects), then the block's size
                calls(leg, 10)
                tm.start()
                calls(leg, 20)
                block[leg] = max(20, int(args.window_ms * 20 / tm.stop()))
            for _ in range(args.rounds):
                for leg in us:
                    tm.start()
                    calls(leg, block[leg])
                    us[leg].append(tm.stop() * 1e3 / block[leg])
            row = dict(gemm=name, T=T, N=N, K=K, rounds=args.rounds, calls_per_block=block)
            for leg, nb in (("fp8", b8), ("fp16", b16)):
                a = np.array(us[leg])
                row[leg] = dict(us=round(float(np.median(a)), 2),
                                spread=round(float((a.max() - a.min()) / np.median(a)), 3),
                                weight_bytes=int(nb),
                                weight_GBps=round(nb * (-(-T // 64) if leg == "fp8" else 1) /
                                                  float(np.median(a)) / 1e3, 1))
            row["fp16_over_fp8"] = round(row["fp16"]["us"] / row["fp8"]["us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def timed_legs(args, legs):
    """legs: name -> calls(n); alternating blocks -> name -> {us, spread}, blocks"""
    us, block, tm = {leg: [] for leg in legs}, {}, Timer()
    for leg, calls in legs.items():  # warm-up (code objects), then the block's size
        calls(10)
        tm.start()
        calls(20)
        block[leg] = max(20, int(args.window_ms * 20 / tm.stop()))
    for _ in range(args.rounds):
        for leg, calls in legs.items():
            tm.start()
            calls(block[leg])
            us[leg].append(tm.stop() * 1e3 / block[leg])
    return {leg: dict(us=round(float(np.median(a)), 2),
                      spread=round(float((max(a) - min(a)) / np.median(a)), 3))
            for leg, a in us.items()}, block


def a8_rows(args):
    L, rng, rows = F.lib(), np.random.default_rng(0), []
    block16 = f16(rng.standard_normal(8 << 20) * 0.02)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    Ts = [int(t) for t in args.T.split(",")]
    for name, N, K, epi in SHAPES:
        g = 2 if epi == F.EPI_SILU_MUL else 1
        b16, b8 = g * L.ffmi_linear_packed_bytes(N, K), g * L.ffmi_linear_w8_packed_bytes(N, K)
        (w16, n16), (w8, n8) = copies(b16, block16), copies(b8, block8)
        sc = Buf(np.full(g * L.ffmi_linear_w8_scale_count(N), 2.0**-6, np.float32))
        quant = name in ("o_proj", "down")  # (the other inputs come quantised from a norm)
        for T in Ts:
            X = Buf(f16(rng.standard_normal((T, K))))
            Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K),), np.uint8)
            F.check(L.ffmi_pack_activations(X.ptr, T, K, Xp.ptr, None))
            X8, xs, Y = Buf.empty((T, K), np.uint8), Buf.empty((T,), np.float32), Buf.empty((T, N), np.float16)
            F.check(L.ffmi_quantize_rows_fp8(X.ptr, T, K, X8.ptr, xs.ptr, None))
            nws = max(L.ffmi_linear_workspace_bytes(T, N, K, epi), 16,
                      L.ffmi_linear_w8_onepass_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w8a8_workspace_bytes(T, N, K, epi))
            ws, it = Buf.empty((nws,), np.uint8), [0]

            def wt(base, n, b):
                it[0] += 1
                return ctypes.c_void_p(base.ptr.value + (it[0] % n) * b)

            def a8(n):
                for _ in range(n):
                    if quant:
                        F.check(L.ffmi_quantize_rows_fp8(X.ptr, T, K, X8.ptr, xs.ptr, None))
                    F.check(L.ffmi_linear_w8a8(X8.ptr, xs.ptr, wt(w8, n8, b8), sc.ptr, Y.ptr, T, N, K,
                                               epi | F.W_STREAM, ws.ptr, nws, None))

            def w8a16(n):
                for _ in range(n):
                    F.check(L.ffmi_linear_w8(X.ptr, wt(w8, n8, b8), sc.ptr, Y.ptr, T, N, K,
                                             epi | F.W_STREAM, ws.ptr, nws, None))

            def fp16(n):
                for _ in range(n):
                    F.check(L.ffmi_linear_ws(Xp.ptr, wt(w16, n16, b16), Y.ptr, T, N, K,
                                             epi | F.X_PACKED | F.W_STREAM, ws.ptr, nws, None))
            res, block = timed_legs(args, dict(a8=a8, w8a16=w8a16, fp16=fp16))
            row = dict(gemm=name, T=T, N=N, K=K, rounds=args.rounds, calls_per_block=block,
                       a8_includes_quantise=quant, weight_bytes=dict(fp8=int(b8), fp16=int(b16)), **res)
            row["w8a16_over_a8"] = round(res["w8a16"]["us"] / res["a8"]["us"], 3)
            row["fp16_over_a8"] = round(res["fp16"]["us"] / res["a8"]["us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    norms = []
    for T in Ts:  # the quantising norm against the plain one, residual form
        x1, x2, w = (Buf(f16(rng.standard_normal(s))) for s in ((T, H), (T, H), (H,)))
        res_o, out = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
        X8, xs = Buf.empty((T, H), np.uint8), Buf.empty((T,), np.float32)

        def plain(n):
            for _ in range(n):
                F.check(L.ffmi_residual_rmsnorm(x1.ptr, x2.ptr, w.ptr, res_o.ptr, out.ptr, T, H, 1e-6, None))

        def fused(n):
            for _ in range(n):
                F.check(L.ffmi_rmsnorm_fp8(x1.ptr, x2.ptr, w.ptr, res_o.ptr, X8.ptr, xs.ptr, T, H, 1e-6, None))

        def standalone(n):
            for _ in range(n):
                F.check(L.ffmi_quantize_rows_fp8(out.ptr, T, H, X8.ptr, xs.ptr, None))
        res, _ = timed_legs(args, dict(norm_fp16=plain, norm_fp8=fused, quantize_rows=standalone))
        norms.append(dict(T=T, H=H, **res))
        print(json.dumps(norms[-1]), flush=True)
    return rows, norms


def w4_rows(args):
    L, rng, rows = F.lib(), np.random.default_rng(0), []
    block16 = f16(rng.standard_normal(8 << 20) * 0.02)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    block4 = rng.integers(0, 256, size=16 << 20).astype(np.uint8)  # (every nibble is a value)
    for name, N, K, epi in SHAPES:
        g = 2 if epi == F.EPI_SILU_MUL else 1
        b16, b8 = g * L.ffmi_linear_packed_bytes(N, K), g * L.ffmi_linear_w8_packed_bytes(N, K)
        b4, bs4 = g * L.ffmi_linear_w4_packed_bytes(N, K), g * L.ffmi_linear_w4_scale_bytes(N, K)
        (w16, n16), (w8, n8), (w4, n4) = copies(b16, block16), copies(b8, block8), copies(b4, block4)
        sc8 = Buf(np.full(g * L.ffmi_linear_w8_scale_count(N), 2.0**-6, np.float32))
        sc4 = Buf(np.full(n4 * bs4, 127 - 6, np.uint8))  # (a copy of the scale bytes per weight copy)
        for T in [int(t) for t in args.T.split(",")]:
            X = Buf(f16(rng.standard_normal((T, K))))
            Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K),), np.uint8)
            F.check(L.ffmi_pack_activations(X.ptr, T, K, Xp.ptr, None))
            Y = Buf.empty((T, N), np.float16)
            nws = max(L.ffmi_linear_workspace_bytes(T, N, K, epi), 16,
                      L.ffmi_linear_w8_onepass_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, epi))
            ws, it = Buf.empty((nws,), np.uint8), [0]

            def wt(base, n, b):
                return ctypes.c_void_p(base.ptr.value + (it[0] % n) * b)

            def mxfp4(n):
                for _ in range(n):
                    it[0] += 1
                    F.check(L.ffmi_linear_w4(X.ptr, wt(w4, n4, b4), wt(sc4, n4, bs4), Y.ptr, T, N, K,
                                             epi | F.W_STREAM, ws.ptr, nws, None))

            def fp8(n):
                for _ in range(n):
                    it[0] += 1
                    F.check(L.ffmi_linear_w8(X.ptr, wt(w8, n8, b8), sc8.ptr, Y.ptr, T, N, K,
                                             epi | F.W_STREAM, ws.ptr, nws, None))

            def fp16(n):
                for _ in range(n):
                    it[0] += 1
                    F.check(L.ffmi_linear_ws(Xp.ptr, wt(w16, n16, b16), Y.ptr, T, N, K,
                                             epi | F.X_PACKED | F.W_STREAM, ws.ptr, nws, None))
            res, block = timed_legs(args, dict(mxfp4=mxfp4, fp8=fp8, fp16=fp16))
            row = dict(gemm=name, T=T, N=N, K=K, rounds=args.rounds, calls_per_block=block,
                       weight_bytes=dict(mxfp4=int(b4 + bs4), fp8=int(b8), fp16=int(b16)), **res)
            row["fp8_over_mxfp4"] = round(res["fp8"]["us"] / res["mxfp4"]["us"], 3)
            row["fp16_over_mxfp4"] = round(res["fp16"]["us"] / res["mxfp4"]["us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def w4a8_rows(args):
    L, rng, rows = F.lib(), np.random.default_rng(0), []
    block16 = f16(rng.standard_normal(8 << 20) * 0.02)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    block4 = rng.integers(0, 256, size=16 << 20).astype(np.uint8)  # (every nibble is a value)
    for name, N, K, epi in SHAPES:
        g = 2 if epi == F.EPI_SILU_MUL else 1
        b16, b8 = g * L.ffmi_linear_packed_bytes(N, K), g * L.ffmi_linear_w8_packed_bytes(N, K)
        b4, bs4 = g * L.ffmi_linear_w4_packed_bytes(N, K), g * L.ffmi_linear_w4_scale_bytes(N, K)
        (w16, n16), (w8, n8), (w4, n4) = copies(b16, block16), copies(b8, block8), copies(b4, block4)
        sc8 = Buf(np.full(g * L.ffmi_linear_w8_scale_count(N), 2.0**-6, np.float32))
        sc4 = Buf(np.full(n4 * bs4, 127 - 6, np.uint8))  # (a copy of the scale bytes per weight copy)
        quant = name in ("o_proj", "down")  # (the other inputs come quantised from a norm)
        for T in [int(t) for t in args.T.split(",")]:
            X = Buf(f16(rng.standard_normal((T, K))))
            Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K),), np.uint8)
            F.check(L.ffmi_pack_activations(X.ptr, T, K, Xp.ptr, None))
            X8, xs, Y = Buf.empty((T, K), np.uint8), Buf.empty((T,), np.float32), Buf.empty((T, N), np.float16)
            F.check(L.ffmi_quantize_rows_fp8(X.ptr, T, K, X8.ptr, xs.ptr, None))
            nws = max(L.ffmi_linear_workspace_bytes(T, N, K, epi), 16,
                      L.ffmi_linear_w8a8_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w4a8_workspace_bytes(T, N, K, epi))
            ws, it = Buf.empty((nws,), np.uint8), [0]

            def wt(base, n, b):
                return ctypes.c_void_p(base.ptr.value + (it[0] % n) * b)

            def a8(n, w4_leg):
                for _ in range(n):
                    it[0] += 1
                    if quant:
                        F.check(L.ffmi_quantize_rows_fp8(X.ptr, T, K, X8.ptr, xs.ptr, None))
                    if w4_leg:
                        F.check(L.ffmi_linear_w4a8(X8.ptr, xs.ptr, wt(w4, n4, b4), wt(sc4, n4, bs4), Y.ptr,
                                                   T, N, K, epi | F.W_STREAM, ws.ptr, nws, None))
                    else:
                        F.check(L.ffmi_linear_w8a8(X8.ptr, xs.ptr, wt(w8, n8, b8), sc8.ptr, Y.ptr, T, N, K,
                                                   epi | F.W_STREAM, ws.ptr, nws, None))

            def w4a16(n):
                for _ in range(n):
                    it[0] += 1
                    F.check(L.ffmi_linear_w4(X.ptr, wt(w4, n4, b4), wt(sc4, n4, bs4), Y.ptr, T, N, K,
                                             epi | F.W_STREAM, ws.ptr, nws, None))

            def fp16(n):
                for _ in range(n):
                    it[0] += 1
                    F.check(L.ffmi_linear_ws(Xp.ptr, wt(w16, n16, b16), Y.ptr, T, N, K,
                                             epi | F.X_PACKED | F.W_STREAM, ws.ptr, nws, None))
            res, block = timed_legs(args, dict(w4a8=lambda n: a8(n, True), w4a16=w4a16,
                                               w8a8=lambda n: a8(n, False), fp16=fp16))
            row = dict(gemm=name, T=T, N=N, K=K, rounds=args.rounds, calls_per_block=block,
                       a8_includes_quantise=quant,
                       weight_bytes=dict(mxfp4=int(b4 + bs4), fp8=int(b8), fp16=int(b16)), **res)
            for leg in ("w4a16", "w8a8", "fp16"):
                row[leg + "_over_w4a8"] = round(res[leg]["us"] / res["w4a8"]["us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def mid_worker(w4):
    """stdin: one JSON command per line -- {"shape": i} (weight copies of SHAPES[i]),
    {"T": t} (activations, output, workspace), {"leg": l, "n": n} (n calls); stdout:
    one JSON reply per command, a timed block's milliseconds for the last."""
    fa.set_device(0)
    L, rng, tm = F.lib(), np.random.default_rng(0), Timer()
    block16 = f16(rng.standard_normal(8 << 20) * 0.02)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    block4 = rng.integers(0, 256, size=16 << 20).astype(np.uint8)  # (every nibble is a value)
    # (the multi-pass worker runs its one leg only: no fp16 copies, and under --w4 no fp8 ones)
    first = os.environ.get("FFMI_W4_MULTIPASS" if w4 else "FFMI_W8_MULTIPASS", "0") == "0"
    st, it = {}, 0
    for line in sys.stdin:
        cmd, out = json.loads(line), {}
        if "shape" in cmd:
            st.clear()  # (frees the last shape's copies first)
            name, N, K, epi = SHAPES[cmd["shape"]]
            g = 2 if epi == F.EPI_SILU_MUL else 1
            b16, b8 = g * L.ffmi_linear_packed_bytes(N, K), g * L.ffmi_linear_w8_packed_bytes(N, K)
            st.update(N=N, K=K, epi=epi, b16=b16, b8=b8,
                      w8=copies(b8, block8) if first or not w4 else None,
                      w16=copies(b16, block16) if first else None,
                      sc=Buf(np.full(g * L.ffmi_linear_w8_scale_count(N), 2.0**-6, np.float32)))
            out = dict(weight_bytes=dict(fp8=int(b8), fp16=int(b16)))
            if w4:
                b4, bs4 = g * L.ffmi_linear_w4_packed_bytes(N, K), g * L.ffmi_linear_w4_scale_bytes(N, K)
                st.update(b4=b4, bs4=bs4, w4=copies(b4, block4))
                st["sc4"] = Buf(np.full(st["w4"][1] * bs4, 127 - 6, np.uint8))  # (scale bytes per copy)
                out["weight_bytes"]["mxfp4"] = int(b4 + bs4)
        elif "T" in cmd:
            T, N, K, epi = cmd["T"], st["N"], st["K"], st["epi"]
            X = Buf(f16(rng.standard_normal((T, K))))
            Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K),), np.uint8)
            F.check(L.ffmi_pack_activations(X.ptr, T, K, Xp.ptr, None))
            nws = max(L.ffmi_linear_workspace_bytes(T, N, K, epi),
                      L.ffmi_linear_w8_onepass_workspace_bytes(T, N, K, epi), 16)
            plan = (ctypes.c_int * 6)()
            if w4:
                nws = max(nws, L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, epi))
                F.check(L.ffmi_debug_linear_w4_plan(T, N, K, epi, nws, plan))
            else:
                F.check(L.ffmi_debug_linear_w8_plan(T, N, K, epi, nws, plan))
            st.update(T=T, X=X, Xp=Xp, Y=Buf.empty((T, N), np.float16), nws=nws,
                      ws=Buf.empty((nws,), np.uint8))
            out = dict(plan=list(plan))
        else:
            T, N, K, epi, ws, nws = (st[k] for k in ("T", "N", "K", "epi", "ws", "nws"))
            tm.start()
            for _ in range(cmd["n"]):
                it += 1
                if cmd["leg"] == "fp16":
                    (w, n), b = st["w16"], st["b16"]
                    F.check(L.ffmi_linear_ws(st["Xp"].ptr, ctypes.c_void_p(w.ptr.value + (it % n) * b),
                                             st["Y"].ptr, T, N, K, epi | F.X_PACKED | F.W_STREAM,
                                             ws.ptr, nws, None))
                elif w4 and cmd["leg"] != "fp8":
                    (w, n), b, bs = st["w4"], st["b4"], st["bs4"]
                    F.check(L.ffmi_linear_w4(st["X"].ptr, ctypes.c_void_p(w.ptr.value + (it % n) * b),
                                             ctypes.c_void_p(st["sc4"].ptr.value + (it % n) * bs),
                                             st["Y"].ptr, T, N, K, epi | F.W_STREAM, ws.ptr, nws, None))
                else:
                    (w, n), b = st["w8"], st["b8"]
                    F.check(L.ffmi_linear_w8(st["X"].ptr, ctypes.c_void_p(w.ptr.value + (it % n) * b),
                                             st["sc"].ptr, st["Y"].ptr, T, N, K, epi | F.W_STREAM,
                                             ws.ptr, nws, None))
            out = dict(ms=tm.stop())
        print(json.dumps(out), flush=True)


def mid_rows(args):
    def worker(multipass):
        env = dict(os.environ)
        env["FFMI_W4_MULTIPASS" if args.w4 else "FFMI_W8_MULTIPASS"] = "1" if multipass else "0"
        return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--mid-worker"] +
                                ["--w4"] * args.w4, env=env,
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(w, **cmd):
        w.stdin.write(json.dumps(cmd) + "\n")
        w.stdin.flush()
        line = w.stdout.readline()
        if not line:
            raise RuntimeError(f"worker exited with {w.wait()}")
        return json.loads(line)
    one, multi = worker(False), worker(True)
    legs = {"onepass": one, "multipass": multi, **({"fp8": one} if args.w4 else {}), "fp16": one}
    rows = []
    try:
        for i, (name, N, K, _) in enumerate(SHAPES):
            nb = ask(one, shape=i)["weight_bytes"]
            ask(multi, shape=i)
            for T in [int(t) for t in args.T.split(",")]:
                plans = {"onepass": ask(one, T=T)["plan"], "multipass": ask(multi, T=T)["plan"]}
                assert plans["onepass"][0] == 1 and plans["multipass"][0] == 0, plans
                us, block = {leg: [] for leg in legs}, {}
                for leg, w in legs.items():  # warm-up (code objects), then the block's size
                    ask(w, leg=leg, n=10)
                    block[leg] = max(20, int(args.window_ms * 20 / ask(w, leg=leg, n=20)["ms"]))
                for _ in range(args.rounds):
                    for leg, w in legs.items():
                        us[leg].append(ask(w, leg=leg, n=block[leg])["ms"] * 1e3 / block[leg])
                row = dict(gemm=name, T=T, N=N, K=K, rounds=args.rounds, calls_per_block=block,
                           plan=plans, weight_bytes=nb)
                for leg in legs:
                    a = np.array(us[leg])
                    row[leg] = dict(us=round(float(np.median(a)), 2),
                                    spread=round(float((a.max() - a.min()) / np.median(a)), 3))
                row["multipass_over_onepass"] = round(row["multipass"]["us"] / row["onepass"]["us"], 3)
                row["fp16_over_onepass"] = round(row["fp16"]["us"] / row["onepass"]["us"], 3)
                if args.w4:
                    row["fp8_over_onepass"] = round(row["fp8"]["us"] / row["onepass"]["us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        for w in (one, multi):
            w.stdin.close()
            w.wait()
    return rows


def serve(args):
    B, P, D = 8, 128, 128
    cfg = dict(LLAMA_7B)
    if args.layers:
        cfg["num_layers"] = args.layers
    rm_kw = dict(max_requests_per_batch=B, max_tokens_per_batch=1024, max_sequence_length=512)
    prompts = make_prompts(B, P - 1, cfg["vocab_size"])
    kinds = {"mxfp4": dict(weight_dtype="mxfp4"),
             "mxfp4_a8": dict(weight_dtype="mxfp4", activation_dtype="fp8")} if args.a8 and args.w4 else \
        {"fp8": dict(weight_dtype="fp8"), "fp8_a8": dict(weight_dtype="fp8", activation_dtype="fp8")} \
        if args.a8 else {d: dict(weight_dtype=d) for d in ("fp16", "fp8") + (("mxfp4",) if args.w4 else ())}
    models = {d: fa.Model(cfg, "inc", max_requests=B, max_tokens=1024, max_seq_len=512,
                          weight_seed=20250117, **kw) for d, kw in kinds.items()}

    def generates(m, n):
        new, t0 = 0, time.time()
        for _ in range(n):
            res = fa.generate(fa.RequestManager(**rm_kw), m, prompts, max_length=P + D)
            new += sum(len(r.output_tokens) - len(r.input_tokens) for r in res)
        return new / (time.time() - t0)
    for m in models.values():
        generates(m, 1)  # (graph capture of every shape)
    rates = {d: [] for d in models}
    for _ in range(args.rounds):
        for d, m in models.items():
            rates[d].append(round(generates(m, args.generates), 1))
    med = {d: sorted(v)[len(v) // 2] for d, v in rates.items()}
    out = dict(workload=f"llama7b_incr B={B} P={P} D={D} layers={cfg['num_layers']}",
               generates_per_window=args.generates, tokens_per_s=rates, median=med,
               **({"mxfp4_a8_over_mxfp4": round(med["mxfp4_a8"] / med["mxfp4"], 4)} if args.a8 and args.w4 else
                  {"fp8_a8_over_fp8": round(med["fp8_a8"] / med["fp8"], 4)} if args.a8 else
                  {"fp8_over_fp16": round(med["fp8"] / med["fp16"], 4)}),
               **({"mxfp4_over_fp16": round(med["mxfp4"] / med["fp16"], 4),
                   "mxfp4_over_fp8": round(med["mxfp4"] / med["fp8"], 4)} if args.w4 and not args.a8 else {}),
               weight_bytes={d: m.weight_bytes() for d, m in models.items()})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", action="store_true", help="the M-split kernel's three legs")
    ap.add_argument("--a8", action="store_true", help="the W8A8 legs")
    ap.add_argument("--w4", action="store_true", help="the MXFP4 legs")
    ap.add_argument("--mid-worker", action="store_true", help="(a --mid run's child process)")
    ap.add_argument("--T", default=None, help="default 8,32,168; --mid: 72,128,168,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="length of a timed block")
    ap.add_argument("--serve", type=int, default=1)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--generates", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_w8_bench.json"))
    args = ap.parse_args()
    if args.mid_worker:
        return mid_worker(args.w4)
    args.T = args.T or ("8,32,168,256" if args.a8 and args.w4 else "8,168" if args.a8 else "72,128,168,256" if args.mid else "8,32,168")
    if args.w4 and args.mid:
        res = dict(bench="linear_w4_mid_bench", gemms=mid_rows(args))
        out = args.out.replace("linear_w8_bench.json", "linear_w4_mid_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.a8 and args.w4:
        fa.set_device(0)
        res = dict(bench="linear_w4a8_bench", gemms=w4a8_rows(args))
        if args.serve:
            res["serving"] = serve(args)
        out = args.out.replace("linear_w8_bench.json", "linear_w4a8_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.a8:
        fa.set_device(0)
        gemms, norms = a8_rows(args)
        res = dict(bench="linear_w8a8_bench", gemms=gemms, norms=norms)
        if args.serve:
            res["serving"] = serve(args)
        out = args.out.replace("linear_w8_bench.json", "linear_w8a8_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.w4:
        fa.set_device(0)
        res = dict(bench="linear_w4_bench", gemms=w4_rows(args))
        if args.serve:
            res["serving"] = serve(args)
        out = args.out.replace("linear_w8_bench.json", "linear_w4_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    if args.mid:
        res = dict(bench="linear_w8_mid_bench", gemms=mid_rows(args))
        out = args.out.replace("linear_w8_bench.json", "linear_w8_mid_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    fa.set_device(0)
    res = dict(bench="linear_w8_bench", gemms=gemm_rows(args))
    if args.serve:
        res["serving"] = serve(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
