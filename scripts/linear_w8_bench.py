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
"""
import argparse
import ctypes
import json
import os
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


def serve(args):
    B, P, D = 8, 128, 128
    cfg = dict(LLAMA_7B)
    if args.layers:
        cfg["num_layers"] = args.layers
    rm_kw = dict(max_requests_per_batch=B, max_tokens_per_batch=1024, max_sequence_length=512)
    prompts = make_prompts(B, P - 1, cfg["vocab_size"])
    models = {d: fa.Model(cfg, "inc", max_requests=B, max_tokens=1024, max_seq_len=512,
                          weight_seed=20250117, weight_dtype=d) for d in ("fp16", "fp8")}

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
               fp8_over_fp16=round(med["fp8"] / med["fp16"], 4),
               weight_bytes={d: m.weight_bytes() for d, m in models.items()})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", default="8,32,168")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="length of a timed block")
    ap.add_argument("--serve", type=int, default=1)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--generates", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_w8_bench.json"))
    args = ap.parse_args()
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
