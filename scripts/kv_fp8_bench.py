"""The attention step of a decode batch over an 8-bit and an fp16 KV cache.

One request batch of the bench's decode shape (8 requests, 32 heads, d 128,
one token per request at position ctx), one ffmi_attn_inc call per step,
device events around blocks of steps.  Legs:
  fp8          an FFMI_ATTN_KV_FP8 handle: kv_update_fp8_kernel, then
               attention_fp8_kernel (it has no other route)
  fp16_2launch the fp16 handle under FFMI_ATTN_NO_FUSE=1: kv_update_kernel,
               then attention_kernel -- the same scheme on 2-byte elements
  fp16_fused   the fp16 handle's default: one launch, LDS tail
at ctx 256, 2048 and the handle's maximum.  The legs alternate within each
round, so drift of the device or of its other tenants lands on all of them;
a leg's figure is the median of its rounds with the spread (max - min) /
median.  A timed block is as many steps as fill --window-ms (100 ms) at the
leg's warm-up rate, at least 50.  Caches hold random data (fp16 values / random finite e4m3 bytes).
kv_bytes: the K and V^T bytes one step needs (every key of every request).

--variant NAME runs the fp16 legs of flexflow_amd/libffmi_NAME.so (a build of
the parent commit) in a child process and adds its rows as `parent`: the same
kernels before and after the change, in the same call.

    python scripts/kv_fp8_bench.py [--variant parent] [--out profiles/kv_fp8_attn_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flexflow_amd.ffmi as F  # noqa: E402

HEADS, D, R, MAX_SEQ = 32, 128, 8, 8192


def fill_random(ptr, nbytes, block):
    from hip_util import hip
    off = 0
    while off < nbytes:
        n = min(block.nbytes, nbytes - off)
        assert hip().hipMemcpy(ctypes.c_void_p(ptr.value + off), block.ctypes.data, n, 1) == 0
        off += n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", default=f"256,2048,{MAX_SEQ - 1}")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0, help="length of a timed block")
    ap.add_argument("--variant", default="", help="also time libffmi_<variant>.so's fp16 legs")
    ap.add_argument("--child", action="store_true", help="(internal) print rows, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fp8_attn_bench.json"))
    args = ap.parse_args()
    # (a library of the parent commit lacks the newer entry points)
    probe = ctypes.CDLL(F.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    F.SIGNATURES = {n: s for n, s in F.SIGNATURES.items() if hasattr(probe, n)}
    L = F.lib()
    from hip_util import Buf, Timer, f16
    has_fp8 = hasattr(probe, "ffmi_attn_create_ex")
    legs = (("fp8",) if has_fp8 else ()) + ("fp16_2launch", "fp16_fused")
    rng = np.random.default_rng(0)
    block16 = f16(rng.standard_normal(8 << 20) * 0.5)
    block8 = rng.integers(0, 127, size=16 << 20).astype(np.uint8) | \
        (rng.integers(0, 2, size=16 << 20).astype(np.uint8) << 7)  # (no NaN byte)
    cfg = F.AttnCfg(F.ATTN_INC, HEADS, D, R, MAX_SEQ, 0, 16, 1.0 / np.sqrt(D), 10000.0, 1)
    hs = {}
    for leg in ("fp8", "fp16") if has_fp8 else ("fp16",):
        h = F.attn_create_ex(cfg, HEADS, F.ATTN_KV_FP8) if leg == "fp8" else F.attn_create_gqa(cfg, HEADS)
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        F.check(L.ffmi_attn_kv_ptrs(h, ctypes.byref(k), ctypes.byref(v), None))
        half = F.attn_cache_bytes(h) // 2
        fill_random(k, half, block8 if leg == "fp8" else block16)
        fill_random(v, half, block8 if leg == "fp8" else block16)
        hs[leg] = h
    b = ctypes.c_void_p()
    F.check(L.ffmi_batch_create(16, R, ctypes.byref(b)))
    qkv = Buf(f16(rng.standard_normal((R, 3 * HEADS * D))))
    out = Buf.empty((16, HEADS * D), np.float16)

    def steps(leg, n):
        # (attn_forward reads FFMI_ATTN_NO_FUSE with getenv on EVERY call, which is
        # what lets one process switch the fp16 handle between its two routes; a
        # library that cached the read would silently merge the two fp16 legs)
        if leg == "fp16_2launch":
            os.environ["FFMI_ATTN_NO_FUSE"] = "1"
        else:
            os.environ.pop("FFMI_ATTN_NO_FUSE", None)
        h = hs["fp8" if leg == "fp8" else "fp16"]
        for _ in range(n):
            F.check(L.ffmi_attn_inc(h, b, qkv.ptr, out.ptr, None))

    rows = []
    for ctx in [int(c) for c in args.ctx.split(",")]:
        toks = (F.TokenInfo * R)(*[F.TokenInfo(5, ctx, r, ctx, ctx + 1, 0, 0, 0, 0) for r in range(R)])
        work = (F.AttnWork * R)(*[F.AttnWork(r, r, 1, ctx + 1) for r in range(R)])
        desc = F.BatchDesc(R, R, 0, 0, toks, work, (F.CommitInfo * 1)(), (ctypes.c_uint64 * 1)())
        F.check(L.ffmi_batch_upload(b, ctypes.byref(desc), None))
        us, block = {leg: [] for leg in legs}, {}
        tm = Timer()
        for leg in legs:  # warm-up (code objects, caches), then the block's size
            steps(leg, 20)
            tm.start()
            steps(leg, 50)
            block[leg] = max(50, int(args.window_ms * 50 / tm.stop()))
        for _ in range(args.rounds):
            for leg in legs:
                tm.start()
                steps(leg, block[leg])
                us[leg].append(tm.stop() * 1e3 / block[leg])
        row = dict(heads=HEADS, d=D, requests=R, ctx=ctx, rounds=args.rounds, steps_per_block=block)
        for leg in legs:
            a = np.array(us[leg])
            kv_bytes = 2.0 * R * HEADS * (ctx + 1) * D * (1 if leg == "fp8" else 2)
            row[leg] = dict(us=round(float(np.median(a)), 2),
                            spread=round(float((a.max() - a.min()) / np.median(a)), 3),
                            kv_bytes=int(kv_bytes),
                            kv_GBps=round(kv_bytes / float(np.median(a)) / 1e3, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.child:
        return
    res = dict(bench="kv_fp8_attn_bench", rows=rows)
    if args.variant:  # the parent commit's fp16 legs, a fresh process on the same device
        env = dict(os.environ, FFMI_LIB_VARIANT=args.variant)
        env.pop("FFMI_ATTN_NO_FUSE", None)
        cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ctx", args.ctx,
                             "--rounds", str(args.rounds), "--window-ms", str(args.window_ms)],
                            env=env, capture_output=True, text=True, timeout=600, check=True)
        res[args.variant] = [json.loads(ln) for ln in cp.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
