"""Decode-step attention of a GQA model, three ways, through the C ABI.

Legs, each one ffmi_attn_inc call per launch on the same uploaded batch (one
token per request at position ctx, device events around blocks of launches):
  replicated  an ffmi_attn_create handle of num_heads heads, K/V replicated to
              every query head (the default load of a GQA checkpoint)
  kv_indexed  ffmi_attn_create_gqa, route 1: one workgroup per (request, query
              head), each reading K/V head h // G
  shared      ffmi_attn_create_gqa, route 2: one workgroup per (request, K/V
              head), the group's G query heads as rows of its tile
  auto        ffmi_attn_create_gqa, route 0: the handle's own choice
The legs alternate within each round, so drift of the device or of its other
tenants lands on all of them; a leg's figure is the median of its rounds and
its spread (max - min) / median over them.  The caches hold random fp16 data.
kv_bytes: the K and V^T bytes the algorithm needs for one step (every key of
every request, once per cached head).

    python scripts/gqa_attn_bench.py [--out profiles/gqa_attn_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flexflow_amd.ffmi as F  # noqa: E402
from hip_util import Buf, Timer, f16, hip  # noqa: E402

SHAPES = [(32, 8, 128), (8, 1, 128)]  # Llama-3-8B; a Llama-3-70B shard at TP 8
LEGS = ("replicated", "kv_indexed", "shared", "auto")


def fill_random(ptr, nbytes, block):
    off = 0
    while off < nbytes:
        n = min(block.nbytes, nbytes - off)
        assert hip().hipMemcpy(ctypes.c_void_p(ptr.value + off), block.ctypes.data, n, 1) == 0
        off += n


def make_handle(L, cfg, kvh, route, block):
    h = F.attn_create_gqa(cfg, kvh)
    F.attn_set_gqa_route(h, route)
    k, v = ctypes.c_void_p(), ctypes.c_void_p()
    F.check(L.ffmi_attn_kv_ptrs(h, ctypes.byref(k), ctypes.byref(v), None))
    half = F.attn_cache_bytes(h) // 2
    fill_random(k, half, block)
    fill_random(v, half, block)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", default="512,2048,8192")
    ap.add_argument("--reqs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=32, help="launches per timed block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gqa_attn_bench.json"))
    args = ap.parse_args()
    L = F.lib()
    R = args.reqs
    rng = np.random.default_rng(0)
    block = f16(rng.standard_normal(8 << 20) * 0.5)
    rows = []
    for heads, kvh, d in SHAPES:
        for ctx in [int(c) for c in args.ctx.split(",")]:
            cfg = F.AttnCfg(F.ATTN_INC, heads, d, R, ctx + 32, 0, 16, 1.0 / np.sqrt(d), 10000.0, 1)
            hs = dict(replicated=make_handle(L, cfg, heads, 0, block),
                      kv_indexed=make_handle(L, cfg, kvh, F.GQA_ROUTE_KV_INDEXED, block),
                      shared=make_handle(L, cfg, kvh, F.GQA_ROUTE_GROUP_SHARED, block),
                      auto=make_handle(L, cfg, kvh, F.GQA_ROUTE_AUTO, block))
            b = ctypes.c_void_p()
            F.check(L.ffmi_batch_create(16, R, ctypes.byref(b)))
            toks = (F.TokenInfo * R)(*[F.TokenInfo(5, ctx, r, ctx, ctx + 1, 0, 0, 0, 0)
                                       for r in range(R)])
            work = (F.AttnWork * R)(*[F.AttnWork(r, r, 1, ctx + 1) for r in range(R)])
            desc = F.BatchDesc(R, R, 0, 0, toks, work, (F.CommitInfo * 1)(),
                               (ctypes.c_uint64 * 1)())
            F.check(L.ffmi_batch_upload(b, ctypes.byref(desc), None))
            Hl, Hk = heads * d, kvh * d
            qkv = dict(replicated=Buf(f16(rng.standard_normal((R, 3 * Hl)))))
            qkv_g = Buf(f16(rng.standard_normal((R, Hl + 2 * Hk))))
            out = Buf.empty((16, Hl), np.float16)
            us = {leg: [] for leg in LEGS}
            for leg in LEGS:  # warm-up: code objects, caches
                for _ in range(20):
                    F.check(L.ffmi_attn_inc(hs[leg], b, qkv.get(leg, qkv_g).ptr, out.ptr, None))
            tm = Timer()
            for _ in range(args.rounds):
                for leg in LEGS:
                    q = qkv.get(leg, qkv_g).ptr
                    tm.start()
                    for _ in range(args.block):
                        L.ffmi_attn_inc(hs[leg], b, q, out.ptr, None)
                    us[leg].append(tm.stop() * 1e3 / args.block)
            row = dict(heads=heads, kv_heads=kvh, d=d, requests=R, ctx=ctx,
                       launches_per_leg=args.rounds * args.block)
            for leg in LEGS:
                a = np.array(us[leg])
                cached = heads if leg == "replicated" else kvh
                kv_bytes = 2.0 * R * cached * (ctx + 1) * d * 2
                row[leg] = dict(us=round(float(np.median(a)), 2),
                                spread=round(float((a.max() - a.min()) / np.median(a)), 3),
                                kv_bytes=int(kv_bytes),
                                kv_GBps=round(kv_bytes / float(np.median(a)) / 1e3, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in hs.values():
                L.ffmi_attn_destroy(h)
            L.ffmi_batch_destroy(b)
            del qkv, qkv_g, out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(bench="gqa_attn_bench", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
