"""What LoRA adapters on down_proj cost (FFMI_MODEL_LORA, ffmi_lora_apply).

Kernels: time per ffmi_lora_apply call (two launches: shrink, expand-add) at
LLaMA-7B's down projection (F, H) = (11008, 4096), r = 16, packed x, at T = 8
(a decode step) and T = 168 (a full verify step), with one adapter on every
row and with eight distinct adapters (T = 8: one per row; T = 168: runs of 21
rows).  HIP events around N back-to-back calls after a warm-up of the same
shape, R repeats, min / median / max.  Next to it the byte floor of reading
the step's distinct A and B once (r (F + H) 2 bytes per adapter) at the HBM
peak of 8 TB/s -- the call also reads x and the fp32 partial sums and
updates y, so the floor is a lower bound on the call, not its roofline.

Serving: incremental-decoding tokens/s of the bench's LLaMA-7B workload (8
requests, 128 prompt + 128 decoded tokens, synthetic weights) for a model
without the flag, and a model with it serving no adapter, one r = 16 adapter
on all requests, and eight distinct adapters.  The four settings alternate
over R repeats after a warm-up generate each, each timed window G generates;
"off" is run twice per repeat (off, off2), which shows the run-to-run spread
the flag-off number is to be read against.  LAYERS=n shortens the model
(rehearsals), SERVE=0 skips this part.

One JSON document, printed and written to profiles/lora_bench.json (or
$FFMI_BENCH_OUT/lora_bench.json).

MODULES=q_proj,v_proj (any of q_proj, k_proj, v_proj, o_proj, down_proj; unset:
the run above, unchanged) measures adapters on those modules instead and
writes profiles/lora_modules_bench.json: the time per ffmi_lora_apply_qkv call
(two launches for the q, k, v modules named) at (H, Hl, Hkv) = (4096, 4096,
4096) with the same T, adapter counts and byte floor (r (in + out) 2 bytes per
module and adapter), and the serving rates off / off2 / on_no_adapter /
on_one_adapter (that adapter on all eight requests; EMPTY=0 leaves out
on_no_adapter, a third model instance with the flag and nothing loaded).  The
kernel timing covers the q, k, v modules only: o_proj and down_proj in MODULES
count in the serving rates, and their kernel pair is the one the default run
times (the o site is that pair at F = 4096).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("FFMI_BENCH_OUT") or os.path.join(ROOT, "profiles")  # output directory
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flexflow_amd as fa  # noqa: E402
import flexflow_amd.ffmi as F  # noqa: E402
from bench import LLAMA_7B, make_prompts  # noqa: E402
from hip_util import Buf, Timer, f16  # noqa: E402
from test_gpu_lora import Table, pack_tiles  # noqa: E402
import lora_rule as LR  # noqa: E402

L = F.lib()
N = int(os.environ.get("N", 300))
R = int(os.environ.get("R", 5))
G = int(os.environ.get("G", 2))
RANK = 16
HBM_BYTES_PER_US = 8e6  # 8 TB/s (MI355X_MICROARCH.md)
rng = np.random.default_rng(0)
fa.set_device(0)


def time_it(fn):
    for _ in range(20):
        fn()
    tm = Timer()
    tm.start()
    for _ in range(N):
        fn()
    return tm.stop() * 1e3 / N


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 2), median=round(xs[len(xs) // 2], 2), max=round(xs[-1], 2))


B, P, D = 8, 128, 128  # the serving workload: requests, prompt and decoded tokens


def serve_config():
    """(cfg, RequestManager keywords, Model keywords) of the serving part"""
    cfg = dict(LLAMA_7B)
    if os.environ.get("LAYERS"):
        cfg["num_layers"] = int(os.environ["LAYERS"])
    return (cfg, dict(max_requests_per_batch=B, max_tokens_per_batch=1024, max_sequence_length=512),
            dict(max_requests=B, max_tokens=1024, max_seq_len=512, weight_seed=20250117))


def serve_rates(cfg, rm_kw, settings):
    """settings {name: (model, lora_ids)}, "off" among them: a warm-up generate
    each, then the settings in rotation, G generates per timed window"""
    prompts = make_prompts(B, P - 1, cfg["vocab_size"])

    def generates(model, lora_ids, n):
        new = 0
        t0 = time.time()
        for _ in range(n):
            res = fa.generate(fa.RequestManager(**rm_kw), model, prompts, max_length=P + D,
                              lora_ids=lora_ids)
            new += sum(len(r.output_tokens) - len(r.input_tokens) for r in res)
        return new / (time.time() - t0)

    for m, li in settings.values():
        generates(m, li, 1)  # (graph capture of every shape)
    rates = {k: [] for k in settings}
    for _ in range(R if "R" in os.environ else 3):
        for name, (m, li) in settings.items():
            rates[name].append(round(generates(m, li, G), 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    return dict(workload=f"llama7b_incr B={B} P={P} D={D} layers={cfg['num_layers']}",
                rank=RANK, generates_per_window=G, tokens_per_s=rates, median=med,
                over_off={k: round(v / med["off"], 4) for k, v in med.items()})


MODULES = [m for m in os.environ.get("MODULES", "").split(",") if m]
QKV = ("q_proj", "k_proj", "v_proj")


def modules_run():
    """the MODULES= run (see the module docstring)"""
    Hd, Fd = LLAMA_7B["hidden"], LLAMA_7B["intermediate"]
    import ctypes
    out = dict(modules=MODULES, kernels=[])
    segs = [m for m in QKV if m in MODULES]
    if segs:
        ads = {i: LR.dense(RANK, Hd, Hd, rng) for i in range(LR.MAX_ADAPTERS)}
        tabs = [Table(ads if m in MODULES else {}, Hd, Hd) for m in QKV]
        ptrs = (ctypes.c_void_p * 3)(*[t.dev.ptr.value for t in tabs])
        widths = (ctypes.c_int * 3)(Hd, Hd, Hd)
        for T in (8, 168):
            x = Buf(pack_tiles(f16(rng.standard_normal((T, Hd)))))
            y = Buf(f16(np.zeros((T, 3 * Hd))))
            nws = int(L.ffmi_lora_qkv_workspace_bytes(T, Hd))
            ws = Buf.empty((nws,), np.uint8)
            for name, slots in (("one_adapter", np.zeros(T, np.int32)),
                                ("eight_adapters", (np.arange(T) * 8 // T).astype(np.int32))):
                sb = Buf(slots)

                def call():
                    L.ffmi_lora_apply_qkv(x.ptr, T, Hd, widths, sb.ptr, ptrs, y.ptr, 3 * Hd, 1, ws.ptr,
                                          nws, None, None)

                distinct = len(set(slots.tolist()))
                floor = distinct * len(segs) * RANK * (Hd + Hd) * 2 / HBM_BYTES_PER_US
                t = stats([time_it(call) for _ in range(R)])
                row = dict(T=T, in_dim=Hd, seg_width=[Hd] * 3, segments=segs, rank=RANK, slots=name,
                           distinct_adapters=distinct, launches=N, repeats=R, call_us=t,
                           adapter_bytes_floor_us=round(floor, 3))
                print(json.dumps(row), flush=True)
                out["kernels"].append(row)
    if os.environ.get("SERVE", "1") != "0":
        cfg, rm_kw, kw = serve_config()
        off = fa.Model(cfg, "inc", **kw)
        on = fa.Model(cfg, "inc", lora=True, **kw)
        NLy = cfg["num_layers"]
        g = np.random.default_rng(100)
        dims = {m: (Fd if m == "down_proj" else Hd, Hd) for m in MODULES}
        a = on.load_lora({m: (f16(g.standard_normal((NLy, RANK, i)) / np.sqrt(i)),
                              f16(g.standard_normal((NLy, o, RANK)) * 0.01))
                          for m, (i, o) in dims.items()}, 2.0 * RANK)
        settings = {"off": (off, None), "off2": (off, None), "on_one_adapter": (on, [a] * B)}
        if os.environ.get("EMPTY", "1") != "0":  # (no adapter resident: the step of a model without the flag)
            settings["on_no_adapter"] = (fa.Model(cfg, "inc", lora=True, **kw), None)
        out["serve"] = serve_rates(cfg, rm_kw, settings)
        print(json.dumps(out["serve"]), flush=True)
    os.makedirs(OUT, exist_ok=True)
    name = "lora_modules_bench.json"
    prev = {}
    if os.path.exists(os.path.join(OUT, name)):
        with open(os.path.join(OUT, name)) as f:
            prev = json.load(f)
    prev[",".join(MODULES)] = out  # one entry per MODULES setting
    with open(os.path.join(OUT, name), "w") as f:
        f.write(json.dumps(prev, indent=1) + "\n")


if MODULES:
    modules_run()
    sys.exit(0)

kernels = []
Fd, Hd = LLAMA_7B["intermediate"], LLAMA_7B["hidden"]
ads = {i: LR.dense(RANK, Fd, Hd, rng) for i in range(LR.MAX_ADAPTERS)}
table = Table(ads, Fd, Hd)
for T in (8, 168):
    x = Buf(pack_tiles(f16(rng.standard_normal((T, Fd)))))
    y = Buf(f16(np.zeros((T, Hd))))
    nws = int(L.ffmi_lora_workspace_bytes(T, Fd))
    ws = Buf.empty((nws,), np.uint8)
    for name, slots in (("one_adapter", np.zeros(T, np.int32)),
                        ("eight_adapters", (np.arange(T) * 8 // T).astype(np.int32))):
        sb = Buf(slots)

        def call():
            L.ffmi_lora_apply(x.ptr, T, Fd, Hd, sb.ptr, table.dev.ptr, y.ptr, 1, ws.ptr, nws, None,
                              None)

        distinct = len(set(slots.tolist()))
        floor = distinct * RANK * (Fd + Hd) * 2 / HBM_BYTES_PER_US
        t = stats([time_it(call) for _ in range(R)])
        row = dict(T=T, F=Fd, H=Hd, rank=RANK, slots=name, distinct_adapters=distinct, launches=N,
                   repeats=R, call_us=t, adapter_bytes_floor_us=round(floor, 3))
        print(json.dumps(row), flush=True)
        kernels.append(row)

out = dict(kernels=kernels)
if os.environ.get("SERVE", "1") != "0":
    cfg, rm_kw, kw = serve_config()
    off = fa.Model(cfg, "inc", **kw)
    on = fa.Model(cfg, "inc", lora=True, **kw)
    NLy = cfg["num_layers"]
    ids = []
    for i in range(LR.MAX_ADAPTERS):
        g = np.random.default_rng(100 + i)
        A = f16(g.standard_normal((NLy, RANK, Fd)) / np.sqrt(Fd))
        Bm = f16(g.standard_normal((NLy, Hd, RANK)) * 0.01)
        ids.append(on.load_lora(A, Bm, 2.0 * RANK))
    out["serve"] = serve_rates(cfg, rm_kw, {"off": (off, None), "off2": (off, None),
                                            "on_no_adapter": (on, None),
                                            "on_one_adapter": (on, [ids[0]] * B),
                                            "on_eight_adapters": (on, ids[:B])})
    print(json.dumps(out["serve"]), flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "lora_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
