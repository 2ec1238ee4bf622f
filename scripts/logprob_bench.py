"""Time per launch of the per-token log-probability kernels (ffmi_token_logprobs:
two launches per call) next to the greedy pick they follow (ffmi_arg_topk_ws,
k = 1), in one process on the same logits (N(0, 1.28), the bench model's
spread) at (T, V) = (8, 32000) (a decode step), (24, 32000), (168, 32000) (a
full verify step) and (8, 128256) (LLaMA-3's vocabulary).  HIP events around N
back-to-back calls after a warm-up of the same shape; the two alternate over R
repeats and the min / median / max per call are reported.  The argmax reads the
same bytes and does more per element (expf_ref, the selection), so it is the
yardstick: the log-probability call's median should not exceed it.

Then the incremental-decoding tokens/s of the bench's LLaMA-7B workload (8
requests, 128 prompt + 128 decoded tokens, synthetic weights) with logprobs
off and on, on ONE model: Model.set_logprobs switches between runs, the two
settings alternate over R repeats after a warm-up generate each (graph
capture), each timed window G generates.  LAYERS=n shortens the model
(rehearsals), SERVE=0 skips this part.

One JSON document, printed and written to profiles/logprob_bench.json (or
$FFMI_BENCH_OUT/logprob_bench.json).
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

L = F.lib()
N = int(os.environ.get("N", 500))
R = int(os.environ.get("R", 7))
G = int(os.environ.get("G", 3))
SHAPES = [(8, 32000), (24, 32000), (168, 32000), (8, 128256)]
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


kernels = []
for T, V in SHAPES:
    x = Buf(f16(rng.standard_normal((T, V)) * 1.28))
    ids, pr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    lp = Buf.empty((T,), np.float32)
    nb = int(L.ffmi_arg_topk_workspace_bytes(T))
    tws = Buf(np.zeros(nb // 4, np.uint32))
    lb = int(L.ffmi_token_logprobs_workspace_bytes(T, V))
    lws = Buf.empty((lb,), np.uint8)

    def greedy():
        L.ffmi_arg_topk_ws(x.ptr, T, V, 1, ids.ptr, pr.ptr, tws.ptr, nb, None)

    def logprobs():
        L.ffmi_token_logprobs(x.ptr, T, V, 0.0, None, ids.ptr, lp.ptr, lws.ptr, lb, None)

    def logprobs_tempered():
        L.ffmi_token_logprobs(x.ptr, T, V, 0.9, None, ids.ptr, lp.ptr, lws.ptr, lb, None)

    greedy()  # (valid picks for the calls below)
    tg, tl, tt = [], [], []
    for _ in range(R):
        tg.append(time_it(greedy))
        tl.append(time_it(logprobs))
        tt.append(time_it(logprobs_tempered))
    row = dict(T=T, V=V, launches=N, repeats=R, arg_topk_ws_k1_us=stats(tg),
               token_logprobs_us=stats(tl), token_logprobs_temperature_us=stats(tt),
               ratio_median=round(stats(tl)["median"] / stats(tg)["median"], 2))
    print(json.dumps(row), flush=True)
    kernels.append(row)

out = dict(kernels=kernels)
if os.environ.get("SERVE", "1") != "0":
    B, P, D = 8, 128, 128
    cfg = dict(LLAMA_7B)
    if os.environ.get("LAYERS"):
        cfg["num_layers"] = int(os.environ["LAYERS"])
    rm_kw = dict(max_requests_per_batch=B, max_tokens_per_batch=1024, max_sequence_length=512)
    llm = fa.Model(cfg, "inc", max_requests=B, max_tokens=1024, max_seq_len=512,
                   weight_seed=20250117)
    prompts = make_prompts(B, P - 1, cfg["vocab_size"])

    def generates(n):
        new = 0
        t0 = time.time()
        for _ in range(n):
            res = fa.generate(fa.RequestManager(**rm_kw), llm, prompts, max_length=P + D)
            new += sum(len(r.output_tokens) - len(r.input_tokens) for r in res)
        return new / (time.time() - t0)

    rates = {"off": [], "on": []}
    for _ in range(R if "R" in os.environ else 3):
        for name in rates:
            llm.set_logprobs(name == "on")
            generates(1)  # (set_logprobs drops the captured graphs)
            rates[name].append(round(generates(G), 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    out["serve"] = dict(workload=f"llama7b_incr B={B} P={P} D={D} layers={cfg['num_layers']}",
                        generates_per_window=G, tokens_per_s=rates, median=med,
                        on_over_off=round(med["on"] / med["off"], 4))
    print(json.dumps(out["serve"]), flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "logprob_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
