"""Time per launch of the top-p sampling kernel (ffmi_sample_topp) next to the
greedy tail it replaces (ffmi_arg_topk_ws, k = 1) at V = 32000, T = 8 (a
decode step) and T = 168, in one process on the same logits (N(0, 1.28), the
bench model's spread).  HIP events around N back-to-back launches after a
warm-up of the same shape; the two kernels alternate over R repeats and the
min / median / max per launch are printed.  Run a second time with
FFMI_SAMPLE_HWEXP=1 (the hardware exp2 in place of expf_ref: an A/B switch,
its results are not the rule's) the difference is the share of the time that
is expf_ref evaluation.
One JSON line per shape, also appended to bench_out/sample_topp_bench.jsonl.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("FFMI_BENCH_OUT") or os.path.join(ROOT, "bench_out")  # output directory
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flexflow_amd.ffmi as F  # noqa: E402
from hip_util import Buf, Timer, f16  # noqa: E402

L = F.lib()
V = int(os.environ.get("V", 32000))
N = int(os.environ.get("N", 500))
R = int(os.environ.get("R", 7))
rng = np.random.default_rng(0)


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


for T in (8, 168):
    x = Buf(f16(rng.standard_normal((T, V)) * 1.28))
    u = Buf(((rng.integers(0, 1 << 24, size=T) + 1.0) * 2.0 ** -24).astype(np.float32))
    ids, pr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    nb = int(L.ffmi_arg_topk_workspace_bytes(T))
    tws = Buf(np.zeros(nb // 4, np.uint32))
    sb = int(L.ffmi_sample_topp_workspace_bytes(T, V))
    sws = Buf.empty((sb,), np.uint8)

    def greedy():
        L.ffmi_arg_topk_ws(x.ptr, T, V, 1, ids.ptr, pr.ptr, tws.ptr, nb, None)

    def greedy_one_wg():
        L.ffmi_arg_topk(x.ptr, T, V, 1, ids.ptr, pr.ptr, None)

    def sample():
        L.ffmi_sample_topp(x.ptr, T, V, 0.9, 0.8, u.ptr, ids.ptr, pr.ptr, sws.ptr, sb, None)

    tg, t1, ts = [], [], []
    for _ in range(R):
        tg.append(time_it(greedy))
        t1.append(time_it(greedy_one_wg))
        ts.append(time_it(sample))
    out = dict(T=T, V=V, hwexp=int(os.environ.get("FFMI_SAMPLE_HWEXP", "0") or 0), launches=N,
               repeats=R, arg_topk_ws_k1_us=stats(tg),
               arg_topk_one_workgroup_per_row_k1_us=stats(t1), sample_topp_us=stats(ts),
               ratio_median=round(stats(ts)["median"] / stats(tg)["median"], 2))
    print(json.dumps(out), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "sample_topp_bench.jsonl"), "a") as f:
        f.write(json.dumps(out) + "\n")
