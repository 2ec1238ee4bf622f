"""Time per call of the vocab-sharded top-p sampling kernels alone
(ffmi_vocab_shard_sample_topp over a ONE-rank communicator: the five exchanges
degenerate to nothing, the six launches remain) at Vl = 32000 and Vl = 4000 (an
8-way shard of 32000), next to ffmi_sample_topp at V = 32000, in one process on
the same logits (N(0, 1.28)), by the method of scripts/sample_topp_bench.py:
HIP events around N back-to-back calls after a warm-up of the same shape, the
three alternate over R repeats, min / median / max per call.  T = 8 (a decode
step) and T = 32 (the largest one-chunk batch at P = 8).
What the exchanges cost on xGMI is NOT measured here.
One JSON line per shape, also appended to bench_out/vshard_sample_bench.jsonl.
"""
import ctypes
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
N = int(os.environ.get("N", 300))
R = int(os.environ.get("R", 7))
rng = np.random.default_rng(0)
comm = ctypes.c_void_p()
F.check(L.ffmi_comm_create_peer(1, 0, ctypes.byref(comm)))


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


for T in (8, 32):
    xh = f16(rng.standard_normal((T, V)) * 1.28)
    x, x8 = Buf(xh), Buf(np.ascontiguousarray(xh[:, :V // 8]))
    u = Buf(((rng.integers(0, 1 << 24, size=T) + 1.0) * 2.0 ** -24).astype(np.float32))
    ids, pr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    sb = int(L.ffmi_sample_topp_workspace_bytes(T, V))
    sws = Buf.empty((sb,), np.uint8)
    vb = int(L.ffmi_vocab_shard_sample_scratch_bytes(1, T, V))
    vws = Buf.empty((vb,), np.uint8)

    def sample():
        F.check(L.ffmi_sample_topp(x.ptr, T, V, 0.9, 0.8, u.ptr, ids.ptr, pr.ptr, sws.ptr, sb, None))

    def sharded_full():
        F.check(L.ffmi_vocab_shard_sample_topp(comm, x.ptr, T, V, 0.9, 0.8, u.ptr, ids.ptr, pr.ptr,
                                               vws.ptr, vb, None))

    def sharded_eighth():
        F.check(L.ffmi_vocab_shard_sample_topp(comm, x8.ptr, T, V // 8, 0.9, 0.8, u.ptr, ids.ptr,
                                               pr.ptr, vws.ptr, vb, None))

    # the one-rank sharded pick is the one-GPU kernel's
    sample()
    a = ids.get().copy()
    sharded_full()
    assert np.array_equal(a, ids.get()), (a, ids.get())
    ts, tf, t8 = [], [], []
    for _ in range(R):
        ts.append(time_it(sample))
        tf.append(time_it(sharded_full))
        t8.append(time_it(sharded_eighth))
    out = dict(T=T, V=V, launches=N, repeats=R, sample_topp_us=stats(ts),
               vshard_sample_one_rank_Vl_full_us=stats(tf),
               vshard_sample_one_rank_Vl_eighth_us=stats(t8), Vl_eighth=V // 8,
               note="six launches, exchanges degenerate (one rank): xGMI cost not measured")
    print(json.dumps(out), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vshard_sample_bench.jsonl"), "a") as f:
        f.write(json.dumps(out) + "\n")
L.ffmi_comm_destroy(comm)
