"""The top-p sampling rule (include/ffmi.h ffmi_sample_topp) restated in numpy
on the oracle's fp16 softmax, for the kernel and model tests.

    z = R16(float(x) / float(R16(temperature)))
    p, order = oracle_lib.softmax_topk(z, k=V): every p, sorted (p desc, index asc)
    C = fp64 cumsum of p in that order (exact: multiples of 2^-24, sum < 2)
    t = (double(u) * double(topp)) * double(topp)
    pick the first j with C_j >= t, else the last token of the order
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

_POOL = ThreadPoolExecutor(min(16, os.cpu_count() or 1))


def scaled_logits(x16, temperature):
    """z: the half-by-half division by the temperature (element_unary.cu:136)."""
    th = np.float32(np.float16(temperature))
    return (np.asarray(x16, np.float16).astype(np.float32) / th).astype(np.float16)


def sorted_probs(z16):
    """(ids, p) [T][V] of the oracle's softmax top-V: the reference's sort.
    Row blocks run on a thread pool (the oracle call releases the GIL)."""
    z = np.ascontiguousarray(z16, np.float16).astype(np.float32)
    T, V = z.shape
    step = max(1, min(T, (1 << 19) // V + 1))
    parts = list(_POOL.map(lambda a: O.softmax_topk(z[a:a + step], V, fp16=1), range(0, T, step)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def pick(ids, p, topp, u):
    """(token, its p) per row from the sorted (ids, p) and the uniforms u."""
    T, V = p.shape
    tp = np.float64(np.float32(topp))
    t = (np.asarray(u, np.float32).astype(np.float64) * tp) * tp
    C = np.cumsum(p.astype(np.float64), axis=1)
    j = np.array([min(int(np.searchsorted(C[r], t[r], side="left")), V - 1) for r in range(T)])
    rows = np.arange(T)
    return ids[rows, j].astype(np.int32), p[rows, j].astype(np.float32)


def sample(x16, temperature, topp, u):
    ids, p = sorted_probs(scaled_logits(x16, temperature))
    return pick(ids, p, topp, u)


def grid_uniforms(rng, n):
    """n uniforms on the 2^-24 grid of (0, 1], the ends included when n >= 2."""
    u = (rng.integers(0, 1 << 24, size=n).astype(np.float64) + 1.0) * 2.0 ** -24
    if n >= 2:
        u[0], u[-1] = 2.0 ** -24, 1.0
    return u.astype(np.float32)
