"""Full precision: the reference's --use-full-precision
(inference/spec_infer/spec_infer.cc:102, incr_decoding.cc:77;
ffmi_model_opts.full_precision, runtime/llama_f32.cpp, kernels/f32.hip):
weights, activations, KV cache and softmax in fp32.

The reference runs its exact-diff invariants in this mode
(tests/inference/cpp_inference_tests.sh: the first 30 tokens identical
:104-129, SpecInfer == incremental decoding :183-189, TP = 1 vs TP > 1
:203-217).  GPU and oracle (fp32 mode, pinned to HF transformers fp32 by
test_oracle_golden.py) share every operation and differ only in fp32
summation order, ~1e-7 relative; on the bench's random-weight LLaMA-7B the
top-2 logit gap falls inside that noise at ~1e-5 of positions, so the
reference's bars are demanded literally here -- a divergence is accepted only
at an fp32-level tie (the oracle's gap between the two picks <= 1e-4, reported
if it ever happens).
"""
import ctypes

import os

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import oracle_lib as O
import peer_tasks as PT
from hip_util import Buf, report
from peer_group import run_group
from spec_configs import SPEC, spec_setup

pytestmark = pytest.mark.gpu

SEED = 20250117
LLAMA_7B = dict(num_layers=32, vocab_size=32000, num_heads=32, num_kv_heads=32, hidden=4096,
                intermediate=11008, rms_eps=1e-6, rope_theta=10000.0)
LLAMA_68M = dict(num_layers=2, vocab_size=32000, num_heads=12, num_kv_heads=12, hidden=768,
                 intermediate=3072, rms_eps=1e-6, rope_theta=10000.0)
FP32_TIE = 1e-4  # oracle logit gap below which two fp32 runs may pick differently


@pytest.mark.parametrize("T,N,K", [(1, 16, 32), (5, 48, 96), (8, 4096, 4096), (24, 2304, 768),
                                   (33, 272, 1376), (64, 1000, 3072), (3, 40, 64), (168, 1536, 4096),
                                   (577, 96, 1376), (1024, 512, 4096)])
def test_linear_f32_against_fp64(T, N, K):
    """ffmi_linear_f32 against an fp64 product: every element within the fp32
    error bound of a K-term sum (2e-6 * sum|x w|, the measured MFMA f32 error
    is ~3.5e-7 at K 4096), and bit-identical on a second call (fixed order)."""
    rng = np.random.default_rng(T * 7 + N + K)
    X = rng.uniform(-1, 1, (T, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    ref = X.astype(np.float64) @ W.astype(np.float64).T
    mag = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T
    bx, bw, by = Buf(X), Buf(W), Buf.empty((T, N), np.float32)
    L = F.lib()
    assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0
    y1 = by.get()
    assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0
    y2 = by.get()
    err = np.abs(y1 - ref)
    assert np.all(err <= 2e-6 * mag + 1e-30), float((err / mag).max())
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))


OFF = int(os.environ.get("FFMI_RANDOM_SEED_OFFSET", "0"))  # fresh seeds for one-off sweeps


@pytest.mark.parametrize("seed", range(12 * int(os.environ.get("FFMI_RANDOM_SCALE", "1"))))
def test_linear_f32_random_shapes(seed):
    """ffmi_linear_f32 at random shapes (T 1-1100, N 1-6000 ragged, K a
    multiple of 32 up to 8192) under the same bound and determinism as
    test_linear_f32_against_fp64."""
    rng = np.random.default_rng(8800 + OFF + seed)
    T = int(np.exp(rng.uniform(0, np.log(1100))))
    N = int(rng.integers(1, 6000))
    K = 32 * int(np.exp(rng.uniform(0, np.log(256))))
    X = rng.uniform(-1, 1, (T, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    ref = X.astype(np.float64) @ W.astype(np.float64).T
    mag = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T
    bx, bw, by = Buf(X), Buf(W), Buf.empty((T, N), np.float32)
    L = F.lib()
    assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0, (T, N, K)
    y1 = by.get()
    assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0
    err = np.abs(y1 - ref)
    assert np.all(err <= 2e-6 * mag + 1e-30), (T, N, K, float((err / mag).max()))
    assert np.array_equal(y1.view(np.uint32), by.get().view(np.uint32))


@pytest.mark.parametrize("N,K", [(48, 32), (272, 1376), (1000, 3072)])
def test_linear_f32_rows_independent_of_T(N, K):
    """A row of ffmi_linear_f32 is bit-identical whatever T it is computed in:
    the four default forms (T <= 16, <= 32, <= 64, > 64) all split k over the
    workgroup's 4 waves at the same k-blocks and sum the ranges in the same
    order, so the first T rows of one X, T on both sides of every form's
    threshold, must equal the same rows of the T = 200 result.  The fp32
    "SpecInfer == incremental decoding" bar rests on this (a verify row at
    T = 168 against a decode row at T = 8)."""
    rng = np.random.default_rng(4100 + OFF + N + K)
    X = rng.uniform(-1, 1, (200, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    bx, bw = Buf(X), Buf(W)
    L = F.lib()

    def rows(T):
        by = Buf.empty((T, N), np.float32)
        assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0
        return by.get().view(np.uint32)

    full = rows(200)
    differing = {}
    for T in (1, 5, 16, 17, 32, 33, 64, 65, 128, 200):
        n = int((rows(T) != full[:T]).any(axis=1).sum())
        if n:
            differing[T] = n
    report("linear_f32_rows_independent_of_T", N=N, K=K, rows_differing_by_T=differing)
    assert not differing, differing


# the T > 64 shapes of test_linear_f32_against_fp64
TILE_CASES = [(168, 1536, 4096), (577, 96, 1376), (1024, 512, 4096)]


def _tile_case_operands(T, N, K):
    rng = np.random.default_rng(T * 7 + N + K)
    return (rng.uniform(-1, 1, (T, K)).astype(np.float32),
            rng.uniform(-1, 1, (N, K)).astype(np.float32))


def _linear_f32_outputs(env, conn):
    try:
        os.environ.update(env)
        L = F.lib()
        out = []
        for T, N, K in TILE_CASES:
            X, W = _tile_case_operands(T, N, K)
            bx, bw, by = Buf(X), Buf(W), Buf.empty((T, N), np.float32)
            F.check(L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None))
            out.append(by.get())
        conn.send(("ok", out))
    except BaseException as e:  # noqa: BLE001 -- reported to the parent
        conn.send(("err", repr(e)))
    finally:
        conn.close()


def test_linear_f32_tile_form_against_fp64():
    """FFMI_F32_GEMM_TILE=1 (the 2 x 2-wave, 32 x 32-per-wave A/B form of the
    T > 64 launch, one k chain per wave) under test_linear_f32_against_fp64's
    bound.  The switch is read once per process, so the form runs in a fresh
    `spawn` process; its sums are ordered differently from the default form's,
    so the outputs must also differ from this process's somewhere (the switch
    took effect)."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    a, b = ctx.Pipe()
    p = ctx.Process(target=_linear_f32_outputs, args=({"FFMI_F32_GEMM_TILE": "1"}, b))
    p.start()
    try:
        assert a.poll(180), "tile-form process did not answer"
        st, res = a.recv()
    finally:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert st == "ok", res
    L = F.lib()
    worst, same = 0.0, True
    for (T, N, K), y in zip(TILE_CASES, res):
        X, W = _tile_case_operands(T, N, K)
        ref = X.astype(np.float64) @ W.astype(np.float64).T
        mag = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T
        err = np.abs(y - ref)
        worst = max(worst, float((err / mag).max()))
        assert np.all(err <= 2e-6 * mag + 1e-30), (T, N, K, float((err / mag).max()))
        bx, bw, by = Buf(X), Buf(W), Buf.empty((T, N), np.float32)
        assert L.ffmi_linear_f32(bx.ptr, bw.ptr, by.ptr, T, N, K, None) == 0
        same = same and np.array_equal(by.get().view(np.uint32), y.view(np.uint32))
    report("linear_f32_tile_form", max_rel_err=worst, identical_to_default=same)
    assert not same, "FFMI_F32_GEMM_TILE=1 gave the default form's bits: switch not applied?"


def ulps32(a, b):
    """distance in fp32 ulps (monotonic int mapping)"""
    def key(x):
        u = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("H", [768, 4096])
def test_rmsnorm_f32_against_oracle(H):
    """ffmi_rmsnorm_f32 / ffmi_residual_rmsnorm_f32 vs the oracle's fp32 mode
    (the same fp32 operations; only the fp64 sum of squares is reordered):
    within 1 ulp, >= 99% bit-identical, the residual sum bit-exact"""
    rng = np.random.default_rng(H)
    T, eps = 13, 1e-6
    x1 = rng.standard_normal((T, H)).astype(np.float32)
    x2 = rng.standard_normal((T, H)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, H).astype(np.float32)
    L = F.lib()
    b1, b2, bw = Buf(x1), Buf(x2), Buf(w)
    out, res = Buf.empty((T, H), np.float32), Buf.empty((T, H), np.float32)
    assert L.ffmi_rmsnorm_f32(b1.ptr, bw.ptr, out.ptr, T, H, ctypes.c_float(eps), None) == 0
    d = ulps32(out.get(), O.rmsnorm(x1, w, eps, fp16=0))
    assert d.max() <= 1 and (d == 0).mean() >= 0.99, (int(d.max()), float((d == 0).mean()))
    assert L.ffmi_residual_rmsnorm_f32(b1.ptr, b2.ptr, bw.ptr, res.ptr, out.ptr, T, H,
                                       ctypes.c_float(eps), None) == 0
    rr, ro = O.residual_rmsnorm(x1, x2, w, eps, fp16=0)
    assert np.array_equal(res.get(), rr)
    d = ulps32(out.get(), ro)
    assert d.max() <= 1 and (d == 0).mean() >= 0.99


def test_silu_mul_f32_against_oracle():
    """SigmoidSiluMulti on fp32: the device expf against the host's (each
    within ~1 ulp of exp) carried through 1/(1 + e), a * sg and * b: <= 4 ulp,
    >= 90% bit-identical"""
    rng = np.random.default_rng(9)
    a = (4 * rng.standard_normal(50000)).astype(np.float32)
    b = rng.standard_normal(50000).astype(np.float32)
    ba, bb, bo = Buf(a), Buf(b), Buf.empty((50000,), np.float32)
    assert F.lib().ffmi_silu_mul_f32(ba.ptr, bb.ptr, bo.ptr, 50000, None) == 0
    d = ulps32(bo.get(), O.silu_mul(a, b, fp16=0))
    assert d.max() <= 4 and (d == 0).mean() >= 0.9, (int(d.max()), float((d == 0).mean()))


@pytest.mark.parametrize("k", [1, 3])
def test_arg_topk_f32_against_oracle(k):
    """softmax + arg-top-k on fp32 probabilities, lowest index among equal
    probabilities (planted exact ties, also across the top-k boundary)"""
    rng = np.random.default_rng(k)
    T, V = 24, 32000
    z = rng.standard_normal((T, V)).astype(np.float32)
    for t in range(0, T, 3):  # ties: the row's max copied to a lower and a higher index
        j = int(z[t].argmax())
        z[t, (j + 7) % V] = z[t, j]
        z[t, (j + V - 5) % V] = z[t, j]
    bz, bi, bp = Buf(z), Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
    assert F.lib().ffmi_arg_topk_f32(bz.ptr, T, V, k, bi.ptr, bp.ptr, None) == 0
    ids, probs = O.softmax_topk(z, k, fp16=0)
    assert np.array_equal(bi.get(), ids)
    assert ulps32(bp.get(), probs).max() <= 2


def _rmsnorm_f32_calls(x1, x2, w, eps=1e-6):
    """(norm of x1, residual sum, norm of the sum, the same two with
    residual_out aliasing x1 -- the model's in-place form) from the GPU"""
    T, H = x1.shape
    L = F.lib()
    b1, b2, bw = Buf(x1), Buf(x2), Buf(w)
    out, res = Buf.empty((T, H), np.float32), Buf.empty((T, H), np.float32)
    e = ctypes.c_float(eps)
    assert L.ffmi_rmsnorm_f32(b1.ptr, bw.ptr, out.ptr, T, H, e, None) == 0
    plain = out.get()
    assert L.ffmi_residual_rmsnorm_f32(b1.ptr, b2.ptr, bw.ptr, res.ptr, out.ptr, T, H, e,
                                       None) == 0
    rsum, rout = res.get(), out.get()
    out2 = Buf.empty((T, H), np.float32)
    assert L.ffmi_residual_rmsnorm_f32(b1.ptr, b2.ptr, bw.ptr, b1.ptr, out2.ptr, T, H, e,
                                       None) == 0
    return plain, rsum, rout, b1.get(), out2.get()


@pytest.mark.parametrize("H", [1, 7, 255, 256, 257, 1000, 4099, 11008])
def test_rmsnorm_f32_shapes_edges_and_aliasing(H):
    """ffmi_rmsnorm_f32 / ffmi_residual_rmsnorm_f32 vs the oracle's fp32 mode
    at H below, at and off the 256 threads (one element or fewer per thread,
    ragged strides, LLaMA-7B's intermediate width) x T 1 and 300.

    Random-normal rows: <= 1 ulp, >= 99% bit-identical -- the share is taken
    over the random-normal rows only (all elements of both T, the plain and
    the residual call) -- and the residual sum bit-exact.  Edge rows (all
    zeros; rows scaled by 1e-20, where eps dominates the mean square; rows
    scaled by 1e15) are outside the share: each within 1 ulp, the residual sum
    bit-exact, and the zero row's output exactly 0 and finite.

    residual_out == x1 (the only form the model uses) must give the bits of
    the non-aliased call, sum and output."""
    eps = 1e-6
    rng = np.random.default_rng(4200 + OFF + H)
    w = rng.uniform(0.5, 1.5, H).astype(np.float32)
    exact = []
    for T in (1, 300):
        x1 = rng.standard_normal((T, H)).astype(np.float32)
        x2 = rng.standard_normal((T, H)).astype(np.float32)
        plain, rsum, rout, asum, aout = _rmsnorm_f32_calls(x1, x2, w, eps)
        d = ulps32(plain, O.rmsnorm(x1, w, eps, fp16=0))
        assert d.max() <= 1, (T, int(d.max()))
        exact.append((d == 0).ravel())
        rr, ro = O.residual_rmsnorm(x1, x2, w, eps, fp16=0)
        assert np.array_equal(rsum.view(np.uint32), rr.view(np.uint32)), T
        d = ulps32(rout, ro)
        assert d.max() <= 1, (T, int(d.max()))
        exact.append((d == 0).ravel())
        assert np.array_equal(asum.view(np.uint32), rsum.view(np.uint32)), T
        assert np.array_equal(aout.view(np.uint32), rout.view(np.uint32)), T
    share = float(np.concatenate(exact).mean())
    # edge rows: zeros | eps-dominated | large
    e1 = rng.standard_normal((3, H)).astype(np.float32)
    e2 = rng.standard_normal((3, H)).astype(np.float32)
    for x in (e1, e2):
        x[0] = 0.0
        x[1] *= np.float32(1e-20)
        x[2] *= np.float32(1e15)
    plain, rsum, rout, asum, aout = _rmsnorm_f32_calls(e1, e2, w, eps)
    rr, ro = O.residual_rmsnorm(e1, e2, w, eps, fp16=0)
    edge_ulp = np.maximum(ulps32(plain, O.rmsnorm(e1, w, eps, fp16=0)), ulps32(rout, ro)).max(axis=1)
    report("rmsnorm_f32_shapes", H=H, random_rows_exact_share=share,
           edge_rows_max_ulp=[int(u) for u in edge_ulp])
    assert np.all(edge_ulp <= 1), edge_ulp
    assert np.array_equal(rsum.view(np.uint32), rr.view(np.uint32))
    for o in (plain, rout):
        assert np.isfinite(o).all()
        assert np.all(o[0] == 0.0)
    assert np.array_equal(asum.view(np.uint32), rsum.view(np.uint32))
    assert np.array_equal(aout.view(np.uint32), rout.view(np.uint32))
    assert share >= 0.99, share


# a: 0, -0, +-1, +-20, +-80 (<= 4 ulp), then +-1e4 (saturated: exact)
SILU_PLANTED = np.array([0.0, -0.0, 1.0, -1.0, 20.0, -20.0, 80.0, -80.0, 1e4, -1e4], np.float32)


def _silu_mul_f32_case(n, rng):
    """one ffmi_silu_mul_f32 call on random inputs as in
    test_silu_mul_f32_against_oracle, SILU_PLANTED written over the first and
    the last 10 values of a where n allows; the planted values are checked
    here, returns the ulp distances of the random ones"""
    a = (4 * rng.standard_normal(n)).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    planted = np.zeros(n, bool)
    if n >= 2 * len(SILU_PLANTED):
        a[:10], a[-10:] = SILU_PLANTED, SILU_PLANTED
        planted[:10] = planted[-10:] = True
    ba, bb, bo = Buf(a), Buf(b), Buf.empty((n,), np.float32)
    assert F.lib().ffmi_silu_mul_f32(ba.ptr, bb.ptr, bo.ptr, n, None) == 0
    got, ref = bo.get(), O.silu_mul(a, b, fp16=0)
    d = ulps32(got, ref)
    sat = planted & (np.abs(a) == np.float32(1e4))
    assert np.isfinite(got[planted]).all()
    assert np.array_equal(got[sat], ref[sat]), (got[sat], ref[sat])  # (-0 == 0)
    # a = 1e4: sigmoid 1, out = a * b; a = -1e4: sigmoid 0, out = +-0
    assert np.array_equal(got[sat & (a > 0)], (a * b)[sat & (a > 0)])
    assert np.all(got[sat & (a < 0)] == 0.0)
    rest = planted & ~sat
    assert d[rest].max(initial=0) <= 4, d[rest]
    return d[~planted]


def test_silu_mul_f32_short_lengths():
    """ffmi_silu_mul_f32 at n 1, 255 and 257 (one thread, a ragged block, one
    thread of a second block) with planted a = 0, -0, +-1, +-20, +-80 (<= 4
    ulp) and +-1e4 (saturated sigmoid: out = a * b or +-0, equal to the
    oracle with -0 counted equal to 0).  Random values: <= 4 ulp; >= 90%
    bit-identical, taken over the random values of the three lengths
    together (a share of one value says nothing)."""
    rng = np.random.default_rng(4400 + OFF)
    d = np.concatenate([_silu_mul_f32_case(n, rng) for n in (1, 255, 257)])
    report("silu_mul_f32_short_lengths", max_ulp=int(d.max()), exact_share=float((d == 0).mean()))
    assert d.max() <= 4 and (d == 0).mean() >= 0.9, (int(d.max()), float((d == 0).mean()))


def test_silu_mul_f32_grid_stride():
    """n = 65536 * 256 + 3: past the launch's 65536-block cap, so the first
    three threads take a second trip of the grid-stride loop; the planted
    values sit in the first block and in the second trip.  Bars as
    test_silu_mul_f32_against_oracle: <= 4 ulp, >= 90% bit-identical."""
    n = 65536 * 256 + 3
    d = _silu_mul_f32_case(n, np.random.default_rng(4401 + OFF))
    report("silu_mul_f32_grid_stride", n=n, max_ulp=int(d.max()),
           exact_share=float((d == 0).mean()))
    assert d.max() <= 4 and (d == 0).mean() >= 0.9, (int(d.max()), float((d == 0).mean()))


def _topk_f32(z, k):
    """(GPU ids, GPU probs, oracle ids, oracle probs) of ffmi_arg_topk_f32"""
    z = np.ascontiguousarray(z, np.float32)
    T, V = z.shape
    bz, bi, bp = Buf(z), Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
    assert F.lib().ffmi_arg_topk_f32(bz.ptr, T, V, k, bi.ptr, bp.ptr, None) == 0
    ids, probs = O.softmax_topk(z, k, fp16=0)
    return bi.get(), bp.get(), ids, probs


@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 32001])
def test_arg_topk_f32_shape_sweep(V):
    """ffmi_arg_topk_f32 at V below, at and off the wave (64) and the 1024
    threads (idle threads, k == V, a ragged second trip), every k <= min(4, V),
    T 1 and 7, random-normal rows scaled by 3: ids exact, probabilities <= 2
    ulp against the oracle's fp32 mode"""
    rng = np.random.default_rng(5200 + OFF + V)
    worst = 0
    for T in (1, 7):
        z = (3 * rng.standard_normal((T, V))).astype(np.float32)
        for k in range(1, min(4, V) + 1):
            gi, gp, ids, probs = _topk_f32(z, k)
            assert np.array_equal(gi, ids), (T, k, gi, ids)
            u = int(ulps32(gp, probs).max())
            worst = max(worst, u)
            assert u <= 2, (T, k, u)
    report("arg_topk_f32_shape_sweep", V=V, max_prob_ulp=worst)


@pytest.mark.parametrize("V", [5, 1000, 32001])
def test_arg_topk_f32_degenerate_rows(V):
    """k = 4 on rows whose order the probabilities do not decide: all logits
    equal (ids 0..3); one logit 200 above the rest at index 0, mid-row and
    V - 1 (every runner-up has probability exactly 0: the lowest remaining
    indices); some, not all, entries -inf (half of a row, and all but two);
    rows offset by +1e4 (fp32 spacing ~1e-3: many tied logits) and -1e4.  Ids
    exact, probabilities <= 2 ulp against the oracle's fp32 mode."""
    rng = np.random.default_rng(5300 + OFF + V)
    k = 4
    base = (3 * rng.standard_normal((9, V))).astype(np.float32)
    z = base.copy()
    z[0] = np.float32(0.37)
    peaks = [0, V // 2, V - 1]
    for r, j in zip((1, 2, 3), peaks):
        z[r, j] = z[r].max() + np.float32(200.0)
    z[4, rng.permutation(V)[:V // 2]] = -np.inf
    z[5, rng.permutation(V)[:V - 2]] = -np.inf
    z[6] += np.float32(1e4)
    z[7] -= np.float32(1e4)
    z[8] = np.float32(-1e4)  # all equal again, far from 0
    gi, gp, ids, probs = _topk_f32(z, k)
    assert np.array_equal(ids[0], np.arange(k)) and np.array_equal(ids[8], np.arange(k))
    for r, j in zip((1, 2, 3), peaks):
        assert ids[r].tolist() == [j] + [i for i in range(k + 1) if i != j][:k - 1]
        assert np.all(probs[r, 1:] == 0.0)
    assert np.all(probs[5, 2:] == 0.0) and np.all(probs[5, :2] > 0.0)
    assert np.array_equal(gi, ids), (gi, ids)
    u = ulps32(gp, probs)
    report("arg_topk_f32_degenerate_rows", V=V, max_prob_ulp=int(u.max()))
    assert u.max() <= 2, u


def _flat_rows(c, w, V, seed):
    u = np.random.default_rng(seed).uniform(-1.0, 0.0, (64, V))
    return (c + u * w).astype(np.float32)


def _sensitive_rows(z, ids, probs):
    """rows whose oracle top-k holds two distinct logits with the same fp32
    probability: there the index rule decides between unequal logits, and one
    ulp of expf changes the ids"""
    n = 0
    for t in range(z.shape[0]):
        zt, pt = z[t, ids[t]], probs[t]
        n += any(pt[i] == pt[j] and zt[i] != zt[j]
                 for i in range(len(zt)) for j in range(i + 1, len(zt)))
    return n


# (c, w, V) whose oracle rows must be sensitive on at least a quarter of the rows
FLAT_SENSITIVE = {(0.7, 1e-5, 1000), (0.7, 1e-3, 32000)}


@pytest.mark.parametrize("V", [1000, 32000])
@pytest.mark.parametrize("w", [1e-5, 1e-3])
@pytest.mark.parametrize("c", [0.7, 0.05])
def test_arg_topk_f32_flat_rows(c, w, V):
    """Flat rows, z = float32(c + u * w) with u uniform in [-1, 0), T = 64,
    k = 4: every term of the softmax is expf of a value within w of 0, where
    a device expf one ulp off the host's moves a probability across a tie and
    reorders the ids (the fp16 top-k's round-5 finding).  Ids exact,
    probabilities <= 2 ulp against the oracle's fp32 mode.  Guard against a
    vacuous run: at (0.7, 1e-5, 1000) and (0.7, 1e-3, 32000) at least a
    quarter of the oracle's own rows must be sensitive (_sensitive_rows; 26
    and 38 of 64 at the default seed, 64 of 64 at c = 0.05, w = 1e-5)."""
    z = _flat_rows(c, w, V, 1 + OFF)
    gi, gp, ids, probs = _topk_f32(z, 4)
    sens = _sensitive_rows(z, ids, probs)
    rows_off = int((gi != ids).any(axis=1).sum())
    u = ulps32(gp, probs)
    report("arg_topk_f32_flat_rows", c=c, w=w, V=V, sensitive_rows=sens, rows_with_other_ids=rows_off,
           max_prob_ulp=int(u.max()), probs_exact_share=float((u == 0).mean()))
    if (c, w, V) in FLAT_SENSITIVE:
        assert sens >= 16, sens
    assert rows_off == 0, (rows_off, sens)
    assert u.max() <= 2, int(u.max())


def oracle_greedy(om, prompts, n_new):
    """the fp32 oracle's own greedy continuation of every prompt (BOS
    included), batched: the prompts in one multi-request step, then one
    decode step per token; returns (sequences, logits rows [B][n_new][V])"""
    B = len(prompts)
    counts = [len(p) for p in prompts]
    lg = om.forward_multi(list(range(B)), counts, [0] * B, np.concatenate(prompts))
    last = lg[np.cumsum(counts) - 1]
    seqs = [list(p) for p in prompts]
    rows = []
    for step in range(n_new):
        ids, _ = O.softmax_argmax(last, fp16=0)
        rows.append(last)
        for s, i in zip(seqs, ids):
            s.append(int(i))
        if step + 1 < n_new:
            last = om.decode_batch(list(range(B)), [s[-1] for s in seqs],
                                   [len(s) - 1 for s in seqs])
    return seqs, np.stack(rows, 1)


def compare(gpu, ref, rows, n_prompts):
    """per sequence: identical, or the first divergence an fp32 tie of the
    oracle row there; returns (identical count, divergences)"""
    same, div = 0, []
    for b, (g, r) in enumerate(zip(gpu, ref)):
        if list(g) == list(r):
            same += 1
            continue
        t = next(i for i in range(min(len(g), len(r))) if g[i] != r[i])
        row = rows[b][t - n_prompts[b]]
        gap = float(row[r[t]] - row[g[t]])
        div.append(dict(seq=b, pos=t - n_prompts[b], gpu=int(g[t]), oracle=int(r[t]), gap=gap))
        assert gap <= FP32_TIE, div[-1]
    return same, div


def run(cfg, ps, max_length, spec, B, mtb=256, seq=256):
    """spec: False (incr decoding), True / a tests/spec_configs.py name"""
    kw = dict(max_requests=B, max_seq_len=seq, full_precision=True)
    if spec:
        rm, ssms, vt, tt = spec_setup("w113" if spec is True else spec, LLAMA_68M, B, mtb, seq,
                                      full_precision=True)
        llm = fa.Model(cfg, "tree", max_tokens=vt, max_tree_tokens=tt, weight_seed=SEED, **kw)
        res = fa.generate(rm, llm, ps, max_length=max_length, spec=True)
        for m in ssms:
            m.close()
    else:
        llm = fa.Model(cfg, "inc", max_tokens=mtb, weight_seed=SEED, **kw)
        rm = fa.RequestManager(max_requests_per_batch=B, max_tokens_per_batch=mtb,
                               max_sequence_length=seq)
        res = fa.generate(rm, llm, ps, max_length=max_length)
    llm.close()
    return [r.output_tokens for r in res], rm.stats().llm_steps


def prompts(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, 32000, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


def test_full_precision_2layer_teacher_forced_logits():
    """2 layers at LLaMA-7B widths: one prefill step over 4 prompts, logits
    against the fp32 oracle within 1e-4 (the HF-alignment tolerance the oracle
    itself meets against transformers, test_oracle_golden.py)"""
    cfg = dict(LLAMA_7B, num_layers=2)
    ps = [[1] + p for p in prompts(4, 33, 34, 3)]  # equal lengths: the prefill is the last step
    m = fa.Model(cfg, "inc", max_requests=4, max_tokens=256, max_seq_len=256, weight_seed=SEED,
                 full_precision=True)
    m.set_debug(True)
    fa.generate(fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=256,
                                  max_sequence_length=256), m, [p[1:] for p in ps],
                max_length=max(map(len, ps)) + 1)
    lg = m.debug_tensor("logits")
    m.close()
    om = O.Model(cfg, SEED, fp16=0, max_requests=4, max_seq=256)
    ref = om.forward_multi([0, 1, 2, 3], [len(p) for p in ps], [0] * 4, np.concatenate(ps))
    assert lg.shape == ref.shape
    err = np.abs(lg - ref)
    report("full_precision_2L_logits", max_abs_err=float(err.max()),
           logit_std=float(ref.std()), rows=int(ref.shape[0]))
    assert err.max() <= 1e-4, float(err.max())


@pytest.fixture(scope="module")
def bench_7b():
    """LLaMA-7B, 32 layers, fp32 (27 GB on the GPU and on the host oracle):
    8 prompts, 40 new tokens, incr decoding and SpecInfer with the fp32 68M SSM"""
    ps = prompts(8, 8, 24, 77)
    n_prompts = [len(p) + 1 for p in ps]
    NEW = 40
    max_length = max(n_prompts) + NEW
    incr, incr_steps = run(LLAMA_7B, ps, max_length, False, 8)
    spec, spec_steps = {}, {}
    for name in SPEC:  # (1,1,3), tree width 4, 4 SSMs
        spec[name], spec_steps[name] = run(LLAMA_7B, ps, max_length, name, 8)
    om = O.Model(LLAMA_7B, SEED, fp16=0, max_requests=8, max_seq=2 * max_length)
    # every request continues to max_length: the oracle runs the longest
    # continuation for all and the comparison uses each sequence's length
    ref, rows = oracle_greedy(om, [[1] + p for p in ps], max_length - min(n_prompts))
    ref = [r[:max_length] for r in ref]
    return dict(ps=ps, n_prompts=n_prompts, incr=incr, spec=spec, ref=ref, rows=rows,
                incr_steps=incr_steps, spec_steps=spec_steps)


def test_full_precision_7b_incr_equals_oracle(bench_7b):
    """the reference's bar (cpp_inference_tests.sh:104-129: first 30 tokens
    identical) on the 32-layer bench model: every token of every request"""
    b = bench_7b
    same, div = compare(b["incr"], b["ref"], b["rows"], b["n_prompts"])
    report("full_precision_7b_32L_incr_vs_oracle", identical=same, requests=len(b["ps"]),
           divergences=div, tokens=sum(len(s) - n for s, n in zip(b["incr"], b["n_prompts"])))
    assert same + len(div) == len(b["ps"])


@pytest.mark.parametrize("spec", list(SPEC))
def test_full_precision_7b_spec_equals_incr(bench_7b, spec):
    """SpecInfer == incremental decoding (cpp_inference_tests.sh:183-189), with
    widths (1,1,3), tree width 4 and 4 SSMs"""
    b = bench_7b
    same = sum(a == c for a, c in zip(b["spec"][spec], b["incr"]))
    report(f"full_precision_7b_32L_spec_vs_incr_{spec}", identical=same, requests=len(b["ps"]),
           incr_steps=b["incr_steps"], spec_steps=b["spec_steps"][spec])
    if same < len(b["ps"]):  # only at an fp32 tie of the oracle's row
        compare(b["spec"][spec], b["ref"], b["rows"], b["n_prompts"])


def test_full_precision_tp8_processes_equal_tp1():
    """TP = 8 (8 rank processes, o / down all-reduced in fp32 over the xGMI
    transport) against TP = 1, incremental decoding and SpecInfer: the
    reference's TP-invariance diff (cpp_inference_tests.sh:203-217)"""
    ps = prompts(3, 8, 16, 5)
    max_length = max(map(len, ps)) + 1 + 32
    out = {}
    for spec in (False, True):
        g = run_group(8, PT.tp_generate_f32_task, (LLAMA_7B, SEED, ps, max_length, spec, LLAMA_68M),
                      max_bytes=(256 + 23 * 3 + 16) * 4096 * 4, timeout=900)
        for r in range(8):
            assert g[r]["tokens"] == g[0]["tokens"], r
        one, _ = run(LLAMA_7B, ps, max_length, spec, 3, seq=128)  # the ranks' cache size
        out[spec] = (g[0]["tokens"], one)
    same = {("spec" if k else "incr"): sum(a == b for a, b in zip(*v)) for k, v in out.items()}
    report("full_precision_7b_tp8_vs_tp1", requests=len(ps), **same)
    assert out[False][0] == out[False][1], same
    assert out[True][0] == out[True][1], same


def test_full_precision_negative_control_rope_fault():
    """The literal fp32 bars must FAIL a real bug: 4 layers at LLaMA-7B widths,
    4 prompts, 16 new tokens.  Clean: every token equals the fp32 oracle's
    greedy decode.  Layer 2's RoPE one position off for decode tokens
    (ffmi_model_debug_fault FFMI_FAULT_ROPE_POS on the DT_FLOAT handles): at
    least one request must leave the oracle's sequence at a pick whose oracle
    logit gap is far beyond an fp32 tie (FP32_TIE)."""
    cfg = dict(LLAMA_7B, num_layers=4)
    ps = prompts(4, 16, 17, 31)
    n_prompt = 17  # with BOS
    NEW = 16
    m = fa.Model(cfg, "inc", max_requests=4, max_tokens=256, max_seq_len=128, weight_seed=SEED,
                 full_precision=True)
    runs = {}
    for fault in (False, True):
        m.debug_fault(F.FAULT_ROPE_POS if fault else F.FAULT_NONE, 2, n_prompt)
        res = fa.generate(fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=256,
                                            max_sequence_length=128), m, ps,
                          max_length=n_prompt + NEW)
        runs[fault] = [r.output_tokens for r in res]
    m.debug_fault(F.FAULT_NONE)
    m.close()
    om = O.Model(cfg, SEED, fp16=0, max_requests=4, max_seq=128)
    ref, rows = oracle_greedy(om, [[1] + p for p in ps], NEW)
    same, div = compare(runs[False], ref, rows, [n_prompt] * 4)
    gaps = []
    for b, (g, r) in enumerate(zip(runs[True], ref)):
        if list(g) != list(r):
            t = next(i for i in range(len(g)) if g[i] != r[i])
            row = rows[b][t - n_prompt]
            gaps.append(float(row[r[t]] - row[g[t]]))
    report("full_precision_negative_control_rope_layer2", clean_identical=same,
           clean_divergences=div, faulted_divergence_gaps=gaps)
    assert same == 4, div
    assert gaps and max(gaps) > 100 * FP32_TIE, ("fault NOT detected", gaps)
