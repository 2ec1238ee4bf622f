"""W8A8 at the kernel level (kernels/gemm_w8a8.hip, the quantising norm of
norm.hip): the row quantiser against a numpy restatement bit for bit, the fused
norm against norm-then-quantise, and the fp8-MFMA GEMM against float64 over the
bytes with the inputs and bars of tests/test_gpu_linear_w8.py, every checked row
also run alone.

The GEMM's bar.  Products of two e4m3 values are exact in fp32, but
v_mfma_f32_16x16x32_fp8_fp8 does not sum its 32 products as an fp32 chain does:
on the same operands (a = 1) the f16 instruction of the W8A16 kernel is within
1 ulp of float64 on every output and 99.9 % exact, the fp8 instruction 93 %
exact with 0.5 % of the outputs beyond 2 ulp.  The excess scales with the sum of
the absolute products, B = a[t] s[n] sum_k |x8 q| (through SiLU-mul: 1.1 |up|
B_gate + |silu(gate)| B_up), not with the result: measured over CASES, the worst
(|y - ref| - bar) / B is 2^-17.05 (T 257, N 40, K 128, no epilogue) and 2^-17.27
under SiLU-mul (T 168, N NBIG, K 4096).  So an output passes when it is within
the project's bar (close16: 2 ulp, SiLU-mul 3 ulp or 1e-3) of the float64
reference, or within that bar plus ACCUM * B, ACCUM = 2^-16: the float64
reference plus the measured excess of the instruction, one binade up.
Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
from hip_util import Buf, f16, ulp_diff
from test_gpu_kernels import close16
from test_gpu_kv_fp8 import dequantise, quantise
from test_gpu_linear_w8 import GUARD, NBIG, PLANTED, Case

pytestmark = pytest.mark.gpu
W = F.W_STREAM
ACCUM = 2.0**-16  # the fp8 MFMA's measured accumulation excess per unit of sum |x8 q| (see above)


def block_order(q, inverse=False):
    """[T][K] natural column order <-> X8's: per 64 columns, chunk (hi, g) at 16 g + 8 hi"""
    T, K = q.shape
    shape = (T, K // 64, 4, 2, 8) if inverse else (T, K // 64, 2, 4, 8)
    return np.ascontiguousarray(q.reshape(shape).transpose(0, 1, 3, 2, 4)).reshape(T, K)


def host_rows(X):
    """(X8 [T][K] bytes, a [T] fp32) by the rule of include/ffmi.h"""
    amax = np.abs(X.astype(np.float32)).max(axis=1)
    a = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    return block_order(np.stack([quantise(x.view(np.uint16), s) for x, s in zip(X, a)])), a


def guarded(fn, T, K):
    """fn(X8 pointer, a pointer) -> (X8, a), guard words after both checked"""
    xb = Buf(np.full(T * K + GUARD, 0x5a, np.uint8))
    ab = Buf(np.full(T + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(fn(xb.ptr, ab.ptr))
    x, a = xb.get(), ab.get()
    assert (x[T * K:] == 0x5a).all() and (a[T:] == 0x5a5a5a5a).all()
    return x[:T * K].reshape(T, K), a[:T].view(np.float32)


def dev_rows(X):
    xs = Buf(X)
    return guarded(lambda x8, a: F.lib().ffmi_quantize_rows_fp8(xs.ptr, *X.shape, x8, a, None), *X.shape)


def rows(T, K):
    """row 0: absmax 7, so a = 2^-6 exactly and x / a hits PLANTED; row 1 all zero"""
    rng = np.random.default_rng([T, K])
    X = f16(rng.standard_normal((T, K)))
    X[0] = f16(rng.integers(-200, 200, K) * 2.0**-6)
    X[0, :len(PLANTED)] = (PLANTED * 2.0**-6).astype(np.float16)
    if T > 1:
        X[1] = 0
    return X


@pytest.mark.parametrize("K", [64, 576])
@pytest.mark.parametrize("T", [1, 5])
def test_quantize_rows_and_the_fused_norm_bit_for_bit(T, K):
    L, X = F.lib(), rows(T, K)
    want8, want_a = host_rows(X)
    assert want_a[0] == 2.0**-6 and {0x7e, 0xfe, 0x80} <= set(want8[0].tolist())
    assert T == 1 or want_a[1] == 1
    got8, got_a = dev_rows(X)
    assert np.array_equal(got8, want8) and np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))
    assert not ((got8 & 0x7f) == 0x7f).any()  # the NaN byte is never written
    # the quantising norm == norm, then quantise: on the same rows, plain and residual
    w, x2 = Buf(f16(1 + 0.1 * np.random.default_rng(K).standard_normal(K))), Buf(rows(T + 1, K)[1:])
    x1, res, out = Buf(X), Buf.empty((T, K), np.float16), Buf.empty((T, K), np.float16)
    for second in (None, x2.ptr):
        if second:
            F.check(L.ffmi_residual_rmsnorm(x1.ptr, second, w.ptr, res.ptr, out.ptr, T, K, 1e-6, None))
            want_res = res.get().copy()
        else:
            F.check(L.ffmi_rmsnorm(x1.ptr, w.ptr, out.ptr, T, K, 1e-6, None))
        want8, want_a = host_rows(out.get())
        got8, got_a = guarded(lambda x8, a: L.ffmi_rmsnorm_fp8(
            x1.ptr, second, w.ptr, res.ptr if second else None, x8, a, T, K, 1e-6, None), T, K)
        assert np.array_equal(got8, want8), second
        assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), second
        assert not second or np.array_equal(res.get(), want_res)


def linear_w8a8(c, x8, a, stream):
    """ffmi_linear_w8a8 with guard words before X8, after Y and after the workspace"""
    L, (T, K), N = F.lib(), x8.shape, c.N
    epi = (F.EPI_SILU_MUL if c.silu else F.EPI_NONE) | stream
    nws = L.ffmi_linear_w8a8_workspace_bytes(T, N, K, epi)
    xg = np.concatenate([np.full(GUARD, 0x5a, np.uint8), x8.ravel()])
    xb, ab, yb = Buf(xg), Buf(np.ascontiguousarray(a)), Buf(np.full(T * N + GUARD, 0x5a5a, np.uint16))
    wb = Buf(np.full(nws // 4 + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(L.ffmi_linear_w8a8(ctypes.c_void_p(xb.ptr.value + GUARD), ab.ptr, c.wp.ptr, c.sc.ptr, yb.ptr,
                               T, N, K, epi, wb.ptr, nws, None))
    y = yb.get()
    assert (y[T * N:] == 0x5a5a).all() and (wb.get()[nws // 4:] == 0x5a5a5a5a).all()
    assert np.array_equal(xb.get(), xg)
    return y[:T * N].reshape(T, N)  # (uint16)


# T: one row; a full and a ragged m-tile; every MTW boundary; the verify size; a
# pass boundary with a one-row last pass.  N: one tile, a padded tile, a full and
# a ragged column group.  K: one double step (shorter than any ring), two, 576
# (S = 2: slices of 5 and 4 steps), 4096 (S = 8)
CASES = [(1, 16, 64, 0), (16, 40, 128, W), (17, NBIG, 576, 0), (64, NBIG, 4096, W), (65, 16, 576, 0),
         (129, NBIG, 576, W), (168, NBIG, 4096, 0), (193, 40, 64, W), (256, NBIG, 4096, 0),
         (257, 40, 128, W)]


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("T,N,K,stream", CASES)
def test_linear_w8a8_against_float64_and_rows_alone(T, N, K, stream, silu):
    c = Case(N, K, silu)
    x8, a = dev_rows(rows(T, K))
    y = linear_w8a8(c, x8, a, stream)
    # a[t] * s[n] * (deq(X8) . deq(W8)^T) in float64: Case.ref on the dequantised rows
    xd = a.astype(np.float64)[:, None] * dequantise(block_order(x8, inverse=True), 1.0)
    ref, y16 = c.ref(xd), y.view(np.float16)
    B = [s * (np.abs(xd) @ np.abs(d).T) for d, s in zip(c.deq, c.s)]
    if silu:
        g, u = (s * (xd @ d.T) for d, s in zip(c.deq, c.s))
        B = [1.1 * np.abs(u) * B[0] + np.abs(g / (1 + np.exp(-g))) * B[1]]
    ulps = 3 if silu else 2  # (tests/test_gpu_linear_w8.py)
    err = np.abs(y16.astype(np.float64) - ref)
    within = err <= ulps * np.spacing(np.abs(f16(ref))) + ACCUM * B[0]
    print(f"T={T} N={N} K={K} silu={silu}: exact {(ulp_diff(y16, f16(ref)) == 0).mean():.4f}, "
          f"{(ulp_diff(y16, f16(ref)) > ulps).sum()} of {ref.size} beyond {ulps} ulp")
    # (an output within the accumulation term stands as the reference; the rest by the project's bar)
    close16(np.where(within, ref, y16), ref, max_ulp=ulps, exact_frac=0.0, atol=1e-3 if silu else None)
    for t in sorted({t for t in (0, 15, 16, 63, 64) if t < T} | {T - 1}):
        assert np.array_equal(y[t], linear_w8a8(c, x8[t:t + 1], a[t:t + 1], stream)[0]), t
