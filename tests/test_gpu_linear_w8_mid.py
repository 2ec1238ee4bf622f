"""The M-split fp8-weight GEMM (kernels/gemm_w8_mid.hip: 65 .. 256 rows in one
weight pass) at its edges, with the inputs and bars of tests/test_gpu_linear_w8.py:
against float64 over the unpacked bytes, and bit-equal to the multi-pass route
and to every row run alone.  Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
from hip_util import Buf, f16
from test_gpu_kernels import close16
from test_gpu_linear_w8 import GUARD, NBIG, Case

pytestmark = pytest.mark.gpu
W = F.W_STREAM
# T: one live row in the second wave; the MTW 2 -> 3 and 3 -> 4 boundaries; the
# verify step; the launch boundary with a one-row last pass.  N: one tile, a
# padded tile, a full column group and a ragged one.  K: one double step (shorter
# than the ring), two, 576 (S = 2: slices of 5 and 4 steps), 4096 (S = 8).
CASES = [(65, 16, 576, W), (65, NBIG, 64, 0), (128, 40, 576, W), (129, NBIG, 576, 0),
         (129, 16, 128, W), (168, NBIG, 4096, W), (192, NBIG, 576, W), (192, 40, 64, 0),
         (193, 40, 576, W), (256, 16, 576, W), (256, NBIG, 4096, 0), (257, NBIG, 576, W),
         (257, 40, 128, 0)]


def run(c, X, stream, onepass):
    """ffmi_linear_w8 with the one-pass or the minimum workspace, guard words
    before X, after Y and after the workspace"""
    L, (T, K), N = F.lib(), X.shape, c.N
    epi = (F.EPI_SILU_MUL if c.silu else F.EPI_NONE) | stream
    size = L.ffmi_linear_w8_onepass_workspace_bytes if onepass else L.ffmi_linear_w8_workspace_bytes
    nws = size(T, N, K, epi)
    xg = np.full(GUARD + X.size, 0x5a5a, np.uint16)
    xg[GUARD:] = X.view(np.uint16).ravel()
    xb, yb = Buf(xg), Buf(np.full(T * N + GUARD, 0x5a5a, np.uint16))
    wb = Buf(np.full(nws // 4 + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(L.ffmi_linear_w8(ctypes.c_void_p(xb.ptr.value + 2 * GUARD), c.wp.ptr, c.sc.ptr, yb.ptr,
                             T, N, K, epi, wb.ptr, nws, None))
    y = yb.get()
    assert (y[T * N:] == 0x5a5a).all() and (wb.get()[nws // 4:] == 0x5a5a5a5a).all()
    assert np.array_equal(xb.get(), xg)
    return y[:T * N].reshape(T, N)  # (uint16)


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("T,N,K,stream", CASES)
def test_linear_w8_mid_against_float64_the_multi_pass_route_and_rows_alone(T, N, K, stream, silu):
    L, epi, plan = F.lib(), F.EPI_SILU_MUL if silu else F.EPI_NONE, (ctypes.c_int * 6)()
    need = L.ffmi_linear_w8_onepass_workspace_bytes(T, N, K, epi)
    F.check(L.ffmi_debug_linear_w8_plan(T, N, K, epi, need, plan))
    mtw = {65: 2, 128: 2, 129: 3, 168: 3, 192: 3, 193: 4, 256: 4, 257: 4}[T]
    S = 1 if silu else {64: 1, 128: 1, 576: 2, 4096: 8}[K]
    assert list(plan)[:5] == [1, mtw, 8, S, 1 + (T > 256)] and (need > 0) == (S > 1)
    c = Case(N, K, silu)
    X = f16(np.random.default_rng([T, N, K]).standard_normal((T, K)))
    y = run(c, X, stream, True)
    bar = dict(max_ulp=3, atol=1e-3) if silu else dict(max_ulp=2)  # (tests/test_gpu_linear_w8.py)
    close16(y.view(np.float16), c.ref(X), exact_frac=0.0, **bar)
    assert np.array_equal(y, run(c, X, stream, False))
    for t in (0, 63, 64, T - 1):
        assert np.array_equal(y[t], run(c, X[t:t + 1], stream, True)[0]), t
