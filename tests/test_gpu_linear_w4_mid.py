"""The M-split MXFP4-weight GEMM (kernels/gemm_w4_mid.hip: 65 .. 256 rows in one
weight pass) at its edges, with the inputs and bars of tests/test_gpu_linear_w4.py:
against float64 over the unpacked nibbles and scale bytes, and bit-equal to the
multi-pass route and to every row run alone.  Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
from hip_util import Buf, f16
from test_gpu_kernels import close16
from test_gpu_linear_w4 import GUARD, NBIG, Case

pytestmark = pytest.mark.gpu
W = F.W_STREAM
# T: one live row in the second wave; the MTW 2 -> 3 and 3 -> 4 boundaries; the
# verify step; the launch boundary with a one-row last pass.  N: one tile, a
# padded tile, a full column group and a ragged one.  K: one quad step (shorter
# than any ring), two, 640 (S = 2: slices of 3 and 2 steps), 1408 (S = 4: 3 3 3
# 2), 4096 (S = 8 of 4 steps); with SiLU-mul S = 1, so these K are 1, 2, 5, 11
# and 32 steps of one slice: whole ring turns (4, 3, 2 steps at MTW = 2, 3, 4)
# and every tail length.
CASES = [(65, 16, 640, W), (65, NBIG, 128, 0), (128, 40, 640, W), (128, 16, 1408, W),
         (129, NBIG, 1408, 0), (168, NBIG, 4096, W), (192, NBIG, 640, W), (192, 40, 128, 0),
         (193, 40, 1408, W), (256, 16, 640, W), (256, NBIG, 4096, 0), (257, NBIG, 1408, W),
         (257, 40, 256, 0)]


def run(c, X, stream, onepass):
    """ffmi_linear_w4 with the one-pass or the minimum workspace, guard words
    before X, after Y and after the workspace"""
    L, (T, K), N = F.lib(), X.shape, c.N
    epi = (F.EPI_SILU_MUL if c.silu else F.EPI_NONE) | stream
    size = L.ffmi_linear_w4_onepass_workspace_bytes if onepass else L.ffmi_linear_w4_workspace_bytes
    nws = size(T, N, K, epi)
    xg = np.full(GUARD + X.size, 0x5a5a, np.uint16)
    xg[GUARD:] = X.view(np.uint16).ravel()
    xb, yb = Buf(xg), Buf(np.full(T * N + GUARD, 0x5a5a, np.uint16))
    wb = Buf(np.full(nws // 4 + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(L.ffmi_linear_w4(ctypes.c_void_p(xb.ptr.value + 2 * GUARD), c.wp.ptr, c.sc.ptr, yb.ptr,
                             T, N, K, epi, wb.ptr, nws, None))
    y = yb.get()
    assert (y[T * N:] == 0x5a5a).all() and (wb.get()[nws // 4:] == 0x5a5a5a5a).all()
    assert np.array_equal(xb.get(), xg)
    return y[:T * N].reshape(T, N)  # (uint16)


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("T,N,K,stream", CASES)
def test_linear_w4_mid_against_float64_the_multi_pass_route_and_rows_alone(T, N, K, stream, silu):
    L, epi, plan = F.lib(), F.EPI_SILU_MUL if silu else F.EPI_NONE, (ctypes.c_int * 6)()
    need = L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, epi)
    F.check(L.ffmi_debug_linear_w4_plan(T, N, K, epi, need, plan))
    mtw = {65: 2, 128: 2, 129: 3, 168: 3, 192: 3, 193: 4, 256: 4, 257: 4}[T]
    S = 1 if silu else {128: 1, 256: 1, 640: 2, 1408: 4, 4096: 8}[K]
    assert list(plan)[:5] == [1, mtw, 8, S, 1 + (T > 256)] and (need > 0) == (S > 1)
    c = Case(N, K, silu)
    X = f16(np.random.default_rng([T, N, K]).standard_normal((T, K)))
    y = run(c, X, stream, True)
    bar = dict(max_ulp=3, atol=1e-3) if silu else dict(max_ulp=2)  # (tests/test_gpu_linear_w4.py)
    close16(y.view(np.float16), c.ref(X), exact_frac=0.0, **bar)
    assert np.array_equal(y, run(c, X, stream, False))
    for t in (0, 63, 64, T - 1):
        assert np.array_equal(y[t], run(c, X[t:t + 1], stream, True)[0]), t
