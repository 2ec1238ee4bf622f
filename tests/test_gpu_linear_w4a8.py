"""W4A8 at the kernel level (kernels/gemm_w4a8.hip) against float64 over the
unpacked nibbles, scale bytes and e4m3 bytes: the weights of
tests/test_gpu_linear_w4.py (its planted row keeps e = -8 and e = -12 in
neighbouring blocks), the rows of tests/test_gpu_linear_w8a8.py, every checked
row also run alone.  The bar is the project's bare one (close16: 2 ulp, SiLU-mul
3 ulp or 1e-3), no accumulation allowance.  Measured over CASES: 95.8 to 99.2 %
of the outputs exact, at most 0.3 % beyond the ulp count, all of those inside
close16's absolute term.  Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
from hip_util import Buf, f16, ulp_diff
from test_gpu_kernels import close16
from test_gpu_kv_fp8 import dequantise
from test_gpu_linear_w4 import GUARD, NBIG, SPLITS, Case
from test_gpu_linear_w8a8 import block_order, dev_rows, rows

pytestmark = pytest.mark.gpu
W = F.W_STREAM


def linear_w4a8(c, x8, a, stream):
    """ffmi_linear_w4a8 with guard words before X8, after Y and after the workspace"""
    L, (T, K), N = F.lib(), x8.shape, c.N
    epi = (F.EPI_SILU_MUL if c.silu else F.EPI_NONE) | stream
    nws = L.ffmi_linear_w4a8_workspace_bytes(T, N, K, epi)
    S = 1 if c.silu else SPLITS.get(K, 1)
    assert nws == (S * min(T, 256) * ((N + 15) // 16) * 16 * 4 if S > 1 else 0)
    xg = np.concatenate([np.full(GUARD, 0x5a, np.uint8), x8.ravel()])
    xb, ab, yb = Buf(xg), Buf(np.ascontiguousarray(a)), Buf(np.full(T * N + GUARD, 0x5a5a, np.uint16))
    wb = Buf(np.full(nws // 4 + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(L.ffmi_linear_w4a8(ctypes.c_void_p(xb.ptr.value + GUARD), ab.ptr, c.wp.ptr, c.sc.ptr, yb.ptr,
                               T, N, K, epi, wb.ptr, nws, None))
    y = yb.get()
    assert (y[T * N:] == 0x5a5a).all() and (wb.get()[nws // 4:] == 0x5a5a5a5a).all()
    assert np.array_equal(xb.get(), xg)
    return y[:T * N].reshape(T, N)  # (uint16)


# T: one row; the last T of the tile split (with a padded tile); the first of the
# row split; every MTW boundary; the verify size; a one-row second pass.  K: one
# quad step (shorter than any ring), two, 1408 (S = 4: 3 3 3 2 steps), 4096 (S = 8)
CASES = [(1, 16, 128, 0), (16, 40, 256, W), (17, NBIG, 1408, 0), (64, NBIG, 4096, W), (65, 16, 1408, 0),
         (129, NBIG, 128, W), (168, NBIG, 4096, 0), (193, 40, 128, W), (256, NBIG, 4096, 0),
         (257, 40, 256, W)]


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("T,N,K,stream", CASES)
def test_linear_w4a8_against_float64_and_rows_alone(T, N, K, stream, silu):
    c = Case(N, K, silu)
    x8, a = dev_rows(rows(T, K))
    y = linear_w4a8(c, x8, a, stream)
    xd = a.astype(np.float64)[:, None] * dequantise(block_order(x8, inverse=True), 1.0)
    ref, y16 = c.ref(xd), y.view(np.float16)
    ulps, d = 3 if silu else 2, ulp_diff(y16, f16(ref))
    print(f"T={T} N={N} K={K} silu={silu}: exact {(d == 0).mean():.4f}, {(d > ulps).sum()} of {ref.size} "
          f"beyond {ulps} ulp")
    close16(y16, ref, max_ulp=ulps, exact_frac=0.0, atol=1e-3 if silu else None)
    for t in sorted({t for t in (0, 15, 16, 63, 64) if t < T} | {T - 1}):
        assert np.array_equal(y[t], linear_w4a8(c, x8[t:t + 1], a[t:t + 1], stream)[0]), t
