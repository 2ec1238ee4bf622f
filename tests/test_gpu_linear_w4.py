"""OCP MXFP4 weight-only linear layers at the kernel level (kernels/gemm_w4.hip):
the quantiser and the packed layout against a numpy statement of the rule of
include/ffmi.h, the GEMM against float64 over the unpacked nibbles and scale
bytes, and row independence.  Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
from hip_util import Buf, f16, ulp_diff
from test_gpu_kernels import close16

pytestmark = pytest.mark.gpu

NBIG = 4 * 2 * 16 + 16      # one full workgroup (4 waves x 2 tiles) and a ragged one
GUARD = 64                  # guard elements around the GEMM's buffers
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32)
# v of the planted block: saturation (6, 7), every tie, one value that is no tie, -0.0
PLANTED = np.array([6, -6, 7, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, 5.5, -0.0], np.float32)
PLANTED_NIB = [7, 15, 7, 0, 2, 2, 4, 4, 6, 6, 7, 8]
SPLITS = {4096: 8, 1408: 4}  # K -> k-slices at these N without SiLU-mul (1408: 11 quad steps as 3 3 3 2)


def weights(seed, N, K):
    """N(0, 1 / K) (unit-variance sums against x ~ N(0, 1): test_gpu_linear_w8.py
    on why), row 0 all zero; in row 1 (N > 1) block 0 = PLANTED * 2^-8 (amax
    7 * 2^-8, e = -8) and block 1 with amax 2^-20 (e = -12, every code 0)."""
    rng = np.random.default_rng([seed, N, K])
    W = f16(rng.standard_normal((N, K)) / np.sqrt(K))
    W[0] = 0
    if N > 1:
        W[1, :32] = 0
        W[1, :len(PLANTED)] = (PLANTED * 2.0**-8).astype(np.float16)
        W[1, 32:64] = f16(rng.integers(-16, 17, 32) * 2.0**-24)
        W[1, 40] = 2.0**-20
    return W


def host_quant(W):
    """(nibbles [N][K], scale bytes [N][K / 32]) of fp16 W by the rule of include/ffmi.h"""
    N, K = W.shape
    w = W.astype(np.float32).reshape(N, K // 32, 32)
    amax = np.abs(w).max(-1)
    e = np.where(amax > 0, np.maximum(np.frexp(amax)[1] - 1 - 2, -12), 0).astype(np.int32)
    v = np.abs(np.ldexp(w, -e[..., None])).reshape(N, K)
    lo = np.clip(np.searchsorted(GRID, v, side="right") - 1, 0, 7)
    hi = np.minimum(lo + 1, 7)
    dl, dh = v - GRID[lo], GRID[hi] - v
    code = np.where((dl < dh) | (hi == lo), lo, np.where(dl > dh, hi, np.where(lo % 2 == 0, lo, hi)))
    return ((W.view(np.uint16) >> 15) << 3 | code).astype(np.uint8), (e + 127).astype(np.uint8)


def dequantise(nib, sc):
    """float64 [N][K] of nibbles and scale bytes"""
    mag = GRID[nib & 7].astype(np.float64) * np.repeat(np.ldexp(1.0, sc.astype(np.int32) - 127), 32, axis=1)
    return np.where(nib & 8, -mag, mag)


def dev_pack(W, Wu=None):
    """quantize_pack (gate/up with Wu) -> (nibbles Buf, scale bytes Buf)"""
    L, (N, K), g = F.lib(), W.shape, 1 if Wu is None else 2
    wp = Buf.empty((g * L.ffmi_linear_w4_packed_bytes(N, K),), np.uint8)
    sc = Buf.empty((g * L.ffmi_linear_w4_scale_bytes(N, K),), np.uint8)
    a, b = Buf(W), Buf(Wu) if Wu is not None else None
    if Wu is None:
        F.check(L.ffmi_linear_w4_quantize_pack(a.ptr, N, K, wp.ptr, sc.ptr, None))
    else:
        F.check(L.ffmi_linear_w4_quantize_pack_gate_up(a.ptr, b.ptr, N, K, wp.ptr, sc.ptr, None))
    sc.get()  # (synchronises before the sources are freed)
    return wp, sc


def unpack(wp, sc, N, K, gate_up=0):
    nib, s = Buf.empty((N, K), np.uint8), Buf.empty((N, K // 32), np.uint8)
    F.check(F.lib().ffmi_debug_linear_w4_unpack(wp.ptr, sc.ptr, N, K, gate_up, nib.ptr, s.ptr, None))
    return nib.get(), s.get()


@pytest.mark.parametrize("N,K", [(16, 128), (40, 256), (96, 384)])
def test_quantize_pack_nibbles_scales_and_gate_up_interleave(N, K):
    W, Wu = weights(1, N, K), weights(2, N, K)
    (q, s), (qu, su) = host_quant(W), host_quant(Wu)
    assert (s[0] == 127).all() and (q[0] == 0).all()
    assert s[1, 0] == 127 - 8 and q[1, :len(PLANTED)].tolist() == PLANTED_NIB
    assert s[1, 1] == 127 - 12 and not (q[1, 32:64] & 7).any()
    wp, sc = dev_pack(W)
    for got, want in zip(unpack(wp, sc, N, K), (q, s)):
        assert np.array_equal(got, want)
    pad = sc.get().reshape(K // 128, -1, 16, 4)[:, -1, N % 16 or 16:]  # the last tile's padding rows
    assert (pad == 127).all() and not (sc.get() == 0xff).any()
    wp, sc = dev_pack(W, Wu)
    for g, want in ((1, (q, s)), (2, (qu, su))):
        got = unpack(wp, sc, N, K, g)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def linear_w4(X, wp, sc, N, epi):
    """ffmi_linear_w4 with guard patterns before X, after Y and after the workspace"""
    L, (T, K) = F.lib(), X.shape
    xg = np.full(GUARD + X.size, 0x5a5a, np.uint16)
    xg[GUARD:] = X.view(np.uint16).ravel()
    nws = L.ffmi_linear_w4_workspace_bytes(T, N, K, epi)
    xb, yb = Buf(xg), Buf(np.full(T * N + GUARD, 0x5a5a, np.uint16))
    wb = Buf(np.full(nws // 4 + GUARD, 0x5a5a5a5a, np.uint32))
    F.check(L.ffmi_linear_w4(ctypes.c_void_p(xb.ptr.value + 2 * GUARD), wp.ptr, sc.ptr, yb.ptr, T, N,
                             K, epi, wb.ptr, nws, None))
    y, w = yb.get(), wb.get()
    assert (y[T * N:] == 0x5a5a).all() and (w[nws // 4:] == 0x5a5a5a5a).all()
    assert np.array_equal(xb.get(), xg)
    return y[:T * N].view(np.float16).reshape(T, N)


class Case:
    """weights, their device form and the float64 sums over the unpacked device bytes"""

    def __init__(self, N, K, silu):
        self.N, self.K, self.silu = N, K, silu
        W, Wu = weights(3, N, K), weights(4, N, K) if silu else None
        self.wp, self.sc = dev_pack(W, Wu)
        self.deq = [dequantise(*unpack(self.wp, self.sc, N, K, g)) for g in ((1, 2) if silu else (0,))]

    def ref(self, X):
        y = [f16(X.astype(np.float64) @ d.T) for d in self.deq]
        return O.silu_mul(y[0], y[1]) if self.silu else y[0]

    def run(self, X, stream=0):
        return linear_w4(X, self.wp, self.sc, self.N, (F.EPI_SILU_MUL if self.silu else F.EPI_NONE) | stream)


# one row; a partial m-tile; three m-tiles; one pass exactly; a pass boundary with
# a ragged last pass -- over one tile, a padded tile and a ragged last workgroup,
# K of one quad step (prologue predicate, ring drain), two steps, 4096 (S = 8 of 4
# steps, shorter than the ring) and 1408 (slices of 3 3 3 2 steps)
GEMM = [(1, 16, 128, 0), (8, 40, 256, F.W_STREAM), (17, NBIG, 4096, 0), (64, NBIG, 4096, F.W_STREAM),
        (65, 40, 1408, 0), (168, NBIG, 128, F.W_STREAM), (168, 16, 4096, 0), (33, NBIG, 1408, F.W_STREAM)]


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("T,N,K,stream", GEMM)
def test_linear_w4_against_float64(T, N, K, stream, silu):
    L = F.lib()
    S = 1 if silu else SPLITS.get(K, 1)  # the plan splits K where the cases say it does
    tiles = (2 if silu else 1) * ((N + 15) // 16)
    ws = L.ffmi_linear_w4_workspace_bytes(T, N, K, F.EPI_SILU_MUL if silu else F.EPI_NONE)
    assert ws == (S * min(T, 64) * tiles * 16 * 4 if S > 1 else 0)
    c = Case(N, K, silu)
    X = f16(np.random.default_rng([T, N, K]).standard_normal((T, K)))
    y, ref = c.run(X, stream), c.ref(X)
    print(f"T={T} N={N} K={K} silu={silu}: exact {(ulp_diff(y, f16(ref)) == 0).mean():.4f}")
    if silu:
        close16(y, ref, max_ulp=3, exact_frac=0.0, atol=1e-3)
    else:
        close16(y, ref, max_ulp=2, exact_frac=0.0)


@pytest.mark.parametrize("silu", [False, True], ids=["none", "silu_mul"])
@pytest.mark.parametrize("K", [128, 4096])
def test_linear_w4_rows_do_not_depend_on_the_batch(K, silu):
    c = Case(NBIG, K, silu)
    X = f16(np.random.default_rng(K).standard_normal((168, K)))
    y168 = c.run(X)
    for t in (0, 17, 63, 64, 167):
        alone = c.run(X[t:t + 1])[0].view(np.uint16)
        assert np.array_equal(y168[t].view(np.uint16), alone), t
