"""Every launch plan of the M-split GEMM (gemm_mid_kernel, 64 < T), not only
the ones the planner picks: 16 tile shapes (MTW row tiles per wave, set by T,
x NTW weight tiles per workgroup) x split-K factors 1-8 x the plain and the
SiLU-mul epilogue, forced through FFMI_GEMM_PLAN (read per call) and
confirmed before every launch through ffmi_debug_gemm_plan, so that a forced
plan the library rejected fails the test.  Shapes: tests/gemm_plan_cases.py.

a. every plan against the oracle, at the bars of
   test_gpu_kernels.py::test_linear_random_shapes_vs_oracle;
b. one reduction order per (N, K, S): every MTW, NTW, activation / output
   layout, weight-load policy and XCD numbering gives the same bits;
c. nothing written past Y or past a workspace of exactly
   ffmi_linear_workspace_bytes() bytes (ffmi_linear_ws);
d. without a (large enough) workspace a split plan runs unsplit: the bits of
   the forced "NTW,1" plan, the workspace untouched.
"""
import functools

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
from gemm_plan_cases import PATH_MID, T_MTW, T_NTW, TMAX, plan, shape_plans, slab_bytes
from hip_util import Buf, f16, report
from test_gpu_kernels import close16, flip_bound, pack_act_np, silu_box_check, unpack_act_np

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5


@functools.lru_cache(maxsize=None)
def case(N, K, epi):
    """TMAX rows of input and the oracle's results (fp32 gate / up products
    with the epilogue), computed once per shape; tests take T-prefixes"""
    rng = np.random.default_rng(7 * N + K + epi)
    X = f16(rng.standard_normal((TMAX, K)))
    x32 = X.astype(np.float32)
    if epi:
        W = (f16(rng.uniform(-0.05, 0.05, (N, K))), f16(rng.uniform(-0.05, 0.05, (N, K))))
        ref = (O.linear(x32, W[0].astype(np.float32)), O.linear(x32, W[1].astype(np.float32)))
    else:
        W = f16(rng.uniform(-0.05, 0.05, (N, K)))
        ref = (O.linear(x32, W.astype(np.float32), fp16=1),)
    for a in (X,) + ref:
        a.setflags(write=False)
    return X, W, ref


@functools.lru_cache(maxsize=None)
def weights(N, K, epi):
    """packed weights on the device, once per shape"""
    L = F.lib()
    W = case(N, K, epi)[1]
    Wp = Buf.empty((L.ffmi_linear_packed_bytes(N, K) * (2 if epi else 1) // 2,), np.uint16)
    if epi:
        g, u = Buf(W[0]), Buf(W[1])
        F.check(L.ffmi_linear_pack_gate_up(g.ptr, u.ptr, N, K, Wp.ptr, None))
    else:
        src = Buf(W)
        F.check(L.ffmi_linear_pack_weight(src.ptr, N, K, Wp.ptr, None))
    Wp.get()  # (synchronises: the sources may go)
    return Wp


class Inputs:
    """the first T rows of a shape's X on the device, row-major and packed"""

    def __init__(self, T):
        self.T, self.bufs = T, {}

    def x(self, N, K, epi, xp):
        key = (N, K, epi, xp)
        if key not in self.bufs:
            X = case(N, K, epi)[0][:self.T]
            self.bufs[key] = Buf(pack_act_np(X) if xp else X)
        return self.bufs[key]


def force(monkeypatch, T, N, K, epi, ntw, S, flags=0):
    """force the plan and assert that the launch will take it"""
    monkeypatch.setenv("FFMI_GEMM_PLAN", f"{ntw},{S}")
    p = plan(T, N, K, epi | flags)
    want = dict(path=PATH_MID, MTW=T_MTW[T], NTW=ntw, S=S)
    assert {k: p[k] for k in want} == want, (T, N, K, epi, flags, p)
    return p


def guarded(nbytes):
    """a device buffer of nbytes + GUARD bytes, every byte PATTERN"""
    return Buf(np.full(nbytes + GUARD, PATTERN, np.uint8))


def guard_intact(buf, nbytes):
    return bool((buf.get()[nbytes:] == PATTERN).all())


def run(L, inp, T, N, K, epi, xp=0, yp=0, ws=0):
    """one ffmi_linear launch -> [T][N] fp16"""
    Tp = (T + 15) // 16 * 16
    Y = Buf.empty((Tp if yp else T, N), np.float16)
    flags = epi | (F.X_PACKED if xp else 0) | (F.Y_PACKED if yp else 0) | (F.W_STREAM if ws else 0)
    F.check(L.ffmi_linear(inp.x(N, K, epi, xp).ptr, weights(N, K, epi).ptr, Y.ptr, T, N, K, flags,
                          None), (T, N, K, flags))
    y = Y.get()
    return unpack_act_np(y.reshape(-1), T, N) if yp else y


@pytest.mark.parametrize("T,ntw", T_NTW)
def test_every_plan_vs_oracle(monkeypatch, T, ntw):
    """plain: within 2 fp16 ulp (or 1e-4 of the largest output) and >= 99 %
    bit-identical with the binomial margin of the output's size; SiLU-mul: the
    gate/up box check.  A numpy emulation of the slice-ordered fp32 sums at
    these shapes sat >= 99.8 % bit-identical to the oracle."""
    L = F.lib()
    inp = Inputs(T)
    worst = {}
    for N, K, S, epi in shape_plans():
        force(monkeypatch, T, N, K, epi, ntw, S)
        y = run(L, inp, T, N, K, epi)
        ref = case(N, K, epi)[2]
        if epi:
            exact = silu_box_check(y, ref[0][:T], ref[1][:T], (T, ntw, N, K, S))
        else:
            r16 = ref[0][:T].astype(np.float16)
            exact = float((y.view(np.uint16) == r16.view(np.uint16)).mean())
            print(f"T {T} NTW {ntw} N {N} K {K} S {S}: exact {exact:.5f} "
                  f"(bar {flip_bound(0.01, y.size):.5f})")
            close16(y, ref[0][:T], exact_frac=flip_bound(0.01, y.size))
        worst[K, S, epi] = min(exact, worst.get((K, S, epi), 1.0))
    for (K, S, epi), e in sorted(worst.items()):
        report("gemm_plans_vs_oracle", T=T, MTW=T_MTW[T], NTW=ntw, K=K, S=S, epi=epi, exact_min=e)


@functools.lru_cache(maxsize=None)
def base_bits(N, K, S, epi):
    """the TMAX-row result of one fixed plan (4 x 8 tiles, S slices, row-major,
    default numbering): what every other plan with this S must reproduce"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FFMI_MID_XCD", raising=False)
        force(mp, TMAX, N, K, epi, 8, S)
        y = run(F.lib(), Inputs(TMAX), TMAX, N, K, epi).view(np.uint16)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("T,ntw", T_NTW)
def test_one_reduction_order_per_split(monkeypatch, T, ntw):
    """Per output element: the MFMA chain over its slice's k-steps, then the
    slices in order -- fixed by (N, K, S).  So for each S and epilogue every
    (MTW, NTW) gives the same uint16 bits for the rows it shares with the
    TMAX-row base plan, and so do packed activations in, packed output
    (N % 32 == 0), non-temporal weight loads and every XCD numbering of the
    split launches."""
    L = F.lib()
    inp = Inputs(T)
    for N, K, S, epi in shape_plans():
        base = base_bits(N, K, S, epi)[:T]
        variants = [(0, 0, 0), (1, 0, 0), (0, 0, 1)]  # (X packed, Y packed, weight stream)
        if N % 32 == 0:
            variants += [(1, 1, 0), (0, 1, 1)]
        for sw in ("1", "0", "2") if S > 1 else ("1",):  # (unsplit: the map is inert)
            monkeypatch.setenv("FFMI_MID_XCD", sw)
            for xp, yp, ws in variants:
                force(monkeypatch, T, N, K, epi, ntw, S, (F.X_PACKED if xp else 0) |
                      (F.Y_PACKED if yp else 0) | (F.W_STREAM if ws else 0))
                y = run(L, inp, T, N, K, epi, xp, yp, ws).view(np.uint16)
                diff = int((y != base).sum())
                assert diff == 0, (f"{diff} of {y.size} outputs differ from the base plan: T {T} "
                                   f"NTW {ntw} N {N} K {K} S {S} epi {epi} xp {xp} yp {yp} "
                                   f"wstream {ws} FFMI_MID_XCD {sw}")


@pytest.mark.parametrize("T,ntw", T_NTW)
def test_no_write_past_output_or_workspace(monkeypatch, T, ntw):
    """ffmi_linear_ws with GUARD bytes of a fixed pattern right behind Y
    (behind its Tp rows when packed) and behind a workspace of exactly
    ffmi_linear_workspace_bytes(), which is the plan's S slabs: both untouched,
    the result the base plan's bits."""
    L = F.lib()
    inp = Inputs(T)
    Tp = (T + 15) // 16 * 16
    for N, K, S, epi in shape_plans():
        for xp, yp in [(0, 0)] + ([(1, 1)] if N % 32 == 0 else []):
            flags = epi | (F.X_PACKED if xp else 0) | (F.Y_PACKED if yp else 0)
            p = force(monkeypatch, T, N, K, epi, ntw, S, flags & ~1)
            need = L.ffmi_linear_workspace_bytes(T, N, K, flags)
            assert need == slab_bytes(T, N, p["S"], epi), (T, N, K, S, epi, need)
            ybytes = (Tp if yp else T) * N * 2
            Y, ws = guarded(ybytes), guarded(need)
            F.check(L.ffmi_linear_ws(inp.x(N, K, epi, xp).ptr, weights(N, K, epi).ptr, Y.ptr, T, N,
                                     K, flags, ws.ptr, need, None), (T, N, K, flags))
            ctx = (T, ntw, N, K, S, epi, xp, yp)
            assert guard_intact(Y, ybytes), ("write past Y", ctx)
            assert guard_intact(ws, need), ("write past the workspace", ctx)
            y = Y.get()[:ybytes].view(np.uint16)
            y = unpack_act_np(y, T, N) if yp else y.reshape(T, N)
            assert np.array_equal(y, base_bits(N, K, S, epi)[:T]), ctx


@pytest.mark.parametrize("T,ntw", T_NTW)
def test_missing_workspace_runs_unsplit(monkeypatch, T, ntw):
    """Split plans through ffmi_linear_ws with no workspace, and with one a
    byte too small: FFMI_OK, the bits of the forced "NTW,1" plan, and not a
    byte of the too-small workspace written."""
    L = F.lib()
    inp = Inputs(T)
    for N, K, S, epi in shape_plans():
        if S == 1:
            continue
        force(monkeypatch, T, N, K, epi, ntw, 1)
        unsplit = run(L, inp, T, N, K, epi).view(np.uint16)
        force(monkeypatch, T, N, K, epi, ntw, S)
        need = L.ffmi_linear_workspace_bytes(T, N, K, epi)
        assert need == slab_bytes(T, N, S, epi) and need > 0
        small = Buf(np.full(need - 1, PATTERN, np.uint8))  # a guard from offset 0
        for ws, nbytes in ((None, 0), (None, need), (small.ptr, need - 1)):
            Y = guarded(T * N * 2)
            F.check(L.ffmi_linear_ws(inp.x(N, K, epi, 0).ptr, weights(N, K, epi).ptr, Y.ptr, T, N,
                                     K, epi, ws, nbytes, None), (T, N, K, S, epi, nbytes))
            ctx = (T, ntw, N, K, S, epi, ws is not None, nbytes)
            assert guard_intact(Y, T * N * 2), ("write past Y", ctx)
            assert np.array_equal(Y.get()[:T * N * 2].view(np.uint16).reshape(T, N), unsplit), ctx
        assert guard_intact(small, 0), ("too-small workspace written", (T, ntw, N, K, S, epi))
