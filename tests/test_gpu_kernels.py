"""GPU parity of every hot-path kernel against the CPU oracle, through the
C ABI (include/ffmi.h).  Run on an MI355X: pytest -m gpu.

Tolerances (fp16 outputs, fp32 accumulation on both sides; only the order of
fp32 additions differs): linear / attention within 2 fp16 ulp, >= 99.5% of
elements bit-identical; norms within 1 ulp; argmax / top-k / embedding /
weights bit-exact.
"""
import ctypes
import os

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
from hip_util import Buf, f16, hip, report, ulp_diff

pytestmark = pytest.mark.gpu
# FFMI_RANDOM_SCALE: k times the seeds of the random-shape tests (one-off sweeps)
RS = int(os.environ.get("FFMI_RANDOM_SCALE", "1"))
OFF = int(os.environ.get("FFMI_RANDOM_SEED_OFFSET", "0"))  # fresh seeds for one-off sweeps

L = None


def setup_module(module):
    global L
    L = F.lib()


def close16(gpu, ref, max_ulp=2, exact_frac=0.99, atol=None):
    """fp16 results within `max_ulp` ulps OR within `atol` absolute (near-zero
    outputs of long fp32 sums: an fp32 reordering error of ~1e-7 is several
    fp16 ulps there), and >= exact_frac of them bit-identical."""
    g = np.asarray(gpu, np.float16)
    r = np.asarray(ref, np.float32).astype(np.float16)
    d = ulp_diff(g, r)
    if atol is None:
        atol = 1e-4 * max(1.0, float(np.abs(r.astype(np.float32)).max()))
    bad = (d > max_ulp) & (np.abs(g.astype(np.float32) - r.astype(np.float32)) > atol)
    assert not bad.any(), (f"{bad.sum()} elements off by > {max_ulp} ulp and > {atol}; "
                           f"worst at {np.unravel_index(d.argmax(), d.shape)}")
    assert (d == 0).mean() >= exact_frac, f"exact fraction {(d == 0).mean():.4f}"


# ---------------------------------------------------------------- weights
def test_fill_weight_bit_exact_vs_oracle():
    for name, kind, n in [("model.layers.0.self_attn.q_proj.weight", 0, 100003),
                          ("model.norm.weight", 1, 4096)]:
        buf = Buf.empty((n,), np.uint16)
        F.check(L.ffmi_fill_weight(buf.ptr, n, name.encode(), 20250117, kind, None))
        got = buf.get()
        ref = O.gen_weight(name, 20250117, kind, n).astype(np.float16).view(np.uint16)
        assert np.array_equal(got, ref)


# ---------------------------------------------------------------- linear
def packed(W16):
    N, K = W16.shape
    nb = L.ffmi_linear_packed_bytes(N, K)
    src = Buf(W16)
    dst = Buf.empty((nb // 2,), np.uint16)
    F.check(L.ffmi_linear_pack_weight(src.ptr, N, K, dst.ptr, None))
    return dst


@pytest.mark.parametrize("T", [1, 5, 16, 21, 40, 64, 100, 168, 200])
@pytest.mark.parametrize("N,K", [(768, 768), (2304, 768), (4096, 1024), (1376, 4096), (512, 3072)])
def test_linear_matches_oracle(T, N, K):
    rng = np.random.default_rng(T * 7 + N + K)
    X = f16(rng.standard_normal((T, K)))
    W = f16(rng.uniform(-0.05, 0.05, (N, K)))
    Wp = packed(W)
    Xb, Yb = Buf(X), Buf.empty((T, N), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Yb.ptr, T, N, K, F.EPI_NONE, None))
    ref = O.linear(X.astype(np.float32), W.astype(np.float32), fp16=1)
    close16(Yb.get(), ref)


@pytest.mark.parametrize("T", [1, 8, 24, 33, 64])
@pytest.mark.parametrize("N,K", [(32000, 768), (32001, 1024), (16384, 64)])
@pytest.mark.parametrize("xp", [0, 1])
def test_linear_wide_short_k_wave_form(T, N, K, xp):
    """Wide, short-K layers (>= 1024 tiles, K <= 1024: the 68M SSM's
    lm_head) run one wave per tile pair over the whole K
    (gemm_wave_kernel): within 2 fp16 ulp of the oracle, row-major or packed
    activations, ragged N and T, odd tile counts."""
    rng = np.random.default_rng(T + N + K + xp)
    X = f16(rng.standard_normal((T, K)))
    W = f16(rng.uniform(-0.05, 0.05, (N, K)))
    Wp = packed(W)
    Xb, Yb = Buf(X), Buf.empty((T, N), np.float16)
    flags = F.EPI_NONE
    if xp:
        Xb = Buf(pack_act_np(X))
        flags |= F.X_PACKED
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Yb.ptr, T, N, K, flags, None))
    ref = O.linear(X.astype(np.float32), W.astype(np.float32), fp16=1)
    close16(Yb.get(), ref)


@pytest.mark.parametrize("T", [65, 100, 168, 200])
@pytest.mark.parametrize("epi", [0, 1])
def test_linear_packed_activations_bit_identical(T, epi):
    """FFMI_X_PACKED (activation fragment tiles) changes only the load layout:
    the result must be bit-identical to the row-major input."""
    rng = np.random.default_rng(T + epi)
    N, K = 704, 1024
    X = f16(rng.standard_normal((T, K)))
    if epi:
        Wg, Wu = f16(rng.uniform(-0.05, 0.05, (N, K))), f16(rng.uniform(-0.05, 0.05, (N, K)))
        gb, ub = Buf(Wg), Buf(Wu)
        Wp = Buf.empty((2 * L.ffmi_linear_packed_bytes(N, K) // 2,), np.uint16)
        F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, N, K, Wp.ptr, None))
    else:
        Wp = packed(f16(rng.uniform(-0.05, 0.05, (N, K))))
    Xb = Buf(X)
    Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K) // 2,), np.uint16)
    F.check(L.ffmi_pack_activations(Xb.ptr, T, K, Xp.ptr, None))
    Y0, Y1 = Buf.empty((T, N), np.float16), Buf.empty((T, N), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Y0.ptr, T, N, K, epi, None))
    F.check(L.ffmi_linear(Xp.ptr, Wp.ptr, Y1.ptr, T, N, K, epi | F.X_PACKED, None))
    assert np.array_equal(Y0.get().view(np.uint16), Y1.get().view(np.uint16))


def test_pack_activations_matches_numpy_twin():
    rng = np.random.default_rng(3)
    T, K = 37, 256
    X = f16(rng.standard_normal((T, K)))
    Xb = Buf(X)
    Xp = Buf.empty((L.ffmi_packed_activation_bytes(T, K) // 2,), np.uint16)
    F.check(L.ffmi_pack_activations(Xb.ptr, T, K, Xp.ptr, None))
    assert np.array_equal(Xp.get(), pack_act_np(X).view(np.uint16))


@pytest.mark.parametrize("T", [1, 8, 40, 64, 100, 168])
@pytest.mark.parametrize("epi", [0, 1])
def test_linear_packed_in_and_out_bit_identical(T, epi):
    """Skinny and M-split paths with X_PACKED | Y_PACKED == row-major, bit for bit."""
    rng = np.random.default_rng(1000 + T + epi)
    N, K = 704, 512
    X = f16(rng.standard_normal((T, K)))
    if epi:
        Wg, Wu = f16(rng.uniform(-0.05, 0.05, (N, K))), f16(rng.uniform(-0.05, 0.05, (N, K)))
        gb, ub = Buf(Wg), Buf(Wu)
        Wp = Buf.empty((2 * L.ffmi_linear_packed_bytes(N, K) // 2,), np.uint16)
        F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, N, K, Wp.ptr, None))
    else:
        Wp = packed(f16(rng.uniform(-0.05, 0.05, (N, K))))
    Xb = Buf(X)
    Xp = Buf(pack_act_np(X))
    Tp = (T + 15) // 16 * 16
    Y0, Y1 = Buf.empty((T, N), np.float16), Buf.empty((Tp, N), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Y0.ptr, T, N, K, epi, None))
    F.check(L.ffmi_linear(Xp.ptr, Wp.ptr, Y1.ptr, T, N, K, epi | F.X_PACKED | F.Y_PACKED, None))
    y1 = unpack_act_np(Y1.get().reshape(-1), T, N)
    assert np.array_equal(Y0.get().view(np.uint16), y1.view(np.uint16))


@pytest.mark.parametrize("resid", [0, 1])
def test_rmsnorm_packed_output(resid):
    rng = np.random.default_rng(5 + resid)
    T, H = 21, 4096
    x1, x2 = f16(rng.standard_normal((T, H))), f16(rng.standard_normal((T, H)))
    w = f16(1 + 0.1 * rng.standard_normal(H))
    a, b, wb = Buf(x1), Buf(x2), Buf(w)
    r0, o0 = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
    r1, o1 = Buf.empty((T, H), np.float16), Buf.empty((32, H), np.float16)
    x2p = b.ptr if resid else None
    F.check(L.ffmi_rmsnorm_ex(a.ptr, x2p, wb.ptr, r0.ptr, o0.ptr, T, H, 1e-6, 0, None))
    F.check(L.ffmi_rmsnorm_ex(a.ptr, x2p, wb.ptr, r1.ptr, o1.ptr, T, H, 1e-6, F.Y_PACKED, None))
    assert np.array_equal(unpack_act_np(o1.get().reshape(-1), T, H).view(np.uint16),
                          o0.get().view(np.uint16))
    if resid:
        assert np.array_equal(r0.get().view(np.uint16), r1.get().view(np.uint16))


@pytest.mark.parametrize("T", [1, 8, 24, 168])
def test_linear_gate_up_silu_fused(T):
    rng = np.random.default_rng(T)
    Fdim, K = 688, 512
    X = f16(rng.standard_normal((T, K)))
    Wg = f16(rng.uniform(-0.08, 0.08, (Fdim, K)))
    Wu = f16(rng.uniform(-0.08, 0.08, (Fdim, K)))
    nb = 2 * L.ffmi_linear_packed_bytes(Fdim, K)
    gb, ub = Buf(Wg), Buf(Wu)
    Wp = Buf.empty((nb // 2,), np.uint16)
    F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, Fdim, K, Wp.ptr, None))
    Xb, Yb = Buf(X), Buf.empty((T, Fdim), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Yb.ptr, T, Fdim, K, F.EPI_SILU_MUL, None))
    g = O.linear(X.astype(np.float32), Wg.astype(np.float32))
    u = O.linear(X.astype(np.float32), Wu.astype(np.float32))
    ref = O.silu_mul(g, u)
    # an fp16 ulp flip of g or u propagates through two more roundings
    close16(Yb.get(), ref, max_ulp=3, exact_frac=0.99, atol=1e-3)


def flip_bound(rate, n):
    """least bit-identical fraction of n outputs whose fp32 sums, added in
    another order than the oracle's, flip their fp16 rounding at up to `rate`
    each: rate * n + 3 sigma of that count, and at least two flips (a
    500-seed sweep met 3 flips in a 260-output decode row at K = 5120)"""
    return 1.0 - max(2.0, rate * n + 3.0 * np.sqrt(rate * n)) / n


def silu_box_check(y, g, u, ctx=None):
    """the gate/up box check of test_gpu_llama_shapes, for a SiLU-mul GEMM
    result y against the oracle's fp32 gate and up products: >= 98% bit-
    identical to the chain on the oracle's fp16 gate/up, the rest inside the
    chain's range over gate/up within the plain GEMM tolerance (a one-ulp
    flip of g near silu's flat region moves y by several ulps) + 1 output
    ulp.  Returns the bit-identical fraction."""
    g16, u16 = g.astype(np.float16), u.astype(np.float16)
    chain = lambda a, b: O.silu_mul(a.astype(np.float32), b.astype(np.float32))  # noqa: E731
    y16 = y.astype(np.float16)
    exact = (y16 == chain(g16, u16).astype(np.float16)).mean()
    assert exact >= flip_bound(0.02, y.size), (exact, ctx)
    sp = lambda a: np.spacing(np.abs(a).astype(np.float16)).astype(np.float32)  # noqa: E731
    dg = np.maximum(2 * sp(g16), 1e-4 * np.abs(g).max())
    du = np.maximum(2 * sp(u16), 1e-4 * np.abs(u).max())
    pts = [chain(g + a * dg, u + b * du) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    lo, hi = np.min(pts, axis=0), np.max(pts, axis=0)
    slack = sp(np.maximum(np.abs(lo), np.abs(hi)))
    yf = y16.astype(np.float32)
    assert not ((yf < lo - slack) | (yf > hi + slack)).any(), ctx
    return float(exact)


@pytest.mark.parametrize("seed", range(20 * RS))
def test_linear_random_shapes_vs_oracle(seed):
    """ffmi_linear at random shapes against the oracle: T 1-1100 (skinny,
    wave, M-split with 2-4 row tiles per wave and split K, the 256 x 256 tile
    form), N from 16 to 20000 (ragged: not a multiple of 16 or 32), K a
    multiple of 32 up to 8192, with and without the SiLU-mul epilogue, row-
    major or packed activations in and out, weight-stream hint on or off."""
    rng = np.random.default_rng(4242 + OFF + seed)
    for _ in range(3):
        T = int(np.exp(rng.uniform(0, np.log(1100))))
        N = int(rng.choice([int(rng.integers(16, 400)), int(rng.integers(400, 6000)),
                            int(rng.integers(6000, 20000))]))
        K = 32 * int(np.exp(rng.uniform(0, np.log(256))))
        epi = int(rng.integers(0, 2))
        xp = int(rng.integers(0, 2))
        yp = int(rng.integers(0, 2)) if N % 32 == 0 else 0
        flags = (F.EPI_SILU_MUL if epi else F.EPI_NONE) | (F.W_STREAM if rng.integers(0, 2) else 0)
        X = f16(rng.standard_normal((T, K)))
        sc = 1.0 / np.sqrt(K)
        if epi:
            Wg = f16(rng.uniform(-2 * sc, 2 * sc, (N, K)))
            Wu = f16(rng.uniform(-2 * sc, 2 * sc, (N, K)))
            gb, ub = Buf(Wg), Buf(Wu)
            Wp = Buf.empty((2 * L.ffmi_linear_packed_bytes(N, K) // 2,), np.uint16)
            F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, N, K, Wp.ptr, None))
        else:
            W = f16(rng.uniform(-2 * sc, 2 * sc, (N, K)))
            Wp = packed(W)
        Xb = Buf(pack_act_np(X)) if xp else Buf(X)
        Tp = (T + 15) // 16 * 16
        Yb = Buf.empty(((Tp if yp else T), N), np.float16)
        flags |= (F.X_PACKED if xp else 0) | (F.Y_PACKED if yp else 0)
        F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Yb.ptr, T, N, K, flags, None), (T, N, K, flags))
        y = unpack_act_np(Yb.get().reshape(-1), T, N) if yp else Yb.get()
        if epi:
            g = O.linear(X.astype(np.float32), Wg.astype(np.float32))
            u = O.linear(X.astype(np.float32), Wu.astype(np.float32))
            silu_box_check(y, g, u, (T, N, K, flags))
        else:  # (>= 99% bit-identical, with the binomial margin of a small output)
            close16(y, O.linear(X.astype(np.float32), W.astype(np.float32), fp16=1),
                    exact_frac=flip_bound(0.01, y.size))


@pytest.mark.parametrize("Ts", [(1, 8, 40, 64), (65, 100, 168, 192)])
@pytest.mark.parametrize("wstream", [0, 1])
@pytest.mark.parametrize("K", [1024, 1536, 2048])
def test_linear_rows_independent_of_batch(Ts, wstream, K):
    # within a kernel regime (skinny: T <= 64, M-split: T > 64) and weight
    # policy, a row's reduction order must not depend on T (batching
    # invariance)
    flag = F.W_STREAM if wstream else 0
    rng = np.random.default_rng(1)
    N = 1024
    X = f16(rng.standard_normal((max(Ts), K)))
    W = f16(rng.uniform(-0.05, 0.05, (N, K)))
    Wp = packed(W)
    outs = []
    for T in Ts:
        Xb, Yb = Buf(X[:T]), Buf.empty((T, N), np.float16)
        F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Yb.ptr, T, N, K, F.EPI_NONE | flag, None))
        outs.append(Yb.get())
    for o in outs[:-1]:
        assert np.array_equal(o.view(np.uint16), outs[-1][:o.shape[0]].view(np.uint16))


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("T,H", [(1, 768), (8, 4096), (37, 4096), (5, 8192)])
def test_rmsnorm_and_residual(T, H):
    rng = np.random.default_rng(H + T)
    x1 = f16(rng.standard_normal((T, H)))
    x2 = f16(rng.standard_normal((T, H)) * 0.5)
    w = f16(1 + rng.uniform(-0.1, 0.1, H))
    eps = 1e-6
    b1, b2, bw = Buf(x1), Buf(x2), Buf(w)
    out, res = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
    F.check(L.ffmi_rmsnorm(b1.ptr, bw.ptr, out.ptr, T, H, eps, None))
    close16(out.get(), O.rmsnorm(x1.astype(np.float32), w.astype(np.float32), eps), 1, 0.99)
    F.check(L.ffmi_residual_rmsnorm(b1.ptr, b2.ptr, bw.ptr, res.ptr, out.ptr, T, H, eps, None))
    r_ref, o_ref = O.residual_rmsnorm(x1.astype(np.float32), x2.astype(np.float32),
                                      w.astype(np.float32), eps)
    assert np.array_equal(res.get().view(np.uint16), f16(r_ref).view(np.uint16))
    close16(out.get(), o_ref, 1, 0.99)


def _fused_pair(T, H, Kp, N, epi, seed):
    """producer (o/down: residual += X . Wp^T, sums of squares) then consumer
    (qkv or gate/up on the normalised residual) through the test hooks, and
    the unfused kernels on the same inputs"""
    rng = np.random.default_rng(seed)
    X = f16(rng.standard_normal((T, Kp)))
    Wo = f16(rng.uniform(-0.03, 0.03, (H, Kp)))
    r0 = f16(rng.standard_normal((T, H)))
    wn = f16(1 + rng.uniform(-0.1, 0.1, H))
    eps = 1e-6
    Wop = packed(Wo)
    Xb, res = Buf(X), Buf(r0)
    ss = Buf.empty((T, H // 16), np.float32)
    F.check(L.ffmi_debug_fused_residual_linear(Xb.ptr, Wop.ptr, res.ptr, ss.ptr, T, H, Kp, None))
    # unfused producer: the GEMM, then the norm kernel's fp16 residual add
    Yo = Buf.empty((T, H), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wop.ptr, Yo.ptr, T, H, Kp, F.EPI_NONE, None))
    r_ref = f16(r0.astype(np.float32) + Yo.get().astype(np.float32))
    r1 = res.get()
    assert np.array_equal(r1.view(np.uint16), r_ref.view(np.uint16)), "producer residual"
    sq = (r1.astype(np.float32) ** 2).reshape(T, H // 16, 16).sum(axis=2)
    np.testing.assert_allclose(ss.get(), sq, rtol=1e-5, atol=1e-6)
    # consumer vs the norm kernel + GEMM
    if epi:
        Wg = f16(rng.uniform(-0.03, 0.03, (N, H)))
        Wu = f16(rng.uniform(-0.03, 0.03, (N, H)))
        gb, ub = Buf(Wg), Buf(Wu)
        Wq = Buf.empty((L.ffmi_linear_packed_bytes(N, H),), np.uint16)
        F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, N, H, Wq.ptr, None))
    else:
        Wm = f16(rng.uniform(-0.03, 0.03, (N, H)))
        Wq = packed(Wm)
    wb = Buf(wn)
    Y = Buf.empty((T, N), np.float16)
    F.check(L.ffmi_debug_fused_norm_linear(res.ptr, ss.ptr, wb.ptr, eps, Wq.ptr, Y.ptr, T, N, H,
                                           epi, None))
    hb = Buf.empty((T, H), np.float16)
    F.check(L.ffmi_rmsnorm(res.ptr, wb.ptr, hb.ptr, T, H, eps, None))
    Yr = Buf.empty((T, N), np.float16)
    F.check(L.ffmi_linear(hb.ptr, Wq.ptr, Yr.ptr, T, N, H, epi, None))
    h_or = O.rmsnorm(r1.astype(np.float32), wn.astype(np.float32), eps)
    if epi:
        ref = O.silu_mul(O.linear(h_or, Wg.astype(np.float32)), O.linear(h_or, Wu.astype(np.float32)))
    else:
        ref = O.linear(h_or, Wm.astype(np.float32))
    return Y.get(), Yr.get(), ref


@pytest.mark.parametrize("T", [1, 8, 32])
@pytest.mark.parametrize("N,epi", [(12288, 0), (1024, 0), (11008, 1)])
def test_fused_residual_norm_gemm_pair_at_7b_width(T, N, epi):
    """The residual RMSNorm folded into the decode GEMMs (LLaMA-7B decode,
    H 4096: o/down produce, qkv / gate-up consume), checked at kernel level
    against the norm kernel + plain GEMM on the same inputs: the producer's
    residual bit-identical, the consumer within 2 fp16 ulp (3 through the SiLU
    chain) and >= 99% bit-identical (its rms sums the squares per 16-column
    tile, then the tiles: an fp32 reordering), and within the same bound of
    the oracle's rmsnorm + linear."""
    y, yr, ref = _fused_pair(T, 4096, 4096, N, epi, T * 31 + N)
    mu = 3 if epi else 2
    close16(y, yr.astype(np.float32), max_ulp=mu, exact_frac=0.99, atol=1e-3 if epi else None)
    if epi:  # vs the oracle through the SiLU chain: test_gpu_llama_shapes' box bound
        # applies to the unfused GEMM; here the exact fraction (an fp16 flip of
        # gate or up moves a near-zero output by more than 3 ulp)
        assert (y.astype(np.float16) == ref.astype(np.float16)).mean() >= 0.98
    else:
        close16(y, ref, max_ulp=mu, exact_frac=0.98)


@pytest.mark.parametrize("T", [1, 5, 17, 32])
@pytest.mark.parametrize("H", [64, 96, 2080])
def test_fused_norm_consumer_empty_wave_ranges(T, H):
    """Consumer launches whose waves own no k-step (H 64 / 96: 2-3 k-steps
    over 4 waves) or a batch plus a tail (H 2080: 65 k-steps over 8 waves):
    every wave still meets the norm's one barrier (gemm.hip rms_finish) and
    the results hold the bound above."""
    y, yr, ref = _fused_pair(T, H, 64, 256, 0, T * 7 + H)
    close16(y, yr.astype(np.float32), max_ulp=2, exact_frac=0.99)
    close16(y, ref, max_ulp=2, exact_frac=0.98)


# ---------------------------------------------------------------- argmax / topk
@pytest.mark.parametrize("V", [512, 1000, 1001, 32000])
def test_softmax_argmax_topk_exact(V):
    rng = np.random.default_rng(V)
    T = 9
    logits = f16(rng.standard_normal((T, V)) * 2)
    # planted exact ties and near-ties that fp16 softmax collapses
    logits[1, 17] = logits[1, V - 100] = f16(9.0)
    logits[2, 5] = f16(8.0)
    logits[2, 6] = f16(8.0 + 2 ** -7)
    lb = Buf(logits)
    ids, pr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    F.check(L.ffmi_argmax(lb.ptr, T, V, ids.ptr, pr.ptr, None))
    ref_ids, ref_p = O.softmax_argmax(logits.astype(np.float32), fp16=1)
    assert ids.get().tolist() == ref_ids.tolist()
    assert ids.get()[1] == 17
    for k in (1, 2, 3):
        ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
        F.check(L.ffmi_arg_topk(lb.ptr, T, V, k, ids.ptr, pr.ptr, None))
        rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
        assert np.array_equal(ids.get(), rid)
        np.testing.assert_array_equal(pr.get(), rp)


@pytest.mark.parametrize("seed", range(10 * RS))
def test_softmax_topk_random_shapes_exact(seed):
    """Softmax + argmax / top-k (k 1-4) at random shapes, bit-exact against
    the oracle: T 1-300, V from 64 to 140000 (multiples of 8 take the
    register kernel, others and V > 32768 the streaming one), logit scales
    from flat (fp16 p collapses, many candidates) to peaked, planted ties."""
    rng = np.random.default_rng(777 + OFF + seed)
    T = int(rng.integers(1, 301))
    V = int(rng.choice([int(rng.integers(8, 4096)) * 8, int(rng.integers(64, 40000)),
                        32000, 32001, int(rng.integers(32769, 140000))]))
    scale = float(rng.choice([1e-3, 0.05, 1.0, 3.0, 8.0]))
    logits = f16(rng.standard_normal((T, V)) * scale)
    for t in rng.choice(T, size=min(T, 4), replace=False):  # planted exact ties
        m = f16(float(np.abs(logits[t]).max()) + 1.0)
        logits[t, rng.choice(V, size=int(rng.integers(2, 6)), replace=False)] = m
    lb = Buf(logits)
    k = int(rng.integers(1, 5))
    ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
    F.check(L.ffmi_arg_topk(lb.ptr, T, V, k, ids.ptr, pr.ptr, None), (T, V, k))
    rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
    assert np.array_equal(ids.get(), rid.reshape(T, k)), (T, V, k, scale)
    np.testing.assert_array_equal(pr.get(), rp.reshape(T, k))


class TopkWs:
    """A zeroed ffmi_arg_topk_ws workspace for up to Tmax rows (the model's
    split-row top-k); `left_zero` checks the calls re-armed every counter."""

    def __init__(self, Tmax):
        self.nbytes = int(L.ffmi_arg_topk_workspace_bytes(Tmax))
        self.buf = Buf(np.zeros(self.nbytes // 4, np.uint32))

    def __call__(self, lb, T, V, k, ids, pr):
        F.check(L.ffmi_arg_topk_ws(lb.ptr, T, V, k, ids.ptr, pr.ptr, self.buf.ptr, self.nbytes,
                                   None), (T, V, k))

    def counters_zero(self, T):
        return not self.buf.get()[:T].any()


@pytest.mark.parametrize("T", [1, 5, 8, 16, 17, 24, 32, 33, 64, 65, 100, 128, 129, 168, 256])
@pytest.mark.parametrize("V", [4104, 8000, 16000, 32000])
def test_softmax_topk_split_rows_exact(T, V):
    """The split-row form (ffmi_arg_topk_ws: T <= 128 rows over 2-16
    workgroups each, chosen by T; the last workgroup of a row to publish its
    partial sum finishes the row) against the oracle, bit-exact: random rows
    at several scales, planted exact ties across the row, a flat row (more
    candidates than the LDS list), repeated launches on one workspace (the
    per-row counters must be re-armed), k 1-4."""
    rng = np.random.default_rng(T * 100003 + V)
    logits = f16(rng.standard_normal((T, V)) * rng.choice([0.05, 1.0, 3.0], size=(T, 1)))
    logits[0, :] = f16(0.25)  # flat: every logit a candidate
    for t in range(1, min(T, 4)):
        m = f16(float(np.abs(logits[t]).max()) + 1.0)
        logits[t, rng.choice(V, size=3, replace=False)] = m
    lb = Buf(logits)
    ws = TopkWs(256)
    for k in (1, 2, 3, 4):
        rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
        for _ in range(2):
            ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
            ws(lb, T, V, k, ids, pr)
            assert np.array_equal(ids.get(), rid.reshape(T, k)), (k, np.argwhere(ids.get() != rid.reshape(T, k))[:4])
            np.testing.assert_array_equal(pr.get(), rp.reshape(T, k))
        assert ws.counters_zero(T)
    assert ids.get()[0].tolist() == list(range(4))


def test_softmax_topk_split_one_workspace_many_shapes():
    """One workspace for every step size, as the model keeps it: the row
    counters sit at a fixed offset, so a step's partial sums never land on
    the counters of a later step with more rows (round 6: they did, and the
    next step found no last workgroup -- stale ids)."""
    rng = np.random.default_rng(31337)
    ws = TopkWs(256)
    for T in (40, 100, 8, 128, 33, 17, 64, 1, 120, 24, 24, 65, 9, 168, 256, 130):
        V = 32000
        logits = f16(rng.standard_normal((T, V)) * 2.0)
        lb = Buf(logits)
        k = int(rng.integers(1, 5))
        ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
        ws(lb, T, V, k, ids, pr)
        rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
        assert np.array_equal(ids.get(), rid.reshape(T, k)), T
        np.testing.assert_array_equal(pr.get(), rp.reshape(T, k))
        assert ws.counters_zero(256), T


@pytest.mark.parametrize("seed", range(6 * RS))
def test_softmax_topk_split_random_exact(seed):
    """The split-row form at random shapes and scales (T 1-128, V a multiple
    of 8 up to 32768, planted ties), bit-exact against the oracle and against
    the one-workgroup form."""
    rng = np.random.default_rng(4242 + OFF + seed)
    T = int(rng.integers(1, 257))
    V = 8 * int(rng.integers(8, 4097))
    scale = float(rng.choice([1e-3, 0.05, 1.0, 3.0, 8.0]))
    logits = f16(rng.standard_normal((T, V)) * scale)
    for t in rng.choice(T, size=min(T, 4), replace=False):
        m = f16(float(np.abs(logits[t]).max()) + 1.0)
        logits[t, rng.choice(V, size=int(rng.integers(2, 6)), replace=False)] = m
    lb = Buf(logits)
    k = int(rng.integers(1, 5))
    ws = TopkWs(T)
    ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
    ws(lb, T, V, k, ids, pr)
    ids1, pr1 = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
    F.check(L.ffmi_arg_topk(lb.ptr, T, V, k, ids1.ptr, pr1.ptr, None))
    rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
    assert np.array_equal(ids.get(), rid.reshape(T, k)), (T, V, k, scale)
    np.testing.assert_array_equal(pr.get(), rp.reshape(T, k))
    assert np.array_equal(ids.get(), ids1.get()) and np.array_equal(pr.get(), pr1.get())
    assert ws.counters_zero(T)


@pytest.mark.parametrize("seed", range(8 * RS))
def test_rmsnorm_random_shapes(seed):
    """RMSNorm / residual RMSNorm at random T (1-1100) and H (multiple of 8
    up to 16384): residual bit-exact, output within 1 fp16 ulp of the
    oracle and >= 99% bit-identical."""
    rng = np.random.default_rng(555 + OFF + seed)
    T = int(np.exp(rng.uniform(0, np.log(1100))))
    H = 8 * int(rng.integers(1, 2049))
    x1 = f16(rng.standard_normal((T, H)) * float(rng.choice([0.01, 1.0, 30.0])))
    x2 = f16(rng.standard_normal((T, H)))
    w = f16(1 + rng.uniform(-0.5, 0.5, H))
    eps = float(rng.choice([1e-6, 1e-5]))
    b1, b2, bw = Buf(x1), Buf(x2), Buf(w)
    out, res = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
    F.check(L.ffmi_rmsnorm(b1.ptr, bw.ptr, out.ptr, T, H, eps, None))
    close16(out.get(), O.rmsnorm(x1.astype(np.float32), w.astype(np.float32), eps), 1, 0.99)
    F.check(L.ffmi_residual_rmsnorm(b1.ptr, b2.ptr, bw.ptr, res.ptr, out.ptr, T, H, eps, None))
    r_ref, o_ref = O.residual_rmsnorm(x1.astype(np.float32), x2.astype(np.float32),
                                      w.astype(np.float32), eps)
    assert np.array_equal(res.get().view(np.uint16), f16(r_ref).view(np.uint16))
    close16(out.get(), o_ref, 1, 0.99)


@pytest.mark.parametrize("T,V", [(24, 32000), (200, 32000), (3, 4096), (5, 65536)])
def test_softmax_topk_chunked_ties(T, V):
    """Chunked path (one workgroup per 2048 logits, last chunk merges): exact
    ties spread over several chunks resolve to the lowest indices, and rows of
    equal logits pick 0, 1, 2."""
    rng = np.random.default_rng(T + V)
    logits = f16(rng.standard_normal((T, V)) * 3)
    logits[0, :] = f16(0.5)                       # all equal
    for j in (V - 1, 7000 % V, 2049 % V, 4095):    # one maximum in several chunks
        logits[1, j] = f16(12.0)
    logits[2, V // 2] = f16(10.0)                  # near-ties that fp16 p collapses
    logits[2, V // 2 + 1] = f16(10.0 - 2 ** -7)
    logits[2, 3] = f16(10.0 - 2 ** -7)
    lb = Buf(logits)
    for k in (1, 3, 4):
        ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
        F.check(L.ffmi_arg_topk(lb.ptr, T, V, k, ids.ptr, pr.ptr, None))
        rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
        assert np.array_equal(ids.get(), rid), np.argwhere(ids.get() != rid)[:5]
        np.testing.assert_array_equal(pr.get(), rp)
        assert ids.get()[0].tolist() == list(range(k))
    # repeated launches re-arm the per-row arrival counters
    for _ in range(3):
        ids = Buf.empty((T,), np.int32)
        F.check(L.ffmi_argmax(lb.ptr, T, V, ids.ptr, None, None))
        assert ids.get().tolist() == O.softmax_argmax(logits.astype(np.float32), fp16=1)[0].tolist()


@pytest.mark.parametrize("V", [32000, 32001, 128256])
@pytest.mark.parametrize("nties", [2, 63, 64, 65, 127, 128, 129, 700])
def test_softmax_topk_candidate_list_capacity(nties, V):
    """The register kernel puts the candidates' keys in a 128-entry LDS list
    read by one wave (two keys per lane); more candidates fall back to
    workgroup-wide rounds.  Rows with nties equal maxima (and, row 3, half of
    them 2^-7 lower: fp16 p collapses them) on either side of 64 and 128.
    V = 32001 (rows not 16-B aligned) and 128256 (LLaMA-3) take the streaming
    kernel, which uses the same list."""
    rng = np.random.default_rng(nties)
    T = 4
    logits = f16(rng.standard_normal((T, V)))
    for t in range(T):
        idx = rng.choice(V, nties, replace=False)
        logits[t, idx] = f16(7.0 + t)
        if t == 3:
            logits[t, idx[: nties // 2]] = f16(10.0 - 2 ** -7)
    lb = Buf(logits)
    for k in (1, 3, 4):
        ids, pr = Buf.empty((T, k), np.int32), Buf.empty((T, k), np.float32)
        F.check(L.ffmi_arg_topk(lb.ptr, T, V, k, ids.ptr, pr.ptr, None))
        rid, rp = O.softmax_topk(logits.astype(np.float32), k, fp16=1)
        assert np.array_equal(ids.get(), rid), (k, ids.get(), rid)
        np.testing.assert_array_equal(pr.get(), rp)


# ---------------------------------------------------------------- attention
def pack_act_np(X):
    """numpy twin of ffmi_pack_activations: [T][K] -> [T/16][K/32][64 lanes][8]."""
    T, K = X.shape
    Tp = (T + 15) // 16 * 16
    Xp = np.zeros((Tp, K), X.dtype)
    Xp[:T] = X
    return Xp.reshape(Tp // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(-1)


def unpack_act_np(P, T, K):
    Tp = (T + 15) // 16 * 16
    return P[:Tp * K].reshape(Tp // 16, K // 32, 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(Tp, K)[:T]


class AttnCase:
    """Builds token-info batches for ffmi_attn_* and the matching oracle."""

    def __init__(self, mode, heads=2, d=128, max_requests=4, max_seq=96, tree=32, max_tokens=128,
                 out_layout=0, theta=10000.0, llama3=None, fp32=False):
        self.heads, self.d = heads, d
        self.Hl = heads * d
        self.out_layout = out_layout
        self.fp32 = fp32  # DT_FLOAT handle (--use-full-precision): fp32 in, out, caches
        l3 = (1,) + tuple(llama3) if llama3 else (0, 1.0, 1.0, 4.0, 8192)
        cfg = F.AttnCfg(mode, heads, d, max_requests, max_seq, tree, max_tokens,
                        1.0 / np.sqrt(d), theta, out_layout, *l3, int(fp32))
        self.h = ctypes.c_void_p()
        F.check(L.ffmi_attn_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        self.cfg, self.twin = cfg, None  # (twin: run's slabs option)
        self.max_requests = max_requests
        self.b = ctypes.c_void_p()
        F.check(L.ffmi_batch_create(max_tokens, max_requests, ctypes.byref(self.b)))
        slots = ctypes.c_int()
        L.ffmi_attn_kv_ptrs(self.h, None, None, ctypes.byref(slots))
        self.slots = slots.value
        self.tab = O.rope_table(self.slots, d, theta, llama3).reshape(self.slots, d // 2, 2)
        self.kc = {}  # (req, slot) -> (k_rot [heads,d], v [heads,d])
        self.mode = mode

    def rope(self, x, pos):
        x = x.astype(np.float32).reshape(self.heads, self.d)
        h = self.d // 2
        c, s = self.tab[pos, :, 0], self.tab[pos, :, 1]
        a, b = x[:, :h], x[:, h:]
        out = np.concatenate([a * c - b * s, a * s + b * c], axis=1)
        return out if self.fp32 else f16(out).astype(np.float32)

    def caches(self, h):
        """the K and V^T caches of handle h (ffmi_attn_kv_ptrs), as bits"""
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        F.check(L.ffmi_attn_kv_ptrs(h, ctypes.byref(k), ctypes.byref(v), None))
        n = self.max_requests * self.heads * self.slots * self.d
        kc, vc = np.empty(n, np.uint16), np.empty(n, np.uint16)
        assert hip().hipDeviceSynchronize() == 0
        assert hip().hipMemcpy(kc.ctypes.data, k, n * 2, 2) == 0
        assert hip().hipMemcpy(vc.ctypes.data, v, n * 2, 2) == 0
        return kc, vc

    def run(self, infos, masks=None, commits=(), rng=None, slabs=None, slab_pad=0, oproj=None,
            qkv=None):
        """slabs = S: the step's qkv arrives as S deferred split-K slabs
        (partials_rule.make_slabs, [S][T][3 * Hl + slab_pad] fp32) through
        ffmi_debug_attn_partials; a twin handle takes the same batch through
        ffmi_attn_* with qkv = combine(slabs), and its output, K cache and
        V^T cache must equal this handle's bit for bit after the step (fp16
        handles).  The oracle side sees the combined qkv.

        oproj = (Wo fp16 [N][Hl], N, max_T): the step goes through
        ffmi_debug_attn_oproj (with qkv, or with the slabs above), which asks
        the launch to project each head's output rows into a slab buffer
        (oproj_rule.slab_buffer: sentinel words, heads * max_T * N between two
        guards).  The twin comparison above is made as well -- the projection
        must not disturb the attention -- and every word of the buffer outside
        [heads][T][N] (all of it when the launch did not project) must still
        hold the sentinel.  Returns (out, qs, slab, projected), slab float32
        [heads][T][N] or None.

        qkv: the step's qkv rows, given instead of drawn."""
        T = len(infos)
        if qkv is not None:
            assert not slabs and qkv.shape == (T, 3 * self.Hl)
        elif slabs:
            from partials_rule import combine, make_slabs
            assert not self.fp32 and slab_pad % 4 == 0
            N = 3 * self.Hl
            sl = make_slabs(slabs, T, N + slab_pad, N, rng)
            qkv = np.ascontiguousarray(combine(sl)[:, :N])
        elif qkv is None:
            qkv = rng.standard_normal((T, 3 * self.Hl)).astype(np.float32)
            if not self.fp32:
                qkv = f16(qkv)
        self.last_qkv = qkv  # the step's inputs, for tests that read the caches back
        # tree_vis is derived by ffmi_batch_upload from masks/tree_bit
        toks = (F.TokenInfo * T)(*[F.TokenInfo(*i, 0) for i in infos])
        work = []
        t = 0
        while t < T:
            r = infos[t][2]
            w = [r, t, 0, 0]
            while t < T and infos[t][2] == r and w[2] < F.ATTN_QTILE:
                w[3] = max(w[3], infos[t][4], infos[t][5] + infos[t][6])
                w[2] += 1
                t += 1
            work.append(F.AttnWork(*w))
        wk = (F.AttnWork * len(work))(*work)
        cm = (F.CommitInfo * max(1, len(commits)))(*[F.CommitInfo(*c, 0) for c in commits])
        nmask = 0
        mk = (ctypes.c_uint64 * 1)()
        if masks is not None:
            nmask = len(masks)
            flat = np.zeros((nmask, 64), np.uint64)
            for r, m in enumerate(masks):
                flat[r, :len(m)] = m
            mk = (ctypes.c_uint64 * flat.size)(*flat.ravel().tolist())
        desc = F.BatchDesc(T, len(work), len(commits), nmask, toks, wk, cm, mk)
        F.check(L.ffmi_batch_upload(self.b, ctypes.byref(desc), None))
        Tp = (T + 15) // 16 * 16
        qb, ob = Buf(qkv), Buf.empty((Tp, self.Hl), np.float32 if self.fp32 else np.float16)
        fn = {F.ATTN_INC: L.ffmi_attn_inc, F.ATTN_SPEC: L.ffmi_attn_spec,
              F.ATTN_TREE: L.ffmi_attn_tree}[self.mode]
        if slabs or oproj:
            if self.twin is None:
                self.twin = ctypes.c_void_p()
                F.check(L.ffmi_attn_create(ctypes.byref(self.cfg), ctypes.byref(self.twin)))
            sb, tb = Buf(sl) if slabs else None, Buf.empty((Tp, self.Hl), np.float16)
            if oproj:
                import oproj_rule as R
                Wo, No, max_T = oproj
                assert not self.fp32 and Wo.dtype == np.float16 and Wo.shape == (No, self.Hl)
                wp, pj = packed(Wo), ctypes.c_int(-1)
                zb = Buf(R.slab_buffer(self.heads, max_T, No))
                F.check(L.ffmi_debug_attn_oproj(
                    self.h, self.b, None if slabs else qb.ptr, sb.ptr if slabs else None,
                    slabs or 0, N + slab_pad if slabs else 0, ob.ptr, wp.ptr, No,
                    ctypes.c_void_p(zb.ptr.value + 4 * R.GUARD), max_T, ctypes.byref(pj), None))
                assert pj.value in (0, 1)
            else:
                F.check(L.ffmi_debug_attn_partials(self.h, self.b, sb.ptr, slabs, N + slab_pad,
                                                   ob.ptr, None))
            F.check(fn(self.twin, self.b, qb.ptr, tb.ptr, None))
            assert np.array_equal(ob.get().view(np.uint16), tb.get().view(np.uint16)), "slab out"
            for name, a, b in zip(("K", "V^T"), self.caches(self.h), self.caches(self.twin)):
                assert np.array_equal(a, b), f"slab {name} cache"
        else:
            F.check(fn(self.h, self.b, qb.ptr, ob.ptr, None))
        out = ob.get()
        out = unpack_act_np(out.reshape(-1), T, self.Hl) if self.out_layout else out[:T]
        # oracle side: commits, stores, then attention rows
        if commits:
            for (src, req, depth) in commits:
                self.kc[(req, depth)] = self.prev_stage[src]
        stage = {}
        qs = []
        for t, i in enumerate(infos):
            q = self.rope(qkv[t, :self.Hl], i[1])
            k = self.rope(qkv[t, self.Hl:2 * self.Hl], i[1])
            v = qkv[t, 2 * self.Hl:].astype(np.float32).reshape(self.heads, self.d)
            stage[t] = (k, v)
            if i[3] >= 0:
                self.kc[(i[2], i[3])] = (k, v)
            qs.append(q)
        self.prev_stage = stage
        if oproj:
            return out, qs, R.split_buffer(zb.get(), self.heads, T, No, pj.value == 1), pj.value
        return out, qs

    def ref_row(self, q, req, visible_slots):
        ref = np.zeros((self.heads, self.d), np.float32)
        K = np.stack([self.kc[(req, s)][0] for s in visible_slots], 1)  # heads, n, d
        V = np.stack([self.kc[(req, s)][1] for s in visible_slots], 1)
        for hh in range(self.heads):
            ref[hh] = O.attention_row(q[hh], K[hh], V[hh], np.ones(len(visible_slots)),
                                      1.0 / np.sqrt(self.d), fp16=0 if self.fp32 else 1)
        return ref.reshape(-1)

    def check(self, gpu, ref):
        """fp16: close16; fp32: within the fp32 reordering error of the
        softmax-weighted sums (2e-6 absolute on O(1) values)"""
        if self.fp32:
            err = np.abs(np.asarray(gpu, np.float32) - ref)
            assert err.max() <= 2e-6 * max(1.0, float(np.abs(ref).max())), float(err.max())
        else:
            close16(gpu, ref, exact_frac=0.98)


@pytest.mark.parametrize("layout,fp32", [(0, False), (1, False), (0, True)])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_inc_prefill_then_decode(d, layout, fp32):
    rng = np.random.default_rng(d)
    c = AttnCase(F.ATTN_INC, d=d, out_layout=layout, fp32=fp32)
    # step 1: prefill of three requests (chunked positions), step 2: decode/chunk
    lens = {0: 20, 1: 37, 2: 10}
    infos = [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]
    out, qs = c.run(infos, rng=rng)
    got = [out[t] for t in range(len(infos))]
    want = [c.ref_row(qs[t], i[2], range(i[1] + 1)) for t, i in enumerate(infos)]
    infos = [(7, 20, 0, 20, 21, 0, 0, 0), (7, 37, 1, 37, 38, 0, 0, 0)] + \
            [(7, p, 2, p, p + 1, 0, 0, 0) for p in range(10, 15)]
    out, qs = c.run(infos, rng=rng)
    got += [out[t] for t in range(len(infos))]
    want += [c.ref_row(qs[t], i[2], range(i[1] + 1)) for t, i in enumerate(infos)]
    c.check(np.stack(got), np.stack(want))  # (the exact-fraction bar over all rows)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_llama3_rope_scaling(d):
    """llama3 frequency scaling (HF's per-pair bands, tests/test_rope_llama3.py)
    in the handle's RoPE table: original_max_position 64 puts frequency pairs
    in each of the three wavelength bands."""
    rng = np.random.default_rng(200 + d)
    c = AttnCase(F.ATTN_INC, d=d, theta=500000.0, llama3=(8.0, 1.0, 4.0, 64))
    lens = {0: 33, 1: 57}
    infos = [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]
    out, qs = c.run(infos, rng=rng)
    # (the exact-fraction bar over all rows: a d = 32 row has only 64 values)
    close16(out[:len(infos)], np.stack([c.ref_row(qs[t], i[2], range(i[1] + 1))
                                        for t, i in enumerate(infos)]), exact_frac=0.98)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_fused_equals_two_launch_path(d, monkeypatch):
    """One workgroup per request (decode / beam / verify steps) runs commits,
    KV update and attention in one launch; FFMI_ATTN_NO_FUSE=1 runs the
    separate KV-update kernel first.  Outputs and caches must be identical."""
    def scenario():
        rng = np.random.default_rng(77 + d)
        c = AttnCase(F.ATTN_INC, d=d)
        lens = {0: 3, 1: 8, 2: 6}   # prefill: one small item per request -> fused
        infos = [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]
        o1, _ = c.run(infos, rng=rng)
        infos = [(7, n, r, n, n + 1, 0, 0, 0) for r, n in lens.items()]   # decode step
        o2, _ = c.run(infos, rng=rng)
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        slots = ctypes.c_int()
        F.check(L.ffmi_attn_kv_ptrs(c.h, ctypes.byref(k), ctypes.byref(v), ctypes.byref(slots)))
        n = 4 * c.heads * slots.value * c.d
        kc = np.empty(n, np.uint16)
        hip().hipMemcpy(kc.ctypes.data, k, n * 2, 2)
        return o1, o2, kc
    fused = scenario()
    monkeypatch.setenv("FFMI_ATTN_NO_FUSE", "1")
    split = scenario()
    for a, b in zip(fused, split):
        assert np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16))


def tree_masks(parents):
    """mask[key] bit q set iff q is a descendant-or-self of key."""
    n = len(parents)
    m = [0] * n
    for q in range(n):
        a = q
        while a >= 0:
            m[a] |= 1 << q
            a = parents[a]
    return m


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_attention_tree_verify_and_commit(d, fp32):
    rng = np.random.default_rng(100 + d)
    c = AttnCase(F.ATTN_TREE, d=d, fp32=fp32)
    # step 1 (prompt phase in a verify batch): 12 prompt tokens, causal
    infos = [(3, p, 1, p, p + 1, 0, 0, 0) for p in range(12)]
    out, qs = c.run(infos, masks=[[0]] * 2, rng=rng)
    for t, i in enumerate(infos):
        c.check(out[t], c.ref_row(qs[t], 1, range(i[1] + 1)))
    # step 2: token tree rooted at depth 12 (layer order), ntcs = 12
    parents = [-1, 0, 1, 2, 2, 3, 4]  # root a b c1 c2 d1 d2
    depth = [12, 13, 14, 15, 15, 16, 16]
    m = tree_masks(parents)
    infos = [(4, depth[j], 1, 12 + j, 12, 12, 7, j) for j in range(7)]
    out, qs = c.run(infos, masks=[[0], m], rng=rng)
    for j in range(7):
        anc = []
        a = j
        while a >= 0:
            anc.append(12 + a)
            a = parents[a]
        c.check(out[j], c.ref_row(qs[j], 1, list(range(12)) + sorted(anc)))
    # step 3: commit root,a,b,c2 (batch idx 0,1,2,4) to depths 12..15; new
    # tree of 3 nodes at depth 16.. (ntcs = 16)
    commits = [(0, 1, 12), (1, 1, 13), (2, 1, 14), (4, 1, 15)]
    parents = [-1, 0, 0]
    m = tree_masks(parents)
    dep = [16, 17, 17]
    infos = [(4, dep[j], 1, 16 + j, 16, 16, 3, j) for j in range(3)]
    out, qs = c.run(infos, masks=[[0], m], commits=commits, rng=rng)
    for j in range(3):
        vis = list(range(16)) + [16] + ([16 + j] if j else [])
        c.check(out[j], c.ref_row(qs[j], 1, vis))


@pytest.mark.parametrize("d", [64, 128])
def test_attention_tree_fused_equals_two_launch_path(d, monkeypatch):
    """Verify steps (21-token trees for two requests, commits of the previous
    step) through the one-launch path -- with the item's queries split over
    two workgroups (FFMI_ATTN_QSPLIT=2, the TP >= 2 form) and unsplit -- and
    the KV-update + attention path: outputs, K cache and V^T cache
    bit-identical."""
    def scenario():
        rng = np.random.default_rng(300 + d)
        c = AttnCase(F.ATTN_TREE, d=d)
        infos = [(3, p, r, p, p + 1, 0, 0, 0) for r in (0, 2) for p in range(12)]
        o1, _ = c.run(infos, masks=[[0]] * 3, rng=rng)
        parents = [-1, 0, 1] + [2 + (j - 3) // 3 for j in range(3, 21)]
        m = tree_masks(parents)
        depth = [12]
        for j in range(1, 21):
            depth.append(depth[parents[j]] + 1)
        infos = [(4, depth[j], r, 12 + j, 12, 12, 21, j) for r in (0, 2) for j in range(21)]
        o2, _ = c.run(infos, masks=[m, [0], m], rng=rng)
        # accept a path of 4 per request, then a fresh 21-token tree at 16
        commits = [(21 * k + j, r, 12 + i) for k, r in enumerate((0, 2))
                   for i, j in enumerate([0, 1, 2, 5])]
        infos = [(4, depth[j] + 4, r, 16 + j, 16, 16, 21, j) for r in (0, 2) for j in range(21)]
        o3, _ = c.run(infos, masks=[m, [0], m], commits=commits, rng=rng)
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        slots = ctypes.c_int()
        F.check(L.ffmi_attn_kv_ptrs(c.h, ctypes.byref(k), ctypes.byref(v), ctypes.byref(slots)))
        n = 4 * c.heads * slots.value * c.d
        kc, vc = np.empty(n, np.uint16), np.empty(n, np.uint16)
        hip().hipMemcpy(kc.ctypes.data, k, n * 2, 2)
        hip().hipMemcpy(vc.ctypes.data, v, n * 2, 2)
        return o1, o2, o3, kc, vc
    monkeypatch.setenv("FFMI_ATTN_QSPLIT", "2")
    qsplit = scenario()
    monkeypatch.setenv("FFMI_ATTN_QSPLIT", "0")
    fused = scenario()
    monkeypatch.setenv("FFMI_ATTN_NO_FUSE", "1")
    split = scenario()
    for a, b, c in zip(qsplit, fused, split):
        assert np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16))
        assert np.array_equal(np.asarray(b).view(np.uint16), np.asarray(c).view(np.uint16))


def random_layer_tree(rng, n, max_width=4):
    """A random token tree of n nodes in layer order (the scheduler's
    serialisation): parents precede children, depths non-decreasing."""
    parents, depth = [-1], [0]
    layer = [0]
    while len(parents) < n:
        nxt = []
        for p in layer:
            for _ in range(int(rng.integers(1, max_width + 1))):
                if len(parents) == n:
                    break
                parents.append(p)
                depth.append(depth[p] + 1)
                nxt.append(len(parents) - 1)
        layer = nxt or [len(parents) - 1]
    return parents, depth


@pytest.mark.parametrize("path", ["default", "qsplit", "two_launch"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("seed", range(6 * RS))
def test_attention_tree_random_trees_vs_oracle(d, seed, path, monkeypatch):
    _random_tree_case(d, seed, path, monkeypatch, fp32=False)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("seed", range(4 * RS))
def test_attention_f32_random_trees_vs_oracle(d, seed, monkeypatch):
    """the DT_FLOAT attention handle (fp32 caches, --use-full-precision) on
    the same random trees, prefixes and commits: every row within 2e-6 of
    the oracle's fp32 attention"""
    _random_tree_case(d, seed, "default", monkeypatch, fp32=True)


def _random_tree_case(d, seed, path, monkeypatch, fp32, plen_range=(1, 100), max_seq=200,
                      prefill_rows=None):
    """Tree verification at random shapes against the oracle: 1-4 requests
    with random prompt lengths (crossing the 32-key chunks and the LDS tail),
    random layer-order trees of 1-64 nodes (the merged multi-SSM bound: mask
    bit 63; trees over 32 nodes take two work items and the two-launch path),
    then a step that commits a random accepted path and verifies a fresh
    random tree -- every query row checked against O.attention_row (the
    exact-fraction bar over all rows of the test, not per 128-element row);
    through the default launch, the query-split one (the TP >= 2 form) and
    the KV-update + attention pair.  plen_range / max_seq: other prompt
    lengths and the handle to hold them; prefill_rows: check that many
    sampled prefill rows instead of all (long prompts)."""
    if path == "qsplit":
        monkeypatch.setenv("FFMI_ATTN_QSPLIT", "2")
    elif path == "two_launch":
        monkeypatch.setenv("FFMI_ATTN_NO_FUSE", "1")
    rng = np.random.default_rng(1000 + OFF + 10 * d + seed)
    R = int(rng.integers(1, 5))
    c = AttnCase(F.ATTN_TREE, d=d, max_requests=4, max_seq=max_seq, tree=64,
                 max_tokens=max(512, 4 * plen_range[1]), fp32=fp32)
    plen = {r: int(rng.integers(*plen_range)) for r in range(R)}
    infos = [(3, p, r, p, p + 1, 0, 0, 0) for r in range(R) for p in range(plen[r])]
    out, qs = c.run(infos, masks=[[0]] * R, rng=rng)
    got, want = [], []
    rows = range(len(infos))
    if prefill_rows is not None and prefill_rows < len(infos):
        rows = np.random.default_rng(seed).choice(len(infos), size=prefill_rows, replace=False)
    for t in rows:
        i = infos[t]
        got.append(out[t])
        want.append(c.ref_row(qs[t], i[2], range(i[1] + 1)))
    ntcs = dict(plen)
    commits = []
    for step in range(2):
        trees, infos, masks = {}, [], []
        for r in range(R):
            n = int(rng.choice([1, 2, 7, 21, 27, 33, 48, 63, 64]))
            parents, depth = random_layer_tree(rng, n)
            trees[r] = (parents, depth, len(infos))
            masks.append(tree_masks(parents))
            infos += [(4, ntcs[r] + depth[j], r, ntcs[r] + j, ntcs[r], ntcs[r], n, j)
                      for j in range(n)]
        out, qs = c.run(infos, masks=masks, commits=commits, rng=rng)
        for r in range(R):
            parents, depth, off = trees[r]
            for j in range(len(parents)):
                anc, a = [], j
                while a >= 0:
                    anc.append(ntcs[r] + a)
                    a = parents[a]
                got.append(out[off + j])
                want.append(c.ref_row(qs[off + j], r, list(range(ntcs[r])) + sorted(anc)))
        # accept a random root-to-node path per request: commit it in order
        commits = []
        for r in range(R):
            parents, depth, off = trees[r]
            a, path = int(rng.integers(0, len(parents))), []
            while a >= 0:
                path.append(a)
                a = parents[a]
            for k, j in enumerate(reversed(path)):
                commits.append((off + j, r, ntcs[r] + k))
            ntcs[r] += len(path)
    c.check(np.stack(got), np.stack(want))


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_long_context_vs_oracle(d):
    """Long contexts (up to ~3000 keys: ~95 32-key chunks, many per wave):
    a chunked prefill of 3 requests (1024-token steps, requests interleaved;
    48 sampled rows per step) and a decode step at that depth, against the
    oracle."""
    rng = np.random.default_rng(31 + d)
    R = 3
    c = AttnCase(F.ATTN_INC, d=d, heads=2, max_requests=R, max_seq=3200, tree=64, max_tokens=1024)
    plen = {r: int(rng.integers(900, 3000)) for r in range(R)}
    got, want = [], []
    done = {r: 0 for r in range(R)}
    while any(done[r] < plen[r] for r in range(R)):  # 1024-token chunks, requests interleaved
        infos, budget = [], 1024
        for r in range(R):
            n = min(plen[r] - done[r], budget)
            infos += [(3, p, r, p, p + 1, 0, 0, 0) for p in range(done[r], done[r] + n)]
            done[r] += n
            budget -= n
        out, qs = c.run(infos, rng=rng)
        for t in rng.choice(len(infos), size=min(48, len(infos)), replace=False):  # sampled rows
            i = infos[t]
            got.append(out[t])
            want.append(c.ref_row(qs[t], i[2], range(i[1] + 1)))
    infos = [(7, plen[r], r, plen[r], plen[r] + 1, 0, 0, 0) for r in range(R)]
    out, qs = c.run(infos, rng=rng)
    for t, i in enumerate(infos):
        got.append(out[t])
        want.append(c.ref_row(qs[t], i[2], range(i[1] + 1)))
    c.check(np.stack(got), np.stack(want))


@pytest.mark.parametrize("seed", range(8 * RS))
def test_attention_spec_random_beam_trees_vs_oracle(seed):
    """SSM beam steps at random shapes (the 68M SSM's d = 64): 1-4 requests
    with random prompts, then one step per tree layer -- the layer's nodes are
    the queries, earlier layers already stored by earlier steps -- over random
    layer-order trees of up to 64 nodes (widths up to 4, merged-tree sizes);
    every query row against O.attention_row over its prefix + ancestors
    (the exact-fraction bar over all rows of the test)."""
    rng = np.random.default_rng(2000 + OFF + seed)
    R = int(rng.integers(1, 5))
    c = AttnCase(F.ATTN_SPEC, d=64, max_requests=4, max_seq=160, tree=64, max_tokens=512)
    plen = {r: int(rng.integers(1, 100)) for r in range(R)}
    infos = [(3, p, r, p, p + 1, 0, 0, 0) for r in range(R) for p in range(plen[r])]
    c.run(infos, masks=[[0]] * R, rng=rng)
    got, want = [], []
    trees = {r: random_layer_tree(rng, int(rng.choice([2, 9, 21, 33, 64]))) for r in range(R)}
    masks = [tree_masks(trees[r][0]) for r in range(R)]
    depth_max = max(max(trees[r][1]) for r in range(R))
    for layer in range(depth_max + 1):  # the root (layer 0) first
        infos, who = [], []
        for r in range(R):
            parents, depth = trees[r]
            nodes = [j for j in range(len(parents)) if depth[j] == layer]
            if not nodes:
                continue
            ntcs, tl = plen[r], nodes[-1] + 1  # stored so far: layers <= this one
            infos += [(5, ntcs + layer, r, ntcs + j, ntcs, ntcs, tl, j) for j in nodes]
            who += [(r, j) for j in nodes]
        out, qs = c.run(infos, masks=masks, rng=rng)
        for t, (r, j) in enumerate(who):
            anc, a = [], j
            while a >= 0:
                anc.append(plen[r] + a)
                a = trees[r][0][a]
            got.append(out[t])
            want.append(c.ref_row(qs[t], r, list(range(plen[r])) + sorted(anc)))
    c.check(np.stack(got), np.stack(want))


@pytest.mark.parametrize("fp32", [False, True])
def test_attention_spec_beam_layers(fp32):
    _spec_beam_layers(AttnCase(F.ATTN_SPEC, d=64, fp32=fp32), 8, np.random.default_rng(7))


def _spec_beam_layers(c, ntcs, rng, **run_kw):
    """beam layers over a prompt of ntcs + 1 tokens (root = the last one);
    run_kw: further arguments of every AttnCase.run call (slabs)"""
    infos = [(3, p, 0, p, p + 1, 0, 0, 0) for p in range(ntcs + 1)]
    c.run(infos, masks=[[0]], rng=rng, **run_kw)
    # tree so far: root(idx0 @ slot ntcs) -> n1 (idx1) -> {n2, n3} (idx 2,3);
    # this step's layer: n4 (child of n2), n5 (child of n3) at tree idx 4,5
    parents = [-1, 0, 1, 1, 2, 3]
    m = tree_masks(parents)
    # earlier layers were stored by previous steps: emulate with one step
    infos = [(5, ntcs + 1, 0, ntcs + 1, ntcs, ntcs, 2, 1)]
    c.run(infos, masks=[m], rng=rng, **run_kw)
    infos = [(5, ntcs + 2, 0, ntcs + 2 + k, ntcs, ntcs, 4, 2 + k) for k in range(2)]
    c.run(infos, masks=[m], rng=rng, **run_kw)
    infos = [(6, ntcs + 3, 0, ntcs + 4 + k, ntcs, ntcs, 6, 4 + k) for k in range(2)]
    out, qs = c.run(infos, masks=[m], rng=rng, **run_kw)
    for k in range(2):
        j = 4 + k
        anc = []
        a = j
        while a >= 0:
            anc.append(ntcs + a)
            a = parents[a]
        c.check(out[k], c.ref_row(qs[k], 0, list(range(ntcs)) + sorted(anc)))


# ------------------------------------------- fp32 attention past 256 keys
# f32_attention_kernel walks the keys in strides of its 256 threads (scores,
# exp / sum, and the 256 / d key groups of P.V): beyond 256 visible keys a
# thread takes a second and later keys.  Bar of every test below:
# AttnCase.check's fp32 rule, 2e-6 * max(1, max|ref|).  The oracle's fp32 row
# is within 1.9e-7 of an fp64 softmax.V at 300 - 15999 random-normal keys and
# the kernel's grouped fp32 summation within 8.1e-8 (numpy emulation), so the
# bar is ~10x the reference's own error; one dropped key moves an output by
# ~1e-4 or more.
def _max_err(got, want):
    return float(np.abs(np.asarray(got, np.float32) - np.asarray(want, np.float32)).max())


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_f32_inc_past_one_pass_of_keys(d):
    """INC on an fp32 handle, 2 heads: one request prefilled to 1200 keys in
    steps of at most 512 tokens, a short request interleaved with it (first
    in the batch in the second step), then a decode token at 1200.  Checked
    rows: the positions either side of 1, 2 and 4 passes of the 256 threads
    (254-257, 510-513, 1023, 1024), 1199, 16 more at random, the decode
    token, and every row of the short request."""
    rng = np.random.default_rng(4300 + OFF + d)
    c = AttnCase(F.ATTN_INC, d=d, heads=2, max_requests=2, max_seq=1216, tree=32, max_tokens=512,
                 fp32=True)
    fixed = [254, 255, 256, 257, 510, 511, 512, 513, 1023, 1024, 1199]
    pick = set(fixed) | set(rng.choice(1200, size=16, replace=False).tolist())
    got, want = [], []
    steps = [((0, 500), (0, 12)), ((500, 1000), (12, 24)), ((1000, 1200), (24, 31)),
             ((1200, 1201), (31, 32))]
    for n, ((a0, a1), (b0, b1)) in enumerate(steps):
        long_ = [(3, p, 0, p, p + 1, 0, 0, 0) for p in range(a0, a1)]
        short = [(3, p, 1, p, p + 1, 0, 0, 0) for p in range(b0, b1)]
        infos = short + long_ if n == 1 else long_ + short
        assert len(infos) <= 512
        out, qs = c.run(infos, rng=rng)
        for t, i in enumerate(infos):
            if i[2] == 1 or i[1] in pick or i[1] == 1200:
                got.append(out[t])
                want.append(c.ref_row(qs[t], i[2], range(i[1] + 1)))
    assert len(got) >= len(fixed) + 1 + 32
    report("attention_f32_inc_1200_keys", d=d, rows=len(got),
           max_abs_err=_max_err(np.stack(got), np.stack(want)))
    c.check(np.stack(got), np.stack(want))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("seed", range(2 * RS))
def test_attention_f32_random_trees_long_prefix(d, seed, monkeypatch):
    """_random_tree_case on an fp32 handle with prompts of 260-700 tokens, so
    every tree slot and every commit lies beyond key 256 (64 sampled prefill
    rows, every tree row of both verify steps)"""
    _random_tree_case(d, 50 + seed, "default", monkeypatch, fp32=True, plen_range=(260, 701),
                      max_seq=800, prefill_rows=64)


def test_attention_f32_spec_beam_layers_long_prefix():
    """test_attention_spec_beam_layers on an fp32 handle with a 300-token
    prefix: the beam layers' tree slots are in the kernel's second pass"""
    c = AttnCase(F.ATTN_SPEC, d=64, max_seq=352, max_tokens=512, fp32=True)
    _spec_beam_layers(c, 300, np.random.default_rng(4310 + OFF))


@pytest.mark.parametrize("d", [64, 128])
def test_attention_f32_llama3_rope_scaling(d):
    """test_attention_llama3_rope_scaling's configuration on an fp32 handle:
    the handle's host-built llama3 table feeds the fp32 KV update"""
    rng = np.random.default_rng(200 + d)
    c = AttnCase(F.ATTN_INC, d=d, theta=500000.0, llama3=(8.0, 1.0, 4.0, 64), fp32=True)
    lens = {0: 33, 1: 57}
    infos = [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]
    out, qs = c.run(infos, rng=rng)
    want = np.stack([c.ref_row(qs[t], i[2], range(i[1] + 1)) for t, i in enumerate(infos)])
    report("attention_f32_llama3_rope", d=d, max_abs_err=_max_err(out[:len(infos)], want))
    c.check(out[:len(infos)], want)


def _f32_handle_filled_to_the_last_slot(d, total, name):
    """An fp32 INC handle of `total` slots (1 head, 1 request) filled
    cheaply -- fill tokens carry their real pos and store_slot but
    prefix_len = 1 (ffmi_batch_upload does not relate prefix_len to pos, and
    the fp32 kernels ignore the work items) -- then three causal queries with
    the full prefix, the last of which sees the last slot, and one over the
    first half of the cache that stores nothing."""
    rng = np.random.default_rng(4320 + OFF + d + total)
    c = AttnCase(F.ATTN_INC, heads=1, d=d, max_requests=1, max_seq=total - 32, tree=32,
                 max_tokens=2048, fp32=True)
    assert c.slots == total
    fill = total - 3
    for s in range(0, fill, 2048):
        c.run([(3, p, 0, p, 1, 0, 0, 0) for p in range(s, min(fill, s + 2048))], rng=rng)
    mid = total // 2
    infos = [(3, p, 0, p, p + 1, 0, 0, 0) for p in range(fill, total)] + \
            [(3, mid, 0, -1, mid, 0, 0, 0)]
    out, qs = c.run(infos, rng=rng)
    want = np.stack([c.ref_row(qs[t], 0, range(i[4])) for t, i in enumerate(infos)])
    report(name, d=d, slots=total, lds_bytes=(d + 256 + total) * 4,
           max_abs_err=_max_err(out[:len(infos)], want))
    c.check(out[:len(infos)], want)


def test_attention_f32_handle_8192_slots():
    """an fp32 handle of 8192 slots (33.5 KiB of dynamic LDS, 32 passes of the
    256 threads), every slot written, queried to the last one"""
    _f32_handle_filled_to_the_last_slot(128, 8192, "attention_f32_handle_8192_slots")


@pytest.mark.parametrize("d,total", [(128, 16000), (32, 16096)])
def test_attention_f32_handle_at_the_lds_bound(d, total):
    """The largest fp32 handle ffmi_attn_create accepts: (head_dim + 256 +
    slots) * 4 == 64 KiB of dynamic LDS exactly, on top of the kernel's 48 B
    of static LDS.  The launch must be accepted and the row that sees the last
    slot must be right."""
    assert (d + 256 + total) * 4 == 64 * 1024
    _f32_handle_filled_to_the_last_slot(d, total, "attention_f32_handle_at_lds_bound")


# ------------------------------------------------ fp32 KV cache, bit-exact
@pytest.mark.parametrize("d", [64, 128])
def test_attention_f32_kv_cache_bit_exact(d):
    """The fp32 K / V caches read back through ffmi_attn_kv_ptrs
    ([req][head][slot][d]) after every step of a TREE scenario: prefill; a
    tree step; a step that commits an accepted path, has one commit whose
    depth equals a slot stored in the same step (commit_overlap: the
    reference commits, then stores, so the store wins) and one token with
    store_slot = -1 (staged, not stored); a step that commits that token's
    staged row.

    Every written K row must equal a*c - b*s | a*s + b*c in numpy float32
    from O.rope_table (products rounded, then summed: bit for bit the
    oracle's rope_apply), every written V row the input bits, committed slots
    the previous step's staged rows, and every slot the step did not write
    its bits before the step."""
    rng = np.random.default_rng(4330 + OFF + d)
    R = 2
    c = AttnCase(F.ATTN_TREE, d=d, max_requests=R, fp32=True)
    tab = O.rope_table(c.slots, d, 10000.0).reshape(c.slots, d // 2, 2)
    h = d // 2

    def read():
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        F.check(L.ffmi_attn_kv_ptrs(c.h, ctypes.byref(k), ctypes.byref(v), None))
        n = R * c.heads * c.slots * d
        kc, vc = np.empty(n, np.uint32), np.empty(n, np.uint32)
        assert hip().hipMemcpy(kc.ctypes.data, k, n * 4, 2) == 0
        assert hip().hipMemcpy(vc.ctypes.data, v, n * 4, 2) == 0
        shape = (R, c.heads, c.slots, d)
        return kc.reshape(shape), vc.reshape(shape)

    state = dict(staged=None, rows=0)

    def step(infos, masks, commits=()):
        k0, v0 = read()
        c.run(infos, masks=masks, commits=commits, rng=rng)
        k1, v1 = read()
        staged = []
        for t, i in enumerate(infos):  # this step's rotated k and v, the stated formula
            x = c.last_qkv[t, c.Hl:2 * c.Hl].reshape(c.heads, d)
            a, b = x[:, :h], x[:, h:]
            cs, sn = tab[i[1], :, 0], tab[i[1], :, 1]
            kr = np.concatenate([a * cs - b * sn, a * sn + b * cs], axis=1)
            assert kr.dtype == np.float32
            staged.append((kr, c.last_qkv[t, 2 * c.Hl:].reshape(c.heads, d)))
        written = {}
        for src, req, depth in commits:  # commits first, from the previous step's rows
            written[(req, depth)] = state["staged"][src]
        for t, i in enumerate(infos):   # then the step's stores
            if i[3] >= 0:
                written[(i[2], i[3])] = staged[t]
        untouched = np.ones((R, c.slots), bool)
        for (req, slot), (kr, vr) in written.items():
            untouched[req, slot] = False
            assert np.array_equal(k1[req, :, slot], kr.view(np.uint32)), ("K", req, slot)
            assert np.array_equal(v1[req, :, slot], vr.view(np.uint32)), ("V", req, slot)
        for a1, a0 in ((k1, k0), (v1, v0)):
            assert np.array_equal(a1.transpose(0, 2, 1, 3)[untouched],
                                  a0.transpose(0, 2, 1, 3)[untouched])
        state["staged"] = staged
        state["rows"] += len(written)

    step([(3, p, 1, p, p + 1, 0, 0, 0) for p in range(12)], [[0]] * 2)
    parents = [-1, 0, 1, 2, 2, 3, 4]  # root a b c1 c2 d1 d2
    depth = [12, 13, 14, 15, 15, 16, 16]
    step([(4, depth[j], 1, 12 + j, 12, 12, 7, j) for j in range(7)], [[0], tree_masks(parents)])
    # commit root, a, b, c2 to depths 12..15 and d2 to depth 16 -- the slot the
    # new tree's root stores in this step; the new tree's last node stores nothing
    commits = [(0, 1, 12), (1, 1, 13), (2, 1, 14), (4, 1, 15), (6, 1, 16)]
    parents = [-1, 0, 0, 1]
    dep = [16, 17, 17, 18]
    infos = [(4, dep[j], 1, 16 + j if j < 3 else -1, 16, 16, 4, j) for j in range(4)]
    step(infos, [[0], tree_masks(parents)], commits)
    # commit the row that was only staged (token 3), store one more token
    step([(4, 19, 1, 19, 19, 0, 0, 0)], [[0]] * 2, [(0, 1, 16), (1, 1, 17), (3, 1, 18)])
    assert state["rows"] == 12 + 7 + (5 + 3 - 1) + (3 + 1)
    report("attention_f32_kv_cache_bit_exact", d=d, rows_checked=state["rows"])


def test_embedding_exact():
    rng = np.random.default_rng(3)
    V, H, T = 300, 256, 7
    table = f16(rng.standard_normal((V, H)))
    ids = [5, 0, 299, 5, 17, 100, 3]
    toks = (F.TokenInfo * T)(*[F.TokenInfo(i, 0, 0, -1, 1, 0, 0, 0, 0) for i in ids])
    b = ctypes.c_void_p()
    F.check(L.ffmi_batch_create(16, 2, ctypes.byref(b)))
    desc = F.BatchDesc(T, 0, 0, 0, toks, None, None, None)
    F.check(L.ffmi_batch_upload(b, ctypes.byref(desc), None))
    tb, ob = Buf(table), Buf.empty((T, H), np.float16)
    F.check(L.ffmi_embedding(b, tb.ptr, ob.ptr, H, None))
    assert np.array_equal(ob.get(), table[ids])
    L.ffmi_batch_destroy(b)


def test_allreduce_single_rank_and_silu():
    uid = ctypes.create_string_buffer(128)
    F.check(L.ffmi_comm_unique_id(uid))
    comm = ctypes.c_void_p()
    F.check(L.ffmi_comm_create(uid, 1, 0, ctypes.byref(comm)))
    x = f16(np.arange(1000) * 0.01)
    a, b = Buf(x), Buf.empty((1000,), np.float16)
    F.check(L.ffmi_allreduce(comm, a.ptr, b.ptr, 1000, F.F16, None))
    assert np.array_equal(b.get(), x)
    L.ffmi_comm_destroy(comm)
    rng = np.random.default_rng(2)
    g, u = f16(rng.standard_normal(5000) * 3), f16(rng.standard_normal(5000))
    gb, ub, ob = Buf(g), Buf(u), Buf.empty((5000,), np.float16)
    F.check(L.ffmi_silu_mul(gb.ptr, ub.ptr, ob.ptr, 5000, None))
    close16(ob.get(), O.silu_mul(g.astype(np.float32), u.astype(np.float32)), 1, 0.995)


@pytest.mark.parametrize("T", [1, 8, 24, 64, 168, 300])
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("K", [1024, 4096])
def test_linear_weight_stream_hint(T, epi, K):
    """FFMI_W_STREAM (non-temporal weight loads): M-split launches (one and
    several row blocks) and short-K skinny launches give the same bits as the
    default policy; long-K skinny launches (>= 8 batches of k-steps per wave
    at 8 waves) keep 4 waves under the hint, a different fp32 summation
    order, so there the two policies agree within the oracle tolerance."""
    rng = np.random.default_rng(2000 + T + epi)
    N = 1024
    X = f16(rng.standard_normal((T, K)))
    if epi:
        Wg, Wu = f16(rng.uniform(-0.05, 0.05, (N, K))), f16(rng.uniform(-0.05, 0.05, (N, K)))
        gb, ub = Buf(Wg), Buf(Wu)
        Wp = Buf.empty((2 * L.ffmi_linear_packed_bytes(N, K) // 2,), np.uint16)
        F.check(L.ffmi_linear_pack_gate_up(gb.ptr, ub.ptr, N, K, Wp.ptr, None))
    else:
        Wp = packed(f16(rng.uniform(-0.05, 0.05, (N, K))))
    Xb = Buf(X)
    Y0, Y1 = Buf.empty((T, N), np.float16), Buf.empty((T, N), np.float16)
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Y0.ptr, T, N, K, epi, None))
    F.check(L.ffmi_linear(Xb.ptr, Wp.ptr, Y1.ptr, T, N, K, epi | F.W_STREAM, None))
    # the 4-wave rule under the hint is a fixed 64 k-steps per slice (gemm_plan.cpp
    # skinny_tiles), independent of T
    if T > 64 or epi or K // 32 < 64:
        assert np.array_equal(Y0.get().view(np.uint16), Y1.get().view(np.uint16))
    else:
        close16(Y1.get(), Y0.get().astype(np.float32), max_ulp=2, exact_frac=0.9)
