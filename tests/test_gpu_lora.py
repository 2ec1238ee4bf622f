"""Kernel-level tests of the LoRA update (kernels/lora.hip) through
ffmi_lora_apply.  Run on an MI355X: pytest -m gpu.

tests/lora_rule.py holds the rule and both checks: selector adapters (h and y'
bit-exact: every index pinned) and dense adapters (the kernel's own h_out and
y' inside the rule's first-order intervals); tests/test_lora_cpu.py shows that
the intervals hold for any summation order and reject a dropped k-slice and a
swapped adapter.  Every launch also checks that rows without an adapter, the
guard words around y and the h_out rows of rows without an adapter come back
bit-identical.

Reached: (F, H) with 2 .. 11 parts of F, the last one short, an odd k-step
count, H below and above one 256-column block; ranks 1, 12, 16, 64 (1 .. 4
waves of the shrink); T 1 .. 168 (1 .. 11 row tiles, ragged last tile); x
row-major and in packed activation tiles; tiles whose rows name up to three
adapters with gaps; slots that name no loaded adapter.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import lora_rule as LR
from hip_util import Buf, report

pytestmark = pytest.mark.gpu

L = None


def setup_module(module):
    global L
    L = F.lib()


def pack_tiles(a):
    """[rows][K] fp16 -> packed activation tiles over whole 16-row groups
    (ffmi_internal.h act_packed_off), rows padded with a NaN pattern the
    kernel must not let into a real row"""
    a = np.asarray(a)
    rows, K = a.shape
    Rp = (rows + 15) & ~15
    pad = np.full((Rp, K), 0x7E00, np.uint16)
    pad[:rows] = a.view(np.uint16)
    m, n = np.meshgrid(np.arange(Rp), np.arange(K), indexing="ij")
    off = ((((m >> 4) * (K >> 5) + (n >> 5)) * 64 + (m & 15) + 16 * ((n >> 3) & 3)) << 3) + (n & 7)
    out = np.empty(Rp * K, np.uint16)
    out[off.ravel()] = pad.ravel()
    return out


class Table:
    """the device table of ffmi_lora_apply for {id: lora_rule.Adapter}"""

    def __init__(self, adapters, F_, H):
        self.bufs = []
        ent = (F.LoraEntry * LR.MAX_ADAPTERS)()
        for i, ad in adapters.items():
            A = np.zeros((LR.R_MAX, F_), np.float16)
            A[:ad.r] = ad.A
            B = np.zeros((H, LR.R_MAX), np.float16)
            B[:, :ad.r] = ad.B
            a, b = Buf(pack_tiles(A)), Buf(B)
            self.bufs += [a, b]
            ent[i] = F.LoraEntry(a.ptr, b.ptr, float(ad.s16), ad.r)
        self.dev = Buf(np.frombuffer(bytes(ent), np.uint8))


def apply(x, y, slots, table, packed):
    """one launch: (h_out [T][64] fp16 with untouched rows still the sentinel,
    y' [T][H]); asserts the guards around y"""
    T, F_ = x.shape
    H = y.shape[1]
    xb = Buf(pack_tiles(x)) if packed else Buf(x)
    ybuf = np.full(T * H + 2 * LR.GUARD, LR.SENTINEL, np.uint16)
    ybuf[LR.GUARD:LR.GUARD + T * H] = y.view(np.uint16).ravel()
    yb = Buf(ybuf)
    hb = Buf(np.full((T, LR.R_MAX), LR.SENTINEL, np.uint16))
    sb = Buf(np.asarray(slots, np.int32))
    nws = L.ffmi_lora_workspace_bytes(T, F_)
    assert nws == -(-F_ // LR.CHUNK) * T * LR.R_MAX * 4
    ws = Buf(np.full(nws // 4, np.nan, np.float32))
    F.check(L.ffmi_lora_apply(xb.ptr, T, F_, H, sb.ptr, table.dev.ptr,
                              ctypes.c_void_p(yb.ptr.value + 2 * LR.GUARD), int(packed), ws.ptr,
                              nws, hb.ptr, None), "ffmi_lora_apply")
    got = yb.get()
    assert (got[:LR.GUARD] == LR.SENTINEL).all() and (got[-LR.GUARD:] == LR.SENTINEL).all()
    return hb.get().view(np.float16), got[LR.GUARD:-LR.GUARD].view(np.float16).reshape(T, H)


def pattern(T):
    """MIXED_40's runs (3 a0, 1 none, 17 a1, 2 a0, 16 none, 1 a2), repeated and cut to T"""
    s = LR.slots_of(LR.MIXED_40)
    return np.resize(s, T).astype(np.int32)


def data(T, F_, H, seed):
    rng = np.random.default_rng([seed, T, F_, H])
    return LR.f16(rng.standard_normal((T, F_))), LR.f16(rng.standard_normal((T, H)))


def check_untouched(h, out, y, slots, adapters):
    none = ~np.isin(slots, list(adapters))
    assert (out[none].view(np.uint16) == y[none].view(np.uint16)).all(), "a row without adapter written"
    assert (h[none].view(np.uint16) == LR.SENTINEL).all(), "h_out of a row without adapter written"
    for a, ad in adapters.items():  # beyond the rank rounded up to 16: zero
        rows = slots == a
        assert not h[rows][:, (ad.r + 15) & ~15:].any()
        assert not h[rows][:, ad.r:].any(), "zero padding of A read as non-zero"


@pytest.mark.parametrize("F_,H", LR.SHAPES)
def test_selector_adapters_pin_every_index(F_, H):
    tally = LR.Tally()
    for r in LR.RANKS:
        ads = {0: LR.Selector(r, F_, H, 1, -1), 1: LR.Selector(r, F_, H, 2, 1),
               2: LR.Selector(max(1, r // 2), F_, H, 3, 0)}
        tab = Table(ads, F_, H)
        for T in LR.TS:
            x, y = data(T, F_, H, r)
            slots = pattern(T)
            for packed in (0, 1):
                h, out = apply(x, y, slots, tab, packed)
                check_untouched(h, out, y, slots, ads)
                for a, ad in ads.items():
                    rows = slots == a
                    if rows.any():
                        ad.check_h(h[rows][:, :ad.r], x[rows], tally)
                        want = ad.want_y(y[rows], h[rows][:, :ad.r])
                        assert (out[rows].view(np.uint16) == want.view(np.uint16)).all(), (r, T, a)
    report(f"lora_selector[{F_}-{H}]", **tally.finish())


@pytest.mark.parametrize("F_,H", LR.SHAPES)
def test_dense_adapters_stay_in_the_rule_intervals(F_, H):
    worst = 0.0
    for r in LR.RANKS:
        rng = np.random.default_rng([F_, H, r])
        ads = {0: LR.dense(r, F_, H, rng), 1: LR.dense(16, F_, H, rng, alpha=8.0),
               2: LR.dense(LR.RANKS[(LR.RANKS.index(r) + 1) % 4], F_, H, rng, b_scale=0.5)}
        tab = Table(ads, F_, H)
        for T in LR.TS:
            x, y = data(T, F_, H, 100 + r)
            slots = pattern(T)
            for packed in (0, 1):
                h, out = apply(x, y, slots, tab, packed)
                check_untouched(h, out, y, slots, ads)
                for a, ad in ads.items():
                    rows = slots == a
                    if not rows.any():
                        continue
                    hk = np.ascontiguousarray(h[rows][:, :ad.r])
                    ref, e = ad.h_ref(x[rows])
                    ok = LR.in_interval(hk, ref, e)
                    assert ok.all(), (r, T, a, packed, "h", int((~ok).sum()))
                    worst = max(worst, float((np.abs(hk.astype(np.float64) - ref) /
                                              (e + np.abs(ref) * 2.0 ** -11 + 1e-30)).max()))
                    ref, e = ad.y_ref(y[rows], hk)
                    ok = LR.in_interval(out[rows], ref, e)
                    assert ok.all(), (r, T, a, packed, "y", int((~ok).sum()))
                    assert (out[rows] != y[rows]).mean() > 0.3  # (the update is there)
    report(f"lora_dense[{F_}-{H}]", h_err_over_bound_plus_half_ulp=worst)


@pytest.mark.parametrize("F_,H", LR.SHAPES)
def test_a_row_has_the_same_bits_alone_and_in_every_mixed_batch(F_, H):
    rng = np.random.default_rng([F_, H])
    ads = {0: LR.dense(12, F_, H, rng), 1: LR.dense(64, F_, H, rng), 2: LR.dense(1, F_, H, rng)}
    tab = Table(ads, F_, H)
    pool_x, pool_y = data(4, F_, H, 7)  # the rows followed: one per adapter and one without
    pool_s = np.array([0, 1, 2, -1], np.int32)
    alone = [apply(pool_x[i:i + 1], pool_y[i:i + 1], pool_s[i:i + 1], tab, 0) for i in range(4)]
    assert (alone[3][1].view(np.uint16) == pool_y[3].view(np.uint16)).all()
    for T in LR.TS[1:]:
        x, y = data(T, F_, H, 8)
        slots = pattern(T)
        # each followed row placed where the pattern has its adapter (first and last such row)
        put = {}
        for i, a in enumerate(pool_s):
            at = np.nonzero(slots == a)[0]
            for t in {int(at[0]), int(at[-1])} if at.size else ():
                x[t], y[t] = pool_x[i], pool_y[i]
                put[t] = i
        for packed in (0, 1):
            h, out = apply(x, y, slots, tab, packed)
            for t, i in put.items():
                assert (out[t].view(np.uint16) == alone[i][1][0].view(np.uint16)).all(), (T, t, packed)
                assert (h[t].view(np.uint16) == alone[i][0][0].view(np.uint16)).all(), (T, t, packed)
        # the same rows with every other row's adapter changed or removed
        other = np.where(slots == 1, -1, np.where(slots < 0, 1, slots)).astype(np.int32)
        for t, i in put.items():
            other[t] = pool_s[i]
        h, out = apply(x, y, other, tab, 1)
        for t, i in put.items():
            assert (out[t].view(np.uint16) == alone[i][1][0].view(np.uint16)).all(), (T, t)


def test_slots_that_name_no_loaded_adapter_write_nothing():
    F_, H = LR.SHAPES[0]
    rng = np.random.default_rng(5)
    ads = {3: LR.dense(16, F_, H, rng)}
    tab = Table(ads, F_, H)
    x, y = data(20, F_, H, 9)
    for slots in (np.full(20, -1), np.full(20, 5), np.full(20, 8), np.full(20, -7),
                  np.resize([3, 0, 64, -1, 7], 20)):
        slots = np.asarray(slots, np.int32)
        for packed in (0, 1):
            h, out = apply(x, y, slots, tab, packed)
            check_untouched(h, out, y, slots, ads)
            rows = slots == 3
            assert (out[rows] != y[rows]).any() == rows.any()
    # T == 0 launches nothing; a short workspace and F % 32 are refused
    assert L.ffmi_lora_apply(tab.dev.ptr, 0, F_, H, tab.dev.ptr, tab.dev.ptr, tab.dev.ptr, 0, None,
                             0, None, None) == 0
    assert L.ffmi_lora_apply(tab.dev.ptr, 4, F_, H, tab.dev.ptr, tab.dev.ptr, tab.dev.ptr, 0,
                             tab.dev.ptr, 16, None, None) == 1
    assert L.ffmi_lora_apply(tab.dev.ptr, 4, 48, H, tab.dev.ptr, tab.dev.ptr, tab.dev.ptr, 0,
                             tab.dev.ptr, 1 << 20, None, None) == 1
