"""Kernel-level tests of the LoRA update of the fused qkv row (kernels/lora.hip)
through ffmi_lora_apply_qkv.  Run on an MI355X: pytest -m gpu.

The rule and both checks are those of tests/lora_rule.py, applied per segment
(tests/lora_qkv_rule.py): selector adapters (h of every segment and y' bit-exact
from the kernel's own h) and dense adapters (h and y' inside the derived
intervals); tests/test_lora_modules_cpu.py shows that a swapped segment and a
shifted boundary leave the intervals.  Every launch also checks the guard
words around y, the guard columns [sum of the widths, ldy) of every row, rows
without an adapter, and the columns of a segment the row's adapter lacks.

Reached: in_dim 352 (one part plus 96 columns) and 1376 (43 k-steps);
segments (256, 64, 64), whose boundaries 256 and 320 fall inside the second
256-column block, and (128, 128, 128), whose first block holds two segments;
ldy equal to the sum of the widths and 64 beyond it; T 1 .. 168, x row-major
and, for T > 64, in packed activation tiles; ranks 1, 12, 64.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import lora_qkv_rule as QR
import lora_rule as LR
from hip_util import Buf, report
import test_gpu_lora as KL
from test_gpu_lora import Table, pack_tiles, pattern

pytestmark = pytest.mark.gpu

IN_DIMS = (352, 1376)
WIDTHS = ((256, 64, 64), (128, 128, 128))
TS = (1, 17, 65, 168)
RANKS = (1, 12, 64)
CASES = [(f, w) for f in IN_DIMS for w in WIDTHS]
L = None


def setup_module(module):
    global L
    L = KL.L = F.lib()


class Tables:
    """one device table per segment for seg_adapters = 3 x {id: lora_rule.Adapter}"""

    def __init__(self, seg_adapters, in_dim, widths):
        self.tabs = [Table(ads, in_dim, w) for ads, w in zip(seg_adapters, widths)]
        self.ptrs = (ctypes.c_void_p * 3)(*[t.dev.ptr.value for t in self.tabs])
        self.widths = (ctypes.c_int * 3)(*widths)


def apply(x, y, slots, tables, packed):
    """one call: (h_out [3][T][64] fp16 with untouched rows still the sentinel,
    y' [T][ldy]); asserts the guards around y"""
    T, in_dim = x.shape
    ldy = y.shape[1]
    xb = Buf(pack_tiles(x)) if packed else Buf(x)
    ybuf = np.full(T * ldy + 2 * LR.GUARD, LR.SENTINEL, np.uint16)
    ybuf[LR.GUARD:LR.GUARD + T * ldy] = y.view(np.uint16).ravel()
    yb = Buf(ybuf)
    hb = Buf(np.full((3, T, LR.R_MAX), LR.SENTINEL, np.uint16))
    sb = Buf(np.asarray(slots, np.int32))
    nws = L.ffmi_lora_qkv_workspace_bytes(T, in_dim)
    assert nws == 3 * -(-in_dim // LR.CHUNK) * T * LR.R_MAX * 4
    ws = Buf(np.full(nws // 4, np.nan, np.float32))
    F.check(L.ffmi_lora_apply_qkv(xb.ptr, T, in_dim, tables.widths, sb.ptr, tables.ptrs,
                                  ctypes.c_void_p(yb.ptr.value + 2 * LR.GUARD), ldy, int(packed),
                                  ws.ptr, nws, hb.ptr, None), "ffmi_lora_apply_qkv")
    got = yb.get()
    assert (got[:LR.GUARD] == LR.SENTINEL).all() and (got[-LR.GUARD:] == LR.SENTINEL).all()
    return hb.get().view(np.float16), got[LR.GUARD:-LR.GUARD].view(np.float16).reshape(T, ldy)


def data(T, in_dim, widths, ldy, seed):
    """x, and y with sentinel guard columns behind the three segments"""
    rng = np.random.default_rng([seed, T, in_dim, ldy])
    y = LR.f16(rng.standard_normal((T, ldy)))
    y[:, sum(widths):] = np.array(LR.SENTINEL, np.uint16).view(np.float16)
    return LR.f16(rng.standard_normal((T, in_dim))), y


def check_untouched(h, out, y, slots, seg_adapters, widths):
    assert (out[:, sum(widths):].view(np.uint16) == LR.SENTINEL).all(), "a guard column written"
    for s, (c0, c1) in enumerate(QR.bounds(widths)):
        none = ~np.isin(slots, list(seg_adapters[s]))
        assert (out[none, c0:c1].view(np.uint16) == y[none, c0:c1].view(np.uint16)).all(), \
            f"segment {s}: columns of a row without that module written"
        assert (h[s][none].view(np.uint16) == LR.SENTINEL).all(), f"segment {s}: h_out written"
        for a, ad in seg_adapters[s].items():
            assert not h[s][slots == a][:, ad.r:].any(), "zero padding of A read as non-zero"


def launches(in_dim, widths):
    """(T, ldy, packed) of every call of a case"""
    for T in TS:
        for ldy in (sum(widths), sum(widths) + 64):
            for packed in ((0, 1) if T > 64 else (0,)):
                yield T, ldy, packed


@pytest.mark.parametrize("in_dim,widths", CASES)
def test_selector_adapters_pin_every_index_of_every_segment(in_dim, widths):
    tally = LR.Tally()
    for r in RANKS:
        segs = [{0: LR.Selector(r, in_dim, w, 10 + s, -1), 1: LR.Selector(r, in_dim, w, 20 + s, 1),
                 2: LR.Selector(max(1, r // 2), in_dim, w, 30 + s, 0)} for s, w in enumerate(widths)]
        tabs = Tables(segs, in_dim, widths)
        for T, ldy, packed in launches(in_dim, widths):
            x, y = data(T, in_dim, widths, ldy, r)
            slots = pattern(T)
            h, out = apply(x, y, slots, tabs, packed)
            check_untouched(h, out, y, slots, segs, widths)
            for s, (c0, c1) in enumerate(QR.bounds(widths)):
                for a, ad in segs[s].items():
                    rows = slots == a
                    if rows.any():
                        hk = h[s][rows][:, :ad.r]
                        ad.check_h(hk, x[rows], tally)
                        want = ad.want_y(np.ascontiguousarray(y[rows, c0:c1]), hk)
                        assert (out[rows, c0:c1].view(np.uint16) == want.view(np.uint16)).all(), \
                            (r, T, ldy, packed, s, a)
    report(f"lora_qkv_selector[{in_dim}-{widths[0]}]", **tally.finish())


@pytest.mark.parametrize("in_dim,widths", CASES)
def test_dense_adapters_stay_in_the_rule_intervals(in_dim, widths):
    for r in RANKS:
        rng = np.random.default_rng([in_dim, widths[0], r])
        segs = [{0: LR.dense(r, in_dim, w, rng), 1: LR.dense(16, in_dim, w, rng, alpha=8.0),
                 2: LR.dense(RANKS[(RANKS.index(r) + 1) % 3], in_dim, w, rng, b_scale=0.5)}
                for w in widths]
        tabs = Tables(segs, in_dim, widths)
        for T, ldy, packed in launches(in_dim, widths):
            x, y = data(T, in_dim, widths, ldy, 100 + r)
            slots = pattern(T)
            h, out = apply(x, y, slots, tabs, packed)
            check_untouched(h, out, y, slots, segs, widths)
            for s, (c0, c1) in enumerate(QR.bounds(widths)):
                for a, ad in segs[s].items():
                    rows = slots == a
                    if not rows.any():
                        continue
                    hk = np.ascontiguousarray(h[s][rows][:, :ad.r])
                    ref, e = ad.h_ref(x[rows])
                    ok = LR.in_interval(hk, ref, e)
                    assert ok.all(), (r, T, ldy, packed, s, a, "h", int((~ok).sum()))
                    ys = np.ascontiguousarray(y[rows, c0:c1])
                    ref, e = ad.y_ref(ys, hk)
                    got = np.ascontiguousarray(out[rows, c0:c1])
                    ok = LR.in_interval(got, ref, e)
                    assert ok.all(), (r, T, ldy, packed, s, a, "y", int((~ok).sum()))
                    assert (got != ys).mean() > 0.3  # (the update is there)


@pytest.mark.parametrize("in_dim,widths", CASES)
def test_mixed_batch_modules_per_adapter_and_rows_alone(in_dim, widths):
    """MIXED_40: adapter 0 has q and v only, adapter 1 k only, adapter 2 all
    three.  Rows without an adapter and the columns of a segment an adapter
    lacks keep the input's bits (check_untouched), and every row equals the
    same row run alone at T = 1, bit for bit -- h too."""
    rng = np.random.default_rng([in_dim, widths[1]])
    mk = lambda r, w: LR.dense(r, in_dim, w, rng, b_scale=0.5)
    segs = [{0: mk(12, widths[0]), 2: mk(1, widths[0])},
            {1: mk(64, widths[1]), 2: mk(1, widths[1])},
            {0: mk(12, widths[2]), 2: mk(1, widths[2])}]
    tabs = Tables(segs, in_dim, widths)
    slots = LR.slots_of(LR.MIXED_40)
    T = slots.size
    for ldy in (sum(widths), sum(widths) + 64):
        x, y = data(T, in_dim, widths, ldy, 7)
        h, out = apply(x, y, slots, tabs, 0)
        check_untouched(h, out, y, slots, segs, widths)
        for s, (c0, c1) in enumerate(QR.bounds(widths)):
            for a in segs[s]:
                assert (out[slots == a, c0:c1] != y[slots == a, c0:c1]).mean() > 0.3, (s, a)
        for t in range(T):
            h1, o1 = apply(x[t:t + 1], y[t:t + 1], slots[t:t + 1], tabs, 0)
            assert (o1[0].view(np.uint16) == out[t].view(np.uint16)).all(), (ldy, t)
            assert (h1[:, 0].view(np.uint16) == h[:, t].view(np.uint16)).all(), (ldy, t)
    # the same rows with the other segments' modules taken away: a row's bits in
    # a segment do not depend on which other segments are present
    only_q = Tables([segs[0], {}, {}], in_dim, widths)
    hq, oq = apply(x, y, slots, only_q, 0)
    c1 = widths[0]
    assert (oq[:, :c1].view(np.uint16) == out[:, :c1].view(np.uint16)).all()
    assert (oq[:, c1:].view(np.uint16) == y[:, c1:].view(np.uint16)).all()
    assert (hq[0].view(np.uint16) == h[0].view(np.uint16)).all()
    # and they are the bits of ffmi_lora_apply on the segment alone
    yq = np.ascontiguousarray(y[:, :c1])
    yb, sb, xb = Buf(yq), Buf(slots), Buf(x)
    nws = L.ffmi_lora_workspace_bytes(T, in_dim)
    ws = Buf(np.zeros(nws // 4, np.float32))
    F.check(L.ffmi_lora_apply(xb.ptr, T, in_dim, c1, sb.ptr, only_q.tabs[0].dev.ptr, yb.ptr, 0, ws.ptr,
                              nws, None, None), "ffmi_lora_apply")
    assert (yb.get().view(np.uint16).reshape(T, c1) == out[:, :c1].view(np.uint16)).all()


def test_o_site_shape_one_exact_part():
    """(Hl, H) = (256, 256) through ffmi_lora_apply: F is exactly one part, which
    the shapes of tests/test_gpu_lora.py (2 .. 11 parts) do not reach."""
    Hl = H = 256
    tally = LR.Tally()
    rng = np.random.default_rng(256)
    sel = {0: LR.Selector(12, Hl, H, 1, -1), 1: LR.Selector(64, Hl, H, 2, 1), 2: LR.Selector(1, Hl, H, 3, 0)}
    den = {0: LR.dense(12, Hl, H, rng), 1: LR.dense(64, Hl, H, rng, b_scale=0.5), 2: LR.dense(1, Hl, H, rng)}
    tsel, tden = Table(sel, Hl, H), Table(den, Hl, H)
    for T in TS:
        x, y = KL.data(T, Hl, H, 3)
        slots = pattern(T)
        for packed in ((0, 1) if T > 64 else (0,)):
            h, out = KL.apply(x, y, slots, tsel, packed)
            KL.check_untouched(h, out, y, slots, sel)
            hd, outd = KL.apply(x, y, slots, tden, packed)
            KL.check_untouched(hd, outd, y, slots, den)
            for a in sel:
                rows = slots == a
                if not rows.any():
                    continue
                hk = h[rows][:, :sel[a].r]
                sel[a].check_h(hk, x[rows], tally)
                assert (out[rows].view(np.uint16) == sel[a].want_y(y[rows], hk).view(np.uint16)).all()
                hk = np.ascontiguousarray(hd[rows][:, :den[a].r])
                assert LR.in_interval(hk, *den[a].h_ref(x[rows])).all(), (T, a, "h")
                assert LR.in_interval(outd[rows], *den[a].y_ref(y[rows], hk)).all(), (T, a, "y")
    report("lora_o_site[256-256]", **tally.finish())


def test_argument_checks():
    widths = WIDTHS[0]
    tabs = Tables([{}, {}, {}], 352, widths)
    p = tabs.tabs[0].dev.ptr
    call = lambda T, in_dim, w, ldy, ws, nws: L.ffmi_lora_apply_qkv(
        p, T, in_dim, (ctypes.c_int * 3)(*w), p, tabs.ptrs, p, ldy, 0, ws, nws, None, None)
    assert call(0, 352, widths, 384, None, 0) == 0            # T == 0 launches nothing
    assert call(4, 48, widths, 384, p, 1 << 20) == 1          # in_dim % 32
    assert call(4, 352, (256, 60, 64), 384, p, 1 << 20) == 1  # a width that is no multiple of 8
    assert call(4, 352, widths, 383, p, 1 << 20) == 1         # ldy below the sum of the widths
    assert call(4, 352, widths, 384, p, 16) == 1              # a short workspace
    assert call(4, 352, widths, 384, None, 0) == 1
