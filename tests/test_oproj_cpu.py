"""CPU side of the folded output projection's tests: the numpy rule of
tests/oproj_rule.py checks what it claims to (coverage of the selector
weights, the dense bound under three summation orders, four negative
controls), and ffmi_debug_attn_oproj refuses bad arguments before any HIP call
(no device needed)."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oproj_rule as R
from test_partials_cpu import INVALID, P, fake_attn_handle

T_CPU = 16


def test_selector_weights_cover_every_column_of_every_head():
    """One non-zero +-2^e, e in -3..3, per (row, head), inside the head's 64
    columns; at every (heads, N) of the GPU tests the seeds of one family
    (one seed for N >= 64, ceil(64 / N) below) select all 64 columns of every
    head, and another family selects them through other rows."""
    for (heads, N) in R.GPU_SHAPES:
        seeds = R.selector_seeds(N)
        assert len(seeds) == (1 if N >= 64 else -(-64 // N))
        hit = np.zeros((heads, 64), bool)
        for s in seeds:
            w = R.Selector(heads, N, s)
            nz = w.Wo.reshape(N, heads, 64) != 0
            assert (nz.sum(axis=2) == 1).all()
            assert np.array_equal(np.argmax(nz, axis=2), w.kappa)
            val = np.take_along_axis(w.Wo.reshape(N, heads, 64), w.kappa[:, :, None], 2)[:, :, 0]
            assert np.array_equal(val.astype(np.float32), w.coef)
            assert set(np.abs(w.coef).ravel().tolist()) <= {2.0 ** e for e in range(-3, 4)}
            hit[np.arange(heads)[None, :], w.kappa] = True
        assert hit.all(), (heads, N)
        other = R.Selector(heads, N, R.selector_seeds(N, 1)[0])
        assert (other.kappa != R.Selector(heads, N, seeds[0]).kappa).mean() > 0.9


def _sums(prod):
    """float32 sums of [..., 64] products: sequential, reversed, pairwise"""
    assert prod.dtype == np.float32
    seq = np.zeros(prod.shape[:-1], np.float32)
    rev = np.zeros(prod.shape[:-1], np.float32)
    for k in range(64):
        seq += prod[..., k]
        rev += prod[..., 63 - k]
    pair = prod
    while pair.shape[-1] > 1:
        pair = pair[..., 0::2] + pair[..., 1::2]
    assert seq.dtype == rev.dtype == pair.dtype == np.float32
    return seq, rev, pair[..., 0]


def test_dense_bound_holds_for_any_order_and_not_for_a_dropped_term():
    """On every (heads, N) of the GPU tests: float32 sums of the 64 exact
    products taken sequentially, reversed and pairwise lie within
    64 * 2^-24 * sum |out * Wo| of the float64 sum -- the bound is the
    first-order worst case of any order, so it must hold with room to spare
    (under a quarter, asserted) -- and the sequential sum with one term
    dropped leaves it on over 99 % of the elements."""
    worst = 0.0
    for (heads, N) in R.GPU_SHAPES:
        rng = np.random.default_rng([heads, N])
        T = T_CPU if heads * N <= 4096 else 4
        w, out = R.Dense(heads, N, rng), R.fake_out(T, heads, rng)
        tally = R.Tally()
        o = out.astype(np.float32).reshape(T, heads, 64)
        W = w.Wo.astype(np.float32).reshape(N, heads, 64)
        prod = o.transpose(1, 0, 2)[:, :, None, :] * W.transpose(1, 0, 2)[:, None, :, :]
        for slab in _sums(prod):
            w.check(slab, out, tally)
        assert tally.max_ratio <= 0.25, (heads, N, tally.max_ratio)
        worst = max(worst, tally.max_ratio)
        ref, bound = w.ref_and_bound(out)
        less = prod.copy()
        less[..., 17] = 0
        dropped = _sums(less)[0]
        out_of = np.abs(dropped.astype(np.float64) - ref) > bound
        assert out_of.mean() > 0.99, (heads, N, out_of.mean())
        with pytest.raises(AssertionError):
            w.check(dropped, out)
    print(f"largest error / bound over the three orders: {worst:.4f}")


ITEMS = (16, 15, 2, 1)  # q_count of the ragged step's items, rows contiguous


def _faults(w, out, heads, N):
    """name -> slab of a kernel with that fault (None: the shape cannot show it)"""
    good = R.reference_slab(out, w.Wo, heads)
    f = {}
    if N >= 32:
        a, b = 0, N // 16 - 1
        x = good.copy()
        x[..., 16 * a:16 * a + 16], x[..., 16 * b:16 * b + 16] = \
            good[..., 16 * b:16 * b + 16], good[..., 16 * a:16 * a + 16]
        f["tiles_exchanged"] = x
    if heads >= 2:
        f["head_slice_at_h_plus_1"] = R.reference_slab(out, w.Wo, heads, head_shift=1)
    f["k_step_0_dropped"] = R.reference_slab(out, w.Wo, heads, ksteps=(1,))
    f["k_step_1_dropped"] = R.reference_slab(out, w.Wo, heads, ksteps=(0,))
    # rows of queries beyond q_count stored: each item writes 16 rows from its
    # q_start, the rows past its q_count computed from stale LDS rows
    rng = np.random.default_rng(5)
    stale = R.reference_slab(R.fake_out(out.shape[0] + 16, heads, rng), w.Wo, heads)
    x, q0 = good.copy(), 0
    for qc in ITEMS:
        hi = min(q0 + 16, out.shape[0])
        x[:, q0 + qc:hi] = stale[:, q0 + qc:hi]
        q0 += qc
    f["rows_beyond_q_count_stored"] = x
    return good, f


@pytest.mark.parametrize("kind", ["selector", "dense"])
def test_checks_reject_the_faults_they_are_for(kind):
    """Negative controls of the checker on a reference-made slab, at every
    (heads, N) of the GPU tests: the reference passes; two column tiles
    exchanged, head h's weight slice read at h + 1, either k-step (32 columns)
    dropped, and rows of queries beyond q_count stored are each rejected by
    the selector check (every seed of a family that selects the faulty
    columns) and by the dense check.  One tile (N 16) cannot exchange tiles
    and one head cannot shift; every other fault is shown on every shape."""
    shown = set()
    for (heads, N) in R.GPU_SHAPES:
        rng = np.random.default_rng([heads, N, 7])
        out = R.fake_out(sum(ITEMS), heads, rng)
        ws = [R.Selector(heads, N, s) for s in R.selector_seeds(N)] if kind == "selector" \
            else [R.Dense(heads, N, rng)]
        rejected = {}
        for w in ws:
            good, faults = _faults(w, out, heads, N)
            w.check(good, out, R.Tally())
            for name, slab in faults.items():
                try:
                    w.check(slab, out)
                    rejected.setdefault(name, False)
                except AssertionError:
                    rejected[name] = True
        # (a selector seed at N < 64 has no non-zero in some columns: the
        # family as a whole must reject; at N >= 64 the family is one seed)
        assert rejected and all(rejected.values()), (heads, N, rejected)
        shown |= set(rejected)
    assert shown == {"tiles_exchanged", "head_slice_at_h_plus_1", "k_step_0_dropped",
                     "k_step_1_dropped", "rows_beyond_q_count_stored"}


def test_subnormal_sources_may_flush_but_are_capped():
    """A selected fp16-subnormal `out` element may come back as 0 or as the
    exact product, nothing else; above 0.1 % of the compared elements the
    tally refuses."""
    heads, N, T = 2, 64, 4
    w = R.Selector(heads, N, 0)
    out = R.fake_out(T, heads, np.random.default_rng(1))
    out[1, 64 + w.kappa[5, 1]] = np.float16(3 * 2.0 ** -24)
    good = R.reference_slab(out, w.Wo, heads)
    assert good[1, 1, 5] != 0
    for v, field in ((good[1, 1, 5], "kept"), (np.float32(0), "flushed")):
        t, slab = R.Tally(), good.copy()
        slab[1, 1, 5] = v
        w.check(slab, out, t)
        assert t.subnormal == 1 and getattr(t, field) == 1 and t.compared == heads * T * N
        with pytest.raises(AssertionError):
            t.finish()  # 1 of 512 is over the cap
        t.compared = 1000
        assert t.finish()["subnormal_" + field] == 1
    slab = good.copy()
    slab[1, 1, 5] = good[1, 1, 5] * 2
    with pytest.raises(AssertionError):
        w.check(slab, out)
    slab = good.copy()
    slab[0, 0, 0] = 0  # a normal source may not flush
    assert good[0, 0, 0] != 0
    with pytest.raises(AssertionError):
        w.check(slab, out)


def test_split_buffer_guards_and_row_stride():
    """The slab's row stride is the step's T: a slab written with the
    buffer's capacity as stride, a word behind [heads][T][N] or in a guard,
    and any word of an unprojected step's buffer are each refused."""
    heads, T, max_T, N = 3, 5, 8, 16
    buf = R.slab_buffer(heads, max_T, N)
    assert buf.size == heads * max_T * N + 2 * R.GUARD
    assert np.isfinite(buf.view(np.float32)).all()
    assert R.split_buffer(buf, heads, T, N, projected=False) is None
    body = buf[R.GUARD:R.GUARD + heads * T * N]
    body[:] = np.arange(body.size, dtype=np.float32).view(np.uint32)
    slab = R.split_buffer(buf, heads, T, N)
    assert slab.shape == (heads, T, N) and slab[1, 0, 0] == T * N
    with pytest.raises(AssertionError):
        R.split_buffer(buf, heads, T, N, projected=False)
    for at in (0, R.GUARD - 1, R.GUARD + heads * T * N, R.GUARD + heads * max_T * N - 1,
               buf.size - 1, R.GUARD + 2 * max_T * N):  # (the last: head 2 at stride max_T)
        bad = buf.copy()
        bad[at] = 0
        with pytest.raises(AssertionError):
            R.split_buffer(bad, heads, T, N)


def test_attn_oproj_refusals():
    L = F.lib()
    hp = ctypes.cast(fake_attn_handle(), ctypes.c_void_p)
    h32 = ctypes.cast(fake_attn_handle(full_precision=1), ctypes.c_void_p)
    h128 = ctypes.cast(fake_attn_handle(d=128), ctypes.c_void_p)
    width = 3 * 2 * 64
    pj = ctypes.c_int(7)
    ok = dict(h=hp, b=P, qkv=P, slabs=None, S=0, NP=0, out=P, wo=P, N=128, slab=P, max_T=4,
              projected=ctypes.byref(pj))

    def call(**kw):
        a = dict(ok, **kw)
        return L.ffmi_debug_attn_oproj(a["h"], a["b"], a["qkv"], a["slabs"], a["S"], a["NP"],
                                       a["out"], a["wo"], a["N"], a["slab"], a["max_T"],
                                       a["projected"], None)

    sl = dict(qkv=None, slabs=P, S=2, NP=width)
    for bad in (dict(h=None), dict(b=None), dict(out=None), dict(wo=None), dict(slab=None),
                dict(projected=None),
                dict(qkv=None),                    # neither qkv nor slabs
                dict(slabs=P, S=2, NP=width),      # both
                dict(h=h32), dict(h=h128),
                dict(N=0), dict(N=8), dict(N=24), dict(N=1040), dict(N=-16),
                dict(max_T=0), dict(slab=P + 4), dict(slab=P + 8),
                dict(sl, slabs=P + 4), dict(sl, S=0), dict(sl, S=9), dict(sl, NP=width - 4),
                dict(sl, NP=width + 2)):
        assert call(**bad) == INVALID, bad
    assert pj.value == 7  # a refusal writes nothing
