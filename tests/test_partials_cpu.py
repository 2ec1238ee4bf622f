"""CPU side of the split-K slab tests: the numpy rule's data stays sensitive
to the order of the slab additions (tests/partials_rule.py), and the slab /
gather test hooks of include/ffmi.h refuse bad arguments before any HIP call
(no device needed)."""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
from partials_rule import combine, make_slabs, measured_shapes, reorderings

INVALID, UNSUPPORTED = 1, 5
P = 0x10000  # a 16-byte aligned, never dereferenced "device pointer"


def test_slab_data_is_order_sensitive():
    """For every S in 3..16 and every shape of the GPU tests with at least
    2000 results (partials_rule.measured_shapes), summing the slabs
    reversed, with the first and last exchanged, or rotated by one changes at
    least 10 % of the fp16 results: a consumer that combines in another order
    cannot pass the bit-for-bit GPU tests by luck.  (The bar is a condition on
    the data, not a tolerance; the rule meets it with margin, printed below.)
    Every combined value is finite and the padding columns stay NaN."""
    low = {}
    SHAPES = measured_shapes()
    assert len(SHAPES) >= 20 and all(T * N >= 2000 for (T, N, _) in SHAPES)
    for S in range(3, 17):
        fr = {k: [] for k in reorderings(S)}
        for (T, N, NP) in SHAPES:
            slabs = make_slabs(S, T, NP, N, np.random.default_rng(1000 * S + T + N))
            ref = combine(slabs)
            assert np.isfinite(ref[:, :N]).all() and np.isnan(ref[:, N:]).all()
            for name, order in reorderings(S).items():
                got = combine(slabs[order])
                f = float((got[:, :N].view(np.uint16) != ref[:, :N].view(np.uint16)).mean())
                fr[name].append(f)
                assert f >= 0.10, (S, (T, N, NP), name, f)
        low[S] = {k: min(v) for k, v in fr.items()}
        print(f"S={S:2d} least changed fraction: " +
              " ".join(f"{k}={v:.3f}" for k, v in low[S].items()))


def test_combine_is_the_in_order_float32_sum():
    """combine against a scalar loop on a few elements, S = 1 and 2 included
    (S = 2 is one addition: commutative), and finite for every S up to 16"""
    for S in range(1, 17):
        rng = np.random.default_rng(S)
        slabs = make_slabs(S, 3, 16, 11, rng)
        got = combine(slabs)
        assert got.dtype == np.float16 and np.isfinite(got[:, :11]).all()
        for t in range(3):
            for n in range(11):
                acc = np.float32(slabs[0, t, n])
                for s in range(1, S):
                    acc = np.float32(acc + slabs[s, t, n])
                assert np.float16(acc).view(np.uint16) == got[t, n].view(np.uint16)
    two = make_slabs(2, 5, 64, 64, np.random.default_rng(0))
    assert np.array_equal(combine(two).view(np.uint16), combine(two[::-1]).view(np.uint16))


def test_partials_reduce_refusals():
    L = F.lib()
    ok = dict(slabs=P, S=4, NP=32, Y=P, T=3, N=20)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ffmi_debug_partials_reduce(a["slabs"], a["S"], a["NP"], a["Y"], a["T"], a["N"], None)

    for bad in (dict(slabs=None), dict(Y=None), dict(S=0), dict(S=17), dict(NP=24), dict(N=33),
                dict(N=0), dict(T=-1), dict(slabs=P + 4)):
        assert call(**bad) == INVALID, bad


def test_rmsnorm_partials_refusals():
    L = F.lib()
    ok = dict(x1=P, slabs=P, S=4, NP=1024, w=P, res=P, out=P, T=2, H=1024, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ffmi_debug_rmsnorm_partials(a["x1"], a["slabs"], a["S"], a["NP"], a["w"], a["res"],
                                             a["out"], a["T"], a["H"], 1e-6, a["flags"], None)

    for bad in (dict(res=None),                      # no residual_out
                dict(S=17), dict(S=0),
                dict(S=9, H=1032, NP=1040),          # > 8 slabs beyond H 1024
                dict(H=8200, NP=8208),               # beyond one chunk per thread
                dict(H=1020), dict(H=0),
                dict(NP=1016),                       # NP < H
                dict(NP=1026),                       # rows off the 16-byte vectors
                dict(x1=None), dict(slabs=None), dict(w=None), dict(out=None), dict(T=-1),
                dict(flags=0x10), dict(slabs=P + 8)):
        assert call(**bad) == INVALID, bad
    assert call(flags=F.Y_PACKED, H=1016, NP=1024) == UNSUPPORTED
    # the widest accepted forms are not refused for their shape: 16 slabs at
    # H 1024 and 8 at H 8192 pass every check when T == 0 (nothing to launch)
    assert call(S=16, T=0) == 0 and call(S=8, H=8192, NP=8192, T=0) == 0


def fake_attn_handle(full_precision=0, heads=2, d=64):
    """What ffmi_debug_attn_partials reads before its refusals: the handle's
    ffmi_attn_cfg, the first member of struct ffmi_attn (no device to create a
    real handle with here).  Zeroed memory follows it."""
    cfg = F.AttnCfg(F.ATTN_INC, heads, d, 1, 16, 0, 16, 0.125, 10000.0, 0, 0, 1.0, 1.0, 4.0, 8192,
                    full_precision)
    buf = ctypes.create_string_buffer(ctypes.sizeof(cfg) + 256)
    ctypes.memmove(buf, ctypes.byref(cfg), ctypes.sizeof(cfg))
    return buf


def test_attn_partials_refusals():
    L = F.lib()
    h, h32 = fake_attn_handle(), fake_attn_handle(full_precision=1)
    hp = ctypes.cast(h, ctypes.c_void_p)
    width = 3 * 2 * 64

    def call(handle=hp, b=P, slabs=P, S=2, NP=width, out=P):
        return L.ffmi_debug_attn_partials(handle, b, slabs, S, NP, out, None)

    assert call(handle=ctypes.cast(h32, ctypes.c_void_p)) == INVALID  # full precision
    for bad in (dict(NP=width - 4), dict(NP=width + 2), dict(S=9), dict(S=0), dict(handle=None),
                dict(b=None), dict(slabs=None), dict(out=None), dict(slabs=P + 4)):
        assert call(**bad) == INVALID, bad


def test_allreduce_partials_refusals():
    L = F.lib()
    assert L.ffmi_debug_allreduce_partials(None, P, 2, 16, P, 1, 8, None) == INVALID
    c = ctypes.c_void_p()
    F.check(L.ffmi_comm_create_peer(2, 0, ctypes.byref(c)))  # no transport attached
    try:
        for args in ((c, P, 2, 16, P, 1, 8), (c, None, 2, 16, P, 1, 8), (c, P, 2, 16, None, 1, 8),
                     (c, P, 0, 16, P, 1, 8), (c, P, 9, 16, P, 1, 8)):
            assert L.ffmi_debug_allreduce_partials(*args, None) == INVALID, args
    finally:
        L.ffmi_comm_destroy(c)


def test_rmsnorm_gather_refusals():
    L = F.lib()

    def call(b=P, desc=None, table=P, w=P, res=P, out=P, H=64, flags=0, prev=None):
        return L.ffmi_debug_rmsnorm_gather(b, desc, table, w, res, out, H, 1e-6, flags, prev, None)

    for bad in (dict(b=None), dict(table=None), dict(w=None), dict(res=None), dict(out=None),
                dict(H=0), dict(H=60), dict(H=32776), dict(flags=0x10)):
        assert call(**bad) == INVALID, bad
    assert call(H=72, flags=F.Y_PACKED) == UNSUPPORTED
    # a chained id (-1 - i) with nothing to index
    toks = (F.TokenInfo * 2)(F.TokenInfo(3, 0, 0, -1, 1, 0, 0, 0, 0),
                             F.TokenInfo(-1, 0, 0, -1, 1, 0, 0, 0, 0))
    desc = F.BatchDesc(2, 0, 0, 0, toks, None, None, None)
    assert call(desc=ctypes.byref(desc)) == INVALID


@pytest.mark.parametrize("name", ["ffmi_debug_partials_reduce", "ffmi_debug_rmsnorm_partials",
                                  "ffmi_debug_attn_partials", "ffmi_debug_allreduce_partials",
                                  "ffmi_debug_rmsnorm_gather", "ffmi_debug_attn_oproj"])
def test_hooks_are_declared_bound_and_exported(name):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ffmi.h")).read(), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", src) and name in F.SIGNATURES and hasattr(F.lib(), name)
