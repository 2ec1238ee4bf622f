"""Kernel-level tests of the output projection folded into the fused attention
(attention_kernel<64, 1, 8, true, false, PSRC, OP = true>, OprojArgs), through
ffmi_debug_attn_oproj.  Run on an MI355X: pytest -m gpu.

Each (work item, head) workgroup multiplies its rounded fp16 output rows by
its head's 64 columns of the packed Wo and stores fp32 slab `head` of
[heads][T][N].  tests/oproj_rule.py holds the rule and the two checks, both
over the kernel's own `out` read back: selector weights (one +-2^e per (row,
head): every index bit-exact) and dense weights (within 64 * 2^-24 * sum |out *
Wo|, the worst case of any-order fp32 summation); tests/test_oproj_cpu.py
shows that both reject exchanged tiles, a shifted head slice, a dropped k-step
and stored rows of absent queries.  Every step here also goes through
AttnCase.run's common check: out, K and V^T caches bit-identical to a twin
handle on the public ffmi_attn_* call, and every word of the slab buffer
outside [heads][T][N] (guards, the rows between T and max_T) still the
sentinel.

Reached: OP x PSRC 0 / 1; grid z 1 / 2 (FFMI_ATTN_OSPLIT 0 / 2); N 16 .. 1024
with 1, 3, 7, 9, 16, 48 and 64 column tiles, the packed pitch N / 16 differing
from the K extent; heads 1 .. 16; INC, SPEC, TREE (commits in the prologue);
both output layouts; ragged items q_count 1 / 2 / 15 / 16; the fall-backs.
"""
import os

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oproj_rule as R
import oracle_lib as O
import test_gpu_kernels as K
from hip_util import Buf, f16, report, ulp_diff
from partials_rule import combine
from test_gpu_kernels import AttnCase, close16, tree_masks

pytestmark = pytest.mark.gpu
RS = int(os.environ.get("FFMI_RANDOM_SCALE", "1"))
OFF = int(os.environ.get("FFMI_RANDOM_SEED_OFFSET", "0"))

L = None
EPS = 1e-6
PREFILL = {0: 3, 1: 16, 2: 9}  # one item per request: the prefill projects too


def setup_module(module):
    global L
    L = F.lib()
    K.setup_module(K)  # AttnCase lives there and calls through that module's library handle


def bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def weights(heads, N, rng):
    """every weight of one shape: the selector seeds that cover all 64 columns
    of every head, and a dense draw"""
    return [R.Selector(heads, N, s) for s in R.selector_seeds(N)] + [R.Dense(heads, N, rng)]


def step(c, infos, w, max_T, tally, rng, want=1, **kw):
    """one AttnCase step with the projection asked for, checked by w's rule"""
    out, qs, slab, pj = c.run(infos, rng=rng, oproj=(w.Wo, w.N, max_T), **kw)
    assert pj == want, (pj, want)
    if pj:
        w.check(slab, np.asarray(out, np.float16), tally)
    else:
        assert slab is None
    return out, slab


def prefill_infos(lens):
    return [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]


def decode_infos(lens, k=0):
    return [(7, n + k, r, n + k, n + k + 1, 0, 0, 0) for r, n in lens.items()]


def prefill_then_decode(heads, w, seed, tally, layout=0):
    """3 requests of 3, 16 and 9 prompt tokens (T 28 in a 32-row buffer), then
    a decode step (T 3 in an 8-row buffer); returns both steps' (out, slab)"""
    rng = np.random.default_rng(seed)
    c = AttnCase(F.ATTN_INC, heads=heads, d=64, out_layout=layout)
    a = step(c, prefill_infos(PREFILL), w, 32, tally, rng)
    b = step(c, decode_infos(PREFILL), w, 8, tally, rng)
    return a, b


def finish(name, tally, **kv):
    report(name, **tally.finish(), **kv)


# ---------------------------------------------------------------- 1. tiles and strides
@pytest.mark.parametrize("heads,N", R.TILE_GRID)
def test_oproj_tile_and_stride_edges(heads, N, monkeypatch):
    """Every column-tile count that takes another path -- 1 tile (N 16), 3, 7
    (fewer than the 8 waves), 9 (odd under the column split), 48, 64 (8 per
    wave, the upper edge) -- at heads 1 .. 16 with N != heads * 64 in most, so
    that the packed pitch N / 16 and the K extent heads * 2 differ: selector
    weights exact (all 64 columns of every head), dense within the bound,
    projected == 1, unsplit (FFMI_ATTN_OSPLIT=0) and with two workgroups per
    (item, head) (=2), the slabs of the two bit-identical."""
    tally = R.Tally()
    ws = weights(heads, N, np.random.default_rng([heads, N]))
    slabs = {}
    for split in ("0", "2"):
        monkeypatch.setenv("FFMI_ATTN_OSPLIT", split)
        slabs[split] = [prefill_then_decode(heads, w, 100 + i, tally) for i, w in enumerate(ws)]
    for x, y in zip(slabs["0"], slabs["2"]):
        for (o0, s0), (o2, s2) in zip(x, y):
            assert np.array_equal(bits32(s0), bits32(s2))
            assert np.array_equal(o0.view(np.uint16), o2.view(np.uint16))
    finish("oproj_tile_and_stride_edges", tally, heads=heads, N=N)


# ---------------------------------------------------------------- 2. ragged items
@pytest.mark.parametrize("order", [(1, 2, 15, 16), (16, 15, 2, 1)])
def test_oproj_ragged_items(order, monkeypatch):
    """Items of 1, 2, 15 and 16 queries in one step (rows contiguous), in both
    orders, then a second ragged chunk of the same requests: the product of a
    short item's absent queries is computed from stale LDS rows and must not
    be stored.  Such a row would land in the next item's rows, in the next
    head's, or -- the last item of the last head -- behind [heads][T][N], in
    the rows up to max_T = T + 17 that must keep the sentinel.  Both splits."""
    heads, N = R.RAGGED
    tally = R.Tally()
    for split in ("0", "2"):
        monkeypatch.setenv("FFMI_ATTN_OSPLIT", split)
        for i, w in enumerate(weights(heads, N, np.random.default_rng(order))):
            rng = np.random.default_rng(200 + i)
            c = AttnCase(F.ATTN_INC, heads=heads, d=64)
            lens = dict(enumerate(order))
            T = sum(order)
            step(c, prefill_infos(lens), w, T + 17, tally, rng)
            # the next chunk of every request, the counts reversed
            infos = [(5, n + p, r, n + p, n + p + 1, 0, 0, 0)
                     for r, n in lens.items() for p in range(order[3 - r])]
            step(c, infos, w, T + 17, tally, rng)
    finish("oproj_ragged_items", tally, order=list(order))


# ---------------------------------------------------------------- 3. modes
def test_oproj_spec_beam_layers():
    """A SPEC handle (the SSM's real use) at heads 12, N 768: the prompt and
    the beam layers of test_attention_spec_beam_layers, every step projected,
    selector weights exact."""
    heads, N = R.MODES
    tally = R.Tally()
    w = R.Selector(heads, N, 0)
    c, rng, ntcs = AttnCase(F.ATTN_SPEC, heads=heads, d=64), np.random.default_rng(7), 8
    m = tree_masks([-1, 0, 1, 1, 2, 3])
    step(c, [(3, p, 0, p, p + 1, 0, 0, 0) for p in range(ntcs + 1)], w, 16, tally, rng,
         masks=[[0]])
    step(c, [(5, ntcs + 1, 0, ntcs + 1, ntcs, ntcs, 2, 1)], w, 16, tally, rng, masks=[m])
    step(c, [(5, ntcs + 2, 0, ntcs + 2 + k, ntcs, ntcs, 4, 2 + k) for k in range(2)], w, 16,
         tally, rng, masks=[m])
    step(c, [(6, ntcs + 3, 0, ntcs + 4 + k, ntcs, ntcs, 6, 4 + k) for k in range(2)], w, 16,
         tally, rng, masks=[m])
    finish("oproj_spec_beam_layers", tally)


def _tree(n, root_depth):
    parents = [-1, 0, 1] + [2 + (j - 3) // 3 for j in range(3, n)]
    depth = [root_depth]
    for j in range(1, n):
        depth.append(depth[parents[j]] + 1)
    return tree_masks(parents), depth


def test_oproj_tree_commits_in_the_prologue():
    """A TREE handle at heads 12, N 768: a prompt step, a verify step of 13
    tree tokens for each of two requests, then a step carrying the commits of
    an accepted path of 4 (depths below every slot the step stores, so they
    run in the fused kernel's prologue, before the projection) and a second
    tree.  Every step projected, selector weights exact."""
    heads, N = R.MODES
    tally = R.Tally()
    w = R.Selector(heads, N, 1)
    c, rng = AttnCase(F.ATTN_TREE, heads=heads, d=64), np.random.default_rng(8)
    m, depth = _tree(13, 12)
    step(c, [(3, p, r, p, p + 1, 0, 0, 0) for r in (0, 2) for p in range(12)], w, 32, tally, rng,
         masks=[[0]] * 3)
    step(c, [(4, depth[j], r, 12 + j, 12, 12, 13, j) for r in (0, 2) for j in range(13)], w, 32,
         tally, rng, masks=[m, [0], m])
    commits = [(13 * k + j, r, 12 + i) for k, r in enumerate((0, 2))
               for i, j in enumerate([0, 1, 2, 5])]
    step(c, [(4, depth[j] + 4, r, 16 + j, 16, 16, 13, j) for r in (0, 2) for j in range(13)], w,
         32, tally, rng, masks=[m, [0], m], commits=commits)
    finish("oproj_tree_commits", tally)


# ---------------------------------------------------------------- 4. packed output
def test_oproj_packed_output_layout(monkeypatch):
    """out_layout = 1 (activation fragment tiles) at heads 4, N 256: the
    projection reads the rounded rows from LDS, not from `out`; `out` is
    unpacked before it feeds the reference.  Both splits."""
    heads, N = R.PACKED
    tally = R.Tally()
    for split in ("0", "2"):
        monkeypatch.setenv("FFMI_ATTN_OSPLIT", split)
        for i, w in enumerate(weights(heads, N, np.random.default_rng(4))):
            prefill_then_decode(heads, w, 400 + i, tally, layout=1)
    finish("oproj_packed_output_layout", tally)


# ---------------------------------------------------------------- 5. qkv from slabs
@pytest.mark.parametrize("heads,N", R.SLAB_SOURCE)
def test_oproj_qkv_from_slabs(heads, N):
    """PSRC = 1 with OP: the step's qkv as S = 1 / 3 / 8 deferred split-K
    slabs, NP the qkv width and 8 more.  Selector weights exact, and slab and
    out bit-identical to the same steps given qkv = combine(slabs)."""
    tally = R.Tally()
    w = R.Selector(heads, N, 2)
    for S in (1, 3, 8):
        for pad in (0, 8):
            rng = np.random.default_rng(500 + S + pad)
            a = AttnCase(F.ATTN_INC, heads=heads, d=64)
            b = AttnCase(F.ATTN_INC, heads=heads, d=64)
            for infos, max_T in ((prefill_infos(PREFILL), 32), (decode_infos(PREFILL), 8)):
                oa, sa = step(a, infos, w, max_T, tally, rng, slabs=S, slab_pad=pad)
                ob, sb = step(b, infos, w, max_T, tally, None, qkv=a.last_qkv)
                assert np.array_equal(bits32(sa), bits32(sb)), (S, pad)
                assert np.array_equal(oa.view(np.uint16), ob.view(np.uint16)), (S, pad)
    finish("oproj_qkv_from_slabs", tally, heads=heads, N=N)


# ---------------------------------------------------------------- 6. fall-backs
@pytest.mark.parametrize("case", ["block_of_20", "two_items", "tree_21", "T_over_max_T", "no_fuse"])
def test_oproj_fallbacks_do_not_project(case, monkeypatch):
    """Launch geometries the folded projection does not take are host
    decisions, not errors: projected == 0, every word of the slab buffer still
    the sentinel, out and caches equal to the twin's (AttnCase.run).  A
    prefill block of 20 tokens in one request (AttnCase cuts items at 32
    queries, so this is one item of more than 16); a block of 37, which is two
    items of one request; a TREE step of 21 tree tokens; a decode step of 3
    tokens with room for 2; FFMI_ATTN_NO_FUSE=1."""
    heads, N = 3, 144
    w = R.Selector(heads, N, 3)
    rng, tally = np.random.default_rng(6), R.Tally()
    if case == "tree_21":
        c = AttnCase(F.ATTN_TREE, heads=heads, d=64)
        m, depth = _tree(21, 12)
        step(c, [(3, p, 0, p, p + 1, 0, 0, 0) for p in range(12)], w, 32, tally, rng,
             masks=[[0]])
        step(c, [(4, depth[j], 0, 12 + j, 12, 12, 21, j) for j in range(21)], w, 32, tally, rng,
             want=0, masks=[m])
        return
    c = AttnCase(F.ATTN_INC, heads=heads, d=64)
    if case == "block_of_20":
        step(c, prefill_infos({0: 3, 1: 20}), w, 32, tally, rng, want=0)
    elif case == "two_items":
        step(c, prefill_infos({0: 3, 1: 37}), w, 64, tally, rng, want=0)
    elif case == "T_over_max_T":
        step(c, prefill_infos(PREFILL), w, 32, tally, rng)
        step(c, decode_infos(PREFILL), w, 2, tally, rng, want=0)
        step(c, decode_infos(PREFILL, 1), w, 3, tally, rng)  # T == max_T projects
    else:
        monkeypatch.setenv("FFMI_ATTN_NO_FUSE", "1")
        step(c, prefill_infos(PREFILL), w, 32, tally, rng, want=0)
        step(c, decode_infos(PREFILL), w, 8, tally, rng, want=0)


# ---------------------------------------------------------------- 7. composed
@pytest.mark.parametrize("heads,N", R.COMPOSED)
def test_oproj_slab_through_the_residual_norm(heads, N):
    """The projection's value: the decode step's slab (dense weights) fed to
    the residual norm as S = heads slabs of width N, as the model does.
    residual_out and out are the bits of ffmi_rmsnorm_ex(x1, x2 = combine of
    the slab read back) and hold that path's oracle bounds (residual exact,
    out within 1 fp16 ulp, >= 99 % identical); and combine(slab), fp16 of the
    head-order sum, is within 2 fp16 ulp of the oracle's linear on the
    kernel's own out -- the bar test_attention_oproj_equals_o_gemm holds the
    model to, which the exact checks of this file account for bit by bit."""
    tally = R.Tally()
    rng = np.random.default_rng([heads, N, 7])
    w = R.Dense(heads, N, rng)
    _, (out, slab) = prefill_then_decode(heads, w, 700, tally)
    T = slab.shape[1]
    x1 = f16(rng.standard_normal((T, N)))
    nw = f16(1 + rng.uniform(-0.1, 0.1, N))
    x2 = np.ascontiguousarray(combine(slab))
    a, wb, xb, sb = Buf(x1), Buf(nw), Buf(x2), Buf(slab)
    r0, o0 = Buf.empty((T, N), np.float16), Buf.empty((T, N), np.float16)
    r1, o1 = Buf.empty((T, N), np.float16), Buf.empty((T, N), np.float16)
    F.check(L.ffmi_rmsnorm_ex(a.ptr, xb.ptr, wb.ptr, r0.ptr, o0.ptr, T, N, EPS, 0, None))
    F.check(L.ffmi_debug_rmsnorm_partials(a.ptr, sb.ptr, heads, N, wb.ptr, r1.ptr, o1.ptr, T, N,
                                          EPS, 0, None))
    res, got = r1.get(), o1.get()
    assert np.array_equal(res.view(np.uint16), r0.get().view(np.uint16))
    assert np.array_equal(got.view(np.uint16), o0.get().view(np.uint16))
    r_ref, o_ref = O.residual_rmsnorm(x1.astype(np.float32), x2.astype(np.float32),
                                      nw.astype(np.float32), EPS)
    assert np.array_equal(res.view(np.uint16), f16(r_ref).view(np.uint16))
    close16(got, o_ref, 1, 0.99)
    lin = O.linear(np.asarray(out, np.float32), w.Wo.astype(np.float32), fp16=1)
    d = ulp_diff(x2, f16(lin))
    print(f"heads {heads} N {N}: projection vs oracle linear, max ulp {int(d.max())}, "
          f"exact {float((d == 0).mean()):.4f}")
    report("oproj_composed", heads=heads, N=N, max_ulp=int(d.max()),
           exact=float((d == 0).mean()), **tally.finish())
    assert int(d.max()) <= 2


# ---------------------------------------------------------------- 8. randomised
@pytest.mark.parametrize("seed", range(OFF, OFF + 6 * RS))
def test_oproj_random_shapes(seed, monkeypatch):
    """heads 1 .. 16, N any multiple of 16 up to 1024, 1 .. 4 requests with
    prompts of up to 16 tokens, 1 .. 3 decode steps, the column split on or
    off; selector or dense weights and row-major or packed output taken in
    turn by the seed, so that any six seeds in a row hold all four pairs."""
    rng = np.random.default_rng(9000 + seed)
    heads, N = int(rng.integers(1, 17)), 16 * int(rng.integers(1, 65))
    lens = {r: int(rng.integers(1, 17)) for r in range(int(rng.integers(1, 5)))}
    split, layout = str(2 * int(rng.integers(0, 2))), seed % 2
    w = R.Dense(heads, N, rng) if (seed // 2) % 2 else R.Selector(heads, N, seed)
    monkeypatch.setenv("FFMI_ATTN_OSPLIT", split)
    tally = R.Tally()
    c = AttnCase(F.ATTN_INC, heads=heads, d=64, out_layout=layout)
    T = sum(lens.values())
    step(c, prefill_infos(lens), w, T + int(rng.integers(0, 5)), tally, rng)
    for k in range(int(rng.integers(1, 4))):
        step(c, decode_infos(lens, k), w, len(lens) + int(rng.integers(0, 5)), tally, rng)
    finish("oproj_random_shapes", tally, seed=seed, heads=heads, N=N, split=split, layout=layout,
           kind=type(w).__name__)
