"""Kernel-level parity of the consumers of deferred split-K slabs, and of the
embedding gather folded into layer 0's norm, through the test hooks of
include/ffmi.h.  Run on an MI355X: pytest -m gpu.

A split-K GEMM whose consumer can combine leaves fp32 slabs [S][T][NP]; the
value is fp16(slab 0 + slab 1 + ... in slab order), rounded once.  That rule
is exact (tests/partials_rule.py reproduces it bit for bit), so every check
here is bit-identity: a consumer fed with slabs must give the bits of its
plain fp16 path fed with combine(slabs).  The slabs come in cancelling pairs,
so a wrong slab index, a slab taken twice or another order of the additions
changes >= 10 % of the results (tests/test_partials_cpu.py); the padding
columns [N, NP) are NaN.  The oracle bounds of the plain paths (norms: residual
exact, out within 1 fp16 ulp and >= 99 % identical; attention: AttnCase.check)
are held as well, so the twin comparisons are not circular.

Instantiations reached (S picked directly, not through the GEMM planner):
  gemm_reduce_kernel<0, MAXS>, MAXS 2 / 4 / 8 / 16: S 1-16, aligned rows, the
    scalar tail of an unaligned row (N 1022) and of a short column group (N 4);
  rmsnorm_kernel<NT, 1, MAXS, 2>: NT 128 / 256 / 512 / 1024 x MAXS 1 / 2 / 4 /
    8, and MAXS 12 / 16 at NT 128; row-major, packed and in place;
  kv_update_item: the run-time source in kv_update_kernel<32 / 64 / 128>
    (prefill, FFMI_ATTN_NO_FUSE) and PSRC = 1 in the fused attention at one
    query tile (decode, beam steps), two query tiles and the query split
    (tree verification), S 1 / 2 / 3 / 5 / 8 (slabs 0-1 and slabs >= 2);
  rmsnorm_kernel<NT, MAXC, 1, 3>: every NT at MAXC 1, the 1024-thread MAXC 2
    form (H 8200 and its upper edge 16384) and the MAXC 4 form (H 16392 and
    the widest row, 32768), chained ids, the blob fetch.
The all-reduce copy-in (slab_vec) is in tests/test_gpu_peer.py.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
import test_gpu_kernels as K
from hip_util import Buf, f16, hip
from partials_rule import NORM_H, NORM_T, REDUCE_N_NP, REDUCE_T, combine, make_slabs, norm_np
from test_gpu_kernels import AttnCase, close16, tree_masks, unpack_act_np

pytestmark = pytest.mark.gpu

L = None
EPS = 1e-6


def setup_module(module):
    global L
    L = F.lib()
    K.setup_module(K)  # AttnCase lives there and calls through that module's library handle


def bits(a):
    return np.asarray(a).view(np.uint16)


class NormBound:
    """The norm's oracle bound, as test_rmsnorm_and_residual holds it: out
    within 1 fp16 ulp and >= 99 % bit-identical.  The 99 % is taken per call
    where a call has at least the 768 outputs of that test's smallest shape,
    and over all outputs of the test together at the end (a call of 8 outputs
    cannot show 99 %)."""

    def __init__(self):
        self.got, self.ref = [], []

    def add(self, got, ref):
        close16(got, ref, 1, 0.99 if got.size >= 768 else 0.0)
        self.got.append(np.asarray(got, np.float16).ravel())
        self.ref.append(np.asarray(ref, np.float32).ravel())

    def finish(self):
        close16(np.concatenate(self.got), np.concatenate(self.ref), 1, 0.99)


# ---------------------------------------------------------------- reduce pass
SENTINEL = 0xABCD


@pytest.mark.parametrize("T", REDUCE_T)  # 1, 5, 70
def test_partials_reduce_bit_exact(T):
    """gemm_reduce_kernel<0, MAXS> over caller-made slabs, every S in 1..16:
    Y == combine(slabs)[:, :N] bit for bit; aligned rows (N 16, 1024), rows
    whose 8-byte stores are unaligned (N 1022: the scalar tail on odd rows), a
    short last column group (N 1000 = 250 groups, N 4 of a 16-wide slab), NP
    padded past N by up to a tile.  64 sentinel halves behind Y stay put."""
    assert REDUCE_N_NP == ((4, 16), (16, 16), (1000, 1008), (1022, 1024), (1024, 1040))
    for (N, NP) in REDUCE_N_NP:
        for S in range(1, 17):
            slabs = make_slabs(S, T, NP, N, np.random.default_rng(S * 1000 + T * 10 + N))
            want = combine(slabs)[:, :N]
            sb = Buf(slabs)
            y = Buf(np.full(T * N + 64, SENTINEL, np.uint16))
            F.check(L.ffmi_debug_partials_reduce(sb.ptr, S, NP, y.ptr, T, N, None), (S, T, N, NP))
            got = y.get()
            assert np.array_equal(got[:T * N].reshape(T, N), bits(want)), (S, T, N, NP)
            assert (got[T * N:] == SENTINEL).all(), (S, T, N, NP)


# ---------------------------------------------------------------- norm, slab source
def _norm_inputs(T, H, rng):
    x1 = f16(rng.standard_normal((T, H)))
    w = f16(1 + rng.uniform(-0.1, 0.1, H))
    return x1, w


@pytest.mark.parametrize("H", NORM_H)  # 8, 1016, 1024, 1032, 2048, 2056, 4096, 4104, 8192
def test_rmsnorm_partials_equals_fp16_source(H):
    """rmsnorm_kernel<NT, 1, MAXS, 2>: H on both sides of every NT step (one
    chunk; 127 / 128 / 129 chunks; 256 / 257; 512 / 513; 1024), NP = H rounded
    up to a tile and one tile more, T 1 / 3 / 17, S 1..8 and 9..16 (the 12-
    and 16-slab variants) where H <= 1024.  residual_out and out are the bits
    of ffmi_rmsnorm_ex(x1, x2 = combine(slabs)), and hold that path's bounds
    against the oracle: residual exact, out within 1 ulp, >= 99 % identical.
    In place (residual_out == x1, the model's call): the same bits.  With
    FFMI_Y_PACKED (H % 32 == 0, T 17): out unpacks to the row-major result."""
    Ss = list(range(1, 9)) + (list(range(9, 17)) if H <= 1024 else [])
    bound = NormBound()
    for T in NORM_T:  # 1, 3, 17
        rng = np.random.default_rng(H * 31 + T)
        x1, w = _norm_inputs(T, H, rng)
        a, wb = Buf(x1), Buf(w)
        for NP in norm_np(H):
            for S in Ss:
                slabs = make_slabs(S, T, NP, H, rng)
                x2 = np.ascontiguousarray(combine(slabs)[:, :H])
                sb, xb = Buf(slabs), Buf(x2)
                r0, o0 = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
                r1, o1 = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
                F.check(L.ffmi_rmsnorm_ex(a.ptr, xb.ptr, wb.ptr, r0.ptr, o0.ptr, T, H, EPS, 0, None))
                F.check(L.ffmi_debug_rmsnorm_partials(a.ptr, sb.ptr, S, NP, wb.ptr, r1.ptr, o1.ptr,
                                                      T, H, EPS, 0, None), (T, H, NP, S))
                ctx = (T, H, NP, S)
                res, out = r1.get(), o1.get()
                assert np.array_equal(bits(res), bits(r0.get())), ctx
                assert np.array_equal(bits(out), bits(o0.get())), ctx
                r_ref, o_ref = O.residual_rmsnorm(x1.astype(np.float32), x2.astype(np.float32),
                                                  w.astype(np.float32), EPS)
                assert np.array_equal(bits(res), bits(f16(r_ref))), ctx
                bound.add(out, o_ref)
                # in place, as the model runs it
                r2, o2 = Buf(x1), Buf.empty((T, H), np.float16)
                F.check(L.ffmi_debug_rmsnorm_partials(r2.ptr, sb.ptr, S, NP, wb.ptr, r2.ptr, o2.ptr,
                                                      T, H, EPS, 0, None), ctx)
                assert np.array_equal(bits(r2.get()), bits(res)), ctx
                assert np.array_equal(bits(o2.get()), bits(out)), ctx
                if H % 32 == 0 and T == 17:
                    r3, o3 = Buf.empty((T, H), np.float16), Buf.empty((32, H), np.float16)
                    F.check(L.ffmi_debug_rmsnorm_partials(a.ptr, sb.ptr, S, NP, wb.ptr, r3.ptr,
                                                          o3.ptr, T, H, EPS, F.Y_PACKED, None), ctx)
                    assert np.array_equal(bits(unpack_act_np(o3.get().reshape(-1), T, H)),
                                          bits(out)), ctx
                    assert np.array_equal(bits(r3.get()), bits(res)), ctx
    bound.finish()


# ---------------------------------------------------------------- attention, slab source
SLAB_S = (1, 2, 3, 5, 8)
# NP = the qkv width, one tile more, and a width that is a multiple of 4 only
SLAB_PAD = {1: 0, 2: 16, 3: 20, 5: 0, 8: 16}


def _slab_kw(S):
    """AttnCase.run arguments: the step's qkv as S slabs (run then compares the
    twin handle's outputs and caches after the step)"""
    return dict(slabs=S, slab_pad=SLAB_PAD[S])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_inc_slab_source(d):
    """INC: a 3-request prefill with 37 tokens in one request (two work items
    for it: the two-launch path, kv_update_kernel<d> with the run-time slab
    source), then a decode step (fused, one query tile, PSRC = 1).  Outputs, K
    and V^T caches bit-identical to the twin handle after both steps, at S 1 /
    2 / 3 / 5 / 8; the rows of S = 3 against the oracle."""
    for S in SLAB_S:
        rng = np.random.default_rng(d * 100 + S)
        c, kw = AttnCase(F.ATTN_INC, d=d), _slab_kw(S)
        lens = {0: 20, 1: 37, 2: 10}
        infos = [(5, p, r, p, p + 1, 0, 0, 0) for r, n in lens.items() for p in range(n)]
        out, qs = c.run(infos, rng=rng, **kw)
        got = [out[t] for t in range(len(infos))]
        want = [c.ref_row(qs[t], i[2], range(i[1] + 1)) for t, i in enumerate(infos)] if S == 3 else []
        infos = [(7, n, r, n, n + 1, 0, 0, 0) for r, n in lens.items()]
        out, qs = c.run(infos, rng=rng, **kw)
        if S == 3:
            got += [out[t] for t in range(len(infos))]
            want += [c.ref_row(qs[t], i[2], range(i[1] + 1)) for t, i in enumerate(infos)]
            c.check(np.stack(got), np.stack(want))


@pytest.mark.parametrize("path", ["default", "unsplit", "qsplit", "two_launch"])
@pytest.mark.parametrize("d", [64, 128])
def test_attention_tree_slab_source(d, path, monkeypatch):
    """TREE: a prompt step, a 21-node tree for two requests (fused, two query
    tiles), then the commits of an accepted path plus a second tree -- through
    the default launch, the unsplit two-tile one (FFMI_ATTN_QSPLIT=0), the
    query split (=2) and the KV-update + attention pair
    (FFMI_ATTN_NO_FUSE=1).  After every step the outputs and both caches equal
    the twin handle's, so the rows staged from slabs in one step are the rows
    the next step commits; the tree rows of S = 3 against the oracle."""
    env = {"unsplit": ("FFMI_ATTN_QSPLIT", "0"), "qsplit": ("FFMI_ATTN_QSPLIT", "2"),
           "two_launch": ("FFMI_ATTN_NO_FUSE", "1")}
    if path in env:
        monkeypatch.setenv(*env[path])
    parents = [-1, 0, 1] + [2 + (j - 3) // 3 for j in range(3, 21)]
    m = tree_masks(parents)
    depth = [12]
    for j in range(1, 21):
        depth.append(depth[parents[j]] + 1)

    def anc(j):
        out = []
        while j >= 0:
            out.append(j)
            j = parents[j]
        return sorted(out)

    for S in SLAB_S:
        rng = np.random.default_rng(300 + d + S)
        c, kw = AttnCase(F.ATTN_TREE, d=d), _slab_kw(S)
        infos = [(3, p, r, p, p + 1, 0, 0, 0) for r in (0, 2) for p in range(12)]
        c.run(infos, masks=[[0]] * 3, rng=rng, **kw)
        infos = [(4, depth[j], r, 12 + j, 12, 12, 21, j) for r in (0, 2) for j in range(21)]
        out, qs = c.run(infos, masks=[m, [0], m], rng=rng, **kw)
        got, want = [], []
        if S == 3:
            for t, i in enumerate(infos):
                got.append(out[t])
                want.append(c.ref_row(qs[t], i[2], list(range(12)) + [12 + a for a in anc(i[7])]))
        # accept a path of 4 per request, then a fresh 21-token tree at 16
        commits = [(21 * k + j, r, 12 + i) for k, r in enumerate((0, 2))
                   for i, j in enumerate([0, 1, 2, 5])]
        infos = [(4, depth[j] + 4, r, 16 + j, 16, 16, 21, j) for r in (0, 2) for j in range(21)]
        out, qs = c.run(infos, masks=[m, [0], m], commits=commits, rng=rng, **kw)
        if S == 3:
            for t, i in enumerate(infos):
                got.append(out[t])
                want.append(c.ref_row(qs[t], i[2], list(range(16)) + [16 + a for a in anc(i[7])]))
            c.check(np.stack(got), np.stack(want))


def test_attention_spec_slab_source():
    """SPEC at d = 64 (the 68M SSM's heads): the beam-layer steps of
    test_attention_spec_beam_layers with every step's qkv as slabs (fused, one
    query tile); twin-identical outputs and caches after every step, the last
    layer's rows against the oracle (at every S: two rows)."""
    for S in SLAB_S:
        K._spec_beam_layers(AttnCase(F.ATTN_SPEC, d=64), 8, np.random.default_rng(7 + S),
                            **_slab_kw(S))


# ---------------------------------------------------------------- norm, gather source
V = 64


def _desc(ids):
    T = len(ids)
    toks = (F.TokenInfo * T)(*[F.TokenInfo(int(i), 0, 0, -1, 1, 0, 0, 0, 0) for i in ids])
    return F.BatchDesc(T, 0, 0, 0, toks, None, None, None), toks


def _ids(T, rng):
    """token ids over a 64-row table: rows 0 and 63 and repeats among them"""
    ids = rng.integers(0, V, size=T)
    ids[0] = 0
    if T > 1:
        ids[-1] = V - 1
    if T > 3:
        ids[2] = ids[1]
    return ids.astype(np.int64)


def _gather_check(res, out, table, w, rows, ctx, bound, packed=False):
    """residual_out == table[rows] exactly; out == ffmi_rmsnorm of those rows
    bit for bit (beyond ffmi_rmsnorm's H <= 16384: the same plain norm through
    ffmi_rmsnorm_ex with no x2), and within the norm's oracle bound"""
    T, H = len(rows), table.shape[1]
    x = np.ascontiguousarray(table[rows])
    assert np.array_equal(bits(res.get()), bits(x)), ctx
    xb, wb, ob = Buf(x), Buf(w), Buf.empty((T, H), np.float16)
    if H <= 16384:
        F.check(L.ffmi_rmsnorm(xb.ptr, wb.ptr, ob.ptr, T, H, EPS, None))
    else:
        F.check(L.ffmi_rmsnorm_ex(xb.ptr, None, wb.ptr, None, ob.ptr, T, H, EPS, 0, None))
    got = unpack_act_np(out.get().reshape(-1), T, H) if packed else out.get()
    assert np.array_equal(bits(got), bits(ob.get())), ctx
    bound.add(got, O.rmsnorm(x.astype(np.float32), w.astype(np.float32), EPS))


@pytest.mark.parametrize("H", [8, 1024, 1032, 2056, 4104, 8200, 16384, 16392, 32768])
def test_rmsnorm_gather_source(H):
    """rmsnorm_kernel<NT, MAXC, 1, 3>, the embedding lookup inside layer 0's
    norm: NT 128 (H 8, 1024), 256, 512, 1024 and the 1024-thread forms with 2
    chunks per thread (H 8200 = 1025 chunks, 16384 = 2048 chunks, the last
    width launch_rmsnorm gives that form) and 4 (H 16392 = 2049 chunks, 32768
    = 4096, the widest row); T 1 / 7 / 300 of a 512-token batch.  Plain ids from the uploaded device blob; chained ids (-1 - i on
    half of the tokens, prev_ids a permutation); the blob fetch (the step
    staged, not copied: the norm reads the pinned staging and its grid copies
    the blob to the device, over a stale one -- ffmi_embedding, which reads
    the device blob only, must then see the new ids); FFMI_Y_PACKED once."""
    rng = np.random.default_rng(H)
    table = f16(rng.standard_normal((V, H)))
    w = f16(1 + rng.uniform(-0.1, 0.1, H))
    tb, wb = Buf(table), Buf(w)
    bound = NormBound()
    b = ctypes.c_void_p()
    F.check(L.ffmi_batch_create(512, 2, ctypes.byref(b)))
    try:
        for T in (1, 7, 300):
            ids = _ids(T, rng)
            # plain ids, device blob
            desc, _keep = _desc(ids)
            F.check(L.ffmi_batch_upload(b, ctypes.byref(desc), None))
            res, out = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
            F.check(L.ffmi_debug_rmsnorm_gather(b, None, tb.ptr, wb.ptr, res.ptr, out.ptr, H, EPS, 0,
                                                None, None), (T, H))
            _gather_check(res, out, table, w, ids, ("plain", T, H), bound)
            # chained ids: odd tokens carry -1 - i, i an index into prev_ids
            prev = rng.permutation(V).astype(np.int32)
            idx = rng.integers(0, V, size=T)
            chained = np.where(np.arange(T) % 2 == 1, -1 - idx, ids)
            rows = np.where(np.arange(T) % 2 == 1, prev[idx], ids)
            desc, _keep = _desc(chained)
            F.check(L.ffmi_batch_upload(b, ctypes.byref(desc), None))
            pb = Buf(prev)
            res, out = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
            F.check(L.ffmi_debug_rmsnorm_gather(b, None, tb.ptr, wb.ptr, res.ptr, out.ptr, H, EPS, 0,
                                                pb.ptr, None), (T, H))
            _gather_check(res, out, table, w, rows, ("chained", T, H), bound)
            if T == 7:
                continue
            # blob fetch: T = 1 (one workgroup copies the whole blob) and T = 300
            stale, _keep = _desc((ids + 17) % V)
            F.check(L.ffmi_batch_upload(b, ctypes.byref(stale), None))
            desc, _keep = _desc(ids)
            res, out = Buf.empty((T, H), np.float16), Buf.empty((T, H), np.float16)
            F.check(L.ffmi_debug_rmsnorm_gather(b, ctypes.byref(desc), tb.ptr, wb.ptr, res.ptr,
                                                out.ptr, H, EPS, 0, None, None), (T, H))
            _gather_check(res, out, table, w, ids, ("fetch", T, H), bound)
            emb = Buf.empty((T, H), np.float16)
            F.check(L.ffmi_embedding(b, tb.ptr, emb.ptr, H, None))
            assert np.array_equal(bits(emb.get()), bits(table[ids])), ("fetched blob", T, H)
        if H % 32 == 0:  # packed output tiles (T = 300 uploaded last)
            Tp = (T + 15) // 16 * 16
            res, out = Buf.empty((T, H), np.float16), Buf.empty((Tp, H), np.float16)
            F.check(L.ffmi_debug_rmsnorm_gather(b, None, tb.ptr, wb.ptr, res.ptr, out.ptr, H, EPS,
                                                F.Y_PACKED, None, None))
            _gather_check(res, out, table, w, ids, ("packed", T, H), bound, packed=True)
    finally:
        hip().hipDeviceSynchronize()
        L.ffmi_batch_destroy(b)
    bound.finish()
