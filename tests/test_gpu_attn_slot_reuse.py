"""Attention on a recycled request slot: a row depends only on the slots
visible to it, and a step writes only the slots it was asked to write.

Every handle elsewhere in the suite starts zeroed (ffmi_attn_create).  Serving
does not: a request slot passes to the next request with the last occupant's
K, V^T and staging rows in it, and in TREE mode with the rejected speculative
tokens' rows past the accepted prefix.  Every case here runs one script -- a
list of steps whose qkv two equally seeded generators draw -- on two handles
of one config, a fresh one and one dirtied first, and after every step
  * the outputs are equal as bits,
  * on the slots the script has written so far (stores and commits) K and V^T
    are equal as bits,
  * on every other slot of every request the dirty handle still holds its
    dirt, bit for bit.
No tolerance anywhere; the dirty handle's rows are also held to the oracle
(AttnCase.check), so the two handles cannot be wrong alike.

Dirt kinds: `occupant`, a longer earlier request run through the same handle
in the same slots (TREE: a prompt and two verify steps whose trees are only
partly committed); `finite`, every word of both caches a seeded value with
|x| in [256, 65504] and a random sign (a leak of any non-zero weight is far
outside every bar); `nonfinite`, the same from {NaN, +Inf, -Inf}: a masked key
whose V is multiplied by an exactly zero weight still gives NaN.

Slots 0 and 3 of 4 are active, 1 and 2 idle but dirty.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import test_gpu_gqa_attention as GQ
import test_gpu_kernels as K
from hip_util import f16, hip, report

pytestmark = pytest.mark.gpu

L = None
DIRT = ("occupant", "finite", "nonfinite")
CFG = dict(max_requests=4, max_seq=96, tree=32, max_tokens=128)
PATH_ENV = {"default": None, "no_fuse": ("FFMI_ATTN_NO_FUSE", "1"),
            "qsplit": ("FFMI_ATTN_QSPLIT", "2")}
# the 21-node tree of test_attention_tree_fused_equals_two_launch_path and the
# 7-node one of test_attention_tree_verify_and_commit
TREE21 = [-1, 0, 1] + [2 + (j - 3) // 3 for j in range(3, 21)]
TREE7 = [-1, 0, 1, 2, 2, 3, 4]


def setup_module(module):
    global L
    L = F.lib()
    K.L = GQ.L = L  # (AttnCase and GqaPair call through their modules' handles)


# ---------------------------------------------------------------- cache access
def _kv_ptrs(h):
    k, v = ctypes.c_void_p(), ctypes.c_void_p()
    F.check(L.ffmi_attn_kv_ptrs(h, ctypes.byref(k), ctypes.byref(v), None))
    return k, v


def read_kv(c, h, nh):
    """K and V of handle h (nh K/V heads) as bits, both [req][head][slot][d]
    (fp16 handles keep V^T, [req][head][d][slot]: transposed here)"""
    dt = np.uint32 if c.fp32 else np.uint16
    n = c.max_requests * nh * c.slots * c.d
    assert F.attn_cache_bytes(h) == 2 * n * dt().itemsize
    out = []
    assert hip().hipDeviceSynchronize() == 0
    for p in _kv_ptrs(h):
        a = np.empty(n, dt)
        assert hip().hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0
        out.append(a)
    k = out[0].reshape(c.max_requests, nh, c.slots, c.d)
    v = out[1].reshape(k.shape) if c.fp32 else \
        out[1].reshape(c.max_requests, nh, c.d, c.slots).transpose(0, 1, 3, 2)
    return k, v


def write_kv(c, h, nh, k, v):
    """the reverse: [req][head][slot][d] bits into the caches of handle h
    (hipMemcpy host to device through the ffmi_attn_kv_ptrs pointers)"""
    dt = np.uint32 if c.fp32 else np.uint16
    assert k.dtype == dt and v.dtype == dt and k.shape == v.shape == \
        (c.max_requests, nh, c.slots, c.d)
    assert F.attn_cache_bytes(h) == 2 * k.nbytes
    kp, vp = _kv_ptrs(h)
    arrs = (np.ascontiguousarray(k),
            np.ascontiguousarray(v if c.fp32 else v.transpose(0, 1, 3, 2)))
    assert hip().hipDeviceSynchronize() == 0
    for p, a in zip((kp, vp), arrs):
        assert hip().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    for got, want in zip(read_kv(c, h, nh), (k, v)):
        assert np.array_equal(got, want), "dirt read back"


def dirt_words(kind, rng, shape, fp32):
    """seeded cache words: finite with |x| in [256, 65504] and a random sign,
    or non-finite from {NaN, +Inf, -Inf}"""
    if kind == "finite":
        bits = rng.integers(0x5C00, 0x7C00, size=shape).astype(np.uint16)  # 256 .. 65504
        bits |= (rng.integers(0, 2, size=shape) << 15).astype(np.uint16)
        x = bits.view(np.float16).astype(np.float32)
        assert (np.abs(x) >= 256).all() and (np.abs(x) <= 65504).all()
        return x.view(np.uint32) if fp32 else bits
    assert kind == "nonfinite"
    pick = rng.integers(0, 3, size=shape)
    if fp32:
        return np.array([0x7fc00000, 0x7f800000, 0xff800000], np.uint32)[pick]
    return np.array([0x7e00, 0x7c00, 0xfc00], np.uint16)[pick]


def handles(c):
    """(name, handle, K/V heads) of every handle the case steps"""
    out = [("mha", c.h, c.heads)]
    if c.twin is not None:
        out.append(("twin", c.twin, c.heads))
    for route, h in getattr(c, "gqa", {}).items():
        out.append((f"gqa route {route}", h, c.kvh))
    return out


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


# ---------------------------------------------------------------- the pair
def occupy(c, rng, kw):
    """the earlier, longer occupant of every request slot, through c's own run"""
    R = c.max_requests
    if c.mode != F.ATTN_TREE:
        for r in range(R):  # 70 positions per slot
            c.run([(5, p, r, p, p + 1, 0, 0, 0) for p in range(70)],
                  masks=None if c.mode == F.ATTN_INC else [[0]] * R, rng=rng, **kw)
        return
    # a 30-token prompt, a 21-node tree at 30 of which 4 are accepted, a
    # second tree at 34 that is never committed: rejected rows in the slots
    # 34 .. 54, staging rows of both steps in `stage`
    m, depth = K.tree_masks(TREE21), [0]
    for j in range(1, 21):
        depth.append(depth[TREE21[j]] + 1)
    c.run([(3, p, r, p, p + 1, 0, 0, 0) for r in range(R) for p in range(30)],
          masks=[[0]] * R, rng=rng, **kw)
    c.run([(4, 30 + depth[j], r, 30 + j, 30, 30, 21, j) for r in range(R) for j in range(21)],
          masks=[m] * R, rng=rng, **kw)
    commits = [(21 * r + j, r, 30 + i) for r in range(R) for i, j in enumerate([0, 1, 2, 5])]
    c.run([(4, 34 + depth[j], r, 34 + j, 34, 34, 21, j) for r in range(R) for j in range(21)],
          masks=[m] * R, commits=commits, rng=rng, **kw)


class Pair:
    """A fresh and a dirtied case of one config, stepped on the same inputs and
    compared after every step.  Stands in for a case towards the scripts (run,
    ref_row, check: the dirty one's)."""

    def __init__(self, make, dirt, seed, **kw):
        self.fresh, self.dirty = make(), make()
        f, d = self.fresh, self.dirty
        self.kw = kw  # further arguments of every run (slabs, oproj)
        if kw:  # the twin handle run makes on first use: made now, dirtied alike
            d.twin = ctypes.c_void_p()
            F.check(L.ffmi_attn_create(ctypes.byref(d.cfg), ctypes.byref(d.twin)))
        if hasattr(d, "gqa"):
            d.written[:] = True  # (GqaPair.run: no slot of this one is expected zero)
        if dirt == "occupant":
            occupy(d, np.random.default_rng([seed, 1]), kw)
        else:
            rng = np.random.default_rng([seed, 2])
            nb = getattr(d, "kvh", d.heads)
            shape = (d.max_requests, nb, d.slots, d.d)
            k, v = (dirt_words(dirt, rng, shape, d.fp32) for _ in range(2))
            for _, h, nh in handles(d):  # an MHA handle beside GQA ones: heads repeated
                write_kv(d, h, nh, np.repeat(k, nh // nb, axis=1), np.repeat(v, nh // nb, axis=1))
        self.snap = {name: read_kv(d, h, nh) for name, h, nh in handles(d)}
        self.rngs = [np.random.default_rng([seed, 0]) for _ in range(2)]
        self.written = np.zeros((d.max_requests, d.slots), bool)
        self.outs, self.rows, self.words = [], 0, 0
        self.mode = d.mode

    def run(self, infos, masks=None, commits=(), rng=None, **kw):
        assert rng is None and not kw
        res = [c.run(infos, masks=masks, commits=commits, rng=g, **self.kw)
               for c, g in zip((self.fresh, self.dirty), self.rngs)]
        where = f"step {len(self.outs)}"
        assert np.array_equal(bits(res[0][0]), bits(res[1][0])), f"{where}: outputs"
        if len(res[0]) == 4:  # the folded o projection's slabs
            assert res[0][3] == res[1][3] == 1, f"{where}: not projected"
            assert np.array_equal(bits(res[0][2]), bits(res[1][2])), f"{where}: o-proj slabs"
        for i in infos:
            if i[3] >= 0:
                self.written[i[2], i[3]] = True
        for (_, req, depth) in commits:
            self.written[req, depth] = True
        hf, hd = handles(self.fresh), handles(self.dirty)
        assert [x[0] for x in hf] == [x[0] for x in hd] == list(self.snap)
        for (name, a, nh), (_, b, _) in zip(hf, hd):
            for what, x, y, z in zip(("K", "V"), read_kv(self.fresh, a, nh),
                                     read_kv(self.dirty, b, nh), self.snap[name]):
                w = np.broadcast_to(self.written[:, None, :, None], x.shape)
                assert np.array_equal(x[w], y[w]), f"{where}, {name}: written {what} slots"
                assert np.array_equal(y[~w], z[~w]), f"{where}, {name}: {what} dirt disturbed"
                self.words += x.size
        self.rows += len(infos)
        self.outs.append(bits(res[1][0]).copy())
        return res[1]

    def ref_row(self, q, req, vis):
        return self.dirty.ref_row(q, req, vis)

    def check(self, gpu, ref):
        self.dirty.check(gpu, ref)

    def final(self):
        """what the paths must agree on: every step's output and the dirty
        handle's whole caches"""
        return self.outs + [a.copy() for a in read_kv(self.dirty, self.dirty.h, self.dirty.heads)]

    def finish(self, name, **kv):
        report("attn_slot_reuse", case=name, rows=self.rows, cache_words=self.words, **kv)
        for c in (self.fresh, self.dirty):
            for nm, h, _ in handles(c):
                if nm != "mha":
                    L.ffmi_attn_destroy(h)
            L.ffmi_attn_destroy(c.h)
            L.ffmi_batch_destroy(c.b)


class HostCase:
    """The scripts on the CPU alone, in numpy float64: the expected row of
    every query, asserted finite (so the dirt is the only source of a
    non-finite value on the GPU).  The host side of AttnCase.run without a
    handle."""

    def __init__(self, mode, heads=2, d=128, fp32=False, seed=0):
        self.mode, self.heads, self.d, self.fp32 = mode, heads, d, fp32
        self.rng = np.random.default_rng([seed, 0])
        self.kc, self.rows = {}, 0

    def rope(self, x, pos):
        x = x.astype(np.float64).reshape(self.heads, self.d)
        h = self.d // 2
        ang = pos * 10000.0 ** (-np.arange(h) / h)
        a, b = x[:, :h], x[:, h:]
        return np.concatenate([a * np.cos(ang) - b * np.sin(ang),
                               a * np.sin(ang) + b * np.cos(ang)], axis=1)

    def run(self, infos, masks=None, commits=(), rng=None):
        Hl = self.heads * self.d
        qkv = self.rng.standard_normal((len(infos), 3 * Hl)).astype(np.float32)
        if not self.fp32:
            qkv = f16(qkv)
        for (src, req, depth) in commits:
            self.kc[(req, depth)] = self.stage[src]
        self.stage, qs = {}, []
        for t, i in enumerate(infos):
            k = self.rope(qkv[t, Hl:2 * Hl], i[1])
            self.stage[t] = (k, qkv[t, 2 * Hl:].astype(np.float64).reshape(self.heads, self.d))
            if i[3] >= 0:
                self.kc[(i[2], i[3])] = self.stage[t]
            qs.append(self.rope(qkv[t, :Hl], i[1]))
        return np.zeros((len(infos), Hl)), qs

    def ref_row(self, q, req, vis):
        Kh = np.stack([self.kc[(req, s)][0] for s in vis], 1)  # heads, n, d
        Vh = np.stack([self.kc[(req, s)][1] for s in vis], 1)
        s = np.einsum("hd,hnd->hn", q, Kh) / np.sqrt(self.d)
        p = np.exp(s - s.max(1, keepdims=True))
        return np.einsum("hn,hnd->hd", p / p.sum(1, keepdims=True), Vh).reshape(-1)

    def check(self, gpu, ref):
        ref = np.asarray(ref)
        assert ref.size and np.isfinite(ref).all()
        self.rows += ref.reshape(-1, self.heads * self.d).shape[0]


# ---------------------------------------------------------------- the scripts
def ancestors(parents, j):
    out = []
    while j >= 0:
        out.append(j)
        j = parents[j]
    return sorted(out)


def inc_script(p):
    """INC on slots 0 and 3: a 37-token prefill (two work items: the unfused
    kernels); a decode of it beside a 5-token prefill (one item each: fused);
    chunks of 23 and 24 tokens (fused, two query tiles); six decode steps over
    kv_len 62 .. 67 and 30 .. 35 (31 -> 32 -> 33 and 63 -> 64 -> 65: the last
    chunk full, one key into the next).  Every row against the oracle."""
    got, want = [], []

    def step(infos):
        res = p.run(infos)
        for t, i in enumerate(infos):
            got.append(res[0][t])
            want.append(p.ref_row(res[1][t], i[2], range(i[1] + 1)))

    def toks(r, a, b):
        return [(7, q, r, q, q + 1, 0, 0, 0) for q in range(a, b)]
    step(toks(0, 0, 37))
    step(toks(0, 37, 38) + toks(3, 0, 5))
    step(toks(0, 38, 61) + toks(3, 5, 29))
    for n in range(6):
        step(toks(0, 61 + n, 62 + n) + toks(3, 29 + n, 30 + n))
    p.check(np.stack(got), np.stack(want))


def short_inc_script(p):
    """INC, one item of at most 16 queries per request in every step (fused;
    the folded o projection's launch): prefills of 16 and 9 tokens, chunks of
    14 and 5, three decode steps over kv_len 31 -> 32 -> 33 and 15 -> 17"""
    got, want = [], []

    def step(infos):
        res = p.run(infos)
        for t, i in enumerate(infos):
            got.append(res[0][t])
            want.append(p.ref_row(res[1][t], i[2], range(i[1] + 1)))

    def toks(r, a, b):
        return [(7, q, r, q, q + 1, 0, 0, 0) for q in range(a, b)]
    step(toks(0, 0, 16) + toks(3, 0, 9))
    step(toks(0, 16, 30) + toks(3, 9, 14))
    for n in range(3):
        step(toks(0, 30 + n, 31 + n) + toks(3, 14 + n, 15 + n))
    p.check(np.stack(got), np.stack(want))


def tree_script(p):
    """TREE on slots 0 and 3: 12 prompt tokens each; the 7-node tree of
    test_attention_tree_verify_and_commit on slot 0 beside the 21-node tree of
    test_attention_tree_fused_equals_two_launch_path on slot 3 (12 + 21 > 32:
    over a chunk boundary); then the commits of an accepted path of 4 on both
    (root a b c2; nodes 0 1 2 5), a 3-node tree and a fresh 21-node tree at
    16.  Every row against the oracle."""
    got, want = [], []
    idle = [0]
    m7, m21, m3 = K.tree_masks(TREE7), K.tree_masks(TREE21), K.tree_masks([-1, 0, 0])
    d7, d3, d21 = [0, 1, 2, 3, 3, 4, 4], [0, 1, 1], [0]
    for j in range(1, 21):
        d21.append(d21[TREE21[j]] + 1)

    def step(infos, masks, vis, commits=()):
        out, qs = p.run(infos, masks=masks, commits=commits)
        for t, i in enumerate(infos):
            got.append(out[t])
            want.append(p.ref_row(qs[t], i[2], vis[t]))
    infos = [(3, q, r, q, q + 1, 0, 0, 0) for r in (0, 3) for q in range(12)]
    step(infos, [idle] * 4, [range(i[1] + 1) for i in infos])
    infos = [(4, 12 + d7[j], 0, 12 + j, 12, 12, 7, j) for j in range(7)] + \
            [(4, 12 + d21[j], 3, 12 + j, 12, 12, 21, j) for j in range(21)]
    vis = [list(range(12)) + [12 + a for a in ancestors(TREE7, j)] for j in range(7)] + \
          [list(range(12)) + [12 + a for a in ancestors(TREE21, j)] for j in range(21)]
    step(infos, [m7, idle, idle, m21], vis)
    commits = [(j, 0, 12 + i) for i, j in enumerate([0, 1, 2, 4])] + \
              [(7 + j, 3, 12 + i) for i, j in enumerate([0, 1, 2, 5])]
    infos = [(4, 16 + d3[j], 0, 16 + j, 16, 16, 3, j) for j in range(3)] + \
            [(4, 16 + d21[j], 3, 16 + j, 16, 16, 21, j) for j in range(21)]
    vis = [list(range(16)) + [16 + a for a in ancestors([-1, 0, 0], j)] for j in range(3)] + \
          [list(range(16)) + [16 + a for a in ancestors(TREE21, j)] for j in range(21)]
    step(infos, [m3, idle, idle, m21], vis, commits)
    p.check(np.stack(got), np.stack(want))


def spec_script(p):
    """the beam-layer sequence of test_attention_spec_beam_layers"""
    K._spec_beam_layers(p, 8, None)


SCRIPTS = {F.ATTN_INC: inc_script, F.ATTN_TREE: tree_script, F.ATTN_SPEC: spec_script}


def set_path(monkeypatch, path):
    if PATH_ENV[path]:
        monkeypatch.setenv(*PATH_ENV[path])


def run_case(name, mode, dirt, seed, script=None, make=None, run_kw=None, **case_kw):
    make = make or (lambda: K.AttnCase(mode, **CFG, **case_kw))
    p = Pair(make, dirt, seed, **(run_kw or {}))
    (script or SCRIPTS[mode])(p)
    final = p.final()
    p.finish(name, dirt=dirt, **{k: v for k, v in case_kw.items() if not callable(v)})
    return final


# ---------------------------------------------------------------- the tests
# (layout, fp32, path): the fp32 handle has one path
INC_FORMS = [(0, False, "default"), (0, False, "no_fuse"), (1, False, "default"),
             (1, False, "no_fuse"), (0, True, "default")]
TREE_FORMS = [(False, "default"), (False, "qsplit"), (False, "no_fuse"), (True, "default")]


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("layout,fp32,path", INC_FORMS)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_inc_slot_reuse(d, layout, fp32, path, dirt, monkeypatch):
    set_path(monkeypatch, path)
    run_case(f"inc/{path}", F.ATTN_INC, dirt, 1000 + d, d=d, out_layout=layout, fp32=fp32)


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("fp32,path", TREE_FORMS)
@pytest.mark.parametrize("d", [64, 128])
def test_tree_slot_reuse(d, fp32, path, dirt, monkeypatch):
    set_path(monkeypatch, path)
    run_case(f"tree/{path}", F.ATTN_TREE, dirt, 2000 + d, d=d, fp32=fp32)


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("fp32", [False, True])
def test_spec_slot_reuse(fp32, dirt):
    run_case("spec/default", F.ATTN_SPEC, dirt, 3000, d=64, fp32=fp32)


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("mode", [F.ATTN_INC, F.ATTN_TREE])
@pytest.mark.parametrize("heads,kvh,d", [(8, 2, 128), (16, 1, 64)])
def test_gqa_slot_reuse(heads, kvh, d, mode, dirt):
    """GQA handles under the kv-indexed, the group-shared and the automatic
    route beside the MHA handle of replicated K/V (GqaPair, which also holds
    each GQA handle to the MHA one after every step), all dirtied alike"""
    run_case(f"gqa/{'inc' if mode == F.ATTN_INC else 'tree'}", mode, dirt, 4000 + heads,
             make=lambda: GQ.GqaPair(mode, heads=heads, kvh=kvh, d=d, **CFG))


@pytest.mark.parametrize("dirt", DIRT)
def test_slab_source_slot_reuse(dirt):
    """the step's qkv as 3 deferred split-K slabs (ffmi_debug_attn_partials):
    AttnCase.run's twin handle dirtied like the handle itself, so its
    whole-cache comparison of the two stays valid"""
    run_case("inc/slabs", F.ATTN_INC, dirt, 5000, d=64, run_kw=dict(slabs=3, slab_pad=20))


@pytest.mark.parametrize("dirt", DIRT)
def test_folded_oproj_slot_reuse(dirt):
    """the o projection folded into the fused attention
    (ffmi_debug_attn_oproj): projected in every step of the script, and the
    fp32 slabs of the two handles equal as bits as well"""
    import oproj_rule as R
    w = R.Dense(2, 128, np.random.default_rng(6000))
    run_case("inc/oproj", F.ATTN_INC, dirt, 6000, script=short_inc_script, d=64,
             run_kw=dict(oproj=(w.Wo, w.N, 128)))


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("mode,d", [(F.ATTN_INC, 32), (F.ATTN_INC, 64), (F.ATTN_INC, 128),
                                    (F.ATTN_TREE, 64), (F.ATTN_TREE, 128)])
def test_paths_agree_on_a_dirty_handle(mode, d, dirt, monkeypatch):
    """The one-launch path, the KV-update + attention pair and (TREE) the query
    split on handles of the same dirt: every step's output and the whole K and
    V^T caches bit-identical (the fused versus two-launch tests of
    test_gpu_kernels assert this on fresh handles only)."""
    paths = ["default", "no_fuse"] + (["qsplit"] if mode == F.ATTN_TREE else [])
    finals = []
    for path in paths:
        with monkeypatch.context() as mp:
            set_path(mp, path)
            finals.append(run_case(f"paths/{path}", mode, dirt, 7000 + d, d=d))
    for path, other in zip(paths[1:], finals[1:]):
        assert len(other) == len(finals[0])
        for i, (a, b) in enumerate(zip(finals[0], other)):
            assert np.array_equal(a, b), f"default vs {path}: item {i} (outputs, then K, V)"


@pytest.mark.parametrize("mode,d,fp32", [(F.ATTN_INC, 32, False), (F.ATTN_INC, 128, True),
                                         (F.ATTN_TREE, 64, False), (F.ATTN_SPEC, 64, False)])
def test_expected_rows_are_finite_on_the_cpu(mode, d, fp32):
    """the scripts in numpy alone, seeded as above: every expected row is
    finite, so a non-finite output can only come from the dirt"""
    seed = {F.ATTN_INC: 1000 + d, F.ATTN_TREE: 2000 + d, F.ATTN_SPEC: 3000}[mode]
    c = HostCase(mode, d=d, fp32=fp32, seed=seed)
    SCRIPTS[mode](c)
    assert c.rows > 0
