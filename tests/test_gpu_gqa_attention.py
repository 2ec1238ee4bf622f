"""Native grouped-query attention handles (ffmi_attn_create_gqa) against MHA
handles of the same query heads, bit for bit.

A GQA handle of (num_heads, num_kv_heads) and an ffmi_attn_create handle of
num_heads heads take the same batches and the same q; the MHA handle's k / v
columns are the GQA ones repeated per query head (head h reads K/V head
h // G, HF repeat_kv).  Every head's arithmetic is then the same on both, so
after every step
  * the outputs are equal as bits,
  * GQA cache K/V head j equals MHA cache heads j G .. j G + G - 1 as bits,
  * every GQA cache slot no step wrote is still zero,
under route 1 (kv-indexed: one workgroup per item and query head), route 2
(group-shared wherever every item's queries x G fit the 16-row tile: one
workgroup per item and K/V head) and the automatic choice, each against the
MHA handle.  No tolerance anywhere but in the oracle test, which holds the
handle to the attention bar of DESIGN section 3 (2 fp16 ulp).
"""
import ctypes
import functools

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import test_gpu_kernels as K
from hip_util import Buf, f16, hip

pytestmark = pytest.mark.gpu

L = None

# (num_heads, num_kv_heads, d)
SHAPES = [(8, 2, 128),   # G = 4
          (8, 1, 64),    # multi-query, G = 8
          (16, 1, 64),   # G = 16: one query fills the tile
          (6, 2, 128),   # G = 3, not a power of two
          (4, 4, 128)]   # G = 1: the plain handle, the old kernels
ROUTES = (F.GQA_ROUTE_KV_INDEXED, F.GQA_ROUTE_GROUP_SHARED, F.GQA_ROUTE_AUTO)


def setup_module(module):
    global L
    L = F.lib()
    K.L = L  # (test_gpu_kernels sets it in its own setup_module)


class GqaPair(K.AttnCase):
    """K.AttnCase (the MHA handle, its batch builder and host-side cache
    model) plus GQA handles of kvh K/V heads, one per route, stepped on the
    same uploaded batch and compared after every step."""

    def __init__(self, mode, heads=8, kvh=2, d=128, oracle=False, **kw):
        super().__init__(mode, heads=heads, d=d, **kw)
        assert not self.fp32 and heads % kvh == 0
        self.kvh, self.G, self.oracle = kvh, heads // kvh, oracle
        self.gqa = {}
        for route in ROUTES:
            h = F.attn_create_gqa(self.cfg, kvh)
            F.attn_set_gqa_route(h, route)
            self.gqa[route] = h
        self.written = np.zeros((self.max_requests, self.slots), bool)
        self.steps = 0

    def close(self):
        for h in self.gqa.values():
            L.ffmi_attn_destroy(h)
        L.ffmi_attn_destroy(self.h)
        L.ffmi_batch_destroy(self.b)

    def gqa_caches(self, h):
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        slots = ctypes.c_int()
        F.check(L.ffmi_attn_kv_ptrs(h, ctypes.byref(k), ctypes.byref(v), ctypes.byref(slots)))
        assert slots.value == self.slots
        n = self.max_requests * self.kvh * self.slots * self.d
        assert F.attn_cache_bytes(h) == 2 * n * 2
        kc, vc = np.empty(n, np.uint16), np.empty(n, np.uint16)
        assert hip().hipDeviceSynchronize() == 0
        assert hip().hipMemcpy(kc.ctypes.data, k, n * 2, 2) == 0
        assert hip().hipMemcpy(vc.ctypes.data, v, n * 2, 2) == 0
        return kc, vc

    def run(self, infos, masks=None, commits=(), rng=None):
        T, Hl, Hk, G = len(infos), self.Hl, self.kvh * self.d, self.G
        g = f16(rng.standard_normal((T, Hl + 2 * Hk)))  # [q | k | v] at the GQA widths

        def rep(x):  # K/V head j -> query heads j G .. j G + G - 1
            return np.repeat(x.reshape(T, self.kvh, self.d), G, axis=1).reshape(T, Hl)
        mha = np.ascontiguousarray(
            np.concatenate([g[:, :Hl], rep(g[:, Hl:Hl + Hk]), rep(g[:, Hl + Hk:])], axis=1))
        res = super().run(infos, masks=masks, commits=commits, qkv=mha)  # (uploads the batch)
        want = np.asarray(res[0]).view(np.uint16)
        km, vm = self.caches(self.h)
        R, S, d = self.max_requests, self.slots, self.d
        km = km.reshape(R, self.kvh, G, S, d)
        vm = vm.reshape(R, self.kvh, G, d, S)
        for i in infos:
            if i[3] >= 0:
                self.written[i[2], i[3]] = True
        for (_, req, depth) in commits:
            self.written[req, depth] = True
        fn = {F.ATTN_INC: L.ffmi_attn_inc, F.ATTN_SPEC: L.ffmi_attn_spec,
              F.ATTN_TREE: L.ffmi_attn_tree}[self.mode]
        Tp = (T + 15) // 16 * 16
        qb = Buf(g)
        for route, h in self.gqa.items():
            ob = Buf.empty((Tp, Hl), np.float16)
            F.check(fn(h, self.b, qb.ptr, ob.ptr, None))
            out = ob.get()
            out = K.unpack_act_np(out.reshape(-1), T, Hl) if self.out_layout else out[:T]
            where = f"step {self.steps} route {route}"
            assert np.array_equal(np.asarray(out).view(np.uint16), want), f"{where}: output"
            if route == F.GQA_ROUTE_AUTO:
                continue  # (one of the two routes above: outputs only)
            kg, vg = self.gqa_caches(h)
            kg, vg = kg.reshape(R, self.kvh, 1, S, d), vg.reshape(R, self.kvh, 1, d, S)
            assert np.array_equal(np.broadcast_to(kg, km.shape), km), f"{where}: K cache"
            assert np.array_equal(np.broadcast_to(vg, vm.shape), vm), f"{where}: V^T cache"
            un = ~self.written
            assert not kg[:, :, 0][np.broadcast_to(un[:, None, :], (R, self.kvh, S))].any(), \
                f"{where}: unwritten K slots"
            assert not vg[:, :, 0][np.broadcast_to(un[:, None, None, :],
                                                   (R, self.kvh, d, S))].any(), \
                f"{where}: unwritten V^T slots"
        self.steps += 1
        return res

    # the differential scenarios need no oracle rows
    def ref_row(self, q, req, visible_slots):
        if self.oracle:
            return super().ref_row(q, req, visible_slots)
        return np.zeros(self.Hl, np.float32)

    def check(self, gpu, ref):
        if self.oracle:
            super().check(gpu, ref)


def inc_scenario(c, rng, decode_steps=40, collect=None):
    """INC, three requests (and a fourth that joins): prompts of 5, 33 and 70
    tokens in one step (items of 16 queries: the non-shared routes), 40 decode
    steps (kv_len crosses 32-key chunks and the LDS tail's alignment), a step
    that mixes a fresh 20-token chunk with decodes, then steps of 2, 4 and 5
    tokens per request (at G = 4: 8 and 16 rows are eligible for the
    group-shared form, 20 are not)."""
    def step(infos):
        out, qs = c.run(infos, rng=rng)
        if collect is not None:
            for t, i in enumerate(infos):
                collect.append((out[t], c.ref_row(qs[t], i[2], range(i[1] + 1))))
    n = {0: 5, 1: 33, 2: 70}
    step([(5, p, r, p, p + 1, 0, 0, 0) for r in n for p in range(n[r])])
    for _ in range(decode_steps):
        step([(7, n[r], r, n[r], n[r] + 1, 0, 0, 0) for r in n])
        for r in n:
            n[r] += 1
    step([(7, n[r], r, n[r], n[r] + 1, 0, 0, 0) for r in n] +
         [(5, p, 3, p, p + 1, 0, 0, 0) for p in range(20)])
    for r in n:
        n[r] += 1
    n[3] = 20
    for k in (2, 4, 5):
        step([(7, p, r, p, p + 1, 0, 0, 0) for r in n for p in range(n[r], n[r] + k)])
        for r in n:
            n[r] += k


@pytest.mark.parametrize("heads,kvh,d,layout",
                         [s + (0,) for s in SHAPES + [(32, 8, 128)]] + [(8, 2, 128, 1)])
def test_gqa_inc_prefill_decode_chunks(heads, kvh, d, layout):
    """(layout 1: the packed output tiles the model's handles write)"""
    c = GqaPair(F.ATTN_INC, heads=heads, kvh=kvh, d=d, max_requests=4, max_seq=160, tree=0,
                max_tokens=128, out_layout=layout)
    try:
        inc_scenario(c, np.random.default_rng(heads * 100 + kvh))
    finally:
        c.close()


@pytest.mark.parametrize("heads,kvh,d", [(8, 2, 128), (8, 1, 64)])
def test_gqa_inc_two_launch_path(heads, kvh, d, monkeypatch):
    """FFMI_ATTN_NO_FUSE=1: kv_update_kernel + attention, the group-shared form
    reading the rotated q from memory."""
    monkeypatch.setenv("FFMI_ATTN_NO_FUSE", "1")
    c = GqaPair(F.ATTN_INC, heads=heads, kvh=kvh, d=d, max_requests=4, max_seq=160, tree=0,
                max_tokens=128)
    try:
        inc_scenario(c, np.random.default_rng(7 + heads), decode_steps=30)
    finally:
        c.close()


@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_gqa_spec_beam_layers_width_3(heads, kvh, d):
    """SPEC: beam layers of width 3 over a 40-token prefix (and a second
    request over 17), one step per tree layer."""
    rng = np.random.default_rng(heads * 10 + kvh)
    c = GqaPair(F.ATTN_SPEC, heads=heads, kvh=kvh, d=d, max_requests=2, max_seq=96, tree=32,
                max_tokens=64)
    try:
        plen = {0: 40, 1: 17}
        c.run([(3, p, r, p, p + 1, 0, 0, 0) for r in plen for p in range(plen[r])],
              masks=[[0]] * 2, rng=rng)
        parents = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
        depth = [0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
        m = K.tree_masks(parents)
        for layer in range(5):
            nodes = [j for j in range(len(parents)) if depth[j] == layer]
            infos = [(5, plen[r] + layer, r, plen[r] + j, plen[r], plen[r], nodes[-1] + 1, j)
                     for r in plen for j in nodes]
            c.run(infos, masks=[m, m], rng=rng)
    finally:
        c.close()


@pytest.mark.parametrize("seed,path", [(0, "default"), (1, "default"), (0, "qsplit_off"),
                                       (1, "two_launch")])
@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_gqa_tree_random_trees_with_commits(heads, kvh, d, seed, path, monkeypatch):
    """TREE: test_gpu_kernels' random layer-order trees of up to 64 nodes with
    commits of random accepted paths, every step through GqaPair.run.  Trees
    over 16 nodes take, by default, the query-split form on these small grids;
    qsplit_off (FFMI_ATTN_QSPLIT=0) the two-tile fused kernel; two_launch
    (FFMI_ATTN_NO_FUSE=1) kv_update_kernel and the unfused kernels."""
    monkeypatch.setattr(K, "AttnCase", functools.partial(GqaPair, heads=heads, kvh=kvh))
    if path == "qsplit_off":
        monkeypatch.setenv("FFMI_ATTN_QSPLIT", "0")
        path = "default"
    K._random_tree_case(d, seed, path, monkeypatch, fp32=False)


@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_gqa_tree_commit_onto_stored_slot_and_long_commit(heads, kvh, d):
    """TREE: a commit whose depth is a slot the same step stores (the commit
    launch goes first, then the store wins), and a step with more commits
    than the fused prologue takes (the two-launch path with a small tree)."""
    rng = np.random.default_rng(heads + kvh)
    c = GqaPair(F.ATTN_TREE, heads=heads, kvh=kvh, d=d, max_requests=2, max_seq=96, tree=32,
                max_tokens=64)
    try:
        c.run([(3, p, 1, p, p + 1, 0, 0, 0) for p in range(12)], masks=[[0]] * 2, rng=rng)
        parents = [-1, 0, 1, 2, 2, 3, 4]
        depth = [12, 13, 14, 15, 15, 16, 16]
        c.run([(4, depth[j], 1, 12 + j, 12, 12, 7, j) for j in range(7)],
              masks=[[0], K.tree_masks(parents)], rng=rng)
        # root, a, b, c2 -> depths 12 .. 15; the new tree's root is stored at 15
        commits = [(0, 1, 12), (1, 1, 13), (2, 1, 14), (4, 1, 15)]
        chain = [-1] + list(range(10))  # an 11-node chain
        out, qs = c.run([(4, 15 + j, 1, 15 + j, 15, 15, 11, j) for j in range(11)],
                        masks=[[0], K.tree_masks(chain)], commits=commits, rng=rng)
        # (the oracle too: committed slots 12 .. 14, slot 15 as this step stored it)
        K.close16(out, np.stack([K.AttnCase.ref_row(c, qs[j], 1, range(16 + j))
                                 for j in range(11)]), exact_frac=0.98)
        # accept 10 of the chain (more than the 8 commits a work item carries)
        commits = [(j, 1, 15 + j) for j in range(10)]
        c.run([(4, 25 + j, 1, 25 + j, 25, 25, 2, j) for j in range(2)],
              masks=[[0], K.tree_masks([-1, 0])], commits=commits, rng=rng)
        c.run([(4, 25, 1, 25, 25, 25, 1, 0)], masks=[[0], [1]], rng=rng)
    finally:
        c.close()


def test_gqa_inc_against_the_oracle():
    """The INC scenario at (8, 2, 128): every (query, head) row against
    O.attention_row over the K/V of head h // G, within 2 fp16 ulp (the
    attention bar, K.close16 as AttnCase.check applies it)."""
    c = GqaPair(F.ATTN_INC, heads=8, kvh=2, d=128, max_requests=4, max_seq=160, tree=0,
                max_tokens=128, oracle=True)
    try:
        rows = []
        inc_scenario(c, np.random.default_rng(2024), collect=rows)
        c.check(np.stack([g for g, _ in rows]), np.stack([w for _, w in rows]))
    finally:
        c.close()


@pytest.mark.parametrize("heads,kvh,d", SHAPES + [(32, 8, 128)])
def test_gqa_cache_bytes(heads, kvh, d):
    R, S, tree = 3, 100, 23
    cfg = F.AttnCfg(F.ATTN_TREE, heads, d, R, S, tree, 32, 1.0 / np.sqrt(d), 10000.0, 0,
                    0, 1.0, 1.0, 4.0, 8192, 0)
    h = F.attn_create_gqa(cfg, kvh)
    try:
        slots = ctypes.c_int()
        F.check(L.ffmi_attn_kv_ptrs(h, None, None, ctypes.byref(slots)))
        assert slots.value == (S + tree + 31) // 32 * 32
        assert F.attn_cache_bytes(h) == 2 * R * kvh * slots.value * d * 2
    finally:
        L.ffmi_attn_destroy(h)
