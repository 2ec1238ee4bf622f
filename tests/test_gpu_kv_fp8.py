"""FFMI_ATTN_KV_FP8 handles (ffmi_attn_create_ex) beside the fp16 handle of
K.AttnCase, stepped on the same uploaded batches and the same qkv.

After every step the byte caches equal the host quantiser (x / scale in fp32,
clipped to +-448, nearest-even e4m3fn) applied to the fp16 handle's whole
caches, and every output row meets DESIGN section 3's attention bar (2 fp16
ulp, AttnCase.check) against O.attention_row over the DEQUANTISED bytes read
back.  V carries planted values that pin the format: +-1000 (saturation), 17
and 19 (ties), 2^-9 {0.5, 1, 1.5} and 2^-7 (subnormals, the bottom tie), -0.0.
"""
import ctypes
import functools

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
import test_gpu_kernels as K
from hip_util import Buf, f16, hip

pytestmark = pytest.mark.gpu

L = None
SHAPES = [(4, 4, 128), (4, 4, 64), (8, 2, 128), (6, 2, 64)]  # (heads, kv_heads, d)
SCALES = [(1.0, 1.0), (0.5, 3.0)]
PLANTED = np.array([1000, -1000, 17, 19, 2.0**-10, 2.0**-9, 1.5 * 2.0**-9, 2.0**-7, -0.0],
                   np.float16)
# e4m3fn magnitudes of codes 0 .. 126 (127 is NaN): subnormals m 2^-9, then (8 + m) 2^(e - 10)
_c = np.arange(127)
TAB = np.where(_c < 8, _c * 2.0**-9, (8 + (_c & 7)) * 2.0 ** ((_c >> 3) - 10.0))
assert (TAB[1], TAB[7], TAB[8], TAB[126]) == (2.0**-9, 7 * 2.0**-9, 2.0**-6, 448.0)


def setup_module(module):
    global L
    L = F.lib()
    K.L = L


def quantise(bits16, scale):
    """fp16 bits -> e4m3fn bytes of clip(x / scale): the nearest code of TAB, ties
    to the even one.  (Not torch.float8_e4m3fn: importing torch into the process
    that holds libffmi's HIP runtime aborts at exit.  Compared once on the CPU,
    the two agree on every non-NaN fp16 input at scales 1, 0.5 and 3.)"""
    y = np.clip(bits16.view(np.float16).astype(np.float32) / np.float32(scale), -448, 448)
    a = np.abs(y).astype(np.float64)
    hi = np.searchsorted(TAB, a).clip(0, 126)
    lo = (hi - 1).clip(0)
    dl, dh = a - TAB[lo], TAB[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    return (code | (np.signbit(y) << 7)).astype(np.uint8)


def dequantise(b, scale):
    return (np.where(b & 0x80, -1.0, 1.0) * TAB[b & 0x7f] * scale).astype(np.float32)


class Fp8Pair(K.AttnCase):
    def __init__(self, mode, heads=4, kvh=4, d=128, scales=(1.0, 1.0), **kw):
        super().__init__(mode, heads=heads, d=d, **kw)
        self.kvh, self.G, self.scales = kvh, heads // kvh, scales
        self.h8 = F.attn_create_ex(self.cfg, kvh, F.ATTN_KV_FP8, *scales)
        self.n8 = self.max_requests * kvh * self.slots * d
        assert F.attn_cache_bytes(self.h8) == 2 * self.n8
        self.written = np.zeros((self.max_requests, self.slots), bool)

    def run(self, infos, masks=None, commits=(), rng=None):
        T, Hl, Hk, G = len(infos), self.Hl, self.kvh * self.d, self.G
        g = f16(rng.standard_normal((T, Hl + 2 * Hk)))  # [q | k | v] at the handle's widths
        g[:, Hl + Hk:Hl + Hk + len(PLANTED)] = PLANTED

        def rep(x):  # K/V head j -> the fp16 MHA handle's heads j G .. j G + G - 1
            return np.repeat(x.reshape(T, self.kvh, self.d), G, axis=1).reshape(T, Hl)
        mha = np.ascontiguousarray(
            np.concatenate([g[:, :Hl], rep(g[:, Hl:Hl + Hk]), rep(g[:, Hl + Hk:])], axis=1))
        _, qs = super().run(infos, masks=masks, commits=commits, qkv=mha)  # (uploads the batch)
        R, S, d = self.max_requests, self.slots, self.d
        km, vm = self.caches(self.h)
        km = km.reshape(R, self.kvh, G, S, d)[:, :, 0]
        vm = vm.reshape(R, self.kvh, G, d, S)[:, :, 0]
        fn = {F.ATTN_INC: L.ffmi_attn_inc, F.ATTN_SPEC: L.ffmi_attn_spec,
              F.ATTN_TREE: L.ffmi_attn_tree}[self.mode]
        qb, ob = Buf(g), Buf.empty(((T + 15) // 16 * 16, Hl), np.float16)
        F.check(fn(self.h8, self.b, qb.ptr, ob.ptr, None))
        out = ob.get()
        out = K.unpack_act_np(out.reshape(-1), T, Hl) if self.out_layout else out[:T]
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        F.check(L.ffmi_attn_kv_ptrs(self.h8, ctypes.byref(k), ctypes.byref(v), None))
        k8, v8 = np.empty(self.n8, np.uint8), np.empty(self.n8, np.uint8)
        assert hip().hipDeviceSynchronize() == 0
        assert hip().hipMemcpy(k8.ctypes.data, k, self.n8, 2) == 0
        assert hip().hipMemcpy(v8.ctypes.data, v, self.n8, 2) == 0
        k8, v8 = k8.reshape(km.shape), v8.reshape(vm.shape)
        assert np.array_equal(k8, quantise(km, self.scales[0])), "K bytes"
        assert np.array_equal(v8, quantise(vm, self.scales[1])), "V^T bytes"
        for i in infos:
            if i[3] >= 0:
                self.written[i[2], i[3]] = True
        for (_, req, depth) in commits:
            self.written[req, depth] = True
        un = ~self.written
        assert not k8[np.broadcast_to(un[:, None, :], k8.shape[:3])].any(), "unwritten K slots"
        assert not v8[np.broadcast_to(un[:, None, None, :], v8.shape)].any(), "unwritten V^T slots"
        self.k8f, self.v8f = dequantise(k8, self.scales[0]), dequantise(v8, self.scales[1])
        return out, qs

    def ref_row(self, q, req, visible_slots):
        vis = list(visible_slots)
        ref = np.zeros((self.heads, self.d), np.float32)
        for hh in range(self.heads):
            ref[hh] = O.attention_row(q[hh], self.k8f[req, hh // self.G][vis],
                                      np.ascontiguousarray(self.v8f[req, hh // self.G][:, vis].T),
                                      np.ones(len(vis)), 1.0 / np.sqrt(self.d), fp16=1)
        return ref.reshape(-1)

    def step(self, infos, masks=None, commits=(), rng=None, rows=None):
        """run + every row's visible slots from its own record (the kernel's rule)"""
        out, qs = self.run(infos, masks=masks, commits=commits, rng=rng)
        for t, i in enumerate(infos):
            tree = [i[5] + j for j in range(i[6]) if (masks[i[2]][j] >> i[7]) & 1]
            rows.append((out[t], self.ref_row(qs[t], i[2], list(range(i[4])) + tree)))


def check_rows(c, rows):
    c.check(np.stack([g for g, _ in rows]), np.stack([w for _, w in rows]))


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("heads,kvh,d,layout", [s + (0,) for s in SHAPES] + [(8, 2, 128, 1)])
def test_kv_fp8_inc_prefill_decode_chunks(heads, kvh, d, layout, scales):
    """prompts of 5, 33 and 70 tokens in one step (items of 32 queries: QT = 2),
    28 decode steps (kv_len crosses 32 and 96), a fresh 20-token chunk mixed
    with decodes; layout 1: the packed output tiles of the model's handles"""
    rng, rows = np.random.default_rng(heads * 100 + kvh), []
    c = Fp8Pair(F.ATTN_INC, heads=heads, kvh=kvh, d=d, scales=scales, max_requests=4, max_seq=128,
                tree=0, max_tokens=128, out_layout=layout)
    n = {0: 5, 1: 33, 2: 70}
    c.step([(5, p, r, p, p + 1, 0, 0, 0) for r in n for p in range(n[r])], rng=rng, rows=rows)
    for _ in range(28):
        c.step([(7, n[r], r, n[r], n[r] + 1, 0, 0, 0) for r in n], rng=rng, rows=rows)
        n = {r: n[r] + 1 for r in n}
    c.step([(7, n[r], r, n[r], n[r] + 1, 0, 0, 0) for r in n] +
           [(5, p, 3, p, p + 1, 0, 0, 0) for p in range(20)], rng=rng, rows=rows)
    check_rows(c, rows)


@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_kv_fp8_spec_beam_layers_width_3(heads, kvh, d):
    rng, rows = np.random.default_rng(heads * 10 + kvh), []
    c = Fp8Pair(F.ATTN_SPEC, heads=heads, kvh=kvh, d=d, scales=SCALES[1], max_requests=2,
                max_seq=96, tree=32, max_tokens=64)
    plen = {0: 40, 1: 17}
    c.step([(3, p, r, p, p + 1, 0, 0, 0) for r in plen for p in range(plen[r])],
           masks=[[0]] * 2, rng=rng, rows=rows)
    parents = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    depth = [0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    m = K.tree_masks(parents)
    for layer in range(5):
        nodes = [j for j in range(len(parents)) if depth[j] == layer]
        c.step([(5, plen[r] + layer, r, plen[r] + j, plen[r], plen[r], nodes[-1] + 1, j)
                for r in plen for j in nodes], masks=[m, m], rng=rng, rows=rows)
    check_rows(c, rows)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_kv_fp8_tree_random_trees_with_commits(heads, kvh, d, seed, monkeypatch):
    """test_gpu_kernels' random layer-order trees of up to 64 nodes with commits
    of random accepted paths, every step through Fp8Pair.run"""
    monkeypatch.setattr(K, "AttnCase", functools.partial(Fp8Pair, heads=heads, kvh=kvh,
                                                         scales=SCALES[seed]))
    K._random_tree_case(d, seed, "default", monkeypatch, fp32=False)


@pytest.mark.parametrize("heads,kvh,d", SHAPES)
def test_kv_fp8_tree_commit_onto_stored_slot_and_recycled_request(heads, kvh, d):
    """A commit whose depth is a slot the same step stores (the commit launch
    goes first, then the store wins); then the request slot is recycled by a
    5-token prompt, its last occupant's bytes left in slots 5 .. of the chunk."""
    rng, rows = np.random.default_rng(heads + kvh), []
    c = Fp8Pair(F.ATTN_TREE, heads=heads, kvh=kvh, d=d, scales=SCALES[1], max_requests=2,
                max_seq=96, tree=32, max_tokens=64)
    c.step([(3, p, 1, p, p + 1, 0, 0, 0) for p in range(12)], masks=[[0]] * 2, rng=rng, rows=rows)
    parents, depth = [-1, 0, 1, 2, 2, 3, 4], [12, 13, 14, 15, 15, 16, 16]
    c.step([(4, depth[j], 1, 12 + j, 12, 12, 7, j) for j in range(7)],
           masks=[[0], K.tree_masks(parents)], rng=rng, rows=rows)
    commits = [(0, 1, 12), (1, 1, 13), (2, 1, 14), (4, 1, 15)]  # the new root is stored at 15
    chain = [-1] + list(range(10))
    c.step([(4, 15 + j, 1, 15 + j, 15, 15, 11, j) for j in range(11)],
           masks=[[0], K.tree_masks(chain)], commits=commits, rng=rng, rows=rows)
    c.step([(3, p, 1, p, p + 1, 0, 0, 0) for p in range(5)], masks=[[0]] * 2, rng=rng, rows=rows)
    c.step([(4, 5, 1, 5, 5, 5, 1, 0)], masks=[[0], [1]], rng=rng, rows=rows)
    check_rows(c, rows)


def test_kv_fp8_refusals():
    """decided before any HIP call: the test holds no device memory"""
    def cfg(d=128, mode=F.ATTN_INC, fp32=0):
        return F.AttnCfg(mode, 4, d, 2, 64, 0, 32, 1.0 / np.sqrt(d), 10000.0, 0,
                         0, 1.0, 1.0, 4.0, 8192, fp32)
    for c, ks, vs, st in [(cfg(fp32=1), 1.0, 1.0, "unsupported"), (cfg(d=32), 1.0, 1.0, "unsupported"),
                          (cfg(), 0.0, 1.0, "invalid"), (cfg(), 1.0, float("inf"), "invalid"),
                          (cfg(), float("nan"), 1.0, "invalid")]:
        with pytest.raises(F.FFMIError, match=f"{st}.*kv_fp8"):
            F.attn_create_ex(c, 4, F.ATTN_KV_FP8, ks, vs)
