"""Split-K launches of the M-split GEMM with their workgroups renumbered so
that a k-slice's column blocks share XCDs (ffmi::mid_xcd_map; FFMI_MID_XCD=0
is the plain blockIdx numbering, 1 the default: launches of 4 slices or more,
2 every split launch).  The renumbering only moves workgroups: every output
bit and every slab word must be what it was.

- ffmi_linear (M-split path, T 65 / 80 / 168): switch on (2, 1) == off as
  uint16, row-major and packed X / Y, four split shapes (two with nblk * S
  off a multiple of 8 and a ragged last tile block) and one gate/up-epilogue
  shape (unsplit: the map is inert); each result also within the oracle bar
  of test_gpu_kernels.py::test_linear_matches_oracle.
- the deferred-slab path (consumers combine the slabs): a 2-layer H = 512
  tree-mode model, one verify step of T = 80 rows, captured tensors and
  tokens identical with the switch on (2, 1) and off.
"""
import functools

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import oracle_lib as O
from hip_util import Buf, f16
from test_gpu_kernels import close16, pack_act_np, unpack_act_np

pytestmark = pytest.mark.gpu

SPLIT_SHAPES = [(512, 2048), (256, 4096), (384, 1024), (208, 1056)]
GATE_UP = (352, 512)
TS = [65, 80, 168]


@functools.lru_cache(maxsize=None)
def case(T, N, K, epi):
    """inputs and the oracle's result, computed once per shape"""
    rng = np.random.default_rng(31 * T + N + K + epi)
    X = f16(rng.standard_normal((T, K)))
    if epi:
        Wg, Wu = f16(rng.uniform(-0.05, 0.05, (N, K))), f16(rng.uniform(-0.05, 0.05, (N, K)))
        x32 = X.astype(np.float32)
        ref = O.silu_mul(O.linear(x32, Wg.astype(np.float32)), O.linear(x32, Wu.astype(np.float32)))
        W = (Wg, Wu)
    else:
        W = f16(rng.uniform(-0.05, 0.05, (N, K)))
        ref = O.linear(X.astype(np.float32), W.astype(np.float32), fp16=1)
    for a in (X, ref):
        a.setflags(write=False)
    return X, W, ref


def pack_weights(L, W, N, K, epi):
    nb = L.ffmi_linear_packed_bytes(N, K) * (2 if epi else 1)
    Wp = Buf.empty((nb // 2,), np.uint16)
    if epi:
        g, u = Buf(W[0]), Buf(W[1])
        F.check(L.ffmi_linear_pack_gate_up(g.ptr, u.ptr, N, K, Wp.ptr, None))
    else:
        src = Buf(W)
        F.check(L.ffmi_linear_pack_weight(src.ptr, N, K, Wp.ptr, None))
    Wp.get()  # (synchronises: the sources may go)
    return Wp


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N,K,epi", [(n, k, 0) for n, k in SPLIT_SHAPES] + [GATE_UP + (1,)])
def test_linear_renumbered_bit_identical(monkeypatch, T, N, K, epi):
    L = F.lib()
    split = L.ffmi_linear_workspace_bytes(T, N, K, epi) > 0
    # the planner must really split the four plain shapes (and not gate/up)
    assert split == (not epi), (T, N, K, epi)
    X, W, ref = case(T, N, K, epi)
    Wp = pack_weights(L, W, N, K, epi)
    Xr, Xp = Buf(X), Buf(pack_act_np(X))
    Tp = (T + 15) // 16 * 16
    layouts = [(0, 0), (1, 0)] + ([(1, 1)] if N % 32 == 0 else [])
    outs = {}
    for sw in ("2", "1", "0"):
        monkeypatch.setenv("FFMI_MID_XCD", sw)
        for xp, yp in layouts:
            Y = Buf.empty((Tp, N), np.float16)
            flags = epi | (F.X_PACKED if xp else 0) | (F.Y_PACKED if yp else 0)
            F.check(L.ffmi_linear((Xp if xp else Xr).ptr, Wp.ptr, Y.ptr, T, N, K, flags, None))
            y = Y.get()
            outs[sw, xp, yp] = unpack_act_np(y.reshape(-1), T, N) if yp else y[:T]
    base = outs["0", 0, 0].view(np.uint16)
    for key, y in outs.items():
        assert np.array_equal(y.view(np.uint16), base), key
    close16(outs["2", 0, 0], ref)


CFG = dict(num_layers=2, vocab_size=1000, num_heads=4, num_kv_heads=4, hidden=512,
           intermediate=1408, rms_eps=1e-6, rope_theta=10000.0)
SSM_CFG = dict(CFG, num_layers=1, num_heads=2, num_kv_heads=2, hidden=128, intermediate=256)
OPS = ("attn_norm", "qkv", "attn_out", "o_proj", "ffn_norm", "mlp_act", "down", "hidden")


def test_verify_step_deferred_slabs_bit_identical(monkeypatch):
    """qkv / o / down of a tree-mode model leave their split-K slabs to the
    attention prologue and the residual norms: one verify step of 80 rows
    (BOS + 79 prompt tokens, the request done after its first token) gives
    the same captured tensors and tokens with and without the renumbering."""
    T = 80
    L = F.lib()
    H, Fi = CFG["hidden"], CFG["intermediate"]
    for n, k in ((3 * H, H), (H, H), (H, Fi)):  # these GEMMs are split at this size
        assert L.ffmi_linear_workspace_bytes(T, n, k, 0) > 0, (n, k)
    prompt = np.random.default_rng(80).integers(3, CFG["vocab_size"], size=T - 1).tolist()
    runs = []
    for sw in ("2", "1", "0"):
        monkeypatch.setenv("FFMI_MID_XCD", sw)
        rm = fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=96,
                               max_sequence_length=128, spec_tree_width=(1, 1, 3))
        kw = dict(max_requests=1, max_tokens=96 + 23, max_seq_len=128)
        llm = fa.Model(CFG, "tree", weight_seed=21, **kw)
        ssm = fa.Model(SSM_CFG, "beam", weight_seed=22, **kw)
        rm.register_ssm_model(ssm)
        llm.set_debug(True)
        res = fa.generate(rm, llm, [prompt], max_length=T + 1)
        cap = [llm.debug_tensor(op, l) for l in range(CFG["num_layers"]) for op in OPS]
        cap.append(llm.debug_tensor("hidden", CFG["num_layers"]))
        cap.append(llm.debug_tensor("logits"))
        runs.append((cap, res[0].output_tokens))
        llm.close()
        ssm.close()
    base, tokens = runs[-1]
    assert len(tokens) == T + 1
    for cap, tok in runs[:-1]:
        assert tok == tokens
        for x, y in zip(cap, base):
            assert x.shape[0] == T, x.shape  # the captured step is the 80-row verify step
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
