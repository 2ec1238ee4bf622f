"""The CPU oracle's fp16 forward pass (oracle/oracle.cc orc_model_forward_ex)
over a dict of HF-named tensors, op by op through the oracle's own exported
kernels (oracle_lib.linear / rmsnorm / residual_rmsnorm / silu_mul /
attention_row / rope_table): oracle_lib.Model generates its weights from a
seed and cannot take a merged checkpoint.  forward() on the oracle model's own
tensors returns that model's logits bit for bit, which the tests that use it
assert first.

merge(): W' = fp16(W + (alpha / r) B A) of HF PEFT's merge_and_unload, in
float64, or with the update rounded to fp16 first (the other place a merge
may round).
"""
import numpy as np

import oracle_lib as O
from test_gpu_fulldepth import rope_ref

MODULES = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
           "down_proj": "mlp"}


def forward(state, cfg, tokens):
    """logits [T][V] of one prompt-phase step from position 0"""
    H, nh = cfg["hidden"], cfg["num_heads"]
    nkv = cfg.get("num_kv_heads", nh)
    d, G, eps = H // nh, nh // nkv, cfg.get("rms_eps", 1e-6)
    T = len(tokens)
    tab = O.rope_table(T, d, cfg.get("rope_theta", 10000.0))
    scale = float(np.float32(1) / np.sqrt(np.float32(d)))
    res = state["model.embed_tokens.weight"][np.asarray(tokens)].astype(np.float32)
    mlp = None
    for l in range(cfg["num_layers"]):
        p = f"model.layers.{l}."
        w = lambda n: state[p + n + ".weight"]
        if l == 0:
            h = O.rmsnorm(res, w("input_layernorm"), eps)
        else:
            res, h = O.residual_rmsnorm(res, mlp, w("input_layernorm"), eps)
        q, k, v = (O.linear(h, w(f"self_attn.{x}_proj")) for x in "qkv")
        q = np.stack([rope_ref(q[t], t, d, tab) for t in range(T)])
        k = np.stack([rope_ref(k[t], t, d, tab) for t in range(T)])
        att = np.zeros((T, H), np.float32)
        for hd in range(nh):
            qs, ks = slice(hd * d, (hd + 1) * d), slice((hd // G) * d, (hd // G + 1) * d)
            for t in range(T):
                att[t, qs] = O.attention_row(q[t, qs], k[:, ks], v[:, ks], np.arange(T) <= t, scale)
        o = O.linear(att, w("self_attn.o_proj"))
        res, h = O.residual_rmsnorm(res, o, w("post_attention_layernorm"), eps)
        a = O.silu_mul(O.linear(h, w("mlp.gate_proj")), O.linear(h, w("mlp.up_proj")))
        mlp = O.linear(a, w("mlp.down_proj"))
    _, h = O.residual_rmsnorm(res, mlp, state["model.norm.weight"], eps)
    return O.linear(h, state["lm_head.weight"])


def merge(state, adapters, alpha, round_update=False):
    """a copy of `state` with W' = fp16(W + s B A) for adapters {module: (A
    [L][r][in], B [L][out][r])}, s = alpha / r, the sum in float64;
    round_update: W'' = fp16(W + fp16(s B A))"""
    out = dict(state)
    for mod, (A, B) in adapters.items():
        s = float(alpha) / A.shape[1]
        for l in range(A.shape[0]):
            n = f"model.layers.{l}.{MODULES[mod]}.{mod}.weight"
            upd = s * (B[l].astype(np.float64) @ A[l].astype(np.float64))
            if round_update:
                upd = upd.astype(np.float16).astype(np.float64)
            out[n] = (state[n].astype(np.float64) + upd).astype(np.float16).astype(np.float32)
    return out
