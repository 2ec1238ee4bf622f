"""FFMI_MODEL_W4 (Model(weight_dtype="mxfp4")): the 2-layer, hidden-256 models of
tests/test_gpu_kv_fp8_model.py, MHA and GQA under native_gqa, with OCP MXFP4
linear weights.

Asserted: the resident weight bytes; one prefill's logits against the oracle
over the host-quantised, dequantised weights (and nearer to it than to the
fp16-weight oracle); graph replay gives the eager tokens; SpecInfer equals the
flagged model's own incremental decoding on the token chain; the combination
with the 8-bit KV cache; the refusals.  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import lora_merge_oracle as MO
import oracle_lib as O
from test_gpu_alignment import close_ulp
from test_gpu_gqa_oracle import oracle_state, prefill_logits
from test_gpu_kv_fp8_model import CFGS, LEN, PROMPTS, SSM_CFG, TT, rm, tokens
from test_gpu_linear_w4 import dequantise, host_quant

pytestmark = pytest.mark.gpu


def model(name, mode, dtype="mxfp4", cfg=None, **kw):
    c, flags = CFGS[name]
    kw = dict(dict(max_requests=4, max_tokens=64 + 4 * TT, max_seq_len=96, max_tree_tokens=TT,
                   weight_seed=11), **kw)
    return fa.Model(cfg or c, mode, weight_dtype=dtype, **flags, **kw)


@pytest.mark.parametrize("name", list(CFGS))
def test_w4_model_weight_bytes(name):
    """both forms pad out_dim to 16 and nothing else at these sizes, so the ratio
    is (1024 + 64) / 4096 = 0.2656 of the fp16 bytes exactly"""
    L, (c, _) = F.lib(), CFGS[name]
    H, Fi, V, d = c["hidden"], c["intermediate"], c["vocab_size"], c["hidden"] // c["num_heads"]
    nqkv = H + 2 * c["num_kv_heads"] * d
    shapes = [(nqkv, H), (H, H), (Fi, H), (Fi, H), (H, Fi)]
    want = sum(L.ffmi_linear_w4_packed_bytes(n, k) + L.ffmi_linear_w4_scale_bytes(n, k)
               for n, k in shapes * c["num_layers"] + [(V, H)])
    m4, m16 = model(name, "inc"), model(name, "inc", "fp16")
    assert m4.weight_bytes() == want and want < 0.30 * m16.weight_bytes()
    m4.close(), m16.close()


@pytest.mark.parametrize("name", list(CFGS))
def test_w4_prefill_logits_are_the_oracle_on_the_quantised_weights(name):
    c, _ = CFGS[name]
    om = O.Model(c, 11, fp16=1, max_requests=1, max_seq=128)
    state = oracle_state(om, c)
    prompt = [1] + np.random.default_rng(40).integers(3, c["vocab_size"], size=39).tolist()
    plain = om.forward(0, prompt, 0)
    qstate = dict(state)
    for n, w in state.items():
        if n.endswith("proj.weight") or n == "lm_head.weight":
            qstate[n] = dequantise(*host_quant(w.astype(np.float16))).astype(w.dtype)
    ref = MO.forward(qstate, c, prompt)
    m = model(name, "inc", max_requests=1, max_tokens=64, max_seq_len=128)
    lg = prefill_logits(m, prompt)
    m.close()
    ok, exact = close_ulp(lg, ref)
    near, far = float(np.abs(lg - ref).mean()), float(np.abs(lg - plain).mean())
    print(f"w4 {name}: within 2 ulp / 2e-3 {ok:.5f}, exact {exact:.4f}; mean |logit - ref| {near:.3e} "
          f"against the quantised-weight oracle, {far:.3e} against the fp16-weight oracle")
    assert ok >= 0.999, ok
    assert near < far


@pytest.mark.parametrize("name", list(CFGS))
def test_w4_graph_replay_gives_the_eager_tokens(name, monkeypatch):
    t4 = tokens(model(name, "inc"), rm())
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert tokens(model(name, "inc"), rm()) == t4


@pytest.mark.parametrize("name", list(CFGS))
def test_w4_spec_infer_equals_incremental_decoding_on_the_token_chain(name):
    inc = tokens(model(name, "inc", weight_init="token_chain"), rm())
    r = rm(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=TT)
    ssm = model("mha", "beam", cfg=SSM_CFG, weight_seed=5, weight_init="token_chain")
    r.register_ssm_model(ssm)
    spec = tokens(model(name, "tree", weight_init="token_chain"), r, spec=True)
    ssm.close()
    assert spec == inc


def test_w4_with_the_fp8_kv_cache_generates():
    out = tokens(model("gqa", "inc", kv_cache_dtype="fp8"), rm())
    assert [len(x) for x in out] == [LEN] * len(PROMPTS)


def test_w4_model_refusals():
    for kw in (dict(full_precision=True), dict(tp_size=2), dict(lora=True)):
        with pytest.raises(F.FFMIError, match="unsupported.*w4"):
            model("mha", "inc", **kw)
    with pytest.raises(F.FFMIError, match="unsupported.*w4"):  # intermediate: no multiple of 128
        model("mha", "inc", cfg=dict(CFGS["mha"][0], intermediate=320))
    with pytest.raises(ValueError, match="weight_dtype"):
        model("mha", "inc", "int4")
