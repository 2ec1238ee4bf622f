"""FFMI_MODEL_A8 (Model(weight_dtype="fp8", activation_dtype="fp8")) on the
2-layer, hidden-256 models of tests/test_gpu_linear_w8_model.py, MHA and GQA
under native_gqa, token-chain init, greedy: SpecInfer equals the flagged model's
own incremental decoding, graph replay gives the eager tokens, the tokens are
the W8 model's, and the prefill logits are not (the flag takes effect).
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

from test_gpu_gqa_oracle import prefill_logits
from test_gpu_kv_fp8_model import CFGS, SSM_CFG, TT, rm, tokens
from test_gpu_linear_w8_model import model

pytestmark = pytest.mark.gpu
A8 = dict(activation_dtype="fp8", weight_init="token_chain")


@pytest.mark.parametrize("name", list(CFGS))
def test_a8_spec_infer_graphs_and_the_w8_models_tokens(name, monkeypatch):
    inc = tokens(model(name, "inc", **A8), rm())
    r = rm(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=TT)
    ssm = model("mha", "beam", cfg=SSM_CFG, weight_seed=5, **A8)
    r.register_ssm_model(ssm)
    spec = tokens(model(name, "tree", **A8), r, spec=True)
    ssm.close()
    assert spec == inc
    w8 = tokens(model(name, "inc", weight_init="token_chain"), rm())
    same = sum(a == b for x, y in zip(w8, inc) for a, b in zip(x, y))
    print(f"a8 {name} token chain: {same} of {sum(map(len, inc))} tokens equal the W8 model's")
    assert inc == w8
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert tokens(model(name, "inc", **A8), rm()) == inc


@pytest.mark.parametrize("name", list(CFGS))
def test_a8_prefill_logits_differ_from_w8s_and_fp8_kv_generates(name):
    prompt = [1] + np.random.default_rng(40).integers(3, 1000, size=39).tolist()
    kw = dict(max_requests=1, max_tokens=64, max_seq_len=128)
    m8, ma = model(name, "inc", **kw), model(name, "inc", activation_dtype="fp8", **kw)
    l8, la = prefill_logits(m8, prompt), prefill_logits(ma, prompt)
    m8.close(), ma.close()
    dist = float(np.abs(la.astype(np.float64) - l8).mean())
    print(f"a8 {name}: mean |logit(W8A8) - logit(W8A16)| {dist:.3e}, mean |logit| "
          f"{float(np.abs(l8).mean()):.3e}")
    assert dist > 0
    out = tokens(model(name, "inc", activation_dtype="fp8", kv_cache_dtype="fp8"), rm())
    assert all(len(x) == 40 for x in out)
