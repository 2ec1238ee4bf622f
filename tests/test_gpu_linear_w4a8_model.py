"""FFMI_MODEL_W4 | FFMI_MODEL_A8 (Model(weight_dtype="mxfp4", activation_dtype="fp8"))
on the 2-layer models of tests/test_gpu_linear_w4_model.py, greedy: SpecInfer and
graph replay against the model's own incremental decoding, the flag's effect on
the logits, the two GEMM forms on one prompt, the 8-bit KV cache.  pytest -m gpu."""
import numpy as np
import pytest

import flexflow_amd as fa
from test_gpu_gqa_oracle import prefill_logits
from test_gpu_kv_fp8_model import CFGS, LEN, PROMPTS, SSM_CFG, TT, rm, tokens
from test_gpu_linear_w4_model import model

pytestmark = pytest.mark.gpu
A8 = dict(activation_dtype="fp8", weight_init="token_chain")


@pytest.mark.parametrize("name", list(CFGS))
def test_w4a8_spec_infer_and_graphs_on_the_token_chain(name, monkeypatch):
    inc = tokens(model(name, "inc", **A8), rm())
    r = rm(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=TT)
    ssm = model("mha", "beam", cfg=SSM_CFG, weight_seed=5, **A8)
    r.register_ssm_model(ssm)
    spec = tokens(model(name, "tree", **A8), r, spec=True)
    ssm.close()
    assert spec == inc
    w4 = tokens(model(name, "inc", weight_init="token_chain"), rm())
    same = sum(a == b for x, y in zip(w4, inc) for a, b in zip(x, y))
    print(f"w4a8 {name} token chain: {same} of {sum(map(len, inc))} tokens equal the W4A16 model's")
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert tokens(model(name, "inc", **A8), rm()) == inc


@pytest.mark.parametrize("name", list(CFGS))
def test_w4a8_prefill_logits_differ_from_w4a16s_and_fp8_kv_generates(name):
    prompt = [1] + np.random.default_rng(40).integers(3, 1000, size=39).tolist()
    kw = dict(max_requests=1, max_tokens=64, max_seq_len=128)
    m4, ma = model(name, "inc", **kw), model(name, "inc", activation_dtype="fp8", **kw)
    l4, la = prefill_logits(m4, prompt), prefill_logits(ma, prompt)
    m4.close(), ma.close()
    dist = float(np.abs(la.astype(np.float64) - l4).mean())
    print(f"w4a8 {name}: mean |logit(W4A8) - logit(W4A16)| {dist:.3e}, mean |logit| "
          f"{float(np.abs(l4).mean()):.3e}")
    assert dist > 0
    out = tokens(model(name, "inc", activation_dtype="fp8", kv_cache_dtype="fp8"), rm())
    assert [len(x) for x in out] == [LEN] * len(PROMPTS)


@pytest.mark.parametrize("name", list(CFGS))
def test_w4a8_100_row_prefill_continues_as_the_prompt_fed_16_rows_at_a_time(name):
    prompt = np.random.default_rng(41).integers(3, 1000, size=99).tolist()
    out = []
    for step in (128, 16):  # rows per step: the whole prompt (MTW = 2), blocks (tile split)
        m = model(name, "inc", activation_dtype="fp8", max_requests=1, max_tokens=128, max_seq_len=128)
        r = fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=step, max_sequence_length=128)
        out.append(fa.generate(r, m, [prompt], max_length=112)[0].output_tokens)
        m.close()
    assert len(out[0]) == 112 and out[0] == out[1]
