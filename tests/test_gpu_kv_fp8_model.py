"""FFMI_MODEL_KV_FP8 (Model(kv_cache_dtype="fp8")): a 2-layer, hidden-256 model
with an 8-bit KV cache, as MHA and as GQA under native_gqa.

Asserted: half the fp16 model's cache bytes; graph replay gives the eager
tokens; on the token-chain init SpecInfer equals the fp8 model's own
incremental decoding.  Printed, not asserted: agreement with the fp16 model's
tokens (DESIGN section 8 item 16 has the figures).
"""
import numpy as np
import pytest

import flexflow_amd as fa

pytestmark = pytest.mark.gpu

CFGS = {"mha": (dict(num_layers=2, vocab_size=1000, num_heads=2, num_kv_heads=2, hidden=256,
                     intermediate=512, rms_eps=1e-6, rope_theta=10000.0), {}),
        "gqa": (dict(num_layers=2, vocab_size=1000, num_heads=4, num_kv_heads=2, hidden=256,
                     intermediate=512, rms_eps=1e-6, rope_theta=10000.0), dict(native_gqa=True))}
SSM_CFG = dict(CFGS["mha"][0], num_layers=1, hidden=128, intermediate=256)
LEN, TT = 40, 23
PROMPTS = [np.random.default_rng(5).integers(3, 1000, size=n).tolist() for n in (6, 3, 19, 35)]


def rm(**kw):
    return fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                             max_sequence_length=96, **kw)


def model(name, mode, dtype, **kw):
    cfg, flags = CFGS[name]
    return fa.Model(cfg, mode, max_requests=4, max_tokens=64 + 4 * TT, max_seq_len=96,
                    max_tree_tokens=TT, weight_seed=11, kv_cache_dtype=dtype, **flags, **kw)


def tokens(m, r, **kw):
    out = [x.output_tokens for x in fa.generate(r, m, PROMPTS, max_length=LEN, **kw)]
    m.close()
    return out


@pytest.mark.parametrize("name", list(CFGS))
def test_kv_fp8_model_cache_bytes_graphs_and_fp16_agreement(name, monkeypatch):
    m16, m8 = model(name, "inc", "fp16"), model(name, "inc", "fp8", kv_scales=(0.5, 2.0))
    assert 2 * m8.kv_cache_bytes() == m16.kv_cache_bytes() > 0
    with pytest.raises(fa.ffmi.FFMIError, match="kv_fp8"):  # only a flagged model has scales
        fa.ffmi.check(fa.ffmi.lib().ffmi_model_set_kv_scales(m16.handle, 1.0, 1.0))
    t16, t8 = tokens(m16, rm()), tokens(m8, rm())
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert tokens(model(name, "inc", "fp8", kv_scales=(0.5, 2.0)), rm()) == t8
    same = sum(a == b for x, y in zip(t16, t8) for a, b in zip(x, y))
    print(f"kv_fp8 {name} uniform init: {same} of {sum(map(len, t8))} tokens equal the fp16 model's")


@pytest.mark.parametrize("name", list(CFGS))
def test_kv_fp8_spec_infer_equals_incremental_decoding_on_the_token_chain(name):
    inc = tokens(model(name, "inc", "fp8", weight_init="token_chain"), rm())
    r = rm(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=TT)
    ssm = fa.Model(SSM_CFG, "beam", max_requests=4, max_tokens=64 + 4 * TT, max_seq_len=96,
                   max_tree_tokens=TT, weight_seed=5, weight_init="token_chain",
                   kv_cache_dtype="fp8")
    r.register_ssm_model(ssm)
    spec = tokens(model(name, "tree", "fp8", weight_init="token_chain"), r, spec=True)
    ssm.close()
    assert spec == inc
    t16 = tokens(model(name, "inc", "fp16", weight_init="token_chain"), rm())
    same = sum(a == b for x, y in zip(t16, inc) for a, b in zip(x, y))
    print(f"kv_fp8 {name} token chain: {same} of {sum(map(len, inc))} tokens equal the fp16 model's")


def test_kv_fp8_model_refuses_full_precision_and_late_scales():
    with pytest.raises(fa.ffmi.FFMIError, match="unsupported.*kv_fp8"):
        model("mha", "inc", "fp8", full_precision=True)
    with pytest.raises(ValueError, match="kv_scales"):  # scales without the dtype
        model("mha", "inc", "fp16", kv_scales=(0.5, 2.0))
    m = model("mha", "inc", "fp8")
    fa.generate(rm(), m, PROMPTS[:1], max_length=8)
    with pytest.raises(fa.ffmi.FFMIError, match="invalid.*kv_fp8"):
        fa.ffmi.check(fa.ffmi.lib().ffmi_model_set_kv_scales(m.handle, 1.0, 1.0))
    m.close()
