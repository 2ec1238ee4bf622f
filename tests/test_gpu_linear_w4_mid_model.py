"""FFMI_MODEL_W4 above 64 rows per step: a 100-token prompt prefilled in one
step runs every linear layer through the M-split MXFP4-weight GEMM
(kernels/gemm_w4_mid.hip; down_proj with S = 2 slabs).  The models, the oracle
and the bar of tests/test_gpu_linear_w4_model.py.  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import flexflow_amd as fa
import lora_merge_oracle as MO
import oracle_lib as O
from test_gpu_alignment import close_ulp
from test_gpu_gqa_oracle import oracle_state
from test_gpu_kv_fp8_model import CFGS
from test_gpu_linear_w4 import dequantise, host_quant
from test_gpu_linear_w4_model import model

pytestmark = pytest.mark.gpu
PROMPT = [1] + np.random.default_rng(41).integers(3, 1000, size=99).tolist()


def generate(name, n_new, debug=False):
    """(output tokens, the prefill step's logits if debug) of PROMPT in one 100-row step"""
    m = model(name, "inc", max_requests=1, max_tokens=128, max_seq_len=128)
    m.set_debug(debug)
    out = fa.generate(fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=128,
                                        max_sequence_length=128),
                      m, [PROMPT[1:]], max_length=len(PROMPT) + n_new)[0].output_tokens
    lg = m.debug_tensor("logits") if debug else None
    m.close()
    return out, lg


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_w4_100_row_prefill_logits_are_the_oracle_on_the_quantised_weights(name):
    c, _ = CFGS[name]
    qstate = oracle_state(O.Model(c, 11, fp16=1, max_requests=1, max_seq=128), c)
    for n, w in qstate.items():
        if n.endswith("proj.weight") or n == "lm_head.weight":
            qstate[n] = dequantise(*host_quant(w.astype(np.float16))).astype(w.dtype)
    lg = generate(name, 1, debug=True)[1]
    assert lg.shape[0] == len(PROMPT)
    ok, exact = close_ulp(lg, MO.forward(qstate, c, PROMPT))
    print(f"w4 {name}, 100 rows: within 2 ulp / 2e-3 {ok:.5f}, exact {exact:.4f}")
    assert ok >= 0.999, ok


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_w4_100_row_prefill_graph_replay_gives_the_eager_tokens(name, monkeypatch):
    t4, _ = generate(name, 12)
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert generate(name, 12)[0] == t4
