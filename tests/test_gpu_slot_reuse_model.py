"""A recycled request slot through the whole stack, bit for bit.

One request slot (max_requests = 1).  Run A: a fresh model serves request B
(9-token prompt, max_length 21).  Run B: a second fresh model of the same
weights serves [A, B] from one request manager, A with a 45-token prompt and
max_length 77, so B takes over the slot with A's K/V -- and, under SpecInfer,
A's rejected tree rows and staging rows -- still in every layer's cache, far
past everything B writes.  B's tokens and its per-token log-probabilities (the
float observable; compared as bits) must be the same in both runs.  Greedy
decoding: the sampling counter is keyed by guid, and B's guid differs between
the runs.
"""
import numpy as np
import pytest

import flexflow_amd as fa
from hip_util import report
from test_gpu_e2e import LLM_CFG, SSM_CFG

pytestmark = pytest.mark.gpu

GQA_CFG = dict(LLM_CFG, num_heads=4, num_kv_heads=2)  # d = 64, two query heads per K/V head
A_LEN, A_MAX, B_LEN, B_MAX = 45, 77, 9, 21
TREE = 23


def make(variant):
    """(request manager, llm, spec, models to close) of one fresh stack"""
    kw = dict(max_requests_per_batch=1, max_tokens_per_batch=64, max_sequence_length=128)
    if variant == "spec":
        mk = dict(max_requests=1, max_tokens=64 + TREE, max_seq_len=128, max_tree_tokens=TREE)
        llm = fa.Model(LLM_CFG, "tree", weight_seed=11, logprobs=True, **mk)
        ssm = fa.Model(SSM_CFG, "beam", weight_seed=5, **mk)
        rm = fa.RequestManager(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=TREE, **kw)
        rm.register_ssm_model(ssm)
        return rm, llm, True, [llm, ssm]
    mk = dict(max_requests=1, max_tokens=64, max_seq_len=128, weight_seed=11)
    if variant == "inc":
        llm = fa.Model(LLM_CFG, "inc", logprobs=True, **mk)
    elif variant == "native_gqa":
        llm = fa.Model(GQA_CFG, "inc", native_gqa=True, logprobs=True, **mk)
    else:  # (refuses logprobs: tokens only)
        llm = fa.Model(LLM_CFG, "inc", full_precision=True, **mk)
    return fa.RequestManager(**kw), llm, False, [llm]


def serve(variant, requests):
    rm, llm, spec, models = make(variant)
    guids = [rm.register_new_request(p, max_length=n) for p, n in requests]
    assert all(g > 0 for g in guids)
    if spec:
        rm.serve_spec_infer(llm)
    else:
        rm.serve_incr_decoding(llm)
    res = [rm.get_generation_result(g) for g in guids]
    for m in models:
        m.close()
    return res


@pytest.mark.parametrize("variant", ["inc", "spec", "native_gqa", "full_precision"])
def test_second_occupant_of_a_slot_equals_its_solo_run(variant):
    rng = np.random.default_rng(97)
    V = LLM_CFG["vocab_size"]
    a = (rng.integers(3, V, size=A_LEN).tolist(), A_MAX)
    b = (rng.integers(3, V, size=B_LEN).tolist(), B_MAX)
    solo, = serve(variant, [b])
    first, second = serve(variant, [a, b])
    # otherwise nothing stale lies past what B reaches
    assert len(first.output_tokens) > B_MAX, len(first.output_tokens)
    assert len(solo.output_tokens) == B_MAX
    assert second.output_tokens == solo.output_tokens
    if variant == "full_precision":
        assert solo.logprobs is None and second.logprobs is None
        n = 0
    else:
        assert solo.logprobs[0] is None and second.logprobs[0] is None
        x = np.array(solo.logprobs[1:], np.float32)
        y = np.array(second.logprobs[1:], np.float32)
        n = x.size
        assert n == len(solo.output_tokens) - 1 == y.size and np.isfinite(x).all()
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    report("slot_reuse_model", variant=variant, tokens=len(solo.output_tokens), logprobs=n,
           first_occupant_tokens=len(first.output_tokens))
