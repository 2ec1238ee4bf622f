"""Top-p sampling through the model and the serving API
(Model(generation_config=...), Model.set_sampling; ffmi_model_set_sampling):
the sampled token is the numpy rule (tests/sampling_rule.py) on the GPU's own
logits with u from ffmi_sampling_counter(seed, guid, position), runs are
reproducible from the seed, and the greedy tail comes back.  The 2-layer,
V = 1000 model of tests/test_gpu_e2e.py.
"""
import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import sampling_rule as R
from test_gpu_e2e import LLM_CFG, prompts

pytestmark = pytest.mark.gpu

SEED_W = 11
KW = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=SEED_W)
RM_KW = dict(max_requests_per_batch=4, max_tokens_per_batch=64, max_sequence_length=128)


def uniform(seed, guid, pos):
    return np.float32((F.sampling_counter(seed, guid, pos) + 1) * 2.0 ** -24)


def run(llm, ps, new_tokens):
    return fa.generate(fa.RequestManager(**RM_KW), llm, ps, max_new_tokens=new_tokens)


def test_sampled_token_is_the_rule_on_the_models_logits():
    """One request, max_new_tokens 1..7 under set_debug.  The request manager
    counts max_new_tokens from the prompt without its BOS, as the reference
    (request_manager.cc:334-441), and the prefill step always yields a token:
    run m generates max(1, m - 1) tokens, 1..6 in all.  The last token of each
    run is the rule applied to the last row of the captured logits, and each
    run extends the shorter one (the draw depends on seed, guid and position
    only)."""
    gc, seed = fa.GenerationConfig(do_sample=True, temperature=0.9, topp=0.8), 77
    llm = fa.Model(LLM_CFG, "inc", generation_config=gc, sampling_seed=seed, **KW)
    llm.set_debug(True)
    p = prompts(1, LLM_CFG["vocab_size"], 9, 10, 3)
    prev = None
    for m in range(1, 8):
        rm = fa.RequestManager(**RM_KW)
        # (every manager numbers its requests alike: the same guid in each run)
        r = fa.generate(rm, llm, p, max_new_tokens=m)[0]
        seq = r.output_tokens
        assert len(seq) == len(p[0]) + max(m, 2)  # BOS + prompt + the sampled tokens
        logits = llm.debug_tensor("logits")[-1:].astype(np.float16)
        tok, _ = R.sample(logits, gc.temperature, gc.topp, [uniform(seed, r.guid, len(seq) - 1)])
        assert seq[-1] == int(tok[0]), (m, seq, tok)
        if prev is not None:
            assert (prev[0], seq[:len(prev[1])]) == (r.guid, prev[1])
        prev = (r.guid, seq)


def test_sampling_is_reproducible_from_the_seed():
    """Four requests batched, 16 new tokens each (max_new_tokens 17: it counts
    from the prompt without its BOS), graphs as the model defaults: the
    same seed gives the same tokens (a second model, and the first again after
    another seed), another seed other ones."""
    gc = fa.GenerationConfig(do_sample=True)
    ps = prompts(4, LLM_CFG["vocab_size"], 5, 30, 9)
    a = [r.output_tokens for r in run(fa.Model(LLM_CFG, "inc", generation_config=gc,
                                               sampling_seed=5, **KW), ps, 17)]
    llm = fa.Model(LLM_CFG, "inc", generation_config=gc, sampling_seed=5, **KW)
    b = [r.output_tokens for r in run(llm, ps, 17)]
    assert a == b
    assert all(len(s) == len(p) + 17 for s, p in zip(a, ps))
    llm.set_sampling(gc, seed=6)
    c = [r.output_tokens for r in run(llm, ps, 17)]
    assert c != a
    llm.set_sampling(gc, seed=5)
    assert [r.output_tokens for r in run(llm, ps, 17)] == a
    # the greedy tokens differ from the sampled ones somewhere
    llm.set_sampling(None)
    assert [r.output_tokens for r in run(llm, ps, 17)] != a


def test_small_topp_and_do_sample_off_are_greedy():
    """temperature 1, topp 2^-6 (t <= 2^-12 <= the largest p of every row:
    asserted on the captured logits) samples the argmax, so the tokens are
    greedy decoding's; do_sample = 0 after sampling restores the greedy tail."""
    ps = prompts(3, LLM_CFG["vocab_size"], 5, 30, 13)
    llm = fa.Model(LLM_CFG, "inc", **KW)
    greedy = [r.output_tokens for r in run(llm, ps, 12)]
    llm.set_sampling(fa.GenerationConfig(do_sample=True, temperature=1.0, topp=2.0 ** -6), seed=3)
    assert [r.output_tokens for r in run(llm, ps, 12)] == greedy
    llm.set_sampling(fa.GenerationConfig(do_sample=True), seed=3)
    assert [r.output_tokens for r in run(llm, ps, 12)] != greedy
    llm.set_sampling(fa.GenerationConfig(do_sample=False))
    assert [r.output_tokens for r in run(llm, ps, 12)] == greedy
    # the precondition, on the logits of every step of one request
    llm.set_sampling(fa.GenerationConfig(do_sample=True, temperature=1.0, topp=2.0 ** -6), seed=3)
    llm.set_debug(True)
    for m in range(2, 13):
        r = run(llm, ps[:1], m)[0]
        assert r.output_tokens == greedy[0][:len(ps[0]) + m]
        row = llm.debug_tensor("logits")[-1:].astype(np.float16)
        _, p = R.sorted_probs(R.scaled_logits(row, 1.0))
        assert p[0, 0] >= 2.0 ** -12, (m, p[0, 0])


@pytest.mark.parametrize("kind", ["beam", "tree", "full_precision"])
def test_set_sampling_refusals(kind):
    kw = dict(KW, max_tokens=64 + 23 * 4)
    llm = (fa.Model(LLM_CFG, "inc", full_precision=True, **kw) if kind == "full_precision"
           else fa.Model(LLM_CFG, kind, **kw))
    st = F.lib().ffmi_model_set_sampling(llm.handle, 1, 0.9, 0.8, 1)
    assert st == 5, st  # FFMI_ERR_UNSUPPORTED
    assert b"sampling" in F.lib().ffmi_last_error()
    with pytest.raises(F.FFMIError):
        llm.set_sampling(fa.GenerationConfig(do_sample=True))
    with pytest.raises(F.FFMIError):
        fa.Model(LLM_CFG, "inc" if kind == "full_precision" else kind,
                 full_precision=kind == "full_precision",
                 generation_config=fa.GenerationConfig(do_sample=True), **kw)
