"""Per-token log-probabilities through the model and the serving API
(Model(logprobs=True), Model.set_logprobs; ffmi_model_set_logprobs): every
value is the rule (tests/logprob_rule.py) on the GPU's own logits within the
derived bar, for prompt and generated tokens, greedy, sampled and under
SpecInfer; with it off a step is unchanged.  The 2-layer, V = 1000 model of
tests/test_gpu_e2e.py.
"""
import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import logprob_rule as R
import oracle_lib as O
import peer_logprob_tasks as PT
from peer_group import run_group
from test_gpu_e2e import LLM_CFG, SSM_CFG, prompts

pytestmark = pytest.mark.gpu

V = LLM_CFG["vocab_size"]
KW = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=11)
RM_KW = dict(max_requests_per_batch=4, max_tokens_per_batch=64, max_sequence_length=128)
TREE_KW = dict(KW, max_tokens=64 + 23 * 4, max_tree_tokens=23)


def check_lengths(r):
    assert r.logprobs is not None and len(r.logprobs) == len(r.output_tokens)
    assert r.logprobs[0] is None
    assert all(v <= 0 for v in r.logprobs[1:])


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "do_sample"])
def test_inc_logprobs_are_the_rule_on_the_models_logits(sample):
    """One request under set_debug.  max_new_tokens = 1: the only step is the
    prefill, whose captured logits give every prompt value (row i scores token
    i + 1) and the first generated one (the last row scores its pick).  Then
    max_new_tokens 2..6 (run m generates max(1, m - 1) tokens, as
    tests/test_gpu_sampling_model.py explains): the last value is the rule on
    the last captured row, and each run's values extend the shorter run's bit
    for bit.  Under do_sample z is the row at the temperature and the sampled
    token is scored."""
    gc = fa.GenerationConfig(do_sample=True, temperature=0.9, topp=0.8) if sample else None
    temperature = 0.9 if sample else 0.0
    llm = fa.Model(LLM_CFG, "inc", generation_config=gc, sampling_seed=77, logprobs=True, **KW)
    llm.set_debug(True)
    p = prompts(1, V, 9, 10, 3)
    prev = None
    for m in range(1, 7):
        r = fa.generate(fa.RequestManager(**RM_KW), llm, p, max_new_tokens=m)[0]
        seq, lps = r.output_tokens, r.logprobs
        assert len(seq) == len(p[0]) + max(m, 2)
        check_lengths(r)
        logits = llm.debug_tensor("logits").astype(np.float16)
        if m == 1:
            assert logits.shape[0] == len(seq) - 1  # the prefill: BOS + prompt
            ref = R.logprobs(logits, temperature, seq[1:])
            print("prefill max |lp - ref|", np.abs(np.array(lps[1:]) - ref).max())
            R.assert_within_bar(lps[1:], ref, "prefill")
        ref = R.logprobs(logits[-1:], temperature, seq[-1:])
        R.assert_within_bar(lps[-1:], ref, m)
        if not sample:  # the greedy pick is the likeliest token
            assert seq[-1] == int(O.softmax_argmax(logits[-1:].astype(np.float32), fp16=1)[0][0])
        if prev is not None:
            assert seq[:len(prev[0])] == prev[0] and lps[:len(prev[1])] == prev[1], m
        prev = (seq, lps)


@pytest.mark.parametrize("ssm_kind,max_length", [("small", 40), ("same", 47)])
def test_spec_infer_logprobs_are_the_rule_on_the_verify_logits(ssm_kind, max_length):
    """The tree LLM and beam SSM of tests/test_gpu_e2e.py, one request,
    set_debug on the LLM: the captured logits are the last verify step's
    ([root, tree nodes]).  The tokens that step committed start with the
    root row's pick; each of them must be the pick (lowest index of the largest
    fp16 p) of a row of its own, and its value the rule on that row.  (Which
    row belongs to which token is pinned exactly by tests/test_logprobs_cpu.py.)
    "same": the SSM has the LLM's weights, so whole branches are accepted --
    BOS + 9 prompt tokens, one token from the prefill, then 9 per verify step:
    at max_length 47 the last step commits a full branch, not its root alone."""
    tree = fa.Model(LLM_CFG, "tree", logprobs=True, **TREE_KW)
    tree.set_debug(True)
    ssm = (fa.Model(SSM_CFG, "beam", **dict(TREE_KW, weight_seed=5)) if ssm_kind == "small"
           else fa.Model(LLM_CFG, "beam", **TREE_KW))
    rm = fa.RequestManager(spec_tree_width=(1, 1, 3), max_spec_tree_token_num=23, **RM_KW)
    rm.register_ssm_model(ssm)
    p = prompts(1, V, 9, 10, 3)
    r = fa.generate(rm, tree, p, max_length=max_length, spec=True)[0]
    seq, lps = r.output_tokens, r.logprobs
    assert len(seq) == max_length
    check_lengths(r)
    logits = tree.debug_tensor("logits").astype(np.float16)
    picks = O.softmax_argmax(logits.astype(np.float32), fp16=1)[0]
    n_in = len(p[0]) + 1

    def rows_of(s):
        """distinct rows for the tokens seq[s:], the first on row 0, or None"""
        used, out = set(), []
        for j in range(s, len(seq)):
            cand = [0] if j == s else [q for q in range(len(picks)) if q not in used]
            hit = None
            for q in cand:
                if int(picks[q]) != seq[j]:
                    continue
                ref = R.logprobs(logits[q:q + 1], 0.0, [seq[j]])
                if abs(lps[j] - ref[0]) <= R.bar(ref)[0]:
                    hit = q
                    break
            if hit is None:
                return None
            used.add(hit)
            out.append(hit)
        return out

    # a verify step commits 1 .. MAX_BEAM_DEPTH + 1 tokens, all generated ones
    starts = [s for s in range(max(n_in + 1, len(seq) - 9), len(seq)) if rows_of(s) is not None]
    print("last verify step: rows", len(picks), "feasible first committed positions", starts)
    assert starts, (seq, lps, picks.tolist())
    if ssm_kind == "same":
        assert len(seq) - min(starts) >= 2, starts


def test_off_path_is_the_parents_step():
    """Four batched requests, graphs on: the same tokens with logprobs on and
    off, on a fresh model and after toggling.  Profiled (every op timed, eager
    steps), an off run launches no token_logprobs op and an on run one per
    pick."""
    ps = prompts(4, V, 5, 30, 9)

    def run(llm):
        return fa.generate(fa.RequestManager(**RM_KW), llm, ps, max_new_tokens=17)

    off = run(fa.Model(LLM_CFG, "inc", **KW))
    llm = fa.Model(LLM_CFG, "inc", logprobs=True, **KW)
    on = run(llm)
    assert [r.output_tokens for r in on] == [r.output_tokens for r in off]
    assert all(r.logprobs is None for r in off)
    for r in on:
        check_lengths(r)
    llm.set_logprobs(False)
    llm.set_profiling(2)
    again = run(llm)
    assert [r.output_tokens for r in again] == [r.output_tokens for r in off]
    assert all(r.logprobs is None for r in again)
    st = llm.op_stats()
    assert st["softmax_argmax"]["launches"] > 0 and "token_logprobs" not in st, st.keys()
    llm.set_logprobs(True)
    llm.set_profiling(2)
    prof = run(llm)
    st = llm.op_stats()
    assert st["token_logprobs"]["launches"] == st["softmax_argmax"]["launches"] > 0
    llm.set_profiling(0)
    assert [r.output_tokens for r in prof] == [r.output_tokens for r in off]
    for r in prof:
        check_lengths(r)


@pytest.mark.parametrize("kind", ["beam", "full_precision"])
def test_set_logprobs_refusals(kind):
    llm = (fa.Model(LLM_CFG, "inc", full_precision=True, **TREE_KW) if kind == "full_precision"
           else fa.Model(LLM_CFG, kind, **TREE_KW))
    st = F.lib().ffmi_model_set_logprobs(llm.handle, 1)
    assert st == 5, st  # FFMI_ERR_UNSUPPORTED
    assert b"logprobs" in F.lib().ffmi_last_error()
    with pytest.raises(F.FFMIError):
        llm.set_logprobs(True)
    with pytest.raises(F.FFMIError):
        fa.Model(LLM_CFG, "inc" if kind == "full_precision" else kind,
                 full_precision=kind == "full_precision", logprobs=True, **TREE_KW)


def test_vocab_sharded_model_refuses_logprobs():
    """TP 2 with V / 2 a multiple of 16: lm_head is vocab-sharded, and the
    rows' (M, S) would have to be combined across ranks."""
    cfg = dict(LLM_CFG, vocab_size=1024, num_heads=4, num_kv_heads=4)
    res = run_group(2, PT.vshard_refusal_task, (cfg,), max_bytes=1 << 20)
    for r in res:
        assert r["status"] == 5 and "logprobs" in r["message"] and r["raised"], r
        assert r["logprobs"] is None and r["tokens"] == res[0]["tokens"]
