"""Top-p sampling through a tensor-parallel model with a vocab-sharded lm_head
(ffmi_model_set_sampling -> ffmi_vocab_shard_sample_topp): the sampled token is
the numpy rule (tests/sampling_rule.py) on the ranks' gathered logits with u
from ffmi_sampling_counter(seed, guid, position), every rank emits the same
tokens, runs are reproducible from the seed, and the greedy tail comes back.
CFG4V (V = 1024, 2 layers) at TP 2 and 4 over rank processes of the xGMI
transport, and TP 4 over the in-process shard group.
"""
import threading

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import peer_sampling_tasks as ST
import sampling_rule as R
from peer_group import run_group
from test_gpu_e2e import prompts

pytestmark = pytest.mark.gpu

# V / TP a multiple of 16 at TP 2 and 4: lm_head vocab-sharded
CFG4V = dict(num_layers=2, vocab_size=1024, num_heads=4, num_kv_heads=4, hidden=256,
             intermediate=512, rms_eps=1e-6, rope_theta=10000.0)
V = CFG4V["vocab_size"]


def uniform(seed, guid, pos):
    return np.float32((F.sampling_counter(seed, guid, pos) + 1) * 2.0 ** -24)


def same_on_every_rank(res):
    for r in range(1, len(res)):
        assert res[r] == res[0], f"rank {r}"
    return res[0]


@pytest.mark.parametrize("tp", [2, 4])
def test_sampled_token_is_the_rule_on_the_gathered_logits(tp):
    """One request, max_new_tokens 1..5 under set_debug (run m generates
    max(1, m - 1) tokens, as tests/test_gpu_sampling_model.py explains): the
    last token of each run is the rule on the last row of the logits, the
    ranks' shards concatenated in rank order."""
    gc, seed = dict(do_sample=True, temperature=0.9, topp=0.8), 77
    p = prompts(1, V, 9, 10, 3)[0]
    res = run_group(tp, ST.model_rule_task, (CFG4V, gc, seed, p, list(range(1, 6))),
                    max_bytes=1 << 20)
    prev = None
    for mi, m in enumerate(range(1, 6)):
        runs = [res[r][mi] for r in range(tp)]
        seq, guid = runs[0]["tokens"], runs[0]["guid"]
        for r in range(1, tp):
            assert (runs[r]["tokens"], runs[r]["guid"]) == (seq, guid), (m, r)
        assert len(seq) == len(p) + 1 + max(m, 2) - 1
        assert all(x["logits"].shape == (1, V // tp) for x in runs)
        logits = np.concatenate([x["logits"] for x in runs], axis=1)
        tok, _ = R.sample(logits, gc["temperature"], gc["topp"], [uniform(seed, guid, len(seq) - 1)])
        assert seq[-1] == int(tok[0]), (m, seq, tok)
        if prev is not None:
            assert seq[:len(prev)] == prev
        prev = seq


@pytest.mark.parametrize("tp", [2, 4])
def test_sampling_is_reproducible_from_the_seed(tp):
    """3 requests x 12 tokens, graphs on: the same seed gives the same tokens
    (again on this model after another seed, and on a fresh group), another
    seed other ones."""
    ps = prompts(3, V, 5, 30, 9)
    a5, a6, a5b = same_on_every_rank(run_group(tp, ST.model_seed_task, (CFG4V, ps, 13, [5, 6, 5]),
                                               max_bytes=1 << 20))
    (b5,) = same_on_every_rank(run_group(tp, ST.model_seed_task, (CFG4V, ps, 13, [5]),
                                         max_bytes=1 << 20))
    assert a5 == a5b == b5
    assert a6 != a5
    assert all(len(s) == len(p) + 13 for s, p in zip(a5, ps))


@pytest.mark.parametrize("tp", [2, 4])
def test_small_topp_is_the_tp_models_greedy_decoding(tp):
    """ffmi_model_set_sampling on the vocab-sharded model is FFMI_OK;
    temperature 1, topp 2^-6 (t <= 2^-12 <= the largest p of every row:
    asserted on the gathered logits) reproduces the TP model's own greedy
    tokens; set_sampling(None) restores the greedy tail."""
    ps = prompts(3, V, 5, 30, 13)
    res = run_group(tp, ST.model_greedy_task, (CFG4V, ps, 12), max_bytes=1 << 20)
    for r in range(tp):
        assert res[r]["status"] == F.FFMI_OK, (r, res[r]["status"])
        for k in ("greedy", "small", "sampled", "greedy_again"):
            assert res[r][k] == res[0][k], (k, r)
    g = res[0]["greedy"]
    assert res[0]["small"] == g and res[0]["greedy_again"] == g and res[0]["sampled"] != g
    for si, m in enumerate(range(2, 13)):
        toks = res[0]["steps"][si][0]
        assert toks == g[0][:len(ps[0]) + m] and all(res[r]["steps"][si][0] == toks for r in range(tp))
        row = np.concatenate([res[r]["steps"][si][1] for r in range(tp)], axis=1)
        _, p = R.sorted_probs(R.scaled_logits(row, 1.0))
        assert p[0, 0] >= 2.0 ** -12, (m, p[0, 0])


def test_tp4_local_group_samples_the_rule():
    """TP = 4 as host threads over the in-process shard group (the shape of
    tests/test_gpu_tp_local.py run_tp): identical tokens on every rank, the
    last one the rule on the gathered logits, not the greedy tokens."""
    tp, seed = 4, 21
    gc = fa.GenerationConfig(do_sample=True, temperature=0.9, topp=0.8)
    p = prompts(1, V, 9, 10, 3)
    comms = fa.Comm.local_group(tp)
    models = [fa.Model(CFG4V, "inc", tp_rank=r, tp_size=tp, comm=comms[r], **ST.KW)
              for r in range(tp)]
    for m in models:
        assert F.lib().ffmi_model_set_sampling(m.handle, 1, gc.temperature, gc.topp, seed) == F.FFMI_OK
        m.set_debug(True)

    def generate():
        rms = [fa.RequestManager(**ST.RM_KW) for _ in range(tp)]
        out, err = [None] * tp, []

        def work(r):
            try:
                fa.set_device(0)
                out[r] = fa.generate(rms[r], models[r], p, max_new_tokens=6)[0]
            except Exception as e:  # noqa: BLE001 -- reported below
                err.append((r, e))

        th = [threading.Thread(target=work, args=(r,)) for r in range(tp)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not err, err
        assert all(o is not None for o in out)
        return out

    out = generate()
    seq = out[0].output_tokens
    assert all(o.output_tokens == seq and o.guid == out[0].guid for o in out)
    logits = np.concatenate([m.debug_tensor("logits")[-1:].astype(np.float16) for m in models], axis=1)
    tok, _ = R.sample(logits, gc.temperature, gc.topp, [uniform(seed, out[0].guid, len(seq) - 1)])
    assert seq[-1] == int(tok[0]), (seq, tok)
    for m in models:
        m.set_sampling(None)
    assert generate()[0].output_tokens != seq
    for m in models:
        m.close()
    for c in comms:
        c.close()
