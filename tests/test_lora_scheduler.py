"""The adapter a request names reaches every LLM row the scheduler builds
(PerRequestInfo::lora_id), on the hash model (no GPU): a row of a request with
adapter a >= 0 folds a into its context hash (runtime/hash_model.cpp), SSM rows
do not -- so a lost, stale or misplaced id changes a token, and SpecInfer must
still equal incremental decoding."""
import ctypes
import random

import numpy as np
import pytest

import flexflow_amd as fa
from flexflow_amd import ffmi as F
from test_scheduler import M64, MULTI, V, W4, WIDTHS, mix64, prompts

FOLD = 0xA0761D6478BD642F


def next_tok(ctx, a):
    h = 0x243F6A8885A308D3
    for t in ctx:
        h = mix64((h + t + 1) & M64)
    if a >= 0:
        h = mix64(h ^ ((FOLD * (a + 1)) & M64))
    return (h >> 17) % V


def expected(prompt, max_length, a):
    toks = [1] + list(prompt)
    while len(toks) < max_length:
        toks.append(next_tok(toks, a))
    return toks


def load(model, n):
    ids = []
    for _ in range(n):
        out = ctypes.c_int(-1)
        F.check(F.lib().ffmi_model_lora_load(model.handle, 8, 16.0, None, None, ctypes.byref(out)),
                "hash lora_load")
        ids.append(out.value)
    return ids


def run(ps, ads, ml, spec, batch=4, max_tokens=64, widths=(1, 1, 3), tree=23, ssms=((1234, 30),),
        ext=0, msl=128):
    """ads: per prompt -1 or an index into the three adapters the LLM loads"""
    rm = fa.RequestManager(max_requests_per_batch=batch, max_tokens_per_batch=max_tokens,
                           max_sequence_length=msl, spec_tree_width=widths if spec else (),
                           max_spec_tree_token_num=tree, spec_extensions=ext)
    llm = fa.HashModel(V, "tree" if spec else "inc", max_requests=batch, max_seq_len=msl,
                       max_tree_tokens=tree)
    ids = load(llm, 3)
    assert sorted(ids) == ids and len(set(ids)) == 3
    if spec:
        for salt, dis in ssms:
            rm.register_ssm_model(fa.HashModel(V, "beam", max_requests=batch, max_seq_len=msl,
                                               max_tree_tokens=tree, salt=salt, disagree_pct=dis))
    res = fa.generate(rm, llm, ps, max_length=ml, lora_ids=[ids[a] if a >= 0 else -1 for a in ads])
    rm.close()
    llm.close()  # (gives the ids back)
    return [q.output_tokens for q in res], ids


@pytest.mark.parametrize("block", range(4))
def test_randomized_mixes_spec_equals_incr_equals_alone(block):
    checked = 0
    for seed in range(block * 12, block * 12 + 12):
        r = random.Random(7000 + seed)
        batch, mt = r.choice([1, 2, 3, 4, 8]), r.choice([8, 16, 32, 64, 128])
        widths, tree = r.choice(WIDTHS), r.choice([16, 23, 32, 64])
        nssm = r.choice([1, 1, 2])
        ssms = [(r.randrange(1, 10000), r.choice([0, 10, 30, 60, 100])) for _ in range(nssm)]
        ps = prompts(r.randint(1, 10), V, lo=2, hi=max(3, min(2 * mt, 60)), seed=seed)
        ads = [r.choice([-1, 0, 1, 2]) for _ in ps]
        ml = min(127, max(r.choice([40, 70, 100]), max(len(p) for p in ps) + 3))
        inc, ids = run(ps, ads, ml, False, batch=batch, max_tokens=min(mt, 64))
        # a request's tokens: those of the same request served alone with its adapter
        for p, a, got in zip(ps, ads, inc):
            assert got == expected(p, ml, ids[a] if a >= 0 else -1), (seed, a)
        try:
            sp, _ = run(ps, ads, ml, True, batch=batch, max_tokens=mt, widths=widths, tree=tree,
                        ssms=ssms, ext=W4 | (MULTI if nssm > 1 else 0))
        except F.FFMIError as e:
            assert "SSM loaded less" in str(e), (seed, str(e))
            continue
        assert sp == inc, seed
        checked += 1
    assert checked >= 8


def test_an_adapter_changes_the_tokens_and_alone_equals_batched():
    ps = prompts(4, V, seed=3)
    base, _ = run(ps, [-1] * 4, 60, False)
    mixed, ids = run(ps, [0, -1, 1, 0], 60, False)
    assert mixed[1] == base[1]
    for i in (0, 2, 3):
        assert mixed[i] != base[i] and mixed[i][:len(ps[i]) + 1] == base[i][:len(ps[i]) + 1]
    assert mixed[0] != run([ps[0]], [1], 60, False)[0][0]  # another adapter, other tokens
    for i, a in enumerate([0, -1, 1, 0]):
        assert run([ps[i]], [a], 60, False)[0][0] == mixed[i]
        assert run([ps[i]], [a], 60, True)[0][0] == mixed[i]


def test_unknown_ids_are_rejected_and_unload_waits_for_requests():
    rm = fa.RequestManager(max_sequence_length=64)
    llm = fa.HashModel(V, "inc", max_seq_len=64)
    assert rm.register_new_request([5, 6, 7], max_length=20, lora_id=0) == 0  # nothing loaded
    (a,) = load(llm, 1)
    for bad in (a + 1, 7, 8, 1000, -2):
        assert rm.register_new_request([5, 6, 7], max_length=20, lora_id=bad) == 0
    g = rm.register_new_request([5, 6, 7], max_length=20, lora_id=a)
    assert g > 0
    assert F.lib().ffmi_model_lora_unload(llm.handle, a) == 1   # a registered request names it
    other = fa.HashModel(V, "inc", max_seq_len=64)
    assert F.lib().ffmi_model_lora_unload(other.handle, a) == 1  # not that model's
    rm.serve_incr_decoding(llm)
    assert rm.get_generation_result(g).output_tokens == expected([5, 6, 7], 20, a)
    assert F.lib().ffmi_model_lora_unload(llm.handle, a) == 0
    assert rm.register_new_request([5, 6, 7], max_length=20, lora_id=a) == 0
    assert load(llm, 1) == [a]  # a freed id can be loaded again
    # all eight ids, then none left (FFMI_ERR_OOM); a BEAM model takes none
    more = load(other, F.LORA_MAX_ADAPTERS - 1)
    assert sorted(more + [a]) == list(range(F.LORA_MAX_ADAPTERS))
    out = ctypes.c_int(-1)
    assert F.lib().ffmi_model_lora_load(other.handle, 8, 16.0, None, None, ctypes.byref(out)) == 4
    other.close()
    ssm = fa.HashModel(V, "beam", max_seq_len=64)
    assert F.lib().ffmi_model_lora_load(ssm.handle, 8, 16.0, None, None, ctypes.byref(out)) == 5
    assert b"lora" in F.lib().ffmi_last_error()
    assert F.lib().ffmi_model_lora_load(llm.handle, 65, 16.0, None, None, ctypes.byref(out)) == 5
    assert b"lora" in F.lib().ffmi_last_error()
    # a request still pending when its manager goes away gives its reference back
    rm2 = fa.RequestManager(max_sequence_length=64)
    assert rm2.register_new_request([9, 9], max_length=10, lora_id=a) > 0
    assert F.lib().ffmi_model_lora_unload(llm.handle, a) == 1
    rm2.close()
    assert F.lib().ffmi_model_lora_unload(llm.handle, a) == 0
