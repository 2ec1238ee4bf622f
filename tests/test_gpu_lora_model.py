"""LoRA adapters on down_proj through the model and the serving API
(Model(lora=True), load_lora, register_new_request(lora_id=)).  The 2-layer,
V = 1000 model of tests/test_gpu_e2e.py: hidden 256 < 2048, so neither side
uses the fused residual norms.  Run on an MI355X: pytest -m gpu."""
import os

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import lora_rule as LR
from flexflow_amd import checkpoint
from test_gpu_e2e import LLM_CFG, SSM_CFG, first_divergence, prompts
from hip_util import report, ulp_diff

pytestmark = pytest.mark.gpu

V = LLM_CFG["vocab_size"]
NL, H, FF = LLM_CFG["num_layers"], LLM_CFG["hidden"], LLM_CFG["intermediate"]
KW = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=11)
RM_KW = dict(max_requests_per_batch=4, max_tokens_per_batch=64, max_sequence_length=128)
CAPTURES = [(k, l) for k in ("embed", "attn_norm", "qkv", "attn_out", "o_proj", "ffn_norm",
                             "mlp_act", "down") for l in range(NL if k != "embed" else 1)] + \
           [("hidden", l) for l in range(NL + 1)] + [("logits", 0)]


def adapter(seed, r=16, b_scale=0.05, alpha=None):
    """(A [L][r][F], B [L][H][r], alpha): A ~ N(0, 1) / sqrt(F), B ~ b_scale N(0, 1)"""
    rng = np.random.default_rng([seed, r])
    A = LR.f16(rng.standard_normal((NL, r, FF)) / np.sqrt(FF))
    B = LR.f16(rng.standard_normal((NL, H, r)) * b_scale)
    return A, B, float(2 * r if alpha is None else alpha)


def tokens(llm, ps, ids=None, rm_kw=RM_KW, **kw):
    kw = kw or dict(max_length=64)
    res = fa.generate(fa.RequestManager(**rm_kw), llm, ps, lora_ids=ids, **kw)
    return [r.output_tokens for r in res]


def captures(llm):
    return {kl: llm.debug_tensor(*kl).astype(np.float16) for kl in CAPTURES}


def bits_equal(a, b):
    return a.shape == b.shape and (a.view(np.uint16) == b.view(np.uint16)).all()


# ---------------------------------------------------------------- 1, 2: nothing changes
@pytest.mark.parametrize("zero_b", [False, True], ids=["no_adapter", "zero_B_adapter"])
def test_flag_on_without_an_effective_adapter_equals_flag_off(zero_b):
    ps = prompts(3, V, 5, 30, 3)
    off = fa.Model(LLM_CFG, "inc", **KW)
    on = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    ids = None
    if zero_b:
        A, B, alpha = adapter(1)
        a = on.load_lora(A, np.zeros_like(B), alpha)
        ids = [a] * len(ps)
    assert tokens(on, ps, ids) == tokens(off, ps)
    for m in (off, on):
        m.set_debug(True)
    # the last eager step of each run: the prefill (max_new_tokens 1), then a decode step
    for new in (1, 3):
        t_off = tokens(off, ps[:2], max_new_tokens=new)
        c_off = captures(off)
        assert tokens(on, ps[:2], ids[:2] if ids else None, max_new_tokens=new) == t_off
        c_on = captures(on)
        for kl in CAPTURES:
            assert bits_equal(c_on[kl], c_off[kl]), kl


# ---------------------------------------------------------------- 3: layer 0 by the rule
@pytest.mark.parametrize("r", [12, 64])
def test_layer0_down_is_the_rule_on_the_models_own_captures(r):
    """A base run and an adapter run of one prefill step.  Layer 0 sees no
    adapter before its down projection: MLP_ACT[0] is bit-equal, and DOWN[0] of
    the base run is the y the adapter run updated.  The model does not expose
    h, so the interval for y' also covers h anywhere in its own interval:
    ref, e_y from h_mid = fp16(h_ref), plus |s| * sum_j dh[j] |B[n][j]| with
    dh the distance from h_mid to the farther end of [fp16(h_ref - e_h),
    fp16(h_ref + e_h)]."""
    ps = prompts(2, V, 20, 30, 5)
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    llm.set_debug(True)
    A, B, alpha = adapter(2, r=r, b_scale=0.1)
    a = llm.load_lora(A, B, alpha)
    tokens(llm, ps, max_new_tokens=1)
    base = captures(llm)
    tokens(llm, ps, [a, a], max_new_tokens=1)
    got = captures(llm)
    x, y, y2 = got[("mlp_act", 0)], base[("down", 0)], got[("down", 0)]
    assert bits_equal(x, base[("mlp_act", 0)]) and bits_equal(base[("o_proj", 0)], got[("o_proj", 0)])
    ad = LR.Adapter(A[0], B[0], alpha)
    href, eh = ad.h_ref(x)
    h_mid = href.astype(np.float16)
    lo, hi = (href - eh).astype(np.float16), (href + eh).astype(np.float16)
    dh = np.maximum(hi.astype(np.float64) - h_mid.astype(np.float64),
                    h_mid.astype(np.float64) - lo.astype(np.float64))
    ref, e = ad.y_ref(y, h_mid)
    e = e + abs(float(ad.s16)) * (dh @ np.abs(ad.B.astype(np.float64)).T)
    ok = LR.in_interval(y2, ref, e)
    print("rows", x.shape[0], "outside", int((~ok).sum()), "changed", float((y2 != y).mean()))
    assert ok.all(), int((~ok).sum())
    assert (y2 != y).mean() > 0.5            # the update is there ...
    assert not LR.in_interval(y, ref, e).all()  # ... and the interval would miss its absence
    assert not bits_equal(got[("hidden", 0)], base[("hidden", 0)])


# ---------------------------------------------------------------- 4: mixed batches
def test_mixed_batch_equals_each_request_alone():
    """max_tokens 64: every step stays in the <= 64-row regime whose GEMM sums
    do not depend on T (include/ffmi.h), so batched and alone are compared
    exactly -- first without adapters, the test's own control."""
    ps = prompts(4, V, 5, 14, 9)
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    a = llm.load_lora(*adapter(3, r=16, b_scale=0.5))
    b = llm.load_lora(*adapter(4, r=12, b_scale=0.5))
    big = llm.load_lora(*adapter(5, r=64, b_scale=2.0))
    assert len({a, b, big}) == 3
    control = tokens(llm, ps)
    for p, want in zip(ps, control):
        assert tokens(llm, [p]) == [want]
    ids = [a, -1, b, a]
    mixed = tokens(llm, ps, ids)
    for p, i, want in zip(ps, ids, mixed):
        assert tokens(llm, [p], [i]) == [want], i
    assert mixed[1] == control[1]
    n_changed = sum(m != c for m, c in zip(mixed, control))
    report("lora_mixed_batch", changed=n_changed)
    # an adapter with large B changes the generated tokens, not the prompt
    t_big = tokens(llm, ps[:1], [big])[0]
    assert t_big != control[0] and t_big[:len(ps[0]) + 1] == control[0][:len(ps[0]) + 1]


# ---------------------------------------------------------------- 5: graph replay
def test_graph_replay_sees_fresh_adapter_assignments(monkeypatch):
    """Two batch slots, four requests of different lengths: a request finishes
    and its slot goes to one with another adapter, so consecutive decode steps
    have one shape (T = 2) and different assignments.  Replayed graphs and
    eager steps give the same tokens, those of each request served alone."""
    ps = prompts(4, V, 4, 9, 13)
    lens = [30, 45, 40, 50]
    rm_kw = dict(RM_KW, max_requests_per_batch=2)
    out = {}
    for graphs in (1, 0):
        if graphs:
            monkeypatch.delenv("FFMI_NO_GRAPHS", raising=False)
        else:
            monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
        llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
        ids = [llm.load_lora(*adapter(20 + i, r=(16, 1, 64)[i], b_scale=0.5)) for i in range(3)]
        use = [ids[0], ids[1], -1, ids[2]]
        rm = fa.RequestManager(**rm_kw)
        gs = [rm.register_new_request(p, max_length=n, lora_id=i) for p, n, i in zip(ps, lens, use)]
        rm.serve_incr_decoding(llm)
        out[graphs] = [rm.get_generation_result(g).output_tokens for g in gs]
        if graphs:
            for p, n, i, want in zip(ps, lens, use, out[1]):
                assert tokens(llm, [p], [i], max_length=n) == [want], i
            assert tokens(llm, ps[:1], None, max_length=lens[0])[0] != out[1][0]
    assert out[0] == out[1]


# ---------------------------------------------------------------- 6: SpecInfer
def test_spec_infer_with_an_adapter_agrees_with_incremental_decoding():
    """A TREE LLM with adapters and a plain SSM against incremental decoding
    under the same adapters, by the rule of tests/test_gpu_e2e.py for that
    pair: identical, or the first divergence is a tie within 2 fp16 ulp of the
    two tokens' probabilities -- taken from the adapter model's own logits at
    that position (the CPU oracle has no adapters)."""
    ps = prompts(3, V, 5, 20, 17)
    A, B, alpha = adapter(6, r=16, b_scale=0.5)
    inc = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    a = inc.load_lora(A, B, alpha)
    ids = [a, -1, a]
    want = tokens(inc, ps, ids, max_length=60)
    assert want[0] != tokens(inc, ps[:1], max_length=60)[0]
    rm = fa.RequestManager(**dict(RM_KW, spec_tree_width=(1, 1, 3), max_spec_tree_token_num=23))
    vt = 64 + 23 * 4
    tree = fa.Model(LLM_CFG, "tree", lora=True, **dict(KW, max_tokens=vt, max_tree_tokens=23))
    rm.register_ssm_model(fa.Model(SSM_CFG, "beam", max_requests=4, max_tokens=vt, max_seq_len=128,
                                   max_tree_tokens=23, weight_seed=5))
    # (the tree model loads the same adapter: ids are per process, one owner each)
    a2 = tree.load_lora(A, B, alpha)
    got = [r.output_tokens for r in fa.generate(rm, tree, ps, max_length=60,
                                                lora_ids=[a2 if i >= 0 else -1 for i in ids])]
    same = 0
    inc.set_debug(True)
    for p, i, x, y in zip(ps, ids, want, got):
        if x == y:
            same += 1
            continue
        d = first_divergence(x, y)
        assert d >= len(p) + 1
        tokens(inc, [x[1:d]], [i], max_new_tokens=1)
        row = inc.debug_tensor("logits")[-1].astype(np.float64)
        pr = np.exp(row - row.max())
        p16 = (pr / pr.sum()).astype(np.float16)
        assert ulp_diff(p16[x[d]], p16[y[d]]) <= 2, (d, x[d], y[d])
    report("lora_spec_equals_incr", identical=same, requests=len(ps))
    assert rm.stats().ssm_steps > 0


# ---------------------------------------------------------------- 7: load / unload
def test_load_from_folder_unload_and_refusals(tmp_path):
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    A, B, alpha = adapter(7, r=12, b_scale=0.5)
    ps = prompts(2, V, 5, 12, 21)
    a = llm.load_lora(A, B, alpha)
    want = tokens(llm, ps, [a, a])
    sd = {}
    for l in range(NL):
        p = f"base_model.model.model.layers.{l}.mlp.down_proj."
        sd[p + "lora_A.weight"], sd[p + "lora_B.weight"] = A[l], B[l]
    cfg = dict(peft_type="LORA", r=12, lora_alpha=alpha, target_modules=["down_proj"])
    for dtype in (np.float16, np.float32):
        dst = str(tmp_path / np.dtype(dtype).name)
        assert checkpoint.convert_peft_adapter(sd, cfg, dst, dtype=dtype) == (12, alpha)
        b = llm.load_lora(dst)
        assert b != a and tokens(llm, ps, [b, b]) == want
        llm.unload_lora(b)
    # unload while a registered request names the adapter is refused
    rm = fa.RequestManager(**RM_KW)
    g = rm.register_new_request(ps[0], max_length=40, lora_id=a)
    with pytest.raises(F.FFMIError):
        llm.unload_lora(a)
    rm.serve_incr_decoding(llm)
    assert rm.get_generation_result(g).output_tokens == tokens(llm, ps[:1], [a], max_length=40)[0]
    llm.unload_lora(a)
    assert rm.register_new_request(ps[0], max_length=40, lora_id=a) == 0
    assert llm.load_lora(A, B, alpha) == a  # a freed id can be loaded again
    assert tokens(llm, ps, [a, a]) == want
    # refusals: rank above 64, a folder with another target module, a model without the flag
    for fn in (lambda: llm.load_lora(np.zeros((NL, 65, FF), np.float16),
                                     np.zeros((NL, H, 65), np.float16), 1.0),
               lambda: fa.Model(LLM_CFG, "inc", **KW).load_lora(A, B, alpha)):
        with pytest.raises(F.FFMIError, match="lora"):
            fn()
    open(os.path.join(dst, "layers.0.self_attn.q_proj.lora_A.weight"), "wb").write(b"\0" * 64)
    with pytest.raises(F.FFMIError, match="lora"):
        llm.load_lora(dst)
    ids = [llm.load_lora(A, B, alpha) for _ in range(F.LORA_MAX_ADAPTERS - 1)]
    assert sorted(ids + [a]) == list(range(F.LORA_MAX_ADAPTERS))
    with pytest.raises(F.FFMIError):
        llm.load_lora(A, B, alpha)
    stats_model = fa.Model(LLM_CFG, "inc", lora=True, **KW)  # (every id is taken: OOM, not a crash)
    with pytest.raises(F.FFMIError):
        stats_model.load_lora(A, B, alpha)
    for i in ids:
        llm.unload_lora(i)
    llm.set_profiling(2)
    tokens(llm, ps, [a, -1], max_new_tokens=2)
    assert llm.op_stats()["lora"]["launches"] > 0
