"""LoRA adapters on the attention projections (q, k, v, o) through the model and
the serving API (Model(lora=True), load_lora({module: (A, B)}, alpha),
register_new_request(lora_id=)).  The 2-layer, V = 1000 model of
tests/test_gpu_e2e.py (hidden 256, 2 heads of 128) and, for what the update
means, the tiny GQA fixture config (4 heads of 64 over 2 K/V heads).
Run on an MI355X: pytest -m gpu."""
import os

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import lora_merge_oracle as MO
import lora_rule as LR
import oracle_lib as O
import parity_rules as PR
from flexflow_amd import checkpoint
from hip_util import report, ulp_diff
from test_gpu_alignment import close_ulp
from test_gpu_e2e import (LLM_CFG, SSM68_CFG, SSM_CFG, check_tokens_vs_oracle, first_divergence,
                          prompts)
from test_gpu_gqa_oracle import oracle_state
from test_gpu_lora_model import CAPTURES, KW, RM_KW, bits_equal, captures, tokens

pytestmark = pytest.mark.gpu

V = LLM_CFG["vocab_size"]
NL, H, FF = LLM_CFG["num_layers"], LLM_CFG["hidden"], LLM_CFG["intermediate"]
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
ALL = ATTN + ("down_proj",)
BLOCK = MO.MODULES


def dims(cfg):
    """{module: (in, out)} of the HF tensors"""
    h = cfg["hidden"]
    kv = cfg.get("num_kv_heads", cfg["num_heads"]) * (h // cfg["num_heads"])
    return {"q_proj": (h, h), "k_proj": (h, kv), "v_proj": (h, kv), "o_proj": (h, h),
            "down_proj": (cfg["intermediate"], h)}


def adapter(seed, mods, r=16, b_scale=0.05, cfg=LLM_CFG):
    """{module: (A [L][r][in], B [L][out][r])}: A ~ N(0, 1) / sqrt(in), B ~ b_scale N(0, 1)"""
    rng = np.random.default_rng([seed, r])
    L = cfg["num_layers"]
    return {m: (LR.f16(rng.standard_normal((L, r, i)) / np.sqrt(i)),
                LR.f16(rng.standard_normal((L, o, r)) * b_scale))
            for m, (i, o) in dims(cfg).items() if m in mods}


# ---------------------------------------------------------------- 1: nothing changes
@pytest.mark.parametrize("zero_b", [False, True], ids=["no_adapter", "zero_B_adapter"])
def test_flag_on_without_an_effective_adapter_equals_flag_off(zero_b):
    ps = prompts(3, V, 5, 30, 3)
    off = fa.Model(LLM_CFG, "inc", **KW)
    on = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    ids = None
    if zero_b:
        ad = {m: (A, np.zeros_like(B)) for m, (A, B) in adapter(1, ATTN).items()}
        ids = [on.load_lora(ad, 32.0)] * len(ps)
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


# ---------------------------------------------------------------- 2: each site by the rule
@pytest.mark.parametrize("mod", ATTN)
def test_layer0_site_is_the_rule_on_the_models_own_captures(mod):
    """A base run and an adapter run of one prefill step, one module alone.
    Layer 0 sees no adapter before the module's input: ATTN_NORM[0] (ATTN_OUT[0]
    for o) is bit-equal, and the module's columns of QKV[0] (O_PROJ[0]) of the
    base run are the y the adapter run updated, the other segments' columns
    bit-equal.  The interval is that of tests/test_gpu_lora_model.py: the model
    does not expose h, so it also covers h anywhere in its own interval."""
    ps = prompts(2, V, 20, 30, 5)
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    llm.set_debug(True)
    r, alpha = 12, 24.0
    ad = adapter(2, (mod,), r=r, b_scale=0.1)
    a = llm.load_lora(ad, alpha)
    tokens(llm, ps, max_new_tokens=1)
    base = captures(llm)
    tokens(llm, ps, [a, a], max_new_tokens=1)
    got = captures(llm)
    xk, yk = (("attn_out", 0), ("o_proj", 0)) if mod == "o_proj" else (("attn_norm", 0), ("qkv", 0))
    x = got[xk]
    assert bits_equal(x, base[xk])
    seg = ATTN.index(mod)
    cols = slice(0, H) if mod == "o_proj" else slice(seg * H, (seg + 1) * H)
    y = np.ascontiguousarray(base[yk][:, cols])
    y2 = np.ascontiguousarray(got[yk][:, cols])
    rest = np.ones(base[yk].shape[1], bool)
    rest[cols] = False
    assert bits_equal(np.ascontiguousarray(base[yk][:, rest]), np.ascontiguousarray(got[yk][:, rest]))
    if mod == "o_proj":  # nothing before the o projection moved
        assert bits_equal(base[("qkv", 0)], got[("qkv", 0)])
    A, B = ad[mod]
    rule = LR.Adapter(A[0], B[0], alpha)
    href, eh = rule.h_ref(x)
    h_mid = href.astype(np.float16)
    lo, hi = (href - eh).astype(np.float16), (href + eh).astype(np.float16)
    dh = np.maximum(hi.astype(np.float64) - h_mid.astype(np.float64),
                    h_mid.astype(np.float64) - lo.astype(np.float64))
    ref, e = rule.y_ref(y, h_mid)
    e = e + abs(float(rule.s16)) * (dh @ np.abs(rule.B.astype(np.float64)).T)
    ok = LR.in_interval(y2, ref, e)
    print(mod, "rows", x.shape[0], "outside", int((~ok).sum()), "changed", float((y2 != y).mean()))
    assert ok.all(), int((~ok).sum())
    assert (y2 != y).mean() > 0.5                # the update is there ...
    assert not LR.in_interval(y, ref, e).all()   # ... and the interval would miss its absence
    assert not bits_equal(got[("hidden", 0)], base[("hidden", 0)])


# ---------------------------------------------------------------- 3: mixed batches
def mixed_batch_check():
    """[q+v adapter, none, all-five adapter, q+v adapter] equals each request
    served alone, tokens exactly -- first without adapters, the test's own
    control (max_tokens 64: the GEMM sums of every step do not depend on T)."""
    ps = prompts(4, V, 5, 14, 9)
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    qv = llm.load_lora(adapter(3, ("q_proj", "v_proj"), r=16, b_scale=0.5), 32.0)
    five = llm.load_lora(adapter(4, ALL, r=12, b_scale=0.5), 24.0)
    control = tokens(llm, ps)
    for p, want in zip(ps, control):
        assert tokens(llm, [p]) == [want]
    ids = [qv, -1, five, qv]
    mixed = tokens(llm, ps, ids)
    for p, i, want in zip(ps, ids, mixed):
        assert tokens(llm, [p], [i]) == [want], i
    assert mixed[1] == control[1]
    changed = [m != c for m, c in zip(mixed, control)]
    assert changed[0] and changed[2] and changed[3], changed
    return sum(changed)


def test_mixed_batch_equals_each_request_alone():
    report("lora_modules_mixed_batch", changed=mixed_batch_check())


def test_mixed_batch_equals_each_request_alone_with_fused_norms(monkeypatch):
    """The same with the fused residual norms forced at this width
    (FFMI_FUSE_NORM is read at model creation): they are not bit-identical to
    the norm launches, so while an adapter with a module is resident every
    step takes that module's unfused route, and a request without an adapter
    has the same bits alone and inside the mixed batch."""
    monkeypatch.setenv("FFMI_FUSE_NORM", "2")
    report("lora_modules_mixed_batch_fused_norms", changed=mixed_batch_check())


@pytest.mark.parametrize("mods", [("q_proj", "v_proj"), ("o_proj",)], ids=["q_v", "o"])
def test_one_attention_site_next_to_the_fused_norms_it_leaves_in_place(monkeypatch, mods):
    """FFMI_FUSE_NORM=2 with only a q+v adapter, or only an o adapter, resident
    -- what a hidden >= 2048 model runs under the PEFT default.  The decode
    steps (T <= 4) keep the fused pairs the adapter's sites do not use: q+v --
    the norm-alone launch on the residual the fused down epilogue left, the
    unfused qkv GEMM, and o + gate/up still fused; o -- the unfused o
    projection, the post-attention norm launch and unfused gate/up, then the
    fused down and the next layer's fused qkv prologue.
    A zero-B adapter gives the tokens of the model without the flag, or a
    divergence that is an oracle-checked tie: the fused and the unfused norm
    differ in summation order, the rule of tests/test_gpu_e2e.py::
    test_fused_residual_norm_equals_norm_kernels; with debug captures on, which
    run every step unfused, every capture is bit-equal.  The mixed batch
    [adapter, none, adapter, zero-B] equals each request served alone, exactly."""
    monkeypatch.setenv("FFMI_FUSE_NORM", "2")
    ps = prompts(4, V, 5, 14, 9)
    off = fa.Model(LLM_CFG, "inc", **KW)
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    zero = llm.load_lora({m: (A, np.zeros_like(B)) for m, (A, B) in adapter(1, mods).items()}, 32.0)
    want, got = tokens(off, ps), tokens(llm, ps, [zero] * len(ps))
    ties = 0
    for p, x, y in zip(ps, want, got):
        if x != y:
            ties += 1
            check_tokens_vs_oracle(LLM_CFG, KW["weight_seed"], x, len(p) + 1)
            check_tokens_vs_oracle(LLM_CFG, KW["weight_seed"], y, len(p) + 1)
    ad = llm.load_lora(adapter(3, mods, r=16, b_scale=0.5), 32.0)
    control = tokens(llm, ps)
    for p, w in zip(ps, control):
        assert tokens(llm, [p]) == [w]
    ids = [ad, -1, ad, zero]
    mixed = tokens(llm, ps, ids)
    for p, i, w in zip(ps, ids, mixed):
        assert tokens(llm, [p], [i]) == [w], i
    assert mixed[1] == control[1] and mixed[3] == control[3]
    assert mixed[0] != control[0] and mixed[2] != control[2]
    report("lora_modules_fused_one_site", modules="+".join(mods), zero_b_ties=ties)
    for m in (off, llm):
        m.set_debug(True)
    t_off = tokens(off, ps[:2], max_new_tokens=3)
    c_off = captures(off)
    assert tokens(llm, ps[:2], [zero, zero], max_new_tokens=3) == t_off
    c_on = captures(llm)
    for kl in CAPTURES:
        assert bits_equal(c_on[kl], c_off[kl]), kl


def test_o_adapter_on_a_model_whose_attention_projects_its_own_output():
    """d = 64, hidden 768 (tests/test_gpu_e2e.py SSM68_CFG): decode steps fold
    the o projection into the fused attention, which leaves one fp32 slab per
    head.  With o in the step's mask the slabs are summed in head order and
    rounded once into proj, the value the residual norm computes from them, so
    a row without an adapter keeps its bits: a zero-B o adapter gives the
    tokens and, at a decode step, every capture of the model without the flag,
    bit for bit, and the mixed batch [o adapter, none, o adapter, zero-B]
    equals each request served alone."""
    cfg = SSM68_CFG
    kw = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=9)
    v = cfg["vocab_size"]
    ps = prompts(4, v, 5, 14, 9)
    off = fa.Model(cfg, "inc", **kw)
    llm = fa.Model(cfg, "inc", lora=True, **kw)
    zero = llm.load_lora({m: (A, np.zeros_like(B))
                          for m, (A, B) in adapter(1, ("o_proj",), cfg=cfg).items()}, 32.0)
    ad = llm.load_lora(adapter(3, ("o_proj",), r=16, b_scale=0.5, cfg=cfg), 32.0)
    control = tokens(off, ps)
    assert tokens(llm, ps) == control and tokens(llm, ps, [zero] * 4) == control
    ids = [ad, -1, ad, zero]
    mixed = tokens(llm, ps, ids)
    for p, i, w in zip(ps, ids, mixed):
        assert tokens(llm, [p], [i]) == [w], i
    assert mixed[1] == control[1] and mixed[3] == control[3]
    assert mixed[0] != control[0] and mixed[2] != control[2]
    caps = [(k, l) for k in ("attn_norm", "qkv", "attn_out", "o_proj", "ffn_norm", "mlp_act", "down")
            for l in range(cfg["num_layers"])] + [("hidden", l) for l in range(cfg["num_layers"] + 1)] + \
           [("logits", 0)]
    for m in (off, llm):
        m.set_debug(True)
    for new in (1, 3):  # the prefill (the o GEMM), then a decode step (the folded projection)
        t_off = tokens(off, ps[:2], max_new_tokens=new)
        c_off = {kl: off.debug_tensor(*kl).astype(np.float16) for kl in caps}
        assert tokens(llm, ps[:2], [zero, zero], max_new_tokens=new) == t_off
        for kl in caps:
            assert bits_equal(llm.debug_tensor(*kl).astype(np.float16), c_off[kl]), (new, kl)


# ---------------------------------------------------------------- 4: graph replay
def test_graph_replay_sees_fresh_assignments_and_module_masks(monkeypatch):
    """Two batch slots, four requests of different lengths: a request finishes
    and its slot goes to one with another adapter of other modules, so
    consecutive decode steps have one shape (T = 2) and different module masks.
    Replayed graphs and eager steps give the same tokens, those of each request
    served alone."""
    ps = prompts(4, V, 4, 9, 13)
    lens = [30, 45, 40, 50]
    rm_kw = dict(RM_KW, max_requests_per_batch=2)
    sets = [("q_proj", "v_proj"), ("o_proj",), ("k_proj", "down_proj")]
    out = {}
    for graphs in (1, 0):
        if graphs:
            monkeypatch.delenv("FFMI_NO_GRAPHS", raising=False)
        else:
            monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
        llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
        ids = [llm.load_lora(adapter(20 + i, sets[i], r=(16, 1, 64)[i], b_scale=0.5), 32.0)
               for i in range(3)]
        use = [ids[0], ids[1], -1, ids[2]]
        rm = fa.RequestManager(**rm_kw)
        gs = [rm.register_new_request(p, max_length=n, lora_id=i) for p, n, i in zip(ps, lens, use)]
        rm.serve_incr_decoding(llm)
        out[graphs] = [rm.get_generation_result(g).output_tokens for g in gs]
        if graphs:
            for p, n, i, want in zip(ps, lens, use, out[1]):
                assert tokens(llm, [p], [i], max_length=n) == [want], i
            for k in (0, 1, 3):
                assert tokens(llm, [ps[k]], None, max_length=lens[k])[0] != out[1][k], k
    assert out[0] == out[1]


# ---------------------------------------------------------------- 5: SpecInfer
def test_spec_infer_with_a_q_v_adapter_agrees_with_incremental_decoding():
    """tests/test_gpu_lora_model.py's SpecInfer test with a q+v adapter on the
    TREE LLM: identical to incremental decoding under the same adapter, or the
    first divergence is a tie within 2 fp16 ulp of the two tokens'
    probabilities, from the adapter model's own logits at that position."""
    ps = prompts(3, V, 5, 20, 17)
    ad = adapter(6, ("q_proj", "v_proj"), r=16, b_scale=0.5)
    inc = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    a = inc.load_lora(ad, 32.0)
    ids = [a, -1, a]
    want = tokens(inc, ps, ids, max_length=60)
    assert want[0] != tokens(inc, ps[:1], max_length=60)[0]
    rm = fa.RequestManager(**dict(RM_KW, spec_tree_width=(1, 1, 3), max_spec_tree_token_num=23))
    vt = 64 + 23 * 4
    tree = fa.Model(LLM_CFG, "tree", lora=True, **dict(KW, max_tokens=vt, max_tree_tokens=23))
    rm.register_ssm_model(fa.Model(SSM_CFG, "beam", max_requests=4, max_tokens=vt, max_seq_len=128,
                                   max_tree_tokens=23, weight_seed=5))
    a2 = tree.load_lora(ad, 32.0)
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
    report("lora_modules_spec_equals_incr", identical=same, requests=len(ps))
    assert rm.stats().ssm_steps > 0


# ---------------------------------------------------------------- 6: what PEFT means
GQA_KW = dict(max_requests=1, max_tokens=64, max_seq_len=128)
PEFT_R, PEFT_ALPHA, PEFT_B = 8, 16.0, 0.05


@pytest.fixture(scope="module")
def peft_case(tmp_path_factory):
    """the tiny GQA fixture config (4 query heads over 2 K/V heads) with its
    oracle tensors as a checkpoint, a q/k/v/o adapter, and the oracle's logits
    on the plain and on the merged weights for one 40-token prompt"""
    cfg, _ = O.load_golden("tiny_gqa_d64")
    assert cfg["num_kv_heads"] < cfg["num_heads"]
    om = O.Model(cfg, cfg["seed"], fp16=1, max_requests=1, max_seq=128)
    state = oracle_state(om, cfg)
    rng = np.random.default_rng(40)
    prompt = [1] + rng.integers(3, cfg["vocab_size"], size=39).tolist()
    plain = om.forward(0, prompt, 0)
    assert (MO.forward(state, cfg, prompt) == plain).all()  # the restatement is the oracle
    ad = adapter(6, ATTN, r=PEFT_R, b_scale=PEFT_B, cfg=cfg)
    merged = MO.forward(MO.merge(state, ad, PEFT_ALPHA), cfg, prompt)
    merged2 = MO.forward(MO.merge(state, ad, PEFT_ALPHA, round_update=True), cfg, prompt)
    folder = str(tmp_path_factory.mktemp("peft_base"))
    fa.convert_hf_model(state, folder)
    return dict(cfg=cfg, prompt=prompt, ad=ad, folder=folder, plain=plain, merged=merged,
                ambiguity=float(np.abs(merged - merged2).max()))


def adapter_logits(case, ad, native):
    m = fa.Model(case["cfg"], "inc", weights_folder=case["folder"], native_gqa=native, lora=True,
                 **GQA_KW)
    try:
        a = m.load_lora(ad, PEFT_ALPHA)
        m.set_debug(True)
        rm = fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=64,
                               max_sequence_length=128)
        fa.generate(rm, m, [case["prompt"][1:]], max_length=len(case["prompt"]) + 1, lora_ids=[a])
        lg = m.debug_tensor("logits")
    finally:
        m.close()
    assert lg.shape[0] == len(case["prompt"])
    return lg


def merged_bar(case, lg):
    """share of the logits within the checkpoint tests' bar (2 fp16 ulp or 2e-3,
    tests/test_gpu_alignment.close_ulp) widened by twice the merge's own
    ambiguity: two independent roundings meet"""
    return close_ulp(lg, case["merged"], atol=2e-3 + 2 * case["ambiguity"])[0]


@pytest.mark.parametrize("native", [False, True], ids=["replicated", "native_gqa"])
def test_the_update_means_what_peft_means(peft_case, native):
    """The adapter model on the GPU against the CPU oracle on the merged
    checkpoint W' = fp16(W + (alpha / r) B A), one 40-token prompt teacher-forced
    in a prefill step.  Logits: within 2 fp16 ulp or 2e-3 + 2 x ambiguity on >=
    99.9% -- the bar of the checkpoint tests (tests/test_gpu_gqa_oracle.py) plus
    the merge's own ambiguity, the largest logit gap between the oracle on W'
    and on W'' = fp16(W + fp16((alpha / r) B A)), measured here on the CPU:
    0.00195 (so the bar's absolute part is 0.0059).  The adapter (r = 8, alpha
    = 16, B ~ 0.05 N(0, 1)) moves the logits by 0.30 on average, 1.39 at most:
    50 x the bar on average (the test asserts >= 20 x).  Picks by tests/parity_rules.py's tie rule and
    budget.  Two negative controls must miss the same bar: q's and v's adapters
    exchanged (A whole; B on the rows both have, v's being num_kv_heads * d
    long), and the o adapter dropped."""
    c = peft_case
    tol = 2e-3 + 2 * c["ambiguity"]
    move = np.abs(c["merged"] - c["plain"])
    print("ambiguity", c["ambiguity"], "tolerance", tol, "mean move", float(move.mean()),
          "max move", float(move.max()))
    assert 0 < c["ambiguity"] <= 4e-3, c["ambiguity"]
    assert move.mean() >= 20 * tol, (float(move.mean()), tol)
    lg = adapter_logits(c, c["ad"], native)
    ok = merged_bar(c, lg)
    print("native", native, "within bar", ok, "max |diff|", float(np.abs(lg - c["merged"]).max()))
    report("lora_modules_vs_merged_oracle", native=native, within_bar=ok, ambiguity=c["ambiguity"])
    assert ok >= 0.999, ok
    want, got = PR.picks(c["merged"]), PR.picks(lg)
    verdicts = [PR.classify(c["merged"][t], None, got[t], want[t])
                for t in range(len(want)) if got[t] != want[t]]
    PR.assert_ties(verdicts, len(want))
    # negative controls
    (qa, qb), (va, vb) = c["ad"]["q_proj"], c["ad"]["v_proj"]
    n = vb.shape[1]
    qb2, vb2 = qb.copy(), qb[:, :n].copy()
    qb2[:, :n] = vb
    swapped = dict(c["ad"], q_proj=(va, qb2), v_proj=(qa, vb2))
    dropped = {m: ab for m, ab in c["ad"].items() if m != "o_proj"}
    for name, ad in (("q_v_swapped", swapped), ("o_dropped", dropped)):
        bad = merged_bar(c, adapter_logits(c, ad, native))
        print("negative control", name, "within bar", bad)
        assert bad < 0.999, (name, "NOT detected", bad)


# ---------------------------------------------------------------- 7: folders
def test_folder_load_equals_array_load_and_refusals(tmp_path):
    llm = fa.Model(LLM_CFG, "inc", lora=True, **KW)
    r, alpha = 12, 24.0
    ad = adapter(7, ("q_proj", "v_proj"), r=r, b_scale=0.5)
    ps = prompts(2, V, 5, 12, 21)
    a = llm.load_lora(ad, alpha)
    want = tokens(llm, ps, [a, a])
    assert want != tokens(llm, ps)
    sd = {}
    for m, (A, B) in ad.items():
        for l in range(NL):
            p = f"base_model.model.model.layers.{l}.{BLOCK[m]}.{m}."
            sd[p + "lora_A.weight"], sd[p + "lora_B.weight"] = A[l], B[l]
    cfg = dict(peft_type="LORA", r=r, lora_alpha=alpha, target_modules=["q_proj", "v_proj"])
    for dtype in (np.float16, np.float32):
        dst = str(tmp_path / np.dtype(dtype).name)
        assert checkpoint.convert_peft_adapter(sd, cfg, dst, dtype=dtype) == (r, alpha)
        b = llm.load_lora(dst)
        assert b != a and tokens(llm, ps, [b, b]) == want
        llm.unload_lora(b)
    L = F.lib()
    import ctypes
    out = ctypes.c_int(-1)
    ex = lambda folder, mask: L.ffmi_model_lora_load_folder_ex(llm.handle, folder.encode(), r, alpha,
                                                               mask, ctypes.byref(out))
    Q, K, Vb, Ob, D = (1 << F.LORA_MODULES[m] for m in ALL)
    assert ex(dst, Q | Vb) == 0
    llm.unload_lora(out.value)
    # a file of a module outside the mask; a module in the mask without files; the
    # down-only entry point on this folder; a wrong size; gate / up files
    for mask in (Q, Q | Vb | K, Q | Vb | D):
        assert ex(dst, mask) == 5 and "lora" in L.ffmi_last_error().decode(), mask
    assert L.ffmi_model_lora_load_folder(llm.handle, dst.encode(), r, alpha, ctypes.byref(out)) == 5
    assert "lora" in L.ffmi_last_error().decode()
    open(os.path.join(dst, "layers.1.self_attn.v_proj.lora_B.weight"), "ab").write(b"\0\0")
    assert ex(dst, Q | Vb) == 5 and "lora" in L.ffmi_last_error().decode()
    dst = str(tmp_path / "float16")
    open(os.path.join(dst, "layers.0.mlp.gate_proj.lora_A.weight"), "wb").write(b"\0" * 64)
    assert ex(dst, Q | Vb) == 5 and "lora" in L.ffmi_last_error().decode()
    with pytest.raises(F.FFMIError, match="lora"):
        llm.load_lora(dst)
    # arrays: gate / up unsupported; a module twice, none, an unknown id invalid
    A, B = ad["q_proj"]
    mod = lambda i: F.LoraModule(i, A.ctypes.data, B.ctypes.data)
    load = lambda mods: L.ffmi_model_lora_load_modules(llm.handle, r, alpha, len(mods),
                                                       (F.LoraModule * max(1, len(mods)))(*mods),
                                                       ctypes.byref(out))
    for i in (F.LORA_MODULES["gate_proj"], F.LORA_MODULES["up_proj"]):
        assert load([mod(0), mod(i)]) == 5 and "lora" in L.ffmi_last_error().decode()
    for mods in ([mod(0), mod(0)], [], [mod(7)], [mod(-1)]):
        assert load(mods) == 1 and "lora" in L.ffmi_last_error().decode()
    with pytest.raises(F.FFMIError, match="lora"):
        llm.load_lora({"gate_proj": (A, B)}, alpha)
    assert tokens(llm, ps, [a, a]) == want  # nothing of the refusals stuck
    llm.set_profiling(2)
    tokens(llm, ps, [a, -1], max_new_tokens=2)
    assert llm.op_stats()["lora"]["launches"] > 0


# ---------------------------------------------------------------- launch counts
def test_down_only_and_no_adapter_steps_launch_what_they_launched_before():
    """op_stats of one prefill and one decode step: a model with the flag and
    no adapter launches what a model without the flag launches, and a step
    whose adapters have down_proj only adds, per layer, the slab reduce and the
    two LoRA launches under "lora" and nothing elsewhere -- no qkv or o site."""
    ps = prompts(2, V, 5, 12, 23)
    rng = np.random.default_rng(8)
    dn = (LR.f16(rng.standard_normal((NL, 16, FF)) / 16), LR.f16(rng.standard_normal((NL, H, 16)) * 0.05), 32.0)

    def counts(lora, load, use):
        m = fa.Model(LLM_CFG, "inc", lora=lora, **KW)
        ids = [m.load_lora(*a) for a in load]
        m.set_profiling(2)
        tokens(m, ps, [ids[i] if i >= 0 else -1 for i in use] if use else None, max_new_tokens=2)
        return {k: v["launches"] for k, v in m.op_stats().items()}

    off = counts(False, [], None)
    assert off.get("lora", 0) == 0 and off["gemm_down"] > 0
    assert counts(True, [], None) == off
    assert counts(True, [dn], None) == off  # resident, not named: still the plain step
    down = counts(True, [dn], [0, 0])
    assert {k: v for k, v in down.items() if k != "lora"} == {k: v for k, v in off.items() if k != "lora"}
    assert down["lora"] == off["gemm_down"]  # one LoRA call per down projection, no other site
    qv = (adapter(9, ("q_proj", "v_proj")), 32.0)
    both = counts(True, [dn, qv], [1, 0])
    assert both["lora"] == off["gemm_down"] + off["gemm_qkv"]
    assert {k: v for k, v in both.items() if k != "lora"} == {k: v for k, v in off.items() if k != "lora"}
