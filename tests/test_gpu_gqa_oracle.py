"""Native grouped-query attention and model-level llama3 RoPE against the
HF-pinned CPU oracle.

tests/test_oracle_golden.py pins the oracle's GQA (query head h over K/V head
h // G, HF repeat_kv) and its llama3 RoPE table to HF transformers on the
fixtures tiny_gqa_d64 (4 query heads over 2 K/V heads: only with two K/V heads
do h // G and h % num_kv_heads differ) and tiny_gqa_d128_llama3 (multi-query,
theta 5e5, llama3 scaling).  Here the oracle's fp16 mode pins the GPU: the
native model (K/V projections, qkv GEMM and KV cache at num_kv_heads), the
loader's replicated load of a GQA checkpoint, the TP split of the K/V heads,
SpecInfer over a native cache and llama3 RoPE through a whole model -- each
against a reference that shares no code with the path under test
(test_gpu_gqa_model.py and test_gpu_gqa_attention.py compare GPU routes with
each other: route equality and cache bits, which the oracle cannot see).

Bars: tokens teacher-forced through the oracle under
the tie rules of test_gpu_e2e.check_tokens_vs_oracle / tests/parity_rules.py;
logits within 2 fp16 ulp or 2e-3 on >= 99.9% (test_gpu_alignment.close_ulp);
per-op local checks within 2 fp16 ulp on >= 99.9%, the norms bit-exact
(test_gpu_fulldepth.py); fp32 models within 1e-4 of the fp32 oracle, picks
exact unless the oracle's gap is <= 1e-4 (test_gpu_full_precision.py).
"""
import numpy as np
import pytest

import flexflow_amd as fa
import oracle_lib as O
import test_gpu_gqa_model as GM
from hip_util import report
from test_gpu_alignment import close_ulp
from test_gpu_e2e import check_tokens_vs_oracle
from test_gpu_fulldepth import rope_ref, within
from test_gpu_full_precision import FP32_TIE
from test_gpu_random_models import WIDTHS, check_all, random_cfg, random_requests

pytestmark = pytest.mark.gpu

GQA_TAGS = ["tiny_gqa_d64", "tiny_gqa_d128_llama3"]
KW = dict(max_requests=1, max_tokens=64, max_seq_len=128)


def one_rm():
    return fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=64,
                             max_sequence_length=128)


def llama3_of(cfg):
    return ((cfg["rope_factor"], cfg["rope_low_freq_factor"], cfg["rope_high_freq_factor"],
             cfg["rope_original_max_pos"]) if cfg.get("rope_llama3") else None)


def oracle_state(om, cfg):
    """the oracle's own tensors by HF name, k/v_proj at their GQA size"""
    H, F, V = cfg["hidden"], cfg["intermediate"], cfg["vocab_size"]
    Hkv = cfg["num_kv_heads"] * (H // cfg["num_heads"])
    st = {"model.embed_tokens.weight": (V, H), "model.norm.weight": (H,), "lm_head.weight": (V, H)}
    for l in range(cfg["num_layers"]):
        p = f"model.layers.{l}."
        st.update({p + "input_layernorm.weight": (H,), p + "post_attention_layernorm.weight": (H,),
                   p + "self_attn.q_proj.weight": (H, H), p + "self_attn.k_proj.weight": (Hkv, H),
                   p + "self_attn.v_proj.weight": (Hkv, H), p + "self_attn.o_proj.weight": (H, H),
                   p + "mlp.gate_proj.weight": (F, H), p + "mlp.up_proj.weight": (F, H),
                   p + "mlp.down_proj.weight": (H, F)})
    return {n: om.weight(n).reshape(shape) for n, shape in st.items()}


def prefill_logits(m, prompt):
    """logits [len(prompt)][V] of one prefill step (prompt with its BOS)"""
    m.set_debug(True)
    fa.generate(one_rm(), m, [list(prompt[1:])], max_length=len(prompt) + 1)
    lg = m.debug_tensor("logits")
    m.set_debug(False)
    assert lg.shape[0] == len(prompt)
    return lg


def decode(m, prompt, n_new):
    return fa.generate(one_rm(), m, [list(prompt[1:])],
                       max_length=len(prompt) + n_new)[0].output_tokens


def check_fp32_picks(om, seq, n_prompt):
    """teacher-forced through the fp32 oracle: every pick the oracle's, unless
    the oracle's own gap between the two is an fp32-level tie"""
    lg = om.forward(0, np.array(seq[:-1], np.int32), 0)[n_prompt - 1:]
    ids, _ = O.softmax_argmax(lg, fp16=0)
    for t, g in enumerate(seq[n_prompt:]):
        if ids[t] != g:
            assert float(lg[t][ids[t]] - lg[t][g]) <= FP32_TIE, (t, g, int(ids[t]))


# ------------------------------------------------------------- fixture models
@pytest.mark.parametrize("tag", GQA_TAGS)
def test_incr_decoding_of_gqa_fixture_models(tag):
    """test_incr_decoding_matches_golden_fixture_model for the two GQA
    fixtures: the native model seeded like the fixture, every pick
    teacher-forced through the oracle (whose fp32 mode equals HF's greedy)."""
    cfg, g = O.load_golden(tag)
    prompt = g["prompt"].tolist()
    m = fa.Model(cfg, "inc", weight_seed=cfg["seed"], native_gqa=True, **KW)
    try:
        toks = decode(m, prompt, cfg["n_new"])
    finally:
        m.close()
    assert len(toks) == len(prompt) + cfg["n_new"]
    check_tokens_vs_oracle(cfg, cfg["seed"], toks, len(prompt))


# ---------------------------------------------- checkpoints written by the oracle
@pytest.fixture(scope="module")
def d64():
    cfg, g = O.load_golden("tiny_gqa_d64")
    prompt = g["prompt"].tolist()
    om = O.Model(cfg, cfg["seed"], fp16=1, max_requests=1, max_seq=128)
    return dict(cfg=cfg, prompt=prompt, om=om, state=oracle_state(om, cfg),
                logits=om.forward(0, prompt, 0))


@pytest.mark.parametrize("native", [False, True])
def test_checkpoint_load_against_the_oracle(d64, tmp_path, native):
    """A reference-format checkpoint of the oracle's own tensors, loaded with
    K/V replicated by the loader (file_loader.cc:292-302) and natively: the
    loader's K/V row order and head mapping against the oracle's h // G."""
    cfg, prompt = d64["cfg"], d64["prompt"]
    fa.convert_hf_model(d64["state"], str(tmp_path))
    m = fa.Model(cfg, "inc", weights_folder=str(tmp_path), native_gqa=native, **KW)
    try:
        ok, exact = close_ulp(prefill_logits(m, prompt), d64["logits"])
        toks = decode(m, prompt, cfg["n_new"])
    finally:
        m.close()
    print("checkpoint load, native", native, "within bar", ok, "bit-exact", exact)
    report("gqa_checkpoint_vs_oracle", native=native, within_2ulp=ok, exact=exact)
    assert ok >= 0.999, ok
    check_tokens_vs_oracle(cfg, cfg["seed"], toks, len(prompt))


def test_full_precision_replicated_load_against_the_fp32_oracle(d64, tmp_path):
    """the fp32 model has no native GQA: the loader's replication in
    llama_f32.cpp against the fp32 oracle (which HF pins at rtol 1e-4)"""
    cfg, prompt = d64["cfg"], d64["prompt"]
    om = O.Model(cfg, cfg["seed"], fp16=0, max_requests=1, max_seq=128)
    fa.convert_hf_model(oracle_state(om, cfg), str(tmp_path), dtype=np.float32)
    m = fa.Model(cfg, "inc", weights_folder=str(tmp_path), full_precision=True, **KW)
    try:
        lg = prefill_logits(m, prompt)
        toks = decode(m, prompt, cfg["n_new"])
    finally:
        m.close()
    err = float(np.abs(lg - om.forward(0, prompt, 0)).max())
    print("fp32 replicated load: max |logit error|", err)
    report("gqa_full_precision_replicated_vs_oracle", max_abs_err=err)
    assert err <= 1e-4, err
    check_fp32_picks(om, toks, len(prompt))


def test_negative_control_swapped_k_heads_is_rejected(d64, tmp_path):
    """The logits bar must FAIL a wrong K/V head index: the checkpoint with
    the two K head blocks of k_proj exchanged in every layer (V untouched),
    loaded natively, against the oracle of the unswapped model."""
    cfg, prompt = d64["cfg"], d64["prompt"]
    d = cfg["hidden"] // cfg["num_heads"]
    st = dict(d64["state"])
    for l in range(cfg["num_layers"]):
        n = f"model.layers.{l}.self_attn.k_proj.weight"
        st[n] = np.concatenate([st[n][d:2 * d], st[n][:d]])
    fa.convert_hf_model(st, str(tmp_path))
    m = fa.Model(cfg, "inc", weights_folder=str(tmp_path), native_gqa=True, **KW)
    try:
        ok, exact = close_ulp(prefill_logits(m, prompt), d64["logits"])
    finally:
        m.close()
    print("swapped K heads: within bar", ok, "bit-exact", exact)
    report("gqa_negative_control_swapped_k_heads", within_2ulp=ok, exact=exact)
    assert ok < 0.999, ("swapped K heads NOT detected", ok)


# --------------------------------------------------------- per-op local checks
@pytest.mark.parametrize("tag", GQA_TAGS)
def test_native_per_op_local_checks(tag):
    """test_gpu_fulldepth.py's local view on the native model, a prefill and
    the decode step after it: the oracle's op on the GPU's own captured input
    -- the qkv GEMM at N = H + 2 Hkv against [wq; wk; wv] of the oracle, the
    attention of head h over K/V head h // G with the oracle's RoPE table (the
    llama3 one for the second fixture), both norms bit-exact."""
    cfg, g = O.load_golden(tag)
    prompt = g["prompt"].tolist()
    n, H, nh, nkv = len(prompt), cfg["hidden"], cfg["num_heads"], cfg["num_kv_heads"]
    d, G, eps, L = H // nh, nh // nkv, cfg["rms_eps"], cfg["num_layers"]
    Hkv = nkv * d
    om = O.Model(cfg, cfg["seed"], fp16=1, max_requests=1, max_seq=64)
    tab = O.rope_table(64, d, cfg["rope_theta"], llama3_of(cfg))
    scale = float(np.float32(1) / np.sqrt(np.float32(d)))
    names = ["attn_norm", "qkv", "attn_out", "o_proj", "ffn_norm"]
    m = fa.Model(cfg, "inc", weight_seed=cfg["seed"], native_gqa=True, **KW)
    cap = {}
    try:
        m.set_debug(True)
        for step, length in (("prefill", n + 1), ("decode", n + 2)):
            fa.generate(one_rm(), m, [prompt[1:]], max_length=length)
            for l in range(L):
                c = {op: m.debug_tensor(op, l) for op in names}
                c["res_in"] = m.debug_tensor("embed", 0) if l == 0 else m.debug_tensor("hidden", l - 1)
                cap[(step, l)] = c
    finally:
        m.close()
    for l in range(L):
        p = f"model.layers.{l}."
        wqkv = np.concatenate([om.weight(p + f"self_attn.{x}_proj.weight").reshape(-1, H)
                               for x in "qkv"])
        assert wqkv.shape == (H + 2 * Hkv, H)
        w_in = om.weight(p + "input_layernorm.weight")
        w_post = om.weight(p + "post_attention_layernorm.weight")
        pre, dec = cap[("prefill", l)], cap[("decode", l)]
        assert pre["qkv"].shape == (n, H + 2 * Hkv) and dec["qkv"].shape == (1, H + 2 * Hkv)
        qkv = np.concatenate([pre["qkv"], dec["qkv"]])  # positions 0 .. n
        qr = np.stack([rope_ref(qkv[t, :H], t, d, tab) for t in range(n + 1)])
        kr = np.stack([rope_ref(qkv[t, H:H + Hkv], t, d, tab) for t in range(n + 1)])
        vv = qkv[:, H + Hkv:]
        att = np.zeros((n + 1, H), np.float32)
        for h in range(nh):
            qs, ks = slice(h * d, (h + 1) * d), slice((h // G) * d, (h // G + 1) * d)
            for t in range(n + 1):
                att[t, qs] = O.attention_row(qr[t, qs], kr[:t + 1, ks], vv[:t + 1, ks],
                                             np.ones(t + 1, np.uint8), scale)
        for step, c, att_ref in (("prefill", pre, att[:n]), ("decode", dec, att[n:])):
            loc = {"attn_norm": O.rmsnorm(c["res_in"], w_in, eps),
                   "qkv": O.linear(c["attn_norm"], wqkv),
                   "attn_out": att_ref,
                   "ffn_norm": O.rmsnorm(O.round16(c["res_in"] + c["o_proj"]), w_post, eps)}
            for op, want in loc.items():
                st = within(c[op], want)
                print(tag, "layer", l, step, op, st)
                report("gqa_native_local_op", tag=tag, layer=l, step=step, op=op, **st)
                if op.endswith("norm"):
                    assert st["exact"] == 1.0, (l, step, op, st)
                assert st["within_2ulp"] >= 0.999, (l, step, op, st)


# --------------------------------------------- llama3 RoPE through an MHA model
def llama3_mha_case():
    cfg, _ = O.load_golden("tiny_d128")
    cfg = dict(cfg, rope_theta=500000.0, rope_llama3=1, rope_factor=8.0, rope_low_freq_factor=1.0,
               rope_high_freq_factor=4.0, rope_original_max_pos=64)
    rng = np.random.default_rng(3)
    # 40 positions: past the scaled pairs' first quarter turn at theta 5e5
    return cfg, [1] + rng.integers(3, cfg["vocab_size"], size=39).tolist()


@pytest.mark.parametrize("full_precision", [False, True])
def test_model_level_llama3_rope_on_an_mha_model(full_precision):
    """rope_llama3 through ffmi_model_create (llama_gpu.cpp / llama_f32.cpp
    hand it to their attention handles) on tiny_d128's shape: the fp16 model
    against the fp16 oracle, the fp32 model against the fp32 oracle.  The same
    model without the scaling misses both bars by orders (the scaled pairs
    turn 8 times slower)."""
    cfg, prompt = llama3_mha_case()
    seed, new = cfg["seed"], 16
    om = O.Model(cfg, seed, fp16=0 if full_precision else 1, max_requests=1, max_seq=128)
    plain = O.Model(dict(cfg, rope_llama3=0), seed, fp16=om.fp16, max_requests=1, max_seq=128)
    ref = om.forward(0, prompt, 0)
    assert np.abs(ref - plain.forward(0, prompt, 0)).max() > 1e-2  # the scaling matters here
    m = fa.Model(cfg, "inc", weight_seed=seed, full_precision=full_precision, **KW)
    try:
        lg = prefill_logits(m, prompt)
        toks = decode(m, prompt, new)
    finally:
        m.close()
    if full_precision:
        err = float(np.abs(lg - ref).max())
        print("llama3 fp32: max |logit error|", err)
        report("llama3_model_full_precision_vs_oracle", max_abs_err=err)
        assert err <= 1e-4, err
        check_fp32_picks(om, toks, len(prompt))
    else:
        ok, exact = close_ulp(lg, ref)
        print("llama3 fp16: within bar", ok, "bit-exact", exact)
        report("llama3_model_vs_oracle_fp16", within_2ulp=ok, exact=exact)
        assert ok >= 0.999, ok
        check_tokens_vs_oracle(cfg, seed, toks, len(prompt))


# ------------------------------------------- test_gpu_gqa_model.py's 8-over-2 model
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("gqa_oracle_ckpt"))
    GM.write_checkpoint(folder)  # the name-keyed stream at GQA size: O.Model(GM.CFG, GM.SEED)
    return folder


def test_spec_infer_over_native_gqa_against_the_oracle(ckpt):
    """Tree verification and the beam SSM over native K/V caches (the SSM the
    same checkpoint under the flag), widths (1,1,3): every pick teacher-forced
    through the oracle under parity_rules.assert_ties."""
    ps = GM.prompts()
    vt = 64 + 23 * 4
    kw = dict(max_requests=4, max_tokens=vt, max_seq_len=128, max_tree_tokens=23,
              weights_folder=ckpt, native_gqa=True)
    tree, ssm = fa.Model(GM.CFG, "tree", **kw), fa.Model(GM.CFG, "beam", **kw)
    r = fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                          max_sequence_length=128, spec_tree_width=(1, 1, 3),
                          max_spec_tree_token_num=23)
    r.register_ssm_model(ssm)
    try:
        res = fa.generate(r, tree, ps, max_length=GM.LEN, spec=True)
        steps = r.stats().llm_steps
    finally:
        tree.close()
        ssm.close()
    assert GM.NEW >= 1.5 * steps, steps  # the SSM is the LLM: paths are accepted
    check_all(GM.CFG, GM.SEED, ps, res, GM.LEN, "gqa_native_spec_infer")


def test_tp2_native_against_the_oracle(ckpt):
    """K/V heads 2 -> 1 per rank: every rank the same tokens, and those the
    oracle's under the TP tests' wider tie share (test_gpu_tp_local.py)."""
    ps = GM.prompts()
    out = GM.run_tp_native(ckpt, 2, ps)
    assert out[0] == out[1]
    for p, toks in zip(ps, out[0]):
        assert len(toks) == GM.LEN
        check_tokens_vs_oracle(GM.CFG, GM.SEED, toks, len(p) + 1, tie_ulp=4, max_tie_frac=0.1)


# ------------------------------------------------------------ random GQA models
def random_gqa_cfg(rng):
    """test_gpu_random_models.random_cfg (d 64 or 128, 1-3 layers) with
    num_kv_heads a proper divisor of num_heads (2, 4 or 8 query heads)"""
    cfg = random_cfg(rng)
    d = cfg["hidden"] // cfg["num_heads"]
    if cfg["num_heads"] == 1:
        cfg["num_heads"] = int(rng.choice([2, 4, 8]))
        cfg["hidden"] = cfg["num_heads"] * d
    nh = cfg["num_heads"]
    cfg["num_kv_heads"] = int(rng.choice([k for k in range(1, nh) if nh % k == 0]))
    return cfg


@pytest.mark.parametrize("seed", range(6))
def test_random_gqa_model_incr_decoding_vs_oracle(seed):
    rng = np.random.default_rng(9300 + seed)
    cfg = random_gqa_cfg(rng)
    msl = int(rng.choice([64, 128]))
    ps, ml = random_requests(rng, cfg["vocab_size"], msl)
    B = int(rng.choice([1, 2, 4, 8]))
    mtb = int(rng.choice([16, 32, 64, 128]))
    rm = fa.RequestManager(max_requests_per_batch=B, max_tokens_per_batch=mtb,
                           max_sequence_length=msl)
    m = fa.Model(cfg, "inc", max_requests=B, max_tokens=mtb, max_seq_len=msl,
                 weight_seed=600 + seed, native_gqa=True)
    try:
        res = fa.generate(rm, m, ps, max_length=ml)
    finally:
        m.close()
    check_all(cfg, 600 + seed, ps, res, ml, ("gqa", cfg, B, mtb))


@pytest.mark.parametrize("seed", range(6))
def test_random_gqa_model_spec_infer_vs_oracle(seed):
    """the SSM: the LLM's own shape and weights under the flag (long accepted
    paths over native caches), or a random smaller MHA model.  At most 4
    slots of up to 60-token prompts against a token budget of 64 or 128: the
    SSM loads every prompt within its init and beam batches."""
    rng = np.random.default_rng(9400 + seed)
    cfg = random_gqa_cfg(rng)
    V = cfg["vocab_size"]
    msl = int(rng.choice([64, 128]))
    ps, ml = random_requests(rng, V, msl)
    B = int(rng.choice([1, 2, 4]))
    mtb = int(rng.choice([64, 128]))
    widths = WIDTHS[int(rng.integers(0, len(WIDTHS) - 1))]  # (not incr decoding)
    tree = 33
    vt = mtb + tree * B
    rm = fa.RequestManager(max_requests_per_batch=B, max_tokens_per_batch=mtb,
                           max_sequence_length=msl, spec_tree_width=widths,
                           max_spec_tree_token_num=tree, spec_extensions=fa.ffmi.SPEC_EXT_WIDTH4)
    kw = dict(max_requests=B, max_tokens=vt, max_seq_len=msl, max_tree_tokens=tree)
    llm = fa.Model(cfg, "tree", weight_seed=700 + seed, native_gqa=True, **kw)
    if seed % 2 == 0:
        ssm = fa.Model(cfg, "beam", weight_seed=700 + seed, native_gqa=True, **kw)
    else:
        ssm = fa.Model(random_cfg(rng, vocab=V), "beam", weight_seed=800 + seed, **kw)
    rm.register_ssm_model(ssm)
    try:
        res = fa.generate(rm, llm, ps, max_length=ml, spec=True)
    finally:
        llm.close()
        ssm.close()
    check_all(cfg, 700 + seed, ps, res, ml, ("gqa", cfg, B, mtb, widths))
