"""Models with native grouped-query attention (Model(..., native_gqa=True):
K/V projections, the qkv GEMM and the KV cache at num_kv_heads).

The model: 2 layers, V 1000, H 512, 8 query heads over 2 K/V heads (d 64), a
reference-format checkpoint written with convert_hf_model as
test_gpu_checkpoint.py writes one.  These tests are differential: the
references are the default load of the same checkpoint (K/V replicated to
every query head, the reference's layout, pinned by test_gpu_checkpoint.py)
and, for the attention alone, the oracle's attention_row on the model's own
captured qkv -- route equality and cache sizes, which the oracle cannot see.
The oracle's own GQA model (HF-pinned on tests/golden/tiny_gqa_d64) checks
this model, its TP split and SpecInfer over it in test_gpu_gqa_oracle.py.  Between the replicated and the native model only the qkv GEMM's N
differs (1536 against 768 columns), so its launch plan -- the order of its
fp32 sums -- may differ; every other op sees the same shapes.
"""
import threading

import numpy as np
import pytest

import flexflow_amd as fa
import oracle_lib as O
from hip_util import report, ulp_diff
from parity_rules import assert_ties, classify
from test_gpu_e2e import SSM_CFG
from test_gpu_fulldepth import rope_ref, within

pytestmark = pytest.mark.gpu

CFG = dict(num_layers=2, vocab_size=1000, num_heads=8, num_kv_heads=2, hidden=512,
           intermediate=1024, rms_eps=1e-6, rope_theta=10000.0)
SEED, P, NEW = 47, 12, 32
LEN = P + 1 + NEW  # BOS + prompt + generated
KW = dict(max_requests=4, max_tokens=256, max_seq_len=128)


def prompts():
    rng = np.random.default_rng(5)
    return [rng.integers(3, CFG["vocab_size"], size=P).tolist() for _ in range(3)]


def write_checkpoint(folder):
    H, F, V, L = CFG["hidden"], CFG["intermediate"], CFG["vocab_size"], CFG["num_layers"]
    Hkv = CFG["num_kv_heads"] * (H // CFG["num_heads"])
    names = [("model.embed_tokens.weight", (V, H), 0), ("model.norm.weight", (H,), 1),
             ("lm_head.weight", (V, H), 0)]
    for l in range(L):
        p = f"model.layers.{l}."
        names += [(p + "input_layernorm.weight", (H,), 1),
                  (p + "post_attention_layernorm.weight", (H,), 1),
                  (p + "self_attn.q_proj.weight", (H, H), 0),
                  (p + "self_attn.k_proj.weight", (Hkv, H), 0),
                  (p + "self_attn.v_proj.weight", (Hkv, H), 0),
                  (p + "self_attn.o_proj.weight", (H, H), 0),
                  (p + "mlp.gate_proj.weight", (F, H), 0), (p + "mlp.up_proj.weight", (F, H), 0),
                  (p + "mlp.down_proj.weight", (H, F), 0)]
    st = {n: O.gen_weight(n, SEED, kind, int(np.prod(shape))).reshape(shape)
          for n, shape, kind in names}
    fa.convert_hf_model(st, folder)


def rm(**kw):
    return fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=256,
                             max_sequence_length=128, **kw)


def decode(m, ps, length=LEN, **kw):
    return [r.output_tokens for r in fa.generate(rm(**kw), m, ps, max_length=length)]


def teacher_forced(m, seqs):
    """logits [len(seqs)][n][V] of m along equal-length sequences: one prefill
    under set_debug (it is the step's last, so its capture stays)"""
    n = len(seqs[0])
    assert all(len(s) == n for s in seqs) and n * len(seqs) <= 256
    m.set_debug(True)
    fa.generate(rm(), m, [s[1:] for s in seqs], max_length=n + 1)
    lg = m.debug_tensor("logits")
    m.set_debug(False)
    return lg.reshape(len(seqs), n, -1)


def first_divergence(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def compare_runs(ref_seqs, ref_logits, new_seqs, new_logits, name):
    """new_seqs against ref_seqs: equal, or the first divergence of a sequence
    (later picks follow another prefix) is a tie by parity_rules.classify on
    the teacher-forced rows of the two models at that position, the reference
    model's row as the reference and the other's as the reordered run; at
    most tie_budget of them over the compared picks."""
    verdicts, total = [], 0
    for r, (a, b) in enumerate(zip(ref_seqs, new_seqs)):
        assert len(a) == len(b)
        i = first_divergence(a, b)
        assert i >= P + 1, "the prompts differ"
        total += i - (P + 1) + (i < len(a))
        if i < len(a):
            row1 = None if new_logits is None else new_logits[r, i - 1]
            verdicts.append(dict(classify(ref_logits[r, i - 1], row1, b[i], a[i]), req=r, pos=i))
    report(name, identical=len(ref_seqs) - len(verdicts), requests=len(ref_seqs),
           verdicts=verdicts, picks=total)
    print(name, "identical", len(ref_seqs) - len(verdicts), "of", len(ref_seqs), verdicts)
    assert_ties(verdicts, total)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("gqa_ckpt"))
    write_checkpoint(folder)
    return folder


@pytest.fixture(scope="module")
def base(ckpt):
    """the replicated and the native incremental-decoding runs of the three
    prompts, and both models' teacher-forced logits along the replicated
    run's sequences; the native model stays open for the tests below"""
    ps = prompts()
    rep = fa.Model(CFG, "inc", weights_folder=ckpt, **KW)
    nat = fa.Model(CFG, "inc", weights_folder=ckpt, native_gqa=True, **KW)
    out = dict(prompts=ps, rep=decode(rep, ps), nat=decode(nat, ps), model=nat)
    assert all(len(s) == LEN for s in out["rep"] + out["nat"])
    out["rep_tf"] = teacher_forced(rep, out["rep"])
    out["nat_tf"] = teacher_forced(nat, out["rep"])
    out["nat_tf_own"] = (out["nat_tf"] if out["nat"] == out["rep"]
                         else teacher_forced(nat, out["nat"]))
    out["bytes"] = (rep.kv_cache_bytes(), nat.kv_cache_bytes())
    rep.close()
    yield out
    nat.close()


def test_native_logits_and_tokens_against_the_replicated_load(base):
    d = np.abs(base["nat_tf"] - base["rep_tf"])
    frac = float((d <= 2e-3).mean())
    print("teacher-forced logits: within 2e-3", frac, "max", float(d.max()))
    report("gqa_native_vs_replicated_logits", within_2e3=frac, max_abs=float(d.max()))
    assert frac >= 0.999, (frac, float(d.max()))
    compare_runs(base["rep"], base["rep_tf"], base["nat"], base["nat_tf"],
                 "gqa_native_vs_replicated_tokens")
    assert base["bytes"][1] * 4 == base["bytes"][0]  # 2 of 8 heads cached


def test_native_attention_local_check(base):
    """The oracle's attention on the native model's own captured qkv, both
    layers, a prefill (13 rows) and the decode step after it: head h over the
    K/V of head h // 4; test_gpu_fulldepth.py's local check and its bar (2
    fp16 ulp on >= 99.9% of the elements)."""
    m, p0 = base["model"], base["prompts"][0]
    n, H, d, G = P + 1, CFG["hidden"], 64, 4
    Hkv = CFG["num_kv_heads"] * d
    tab = O.rope_table(64, d, CFG["rope_theta"])
    scale = float(np.float32(1) / np.sqrt(np.float32(d)))
    cap = {}
    m.set_debug(True)
    for step, length in (("prefill", n + 1), ("decode", n + 2)):
        one = fa.RequestManager(max_requests_per_batch=1, max_tokens_per_batch=32,
                                max_sequence_length=128)
        fa.generate(one, m, [p0], max_length=length)
        for l in range(CFG["num_layers"]):
            cap[(step, l)] = (m.debug_tensor("qkv", l), m.debug_tensor("attn_out", l))
    m.set_debug(False)
    for l in range(CFG["num_layers"]):
        qkv_p, att_p = cap[("prefill", l)]
        qkv_d, att_d = cap[("decode", l)]
        assert qkv_p.shape == (n, H + 2 * Hkv) and qkv_d.shape == (1, H + 2 * Hkv)
        qkv = np.concatenate([qkv_p, qkv_d])  # positions 0 .. n
        qr = np.stack([rope_ref(qkv[t, :H], t, d, tab) for t in range(n + 1)])
        kr = np.stack([rope_ref(qkv[t, H:H + Hkv], t, d, tab) for t in range(n + 1)])
        vv = qkv[:, H + Hkv:]
        ref = np.zeros((n + 1, H), np.float32)
        for h in range(CFG["num_heads"]):
            qs, ks = slice(h * d, (h + 1) * d), slice((h // G) * d, (h // G + 1) * d)
            for t in range(n + 1):
                ref[t, qs] = O.attention_row(qr[t, qs], kr[:t + 1, ks], vv[:t + 1, ks],
                                             np.ones(t + 1, np.uint8), scale)
        for name, got, want in (("prefill", att_p, ref[:n]), ("decode", att_d, ref[n:])):
            st = within(got, want)
            print("local attention, layer", l, name, st)
            report("gqa_native_local_attention", layer=l, step=name, **st)
            assert st["within_2ulp"] >= 0.999, (l, name, st)


@pytest.mark.parametrize("draft", ["mha_small", "native_same"])
def test_spec_infer_under_the_flag_equals_incremental_decoding(base, ckpt, draft):
    """test_gpu_e2e.py's rule: identical, or the first divergence is a tie of
    the two tokens' fp16 probabilities within 2 ulp -- on the flagged
    incremental model's own teacher-forced row (the oracle checks every pick
    of this configuration in test_gpu_gqa_oracle.py).
    The SSM: test_gpu_e2e.py's MHA one, or (native_same) the LLM's own
    checkpoint as a BEAM model under the flag, which then has to predict the
    LLM's picks: at least 1.5 tokens per verify step on average, the bar of
    test_spec_infer_equals_incr_on_gpu for an SSM equal to the LLM."""
    ps = base["prompts"]
    vt = 64 + 23 * 4
    tree = fa.Model(CFG, "tree", max_requests=4, max_tokens=vt, max_seq_len=128,
                    max_tree_tokens=23, weights_folder=ckpt, native_gqa=True)
    if draft == "mha_small":
        ssm = fa.Model(SSM_CFG, "beam", max_requests=4, max_tokens=vt, max_seq_len=128,
                       max_tree_tokens=23, weight_seed=5)
    else:
        ssm = fa.Model(CFG, "beam", max_requests=4, max_tokens=vt, max_seq_len=128,
                       max_tree_tokens=23, weights_folder=ckpt, native_gqa=True)
    r = fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                          max_sequence_length=128, spec_tree_width=(1, 1, 3),
                          max_spec_tree_token_num=23)
    r.register_ssm_model(ssm)
    spec = [x.output_tokens for x in fa.generate(r, tree, ps, max_length=LEN, spec=True)]
    steps = r.stats().llm_steps
    print("SpecInfer under the flag:", draft, "verify steps", steps, "for", NEW, "new tokens")
    if draft == "native_same":
        assert NEW >= 1.5 * steps, steps  # (every request decodes NEW tokens in `steps` steps)
    tree.close()
    ssm.close()
    same = 0
    for k, (a, b) in enumerate(zip(base["nat"], spec)):
        assert len(a) == len(b)
        if a == b:
            same += 1
            continue
        i = first_divergence(a, b)
        assert i >= P + 1
        row = base["nat_tf_own"][k, i - 1]
        pr = np.exp(row - row.max())
        p16 = (pr / pr.sum()).astype(np.float16)
        assert ulp_diff(p16[a[i]], p16[b[i]]) <= 2, (k, i)
    report("gqa_native_spec_equals_incr", draft=draft, identical=same, requests=len(ps),
           llm_steps=steps)


def run_tp_native(ckpt, tp, ps):
    """test_gpu_tp_local.py's harness: the shards as host threads over an
    in-process group, every model created with the flag"""
    comms = fa.Comm.local_group(tp)
    models = []
    try:
        for r in range(tp):
            models.append(fa.Model(CFG, "inc", max_requests=4, max_tokens=64, max_seq_len=128,
                                   weights_folder=ckpt, native_gqa=True, tp_rank=r, tp_size=tp,
                                   comm=comms[r]))
        rms = [fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                                 max_sequence_length=128) for _ in range(tp)]
        out, err = [None] * tp, []

        def work(r):
            try:
                fa.set_device(0)
                out[r] = [x.output_tokens
                          for x in fa.generate(rms[r], models[r], ps, max_length=LEN)]
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
    finally:
        for m in models:
            m.close()
        for c in comms:
            c.close()


def test_tp2_native_against_tp1_native(base, ckpt):
    """K/V heads 2 -> 1 per rank.  Every rank the same tokens; against the
    TP 1 native run equal, or ties on its teacher-forced rows (no second row:
    the shards' logits are not captured)."""
    out = run_tp_native(ckpt, 2, base["prompts"])
    assert out[0] == out[1]
    compare_runs(base["nat"], base["nat_tf_own"], out[0], None, "gqa_native_tp2_vs_tp1")


def test_tp4_native_is_refused_by_name(ckpt):
    with pytest.raises(fa.ffmi.FFMIError, match="native_gqa"):
        run_tp_native(ckpt, 4, prompts())


def test_full_precision_with_native_gqa_is_refused(ckpt):
    with pytest.raises(fa.ffmi.FFMIError, match="unsupported"):
        fa.Model(CFG, "inc", weights_folder=ckpt, native_gqa=True, full_precision=True, **KW)


def test_synthetic_gqa_needs_the_flag():
    with pytest.raises(fa.ffmi.FFMIError, match="unsupported"):
        fa.Model(CFG, "inc", weight_seed=3, **KW)


LLAMA3_8B_1L = dict(num_layers=1, vocab_size=32000, num_heads=32, num_kv_heads=8, hidden=4096,
                    intermediate=14336, rms_eps=1e-5, rope_theta=500000.0)


def test_synthetic_llama3_8b_widths_graphs_and_cache_size(monkeypatch):
    """One layer at Llama-3-8B widths, seeded synthetic weights (k/v from the
    name-keyed generator at their GQA size): a prefill and 8 decode steps of 4
    requests; two runs agree, graph replay agrees with eager steps, and the KV
    cache is a quarter of the 32-head MHA model's."""
    rng = np.random.default_rng(8)
    ps = [rng.integers(3, 32000, size=10).tolist() for _ in range(4)]
    kw = dict(max_requests=4, max_tokens=64, max_seq_len=64, weight_seed=80)

    def run():
        m = fa.Model(LLAMA3_8B_1L, "inc", native_gqa=True, **kw)
        r = fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                              max_sequence_length=64)
        toks = [x.output_tokens for x in fa.generate(r, m, ps, max_length=11 + 9)]
        steps, nbytes = r.stats().llm_steps, m.kv_cache_bytes()
        m.close()
        return toks, steps, nbytes

    a, steps, nbytes = run()
    assert steps >= 9 and all(len(t) == 20 for t in a), steps  # the prefill + 8 decode steps
    assert run()[0] == a
    monkeypatch.setenv("FFMI_NO_GRAPHS", "1")
    assert run()[0] == a
    mha = fa.Model(dict(LLAMA3_8B_1L, num_kv_heads=32), "inc", **kw)
    assert mha.kv_cache_bytes() == 4 * nbytes == 2 * 4 * 32 * 64 * 128 * 2
    mha.close()
