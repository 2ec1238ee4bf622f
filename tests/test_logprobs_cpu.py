"""Per-token log-probabilities without a device: the refusals of
ffmi_token_logprobs (decided before any HIP call) and the scheduler's
bookkeeping on the hash test double, whose value for a row is a pure function
of the row's context hash and the scored id -- so incremental decoding and
SpecInfer must record bit-equal values, and any bookkeeping error (a wrong row,
a wrong target, a value that does not follow its token) changes one.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F

M64 = (1 << 64) - 1
V = 1000
W4 = F.SPEC_EXT_WIDTH4


# ---- the kernel entry point's refusals -------------------------------------
def test_token_logprobs_refusals_need_no_device():
    L = F.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call is refused first
    n = int(L.ffmi_token_logprobs_workspace_bytes(4, 32000))
    assert n >= 4 * 8 * 8

    def call(logits=p, T=4, V=32000, temperature=0.0, targets=p, picks=p, out=p, ws=p, nbytes=n):
        return L.ffmi_token_logprobs(logits, T, V, temperature, targets, picks, out, ws, nbytes, None)

    for bad in (dict(T=-1), dict(V=0), dict(V=-5), dict(logits=None), dict(out=None),
                dict(targets=None, picks=None), dict(temperature=-0.5),
                dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(ws=None), dict(nbytes=n - 1), dict(nbytes=0)):
        assert call(**bad) == 1, bad  # FFMI_ERR_INVALID
    big = int(L.ffmi_token_logprobs_workspace_bytes(1, 983041))
    assert call(T=1, V=983041, nbytes=big, ws=p) == 5  # FFMI_ERR_UNSUPPORTED
    # the largest row is taken as far as the argument checks go: with T == 0
    # nothing is launched
    assert call(T=0, V=983040, ws=None, nbytes=0) == 0
    assert call(T=0) == 0
    assert int(L.ffmi_token_logprobs_workspace_bytes(0, 32000)) == 0


# ---- the hash rule, restated (tests/test_scheduler.py's expected()) ----------
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ctx_hash(ctx):
    h = 0x243F6A8885A308D3
    for t in ctx:
        h = mix64((h + t + 1) & M64)
    return h


def hash_logprob(ctx, tok):
    x = mix64(ctx_hash(ctx) ^ (((tok + 1) * 0x9E3779B97F4A7C15) & M64))
    return -float((x >> 40) + 1) * 2.0 ** -24


def expected(prompt, max_length, bos=1, eos=()):
    """(tokens, logprobs) of plain greedy decoding of the hash LM."""
    toks = [bos] + list(prompt)
    while len(toks) < max_length:
        toks.append((ctx_hash(toks) >> 17) % V)
        if toks[-1] in eos:
            toks.pop()
            break
    return toks, [None] + [hash_logprob(toks[:i], toks[i]) for i in range(1, len(toks))]


def prompts(n, lo=3, hi=40, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, V, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


def run_incr(ps, max_length, batch=4, max_tokens=16, eos=(), msl=160, logprobs=True):
    rm = fa.RequestManager(max_requests_per_batch=batch, max_tokens_per_batch=max_tokens,
                           max_sequence_length=msl, eos_token_ids=eos)
    llm = fa.HashModel(V, "inc", max_requests=batch, max_seq_len=msl)
    if logprobs:
        llm.set_logprobs(True)
    return fa.generate(rm, llm, ps, max_length=max_length)


def run_spec(ps, max_length, batch=4, max_tokens=64, widths=(1, 1, 3), disagree=0, tree_tokens=23,
             ext=0, eos=(), msl=160, logprobs=True):
    rm = fa.RequestManager(max_requests_per_batch=batch, max_tokens_per_batch=max_tokens,
                           max_sequence_length=msl, spec_tree_width=widths,
                           max_spec_tree_token_num=tree_tokens, spec_extensions=ext,
                           eos_token_ids=eos)
    llm = fa.HashModel(V, "tree", max_requests=batch, max_seq_len=msl, max_tree_tokens=tree_tokens)
    if logprobs:
        llm.set_logprobs(True)
    rm.register_ssm_model(fa.HashModel(V, "beam", max_requests=batch, max_seq_len=msl,
                                       max_tree_tokens=tree_tokens, salt=1234,
                                       disagree_pct=disagree))
    return fa.generate(rm, llm, ps, max_length=max_length)


def check(res, ps, max_length, eos=()):
    for p, r in zip(ps, res):
        toks, lps = expected(p, max_length, eos=eos)
        assert r.output_tokens == toks
        assert r.logprobs is not None and len(r.logprobs) == len(r.output_tokens)
        assert r.logprobs[0] is None
        assert r.logprobs == lps  # exact: every value is a multiple of 2^-24 in [-1, 0)


def test_hash_rule_values_are_exact_floats():
    lp = hash_logprob([1, 5, 9], 17)
    assert -1.0 <= lp <= -2.0 ** -24 and float(np.float32(lp)) == lp


# ---- incremental decoding ------------------------------------------------------
@pytest.mark.parametrize("batch,max_tokens", [(1, 8), (4, 16), (3, 5)])
def test_incr_logprobs_are_the_rule_on_every_position(batch, max_tokens):
    """Prompt tokens (explicit targets, prompts longer than max_tokens load in
    chunks: the last row of a chunk scores the next chunk's first token) and
    generated tokens (the pick's value), more requests than slots."""
    ps = prompts(7)
    check(run_incr(ps, 70, batch=batch, max_tokens=max_tokens), ps, 70)


def test_incr_dropped_eos_takes_its_value_with_it():
    ps = prompts(4, seed=3)
    full, _ = expected(ps[0], 70)
    eos = full[len(ps[0]) + 6]
    res = run_incr(ps, 70, eos=(eos,))
    check(res, ps, 70, eos=(eos,))
    assert len(res[0].output_tokens) < 70  # (it did stop there)


# ---- SpecInfer == incremental decoding ---------------------------------------
@pytest.mark.parametrize("disagree", [0, 30, 100])
@pytest.mark.parametrize("widths,ext", [((1, 1, 3), 0), ((1, 1, 4), W4), ((2, 2), W4)])
def test_spec_infer_logprobs_equal_incr(widths, ext, disagree):
    ps = prompts(6, seed=11)
    spec = run_spec(ps, 90, widths=widths, ext=ext, disagree=disagree,
                    tree_tokens=32 if ext else 23)
    incr = run_incr(ps, 90)
    for a, b in zip(spec, incr):
        assert a.output_tokens == b.output_tokens
        assert a.logprobs == b.logprobs and a.logprobs[0] is None
    check(spec, ps, 90)


@pytest.mark.parametrize("disagree", [0, 30, 100])
def test_spec_infer_logprobs_chunked_prompts_and_queued_requests(disagree):
    """More requests than slots, prompts longer than max_tokens_per_batch."""
    ps = prompts(9, lo=30, hi=60, seed=5)
    spec = run_spec(ps, 100, batch=3, max_tokens=24, disagree=disagree)
    incr = run_incr(ps, 100, batch=3, max_tokens=24)
    for a, b in zip(spec, incr):
        assert a.output_tokens == b.output_tokens and a.logprobs == b.logprobs
    check(spec, ps, 100)


@pytest.mark.parametrize("max_length", [41, 44, 47, 50])
def test_spec_infer_max_length_cut_leaves_no_value_beyond_the_tokens(max_length):
    """A perfect SSM: the last verify accepts up to 9 tokens, of which only
    those below max_length are kept -- and only their values."""
    ps = prompts(3, lo=20, hi=30, seed=2)
    res = run_spec(ps, max_length, disagree=0)
    check(res, ps, max_length)
    for r in res:
        assert len(r.output_tokens) == max_length == len(r.logprobs)


def test_spec_infer_dropped_eos():
    ps = prompts(4, seed=3)
    full, _ = expected(ps[0], 70)
    eos = full[len(ps[0]) + 6]
    inc = run_incr(ps, 70, eos=(eos,))
    spec = run_spec(ps, 70, eos=(eos,), disagree=30)
    for a, b in zip(spec, inc):
        assert len(a.logprobs) == len(a.output_tokens)
        # (SpecInfer checks EOS per verify step, so it may run past one; what
        # both produced carries the same values)
        n = min(len(a.output_tokens), len(b.output_tokens))
        assert a.output_tokens[:n] == b.output_tokens[:n] and a.logprobs[:n] == b.logprobs[:n]


# ---- off, and the SSM ------------------------------------------------------------
def test_off_gives_none_and_the_same_tokens():
    ps = prompts(5, seed=9)
    for run in (run_incr, run_spec):
        on, off = run(ps, 60), run(ps, 60, logprobs=False)
        for a, b in zip(on, off):
            assert b.logprobs is None and a.logprobs is not None
            assert a.output_tokens == b.output_tokens


def test_toggling_off_again_stops_recording():
    ps = prompts(2, seed=4)
    rm = fa.RequestManager(max_requests_per_batch=2, max_tokens_per_batch=16,
                           max_sequence_length=160)
    llm = fa.HashModel(V, "inc", max_requests=2, max_seq_len=160)
    llm.set_logprobs(True)
    assert all(r.logprobs is not None for r in fa.generate(rm, llm, ps, max_length=50))
    llm.set_logprobs(False)
    assert all(r.logprobs is None for r in fa.generate(rm, llm, ps, max_length=50))


def test_set_logprobs_on_an_ssm_is_unsupported():
    ssm = fa.HashModel(V, "beam", max_requests=2, max_seq_len=64)
    assert F.lib().ffmi_model_set_logprobs(ssm.handle, 1) == 5  # FFMI_ERR_UNSUPPORTED
    assert b"logprobs" in F.lib().ffmi_last_error()
    with pytest.raises(F.FFMIError):
        ssm.set_logprobs(True)


def test_get_logprobs_c_accessor():
    """Entry 0 is 0.0 in C; the count is returned whatever cap is; an unknown
    guid is -1; nothing recorded is 0."""
    rm = fa.RequestManager(max_requests_per_batch=2, max_tokens_per_batch=16,
                           max_sequence_length=160)
    llm = fa.HashModel(V, "inc", max_requests=2, max_seq_len=160)
    L = F.lib()
    g0 = rm.register_new_request([5, 6, 7], max_length=12)
    rm.serve_incr_decoding(llm)
    assert L.ffmi_rm_get_logprobs(rm.handle, g0, None, 0) == 0
    llm.set_logprobs(True)
    g1 = rm.register_new_request([5, 6, 7], max_length=12)
    rm.serve_incr_decoding(llm)
    buf = (ctypes.c_float * 12)()
    assert L.ffmi_rm_get_logprobs(rm.handle, g1, buf, 3) == 12
    assert buf[0] == 0.0 and buf[1] < 0 and buf[2] < 0 and buf[3] == 0.0  # (cap 3)
    assert L.ffmi_rm_get_logprobs(rm.handle, 12345, buf, 12) == -1
