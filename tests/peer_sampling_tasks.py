"""Rank tasks of the vocab-sharded top-p sampling tests (tests/peer_group.py
run_group): ffmi_vocab_shard_sample_topp on each rank's shard, and on rank 0
ffmi_sample_topp and the numpy rule (tests/sampling_rule.py) on the gathered
logits.  Every rank builds the same cases from the same seeds."""
import numpy as np

NEG_INF = np.float16(-np.inf)
SETTINGS = [(1.0, 1.0), (0.7, 0.9), (2.0, 0.6), (0.9, 0.8)]  # tests/test_gpu_sampling.py's


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16)


def grid_uniforms(rng, n):
    import sampling_rule as R
    return R.grid_uniforms(rng, n)


# --- case builders: each returns [(x16 [T][V], temperature, topp, u [T])] ----


def shape_cases(n, T, V):
    """N(0, 3) logits under the four settings, u on the 2^-24 grid, ends included."""
    out = []
    for si, (temperature, topp) in enumerate(SETTINGS):
        rng = np.random.default_rng(V * 1009 + T * 17 + n * 5 + si)
        out.append((f16(rng.standard_normal((T, V)) * 3), temperature, topp, grid_uniforms(rng, T)))
    return out


def flat_cases(n, V):
    u = np.sort(grid_uniforms(np.random.default_rng(V + n), 64))
    return [(np.full((64, V), 0.25, np.float16), 1.0, 1.0, u)]


def tie_cases(n, T, V):
    """Rows of {0, 2^-14, 2^-13, 2^-12} (the fp16 softmax rounds many ids to one
    p) and rows with the same maximum at 4 ids in different shards; u sorted, so
    the pick walks equal-p tokens in global index order."""
    rng = np.random.default_rng(77 + n)
    Vl = V // n
    x = f16(rng.standard_normal((T, V)) * 3)
    for t in range(T):
        if t % 2:
            x[t] = f16(rng.choice([0.0, 2.0 ** -14, 2.0 ** -13, 2.0 ** -12], V))
        else:
            m = f16(float(x[t].max()) + 1.0)
            for s in rng.choice(n, min(n, 4), replace=False):  # (n = 2: two in each shard)
                x[t, s * Vl + rng.choice(Vl, 4 // min(n, 4), replace=False)] = m
    return [(x, temperature, topp, np.sort(grid_uniforms(rng, T))) for temperature, topp in
            ((1.0, 1.0), (0.9, 0.8))]


def fallback_cases(n):
    """Rows whose whole fp16 mass stays below t = 1 (u = topp = 1), with the
    lowest p tied in at least two shards (n = 2):
    six equal logits, p = 0.1666259765625 each (0.99975 in all): the last token;
    five equal logits and three -inf (p = 0.199951171875 each, 0.99976): the
    highest -inf id, 5, not the row's last token."""
    assert n == 2
    a = np.zeros((1, 6), np.float16)
    b = np.array([[0, -np.inf, 0, -np.inf, 0, -np.inf, 0, 0]], np.float16)
    return [(a, 1.0, 1.0, np.ones(1, np.float32)), (b, 1.0, 1.0, np.ones(1, np.float32))]


def inclusive_cases(n, V):
    """A flat row (every token the same key): u = the reference's cumulative
    mass at the last token of shard s, and one grid step above it."""
    import sampling_rule as R
    Vl = V // n
    row = np.zeros((1, V), np.float16)
    _, p = R.sorted_probs(R.scaled_logits(row, 1.0))
    C = np.cumsum(p[0].astype(np.float64))
    u = []
    for s in range(n - 1):
        c = C[(s + 1) * Vl - 1]
        assert np.float64(np.float32(c)) == c and c + 2.0 ** -24 < 1.0
        u += [c, c + 2.0 ** -24]
    u = np.array(u, np.float32)
    return [(np.repeat(row, u.size, axis=0), 1.0, 1.0, u)]


def minus_inf_cases(n, T, V):
    """Half of the entries -inf at random, and shard 1 entirely -inf."""
    rng = np.random.default_rng(7 + n)
    Vl = V // n
    x = f16(rng.standard_normal((T, V)) * 1.28)
    x[rng.random((T, V)) < 0.5] = NEG_INF
    x[:, Vl:2 * Vl] = NEG_INF
    # (topp < 1: t <= 0.81 stays below each row's mass, so no fallback)
    return [(x, temperature, topp, grid_uniforms(rng, T)) for temperature, topp in
            ((0.7, 0.9), (0.9, 0.8))]


def peaked_cases(n, T, V, at):
    rng = np.random.default_rng(5 + n)
    x = f16(rng.standard_normal((T, V)))
    x[:, at] = f16(200.0)
    return [(x, 1.0, 1.0, grid_uniforms(rng, T))]


def two_set_cases(n, T, V):
    """Two different logit sets of different shapes for one scratch."""
    a, b = shape_cases(n, T, V)[3], shape_cases(n, T - 2, V // 2)[1]
    return [a, b, a]


def random_cases(n, seed):
    """Random T (1-40) and Vl (1-5000), logit scales from flat to peaked, planted
    ties, some -inf entries, random settings."""
    rng = np.random.default_rng(8800 + seed)
    T, Vl = int(rng.integers(1, 41)), int(rng.choice([rng.integers(1, 70), rng.integers(1, 5001)]))
    V = n * Vl
    scale = float(rng.choice([1e-3, 0.05, 1.28, 3.0, 8.0]))
    x = f16(rng.standard_normal((T, V)) * scale)
    for t in rng.choice(T, size=min(T, 4), replace=False):
        m = f16(float(np.abs(x[t]).max()) + float(rng.choice([0.0, 0.5, 1.0])))
        x[t, rng.choice(V, size=min(V, int(rng.integers(2, 9))), replace=False)] = m
    if V > 8:
        for t in rng.choice(T, size=min(T, 3), replace=False):
            x[t, rng.random(V) < 0.3] = NEG_INF
            x[t, rng.integers(V)] = f16(1.0)  # (never a row of -inf only)
    temperature = float(rng.choice([0.3, 0.7, 0.9, 1.0, 1.5, 4.0]))
    topp = float(rng.choice([0.05, 0.3, 0.6, 0.8, 0.95, 1.0]))
    return [(x, temperature, topp, grid_uniforms(rng, T))]


BUILDERS = dict(shape=shape_cases, flat=flat_cases, tie=tie_cases, fallback=fallback_cases,
                inclusive=inclusive_cases, minus_inf=minus_inf_cases, peaked=peaked_cases,
                two_set=two_set_cases, random=random_cases)


def vsample_task(fa, comm, rank, n, builder, args):
    """Every case through ONE scratch, back to back (it starts as 0xff bytes:
    NaN records, out-of-range keys).  Returns per case this rank's ids / probs;
    rank 0 adds the one-GPU kernel's and the rule's on the gathered logits and
    each row's fp16 mass."""
    import flexflow_amd.ffmi as F
    from hip_util import Buf
    L = F.lib()
    cases = BUILDERS[builder](n, *args)
    nb = max(int(L.ffmi_vocab_shard_sample_scratch_bytes(n, x.shape[0], x.shape[1] // n))
             for x, _, _, _ in cases)
    scratch = Buf(np.full(nb, 0xff, np.uint8))
    out = []
    for x, temperature, topp, u in cases:
        T, V = x.shape
        Vl = V // n
        assert Vl * n == V
        shard = Buf(np.ascontiguousarray(x[:, rank * Vl:(rank + 1) * Vl]))
        ub = Buf(np.asarray(u, np.float32))
        ids, probs = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
        F.check(L.ffmi_vocab_shard_sample_topp(comm.handle, shard.ptr, T, Vl, temperature, topp,
                                               ub.ptr, ids.ptr, probs.ptr, scratch.ptr, nb, None),
                ("vocab shard sample", T, V, temperature, topp))
        res = {"ids": ids.get(), "probs": probs.get()}
        if rank == 0:
            import sampling_rule as R
            xb = Buf(np.ascontiguousarray(x))
            i1, p1 = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
            nw = int(L.ffmi_sample_topp_workspace_bytes(T, V))
            ws = Buf.empty((max(nw, 16),), np.uint8)
            F.check(L.ffmi_sample_topp(xb.ptr, T, V, temperature, topp, ub.ptr, i1.ptr, p1.ptr,
                                       ws.ptr, nw, None), "sample_topp")
            res["one_ids"], res["one_probs"] = i1.get(), p1.get()
            sid, sp = R.sorted_probs(R.scaled_logits(x, temperature))
            res["ref_ids"], res["ref_probs"] = R.pick(sid, sp, topp, u)
            res["mass"] = sp.astype(np.float64).sum(axis=1)
            res["x"], res["u"], res["topp"] = x, np.asarray(u, np.float32), topp
        out.append(res)
    return out


# --- model tasks (tests/test_gpu_vshard_sampling_model.py) --------------------

KW = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=11)
RM_KW = dict(max_requests_per_batch=4, max_tokens_per_batch=64, max_sequence_length=128)


def model_rule_task(fa, comm, rank, n, cfg, gc, seed, prompt, new_tokens):
    """One request, max_new_tokens in `new_tokens` under set_debug: per run the
    tokens, the guid and this rank's shard of the last row of the logits."""
    llm = fa.Model(cfg, "inc", tp_rank=rank, tp_size=n, comm=comm,
                   generation_config=fa.GenerationConfig(**gc), sampling_seed=seed, **KW)
    llm.set_debug(True)
    out = []
    for m in new_tokens:
        r = fa.generate(fa.RequestManager(**RM_KW), llm, [prompt], max_new_tokens=m)[0]
        out.append({"tokens": r.output_tokens, "guid": r.guid,
                    "logits": llm.debug_tensor("logits")[-1:].astype(np.float16)})
    llm.close()
    return out


def model_seed_task(fa, comm, rank, n, cfg, prompts, new_tokens, seeds):
    """The tokens of one model under each seed in turn (graphs on)."""
    llm = fa.Model(cfg, "inc", tp_rank=rank, tp_size=n, comm=comm, **KW)
    out = []
    for seed in seeds:
        llm.set_sampling(fa.GenerationConfig(do_sample=True), seed=seed)
        out.append([r.output_tokens for r in fa.generate(fa.RequestManager(**RM_KW), llm, prompts,
                                                         max_new_tokens=new_tokens)])
    llm.close()
    return out


def model_greedy_task(fa, comm, rank, n, cfg, prompts, new_tokens):
    """greedy, topp = 2^-6 sampling, default sampling, greedy again; then the
    logit shard of every step of request 0 under the small topp."""
    import flexflow_amd.ffmi as F
    llm = fa.Model(cfg, "inc", tp_rank=rank, tp_size=n, comm=comm, **KW)

    def run(ps, m):
        return [r.output_tokens for r in fa.generate(fa.RequestManager(**RM_KW), llm, ps,
                                                     max_new_tokens=m)]

    out = {"greedy": run(prompts, new_tokens)}
    small = fa.GenerationConfig(do_sample=True, temperature=1.0, topp=2.0 ** -6)
    out["status"] = int(F.lib().ffmi_model_set_sampling(llm.handle, 1, 1.0, 2.0 ** -6, 3))
    out["small"] = run(prompts, new_tokens)
    llm.set_sampling(fa.GenerationConfig(do_sample=True), seed=3)
    out["sampled"] = run(prompts, new_tokens)
    llm.set_sampling(None)
    out["greedy_again"] = run(prompts, new_tokens)
    llm.set_sampling(small, seed=3)
    llm.set_debug(True)
    out["steps"] = []
    for m in range(2, new_tokens + 1):
        toks = run(prompts[:1], m)[0]
        out["steps"].append((toks, llm.debug_tensor("logits")[-1:].astype(np.float16)))
    llm.close()
    return out
