"""Rank tasks of tests/test_gpu_logprobs_model.py (run by tests/peer_group.py,
one process per rank): a tensor-parallel model with a vocab-sharded lm_head
refuses per-token log-probabilities.
"""
KW = dict(max_requests=4, max_tokens=64, max_seq_len=128, weight_seed=11)


def vshard_refusal_task(fa, comm, rank, n, cfg):
    """ffmi_model_set_logprobs on this rank's shard: its status and message,
    what Model.set_logprobs raises, and that the model still decodes."""
    import flexflow_amd.ffmi as F
    llm = fa.Model(cfg, "inc", tp_rank=rank, tp_size=n, comm=comm, **KW)
    st = F.lib().ffmi_model_set_logprobs(llm.handle, 1)
    msg = F.lib().ffmi_last_error().decode()
    try:
        llm.set_logprobs(True)
        raised = False
    except F.FFMIError:
        raised = True
    rm = fa.RequestManager(max_requests_per_batch=4, max_tokens_per_batch=64,
                           max_sequence_length=128)
    r = fa.generate(rm, llm, [[5, 17, 300, 42]], max_new_tokens=4)[0]
    return dict(status=st, message=msg, raised=raised, tokens=r.output_tokens,
                logprobs=r.logprobs)
