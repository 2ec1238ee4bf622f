"""Vocab-sharded top-p sampling (ffmi_vocab_shard_sample_topp; the reference's
vocab-parallel lm_head + Combine, model.cc:3392-3419, feeding the sampling
tail of llama.cc:286-289) over rank processes of the xGMI transport: every
rank's pick is the numpy rule's (tests/sampling_rule.py) on the GATHERED logits
and ffmi_sample_topp's on them -- ids equal, probs bit-identical, the same on
every rank.  No tolerance anywhere.
"""
import os

import numpy as np
import pytest

import peer_sampling_tasks as ST
from peer_group import run_group

pytestmark = pytest.mark.gpu
RS = int(os.environ.get("FFMI_RANDOM_SCALE", "1"))
OFF = int(os.environ.get("FFMI_RANDOM_SEED_OFFSET", "0"))  # fresh seeds for one-off sweeps


def run(n, builder, args, env=None):
    return run_group(n, ST.vsample_task, (builder, args), env=env, max_bytes=1 << 20)


def check(res, what):
    """Sharded (every rank) == one-GPU kernel == numpy rule, per case; returns
    rank 0's per-case results."""
    n = len(res)
    for ci, ref in enumerate(res[0]):
        rid, rp = ref["ref_ids"], ref["ref_probs"]
        bad = np.nonzero(ref["one_ids"] != rid)[0]
        assert bad.size == 0, (what, ci, "one-GPU kernel", bad[:8], ref["one_ids"][bad[:8]], rid[bad[:8]])
        np.testing.assert_array_equal(ref["one_probs"].view(np.uint32), rp.view(np.uint32))
        for r in range(n):
            got = res[r][ci]
            bad = np.nonzero(got["ids"] != rid)[0]
            assert bad.size == 0, (what, ci, f"rank {r}", bad[:8], got["ids"][bad[:8]], rid[bad[:8]],
                                   ref["u"][bad[:8]])
            np.testing.assert_array_equal(got["probs"].view(np.uint32), rp.view(np.uint32),
                                          err_msg=f"{what} case {ci} rank {r}")
    return res[0]


@pytest.mark.parametrize("n,T,V", [(2, 1, 2), (2, 3, 126), (2, 3, 128), (2, 3, 130), (4, 3, 4092),
                                   (4, 3, 4096), (4, 3, 4100), (4, 37, 32000), (8, 24, 32000),
                                   (8, 5, 8)])
def test_vshard_sample_shapes_exact(n, T, V):
    """N(0, 3) logits under the four (temperature, topp) settings of
    tests/test_gpu_sampling.py, u on the 2^-24 grid with both ends: Vl = 1,
    either side of a wave and of the 1024 threads, LLaMA's 32000 at 4 and 8
    ranks (T = 37 at n = 4: more than one block), one token per rank at n = 8."""
    ref = check(run(n, "shape", (T, V)), (n, T, V))
    assert len(ref) == 4
    if T >= 2:
        assert ref[0]["u"][0] == np.float32(2.0 ** -24) and ref[0]["u"][-1] == 1.0


@pytest.mark.parametrize("n,V", [(4, 1000), (8, 32000)])
def test_vshard_sample_flat_row_walks_across_the_shards(n, V):
    """All logits equal: one key, so the owner / rank-remainder path decides
    alone, and the reference's own picks fall in at least 3 shards."""
    ref = check(run(n, "flat", (V,)), (n, V))[0]
    shards = set((ref["ref_ids"] // (V // n)).tolist())
    assert len(shards) >= 3, shards
    assert (np.diff(ref["ref_ids"]) >= 0).all()
    assert ref["ref_ids"][0] == 0 and ref["ref_ids"][-1] == V - 1


@pytest.mark.parametrize("n,T,V", [(2, 16, 512), (4, 16, 4096), (8, 16, 1024)])
def test_vshard_sample_cross_shard_ties(n, T, V):
    """Rows of near-equal logits whose fp16 p tie across the shards, and rows
    with the same maximum at 4 ids in different shards: the pick walks equal-p
    tokens in global index order as u grows."""
    ref = check(run(n, "tie", (T, V)), (n, T, V))
    x, ids = ref[0]["x"], ref[0]["ref_ids"]
    for t in range(0, T, 2):  # the planted maxima
        top = np.nonzero(x[t] == x[t].max())[0]
        assert len(set((top // (V // n)).tolist())) >= min(n, 4) and top.size >= 4
    # under (1, 1) the tied rows (odd t) are picked in more than one shard
    assert len(set((ids[1::2] // (V // n)).tolist())) >= 2


def test_vshard_sample_fallback_is_the_highest_id_of_the_lowest_p():
    """Rows whose whole fp16 mass stays below t = 1: the last token of the
    order, over the shards (sampling.cu:94)."""
    ref = check(run(2, "fallback", ()), "fallback")
    for c in ref:
        assert (c["mass"] < 1.0).all(), c["mass"]  # cumulative mass < t = (1 * 1) * 1
    assert ref[0]["ref_ids"].tolist() == [5] and ref[0]["ref_probs"].tolist() == [0.1666259765625]
    # three -inf ids (1, 3, 5) in both shards: the highest of them, not the row's last token
    assert ref[1]["ref_ids"].tolist() == [5] and ref[1]["ref_probs"].tolist() == [0.0]


@pytest.mark.parametrize("n,V", [(2, 8), (4, 16), (4, 4096)])
def test_vshard_sample_threshold_is_inclusive_at_a_shard_boundary(n, V):
    """Cumulative mass == t exactly at the last token of shard s's share of
    the key: that token, and one grid step above it the first of shard s + 1."""
    ref = check(run(n, "inclusive", (V,)), (n, V))[0]
    Vl = V // n
    want = [i for s in range(n - 1) for i in ((s + 1) * Vl - 1, (s + 1) * Vl)]
    assert ref["ref_ids"].tolist() == want


def test_vshard_sample_minus_inf_entries_are_not_picked():
    n, T, V = 4, 24, 3000
    ref = check(run(n, "minus_inf", (T, V)), "minus_inf")
    for c in ref:
        assert not np.isneginf(c["x"][np.arange(T), c["ref_ids"]]).any()
        assert ((c["ref_ids"] // (V // n)) != 1).all()  # shard 1 is -inf throughout


def test_vshard_sample_peaked_row():
    """One logit 200 above the rest, in shard 2 of 4: that token for every u."""
    ref = check(run(4, "peaked", (32, 5000, 2 * 1250 + 1071)), "peaked")[0]
    assert (ref["ref_ids"] == 2 * 1250 + 1071).all() and (ref["ref_probs"] == 1.0).all()


def test_vshard_sample_row_chunks():
    """FFMI_VSHARD_SAMPLE_CHUNK_ROWS = 2 at T = 5: three chunks, all phases
    per chunk, the results of the one-chunk run."""
    one = check(run(4, "shape", (5, 4096)), "one chunk")
    three = check(run(4, "shape", (5, 4096), env={"FFMI_VSHARD_SAMPLE_CHUNK_ROWS": "2"}), "chunks")
    for a, b in zip(one, three):
        assert np.array_equal(a["ids"], b["ids"])
        assert np.array_equal(a["probs"].view(np.uint32), b["probs"].view(np.uint32))


def test_vshard_sample_back_to_back_calls_share_a_scratch():
    """Two logit sets of different shapes through one scratch, the first again
    after the second: stale keys, state and records of a call do not leak."""
    ref = check(run(4, "two_set", (9, 2048)), "two sets")
    assert len(ref) == 3 and ref[0]["x"].shape != ref[1]["x"].shape
    assert np.array_equal(ref[0]["ids"], ref[2]["ids"])


@pytest.mark.parametrize("seed", range(8 * RS))
def test_vshard_sample_random_shapes_exact(seed):
    n = (2, 4, 8)[(seed + OFF) % 3]
    check(run(n, "random", (seed + OFF,)), ("random", n, seed + OFF))
