"""Top-p sampling kernel (ffmi_sample_topp; llama.cc:286-289, sampling.cu)
against the numpy restatement of its rule on the oracle's fp16 softmax
(tests/sampling_rule.py): ids exact, probs bit-identical.
"""
import os

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import oracle_lib as O
import sampling_rule as R
from hip_util import Buf, f16

pytestmark = pytest.mark.gpu
RS = int(os.environ.get("FFMI_RANDOM_SCALE", "1"))
OFF = int(os.environ.get("FFMI_RANDOM_SEED_OFFSET", "0"))  # fresh seeds for one-off sweeps
L = F.lib()
NEG_INF = np.float16(-np.inf)
SETTINGS = [(1.0, 1.0), (0.7, 0.9), (2.0, 0.6), (0.9, 0.8)]


def gpu_sample(x16, temperature, topp, u):
    x16 = np.ascontiguousarray(x16, np.float16)
    T, V = x16.shape
    lb, ub = Buf(x16), Buf(np.asarray(u, np.float32))
    ids, pr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    n = int(L.ffmi_sample_topp_workspace_bytes(T, V))
    ws = Buf.empty((max(n, 16),), np.uint8)
    F.check(L.ffmi_sample_topp(lb.ptr, T, V, temperature, topp, ub.ptr, ids.ptr, pr.ptr, ws.ptr, n,
                               None), (T, V, temperature, topp))
    return ids.get(), pr.get()


def check(x16, temperature, topp, u, what=None):
    ids, pr = gpu_sample(x16, temperature, topp, u)
    rid, rp = R.sample(x16, temperature, topp, u)
    bad = np.nonzero(ids != rid)[0]
    assert bad.size == 0, (what, bad[:8], ids[bad[:8]], rid[bad[:8]], np.asarray(u)[bad[:8]])
    np.testing.assert_array_equal(pr.view(np.uint32), rp.view(np.uint32))
    return ids, pr


@pytest.mark.parametrize("temperature,topp", SETTINGS)
@pytest.mark.parametrize("T", [1, 3, 24, 257])
@pytest.mark.parametrize("V", [1, 2, 7, 8, 9, 63, 64, 65, 1000, 1023, 1024, 1025, 8184, 8192, 8200,
                               32000, 32001, 32768, 32776, 65536, 140000])
def test_sample_topp_shapes_exact(V, T, temperature, topp):
    """Logits N(0, 1.28) (the bench model's spread), u on the 2^-24 grid with
    both ends, every vocabulary size around the workgroup width, the 16-byte
    vector, the register-resident limit and above."""
    rng = np.random.default_rng(V * 1009 + T * 17 + int(temperature * 10))
    x = f16(rng.standard_normal((T, V)) * 1.28)
    check(x, temperature, topp, R.grid_uniforms(rng, T), (V, T, temperature, topp))


def test_sample_topp_fallback_takes_the_last_token():
    """V = 3, equal logits, topp = u = 1: the row's mass 3 * 0.333251953125 =
    0.999755859375 stays below t = 1, so the pick is the last token of the
    order (sampling.cu:94)."""
    ids, pr = check(np.zeros((1, 3), np.float16), 1.0, 1.0, [1.0])
    assert ids.tolist() == [2] and pr.tolist() == [0.333251953125]
    # with a -inf entry behind them (p = 0) that entry is the last of the order
    x = np.array([[0, 0, 0, -np.inf]], np.float16)
    ids, pr = check(x, 1.0, 1.0, [1.0])
    assert ids.tolist() == [3] and pr.tolist() == [0.0]


def test_sample_topp_threshold_is_inclusive():
    """V = 4, equal logits (p = 0.25 each): C_1 = 0.5 = t picks token 1, one
    grid step above picks token 2; topp = 0.5, u = 1: t = 0.25 = C_0."""
    x = np.zeros((2, 4), np.float16)
    ids, _ = check(x, 1.0, 1.0, [0.5, 0.5 + 2.0 ** -24])
    assert ids.tolist() == [1, 2]
    ids, _ = check(x[:1], 1.0, 0.5, [1.0])
    assert ids.tolist() == [0]


@pytest.mark.parametrize("V", [1000, 32000])
def test_sample_topp_flat_row_walks_the_indices(V):
    """All-equal rows: every token holds the same key, so the pick is decided
    by the rank in index order alone and walks the indices as u grows."""
    u = np.sort(R.grid_uniforms(np.random.default_rng(V), 64))
    ids, _ = check(np.full((64, V), 0.25, np.float16), 1.0, 1.0, u)
    assert (np.diff(ids) >= 0).all() and ids[0] == 0 and ids[-1] == V - 1
    assert len(set(ids.tolist())) > 32


def test_sample_topp_peaked_row():
    """One logit 200 above the rest: that token for every u."""
    rng = np.random.default_rng(5)
    x = f16(rng.standard_normal((64, 5000)))
    x[:, 4321] = f16(200.0)
    ids, pr = check(x, 1.0, 1.0, R.grid_uniforms(rng, 64))
    assert (ids == 4321).all() and (pr == 1.0).all()


def test_sample_topp_equal_top_logits_in_index_order():
    """A row whose top eight logits are equal: the pick among them follows
    index order as u grows."""
    rng = np.random.default_rng(6)
    V, n = 4000, 64
    row = f16(rng.standard_normal(V))
    top = np.sort(rng.choice(V, size=8, replace=False))
    row[top] = f16(12.0)
    u = np.sort(R.grid_uniforms(rng, n))
    # (the eight hold 0.97 of the mass; topp = 0.9 keeps t <= 0.81 inside it)
    ids, _ = check(np.tile(row, (n, 1)), 1.0, 0.9, u)
    assert set(ids.tolist()) <= set(top.tolist()) and (np.diff(ids) >= 0).all()
    assert len(set(ids.tolist())) >= 4


def test_sample_topp_minus_inf_entries_are_not_picked():
    """-inf logits have p = 0: behind every other token in the order, picked
    only by the fallback (test_sample_topp_fallback_takes_the_last_token)."""
    rng = np.random.default_rng(7)
    T, V = 48, 3000
    x = f16(rng.standard_normal((T, V)) * 1.28)
    dead = rng.random((T, V)) < 0.5
    x[dead] = NEG_INF
    # (topp < 1: t <= 0.81 stays below each row's mass, so no fallback)
    for temperature, topp in ((0.7, 0.9), (0.9, 0.8)):
        ids, _ = check(x, temperature, topp, R.grid_uniforms(rng, T))
        assert not dead[np.arange(T), ids].any()


def test_sample_topp_small_topp_is_the_argmax():
    """temperature 1, topp = 2^-6: t <= 2^-12 <= each row's largest p, so the
    pick is the first token of the order, ffmi_argmax's."""
    rng = np.random.default_rng(8)
    T, V = 256, 1000
    x = f16(rng.standard_normal((T, V)) * 1.28)
    _, pmax = O.softmax_argmax(x.astype(np.float32), fp16=1)
    assert pmax.min() >= 2.0 ** -12, pmax.min()
    ids, pr = check(x, 1.0, 2.0 ** -6, R.grid_uniforms(rng, T))
    aid, apr = Buf.empty((T,), np.int32), Buf.empty((T,), np.float32)
    xb = Buf(x)
    F.check(L.ffmi_argmax(xb.ptr, T, V, aid.ptr, apr.ptr, None))
    assert np.array_equal(ids, aid.get())
    np.testing.assert_array_equal(pr, apr.get())


@pytest.mark.parametrize("seed", range(8 * RS))
def test_sample_topp_random_shapes_exact(seed):
    """Random shapes (T 1-40, V 1-140000), logit scales from flat to peaked,
    temperatures and topp over their ranges, planted exact ties."""
    rng = np.random.default_rng(4242 + OFF + seed)
    T = int(rng.integers(1, 41))
    V = int(rng.choice([int(rng.integers(1, 64)), int(rng.integers(1, 4096)) * 8,
                        int(rng.integers(64, 40000)), 32000, int(rng.integers(32769, 140001))]))
    scale = float(rng.choice([1e-3, 0.05, 1.28, 3.0, 8.0]))
    x = f16(rng.standard_normal((T, V)) * scale)
    for t in rng.choice(T, size=min(T, 4), replace=False):
        m = f16(float(np.abs(x[t]).max()) + float(rng.choice([0.0, 0.5, 1.0])))
        x[t, rng.choice(V, size=min(V, int(rng.integers(2, 9))), replace=False)] = m
    temperature = float(rng.choice([0.3, 0.7, 0.9, 1.0, 1.5, 4.0]))
    topp = float(rng.choice([0.05, 0.3, 0.6, 0.8, 0.95, 1.0]))
    check(x, temperature, topp, R.grid_uniforms(rng, T), (T, V, scale, temperature, topp))


def test_sample_topp_invalid_arguments():
    x, u = Buf(np.zeros((2, 8), np.float16)), Buf(np.ones(2, np.float32))
    ids, pr = Buf.empty((2,), np.int32), Buf.empty((2,), np.float32)
    n = int(L.ffmi_sample_topp_workspace_bytes(2, 8))
    ws = Buf.empty((max(n, 16),), np.uint8)

    def call(logits=x.ptr, T=2, V=8, temperature=1.0, topp=1.0, up=u.ptr, idp=ids.ptr,
             wsp=ws.ptr, nbytes=n):
        return L.ffmi_sample_topp(logits, T, V, temperature, topp, up, idp, pr.ptr, wsp, nbytes,
                                  None)

    assert call() == F.FFMI_OK
    assert call(T=0) == F.FFMI_OK
    for bad in (dict(T=-1), dict(V=0), dict(logits=None), dict(up=None), dict(idp=None),
                dict(temperature=0.0), dict(temperature=-1.0), dict(topp=0.0), dict(topp=-0.5),
                dict(topp=1.5), dict(topp=float("nan")), dict(wsp=None), dict(nbytes=n - 1)):
        assert call(**bad) == 1, bad  # FFMI_ERR_INVALID
