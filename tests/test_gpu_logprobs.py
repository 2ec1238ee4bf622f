"""The per-token log-probability kernel (ffmi_token_logprobs) against the
float64 rule on the same fp16 rows (tests/logprob_rule.py): the derived bar
|lp - ref| <= 2^-16 + 2^-21 |ref|, lp <= 0 (exactly 0 at V == 1), and a row's
bits independent of T, of the row's index and of the call.
"""
import numpy as np
import pytest

import flexflow_amd.ffmi as F
import logprob_rule as R
from hip_util import Buf, f16

pytestmark = pytest.mark.gpu
L = F.lib()
T_ALL = 24
KINDS = ("normal", "wide", "flat60000", "onehot", "extreme")
LARGE = ("flat60000", "extreme")  # their scaled logits overflow fp16: temperature 0 only


def chunk_size():
    """The kernel's compile-time chunk: the longest row with one (m, s) pair."""
    one = int(L.ffmi_token_logprobs_workspace_bytes(1, 1))
    lo, hi = 1, 983040
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if int(L.ffmi_token_logprobs_workspace_bytes(1, mid)) == one:
            lo = mid
        else:
            hi = mid - 1
    return lo


C = chunk_size()
VS = [1, 7, 1000, C - 1, C, C + 1, 32000, 32001, 128256]


def gpu_logprobs(x16, temperature, targets, picks):
    x16 = np.ascontiguousarray(x16, np.float16)
    T, V = x16.shape
    xb = Buf(x16)
    tb = None if targets is None else Buf(np.asarray(targets, np.int32))
    pb = None if picks is None else Buf(np.asarray(picks, np.int32))
    out = Buf(np.full(T, 7.0, np.float32))
    n = int(L.ffmi_token_logprobs_workspace_bytes(T, V))
    ws = Buf.empty((max(n, 16),), np.uint8)
    F.check(L.ffmi_token_logprobs(xb.ptr, T, V, temperature, tb.ptr if tb else None,
                                  pb.ptr if pb else None, out.ptr, ws.ptr, n, None),
            (T, V, temperature))
    return out.get()


def make_rows(V, temperature, seed):
    """T_ALL rows cycling through KINDS, with their targets (-1: the pick),
    picks and the ids they score."""
    rng = np.random.default_rng(seed)
    x = np.empty((T_ALL, V), np.float16)
    targets = np.empty(T_ALL, np.int32)
    picks = rng.integers(0, V, size=T_ALL).astype(np.int32)
    for r in range(T_ALL):
        kind = KINDS[r % len(KINDS)]
        if temperature != 0 and kind in LARGE:
            kind = "normal"
        if kind == "normal":
            x[r] = f16(rng.standard_normal(V) * 1.28)
        elif kind == "wide":
            x[r] = f16(np.clip(rng.standard_normal(V) * 8.0, -32, 32))
        elif kind == "flat60000":
            x[r] = f16(60000.0)
        elif kind == "onehot":
            x[r] = f16(-32.0)
            hot = int(rng.integers(0, V))
            x[r, hot] = f16(32.0)
            if r % 2:
                picks[r] = hot
        else:
            x[r] = f16(-65504.0)
            x[r, 0] = f16(65504.0)
        # -1 with the pick, explicit 0, explicit V - 1, an explicit interior id
        targets[r] = (-1, 0, V - 1, int(rng.integers(0, V)))[(r // len(KINDS) + r) % 4]
        if kind == "extreme":
            targets[r] = V - 1
    scored = np.where(targets >= 0, targets, picks)
    return x, targets, picks, scored


@pytest.fixture(scope="module", params=VS, ids=lambda v: f"V{v}")
def case(request):
    """Per V and temperature: the rows, the T = 24 result and the float64
    reference, computed once and shared."""
    V = request.param
    out = {}
    for temperature in (0.0, 0.9, 0.8):
        x, targets, picks, scored = make_rows(V, temperature, V * 31 + int(temperature * 10))
        out[temperature] = dict(x=x, targets=targets, picks=picks, scored=scored,
                                lp=gpu_logprobs(x, temperature, targets, picks),
                                ref=R.logprobs(x, temperature, scored))
    return V, out


@pytest.mark.parametrize("temperature", [0.0, 0.9, 0.8])
def test_logprobs_meet_the_bar(case, temperature):
    V, d = case
    d = d[temperature]
    assert set(d["targets"][d["targets"] >= 0]) >= {0, V - 1} and (d["targets"] < 0).any()
    print("max |lp - ref|", np.abs(d["lp"] - d["ref"]).max(), "max bar", R.bar(d["ref"]).max())
    R.assert_within_bar(d["lp"], d["ref"], (V, temperature))
    assert (d["lp"] <= 0).all()
    if V == 1:
        assert (d["lp"].view(np.uint32) == 0).all()  # exactly +0.0


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_null_targets_score_the_picks(case, temperature):
    V, d = case
    d = d[temperature]
    a = gpu_logprobs(d["x"], temperature, None, d["picks"])
    b = gpu_logprobs(d["x"], temperature, np.full(T_ALL, -1, np.int32), d["picks"])
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    R.assert_within_bar(a, R.logprobs(d["x"], temperature, d["picks"]), (V, temperature))
    # explicit targets everywhere need no picks
    c = gpu_logprobs(d["x"], temperature, d["scored"], None)
    np.testing.assert_array_equal(c.view(np.uint32), d["lp"].view(np.uint32))


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_a_rows_bits_depend_on_the_row_only(case, temperature):
    """The call repeated, and every row of the T = 24 call alone at T = 1 and
    inside a T = 5 call at another index: equal bits."""
    V, d = case
    d = d[temperature]
    want = d["lp"].view(np.uint32)
    again = gpu_logprobs(d["x"], temperature, d["targets"], d["picks"])
    np.testing.assert_array_equal(again.view(np.uint32), want)
    for r in range(T_ALL):
        one = gpu_logprobs(d["x"][r:r + 1], temperature, d["targets"][r:r + 1], d["picks"][r:r + 1])
        assert one.view(np.uint32)[0] == want[r], (V, r, one, d["lp"][r])
    for g in range(0, T_ALL, 5):
        rows = [(g + 4 - j) % T_ALL for j in range(5)]  # (each at another index than in the 24)
        five = gpu_logprobs(d["x"][rows], temperature, d["targets"][rows], d["picks"][rows])
        np.testing.assert_array_equal(five.view(np.uint32), want[rows], err_msg=str((V, g)))
