"""The M-split GEMM planner through ffmi_debug_gemm_plan and
ffmi_linear_workspace_bytes only (host code: no device needed).

- FFMI_GEMM_PLAN is read on every call; a forced plan is honoured when valid
  and ignored (the planner's pick stays) otherwise;
- the workspace is a whole number of fp32 slabs, the launch's own S of them;
- every plan the planner picks for LLaMA layer shapes lies inside the matrix
  tests/test_gpu_gemm_plans.py compares with the oracle, so a planner that
  grows new options cannot leave that coverage unnoticed.
"""
import itertools

import pytest

import flexflow_amd.ffmi as F
from gemm_plan_cases import (MATRIX, NTWS, PATH_MID, PATH_SKINNY, PATH_TILE, PATH_WAVE, ntiles,
                             plan, slab_bytes)

# (hidden, intermediate, heads, vocab)
LLAMA = {"68m": (768, 3072, 12, 32000), "7b": (4096, 11008, 32, 32000),
         "13b": (5120, 13824, 40, 32000), "65b": (8192, 22016, 64, 32000)}
LLAMA_TS = (65, 80, 168, 216, 256, 300, 577, 1024)
# a sweep off the model shapes: ragged N, short K (S <= KT binds), 1-7 row blocks
SWEEP = [(T, N, K, epi) for T in (65, 128, 129, 193, 256, 257, 385, 576, 577, 769, 1100)
         for N, K in ((200, 288), (224, 1056), (4096, 64), (1000, 8192), (11008, 4096),
                      (4096, 11008))
         for epi in (0, 1)]


@pytest.fixture(autouse=True)
def no_forced_plan(monkeypatch):
    monkeypatch.delenv("FFMI_GEMM_PLAN", raising=False)
    monkeypatch.delenv("FFMI_TILE_GEMM", raising=False)


def llama_layers():
    for name, (H, I, heads, V) in LLAMA.items():
        for tp in (1, 2, 4, 8):
            if heads % tp:
                continue
            Vl = V // tp if tp > 1 and (V // tp) % 16 == 0 else V
            yield name, tp, [(3 * H // tp, H, 0), (H, H // tp, 0), (I // tp, H, 1), (H, I // tp, 0),
                             (Vl, H, 0)]


def test_hook_reports_the_path():
    assert plan(32, 4096, 4096) == dict(path=PATH_SKINNY, MTW=0, NTW=0, S=1, mblocks=0, nblk=0)
    assert plan(8, 32000, 768)["path"] == PATH_WAVE
    assert plan(8, 32000, 768, F.EPI_SILU_MUL)["path"] == PATH_SKINNY
    assert plan(64, 4096, 4096)["path"] == PATH_SKINNY
    p = plan(65, 4096, 4096)
    assert (p["path"], p["MTW"], p["mblocks"]) == (PATH_MID, 2, 1)
    assert p["nblk"] == -(-256 // p["NTW"])
    # the 256 x 256 tile form takes packed activations only (T >= 497)
    assert plan(1024, 12288, 4096, F.X_PACKED)["path"] == PATH_TILE
    assert plan(1024, 12288, 4096)["path"] == PATH_MID
    assert plan(496, 12288, 4096, F.X_PACKED)["path"] == PATH_MID
    L = F.lib()
    out = (F.c_int * 6)()
    assert L.ffmi_debug_gemm_plan(168, 4096, 4096, 0, None) == 1
    assert L.ffmi_debug_gemm_plan(0, 4096, 4096, 0, out) == 1
    assert L.ffmi_debug_gemm_plan(168, 4096, 4090, 0, out) == 5


def test_forced_plan_is_read_per_call_and_validated(monkeypatch):
    T, N, K = 168, 4096, 288  # KT = 9
    own = plan(T, N, K)
    for ntw, S in itertools.product(NTWS, range(1, 9)):
        monkeypatch.setenv("FFMI_GEMM_PLAN", f"{ntw},{S}")
        p = plan(T, N, K)
        assert (p["path"], p["MTW"], p["NTW"], p["S"]) == (PATH_MID, 3, ntw, S)
        assert p["nblk"] == -(-256 // ntw) and p["mblocks"] == 1
    # not a tile width / more than 8 slices / more slices than k-steps / junk
    for bad in ("3,2", "5,1", "10,2", "32,1", "0,1", "8,9", "8,0", "8,-1", "8", "x", ""):
        monkeypatch.setenv("FFMI_GEMM_PLAN", bad)
        assert plan(T, N, K) == own, bad
    monkeypatch.delenv("FFMI_GEMM_PLAN")
    assert plan(T, N, K) == own
    own96 = plan(T, N, 96)
    monkeypatch.setenv("FFMI_GEMM_PLAN", "8,4")
    assert plan(T, N, 96) == own96  # S = 4 > KT = 3
    monkeypatch.setenv("FFMI_GEMM_PLAN", "8,3")
    assert plan(T, N, 96)["S"] == 3
    # the other paths are not touched
    monkeypatch.setenv("FFMI_GEMM_PLAN", "8,2")
    assert plan(32, 4096, 4096)["path"] == PATH_SKINNY


def test_forced_plan_of_listed_shapes_only(monkeypatch):
    T = 130
    own = {nk: plan(T, *nk) for nk in ((200, 288), (1056, 224), (4096, 4096))}
    monkeypatch.setenv("FFMI_GEMM_PLAN", "200:288:12,2;224:1056:16,5")
    p = plan(T, 200, 288)
    assert (p["NTW"], p["S"]) == (12, 2)
    p = plan(T, 224, 1056)
    assert (p["NTW"], p["S"]) == (16, 5)
    assert plan(T, 4096, 4096) == own[4096, 4096]
    assert plan(T, 1056, 224) == own[1056, 224]  # (N:K, not K:N)
    # an invalid entry for the shape is skipped, a later valid one applies
    monkeypatch.setenv("FFMI_GEMM_PLAN", "200:288:5,2;200:288:6,3")
    p = plan(T, 200, 288)
    assert (p["NTW"], p["S"]) == (6, 3)
    monkeypatch.setenv("FFMI_GEMM_PLAN", "200:288:5,2")
    assert plan(T, 200, 288) == own[200, 288]


def test_four_row_tiles_never_with_wide_blocks(monkeypatch):
    for force in (None, "12,1", "16,2", "12,8"):
        if force:
            monkeypatch.setenv("FFMI_GEMM_PLAN", force)
        for T, N, K, epi in SWEEP + [(T, 4096, 4096, 0) for T in range(65, 1100, 16)]:
            p = plan(T, N, K, epi)
            assert p["path"] == PATH_MID
            assert p["MTW"] in (2, 3, 4) and p["NTW"] in NTWS and 1 <= p["S"] <= min(8, K // 32)
            assert not (p["MTW"] == 4 and p["NTW"] > 8), (force, T, N, K, epi, p)
            mtiles = (T + 15) // 16
            assert p["mblocks"] == -(-mtiles // (4 * p["MTW"]))
            assert p["nblk"] == -(-ntiles(N, epi) // p["NTW"])
    monkeypatch.setenv("FFMI_GEMM_PLAN", "16,2")
    assert plan(193, 4096, 4096)["NTW"] == 8 and plan(192, 4096, 4096)["NTW"] == 16


def check_workspace(T, N, K, epi, forced):
    """S slabs of T x (tiles x 16) fp32, none unsplit.  The plain epilogue's
    workspace also serves the launches whose consumer combines the slabs
    (the model's qkv / o / down), which the planner may split further: there
    it is a whole number of slabs, at least the launch's own."""
    L = F.lib()
    p = plan(T, N, K, epi)
    assert p["path"] == PATH_MID
    for flags in (0, F.X_PACKED, F.Y_PACKED, F.W_STREAM):
        if flags == F.X_PACKED and plan(T, N, K, epi | flags)["path"] != PATH_MID:
            continue
        ws = L.ffmi_linear_workspace_bytes(T, N, K, epi | flags)
        own = slab_bytes(T, N, p["S"], epi)
        if forced or epi:
            assert ws == own, (T, N, K, epi, flags, p, ws)
        else:
            slab = T * ntiles(N, epi) * 16 * 4
            assert ws >= own and ws % slab == 0, (T, N, K, epi, flags, p, ws)
            assert ws // slab != 1 and ws // slab <= min(8, K // 32), (T, N, K, epi, flags, p, ws)


def test_workspace_is_the_plans_slabs(monkeypatch):
    prefill = 0
    for T, N, K, epi in SWEEP:
        check_workspace(T, N, K, epi, False)
        prefill += plan(T, N, K, epi)["mblocks"] >= 4
    assert prefill >= 12  # the prefill override (>= 4 row blocks) is in the sweep
    p = plan(1100, 4096, 11008)
    assert (p["NTW"], p["S"]) == (8, 2)  # (its K >= 8192 pick)
    for ntw, S in ((2, 1), (6, 2), (8, 3), (12, 5), (16, 8), (4, 7)):
        monkeypatch.setenv("FFMI_GEMM_PLAN", f"{ntw},{S}")
        for T, N, K, epi in SWEEP:
            if S <= K // 32:
                assert plan(T, N, K, epi)["S"] == S
            check_workspace(T, N, K, epi, S <= K // 32)
    assert F.lib().ffmi_linear_workspace_bytes(0, 4096, 4096, 0) == 0


def test_llama_layer_plans_are_inside_the_tested_matrix():
    seen, outside = set(), []
    for name, tp, layers in llama_layers():
        for T, (N, K, epi), xp in itertools.product(LLAMA_TS, layers, (0, F.X_PACKED)):
            p = plan(T, N, K, epi | xp)
            if p["path"] != PATH_MID:
                assert p["path"] == PATH_TILE and xp and T >= 497, (name, tp, T, N, K, p)
                continue
            key = (p["MTW"], p["NTW"], p["S"], epi)
            seen.add(key)
            if key not in MATRIX:
                outside.append((name, tp, T, N, K) + key)
            check_workspace(T, N, K, epi, False)
    assert not outside, outside[:8]
    assert len(seen) >= 64  # (the planner really moves over the matrix: 105 at this writing)
