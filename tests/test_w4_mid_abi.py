"""The ABI of the M-split MXFP4-weight GEMM (include/ffmi.h): the one-pass
workspace size against its arithmetic and the launch plan ffmi_linear_w4
follows, as ffmi_debug_linear_w4_plan reports it.  No GPU."""
import ctypes

import pytest

import flexflow_amd.ffmi as F

INVALID, UNSUPPORTED = 1, 5


def plan(T, N, K, epi, nbytes):
    p = (ctypes.c_int * 6)()
    assert F.lib().ffmi_debug_linear_w4_plan(T, N, K, epi, nbytes, p) == 0
    return dict(zip(("path", "MTW", "NTW", "S", "passes", "groups"), p))


@pytest.mark.parametrize("N,K", [(16, 128), (40, 256), (144, 1408), (4096, 4096), (32000, 4096)])
def test_onepass_workspace_and_plan(N, K):
    L, tiles, groups, steps = F.lib(), (N + 15) // 16, (N + 127) // 128, K // 128
    S = max(1, min(256 // groups, 8, steps // 2))  # (tests/test_w4_abi.py)
    S = -(-steps // -(-steps // S))
    for T in (1, 64, 65, 168, 256, 300):
        least = L.ffmi_linear_w4_workspace_bytes(T, N, K, F.EPI_NONE)
        need = L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, F.EPI_NONE)
        assert need == (S * min(T, 256) * tiles * 16 * 4 if S > 1 else 0)
        assert need >= least and (T > 64 or need == least)
        assert L.ffmi_linear_w4_onepass_workspace_bytes(T, N, K, F.EPI_SILU_MUL | F.W_STREAM) == 0
        p = plan(T, N, K, F.EPI_NONE, need)
        assert p["S"] == plan(1, N, K, F.EPI_NONE, 0)["S"] == S and p["groups"] == groups
        if T <= 64:
            assert (p["path"], p["passes"]) == (0, 1)
            continue
        assert (p["path"], p["NTW"], p["passes"]) == (1, 8, -(-T // 256))
        assert p["MTW"] == max(2, -(-min(T, 256) // 64))
        assert plan(T, N, K, F.EPI_SILU_MUL, 0)["path"] == 1  # S = 1: no workspace needed
        q = plan(T, N, K, F.EPI_NONE, least)
        assert (q["path"], q["passes"]) == ((0, -(-T // 64)) if S > 1 else (1, -(-T // 256)))
        if S > 1:
            assert plan(T, N, K, F.EPI_NONE, need - 4)["path"] == 0


def test_plan_refusals_name_w4():
    L, p = F.lib(), (ctypes.c_int * 6)()
    for st, args in ((INVALID, (168, 16, 128, 0, 0, None)), (INVALID, (0, 16, 128, 0, 0, p)),
                     (UNSUPPORTED, (168, 16, 192, 0, 0, p))):
        assert L.ffmi_debug_linear_w4_plan(*args) == st and "w4" in L.ffmi_last_error().decode()
