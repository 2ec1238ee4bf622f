"""The M-split GEMM plan matrix that tests/test_gpu_gemm_plans.py runs, and
the ffmi_debug_gemm_plan hook, shared with the planner's CPU test
(tests/test_gemm_planner.py).

A plan is (MTW, NTW, S): row tiles per wave (set by T), weight tiles per
workgroup and split-K slices (both forced through FFMI_GEMM_PLAN="NTW,S",
which the library reads on every call).
"""
import ctypes

import flexflow_amd.ffmi as F

PATH_SKINNY, PATH_WAVE, PATH_MID, PATH_TILE = 0, 1, 2, 3
NTWS = (2, 4, 6, 8, 12, 16)
# T -> MTW: 65 is five row tiles (the last holds one row, one wave owns none);
# 300 / 400 are two row blocks at 3 / 4 row tiles per wave
T_MTW = {65: 2, 130: 3, 193: 4, 300: 3, 400: 4}
TMAX = max(T_MTW)
# N = 200: 13 tiles, the last half full, a multiple of no NTW (ragged tile
# blocks, the 2-byte store tail); 224: 14 tiles, % 32 == 0 (Y_PACKED allowed)
NS = (200, 224)
# K -> split factors.  per = ceil(KT / S) k-steps per slice:
#   KT  9: S 1 -> 9; 2 -> 5, 4; 4 -> 3, 3, 3, empty; 8 -> 2, 2, 2, 2, 1, 3 empty
#   KT 33: S 3 -> 11 x 3; 5 -> 7 x 4, 5; 6 -> 6 x 5, 3; 7 -> 5 x 6, 3;
#          8 -> 5 x 6, 3, empty
# slice lengths 1-7, 9, 11: both sides of the 4-deep register ring; S 2 / 3-4
# / 5-8: the three widths of the reduce kernel.  (6 and 7 are here because the
# planner picks them for LLaMA-13B / 7B shards, tests/test_gemm_planner.py.)
K_SPLITS = {288: (1, 2, 4, 8), 1056: (3, 5, 6, 7, 8)}
SPLITS = tuple(sorted({s for ss in K_SPLITS.values() for s in ss}))
EPIS = (0, 1)


def ntws_of(mtw):
    """4 x 12 / 4 x 16 accumulator tiles exceed the register budget"""
    return tuple(n for n in NTWS if mtw < 4 or n <= 8)


T_NTW = [(T, ntw) for T, mtw in T_MTW.items() for ntw in ntws_of(mtw)]
# every (MTW, NTW, S, epilogue) the GPU file compares with the oracle
MATRIX = {(mtw, ntw, S, epi) for mtw in (2, 3, 4) for ntw in ntws_of(mtw) for S in SPLITS
          for epi in EPIS}


def shape_plans():
    """(N, K, S, epi) of every launch a (T, NTW) case makes"""
    return [(N, K, S, epi) for N in NS for K, ss in K_SPLITS.items() for S in ss for epi in EPIS]


def plan(T, N, K, flags=0):
    """{path, MTW, NTW, S, mblocks, nblk} of the launch ffmi_linear makes"""
    out = (ctypes.c_int * 6)()
    F.check(F.lib().ffmi_debug_gemm_plan(T, N, K, flags, out), (T, N, K, flags))
    return dict(zip(("path", "MTW", "NTW", "S", "mblocks", "nblk"), out))


def ntiles(N, epi):
    return (N + 15) // 16 * (2 if epi & 1 else 1)


def slab_bytes(T, N, S, epi):
    """fp32 split-K slabs of an M-split launch (none unsplit)"""
    return S * T * ntiles(N, epi) * 16 * 4 if S > 1 else 0
