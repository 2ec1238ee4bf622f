"""The deferred split-K slab rule in numpy (ffmi_internal.h `Partials`).

A split-K GEMM whose consumer can combine leaves S fp32 slabs [S][T][NP]; the
value of element (t, n) is fp16(slab 0 + slab 1 + ... in slab order), one
float32 accumulator, rounded to half once.  The rule is exact, so a consumer
of slabs must give the bits of its plain fp16 path fed with combine(slabs).

make_slabs draws data on which the ORDER of the additions matters: slabs come
in cancelling pairs (b, a - b) with |b| ~ 4096 and |a| ~ 1, so a partial sum
taken in another order passes through magnitude 4096 (fp32 spacing 2^-11..
2^-12, about half an fp16 ulp of the O(1) results) and loses low bits the
in-order sum keeps.  tests/test_partials_cpu.py measures it: any reordering of
S >= 3 slabs changes well over 10 % of the fp16 results (S = 2 is one
commutative addition).  The results are O(sqrt(S / 2)): finite, nowhere near
the fp16 range.
"""
import numpy as np

# The shapes of the GPU tests (tests/test_gpu_partials.py and the slab test of
# tests/test_gpu_peer.py import these lists), so that the CPU test measures the
# order sensitivity of the data those tests really draw.
REDUCE_T = (1, 5, 70)
REDUCE_N_NP = ((4, 16), (16, 16), (1000, 1008), (1022, 1024), (1024, 1040))
NORM_H = (8, 1016, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
NORM_T = (1, 3, 17)
# attention: qkv rows of the largest step of each scenario x 3 * heads * d
# (2 heads; INC prefill 67 rows at d 32 / 64 / 128, TREE 42 rows at d 64 / 128)
ATTN_T_N = ((67, 192), (67, 384), (67, 768), (42, 384), (42, 768))
# all-reduce copy-in: (rows, cols, NP)
PEER_CASES = ((1, 8, 16), (5, 1000, 1008), (33, 1024, 1040))


def norm_np(H):
    """slab widths of the norm tests: H rounded up to a tile, and a tile more"""
    np0 = (H + 15) // 16 * 16
    return (np0, np0 + 16)


def measured_shapes(min_results=2000):
    """(T, N, NP) of every GPU-test shape with at least min_results results
    (a fraction of 2000 is known to ~1 %; a 4- or 8-result shape cannot show
    one, and draws from the same rule with the same generator), one NP per
    (T, N): the padding columns hold no data."""
    shapes = [(T, N, NP) for T in REDUCE_T for (N, NP) in REDUCE_N_NP]
    shapes += [(T, H, norm_np(H)[0]) for H in NORM_H for T in NORM_T]
    shapes += [(T, N, N) for (T, N) in ATTN_T_N]
    shapes += [tuple(c) for c in PEER_CASES]
    seen, out = set(), []
    for (T, N, NP) in shapes:
        if T * N >= min_results and (T, N) not in seen:
            seen.add((T, N))
            out.append((T, N, NP))
    return out


def combine(slabs):
    """fp16 [T][NP] value of fp32 slabs [S][T][NP]: summed in slab order in one
    float32 accumulator, rounded once (padding columns stay NaN)."""
    slabs = np.asarray(slabs)
    assert slabs.dtype == np.float32 and slabs.ndim == 3
    acc = slabs[0].copy()
    with np.errstate(invalid="ignore"):
        for s in range(1, slabs.shape[0]):
            acc += slabs[s]
        assert acc.dtype == np.float32
        return acc.astype(np.float16)


def make_slabs(S, T, NP, N, rng):
    """fp32 slabs [S][T][NP] in cancelling pairs: for even s with s + 1 < S,
    slab[s] = b and slab[s + 1] = float32(a - b), b ~ 4096 N(0, 1), a ~ N(0, 1);
    an odd last slab is N(0, 1).  Columns [N, NP) are NaN in every slab: a
    consumer that lets a padding column into a result shows it."""
    assert S >= 1 and 1 <= N <= NP
    slabs = np.full((S, T, NP), np.nan, np.float32)
    for s in range(0, S - 1, 2):
        b = (4096.0 * rng.standard_normal((T, N))).astype(np.float32)
        a = rng.standard_normal((T, N)).astype(np.float32)
        slabs[s, :, :N] = b
        slabs[s + 1, :, :N] = a - b
    if S % 2:
        slabs[S - 1, :, :N] = rng.standard_normal((T, N)).astype(np.float32)
    return slabs


def reorderings(S):
    """slab orders a wrong consumer could take: reversed, first and last
    exchanged, rotated by one"""
    ident = list(range(S))
    swap = ident[:]
    swap[0], swap[-1] = swap[-1], swap[0]
    return {"reversed": ident[::-1], "swap_first_last": swap, "rotated": ident[1:] + ident[:1]}
