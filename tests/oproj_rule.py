"""The output projection folded into the fused attention, in numpy
(ffmi_internal.h `OprojArgs`, kernels/attention.hip OP).

Each (work item, head) workgroup multiplies its rounded fp16 output rows by
its head's 64 columns of Wo [N][heads * 64] and stores

    slab[h][t][n] = sum_k out[t][h*64 + k] * Wo[n][h*64 + k]      (fp32)

as slab h of [heads][T][N], T = the step's tokens.  fp16 x fp16 is exact in
fp32, so only the order of 63 fp32 additions is the kernel's own.  Two kinds
of weight turn that into two checks, both over the kernel's own `out`:

Selector weights: one non-zero +-2^e (e in -3..3) per (row n, head h), at
  column kappa(n, h) of the head's 64.  One exact product added to exact
  zeros is exact in any order: slab[h][t][n] == +-2^e * out[t][h*64 + kappa]
  as float32 values (a zero of either sign is equal).  kappa is a fresh
  random permutation of the 64 columns per (head, block of 64 rows), so every
  index of the kernel is pinned: the tile a wave owns, the head's K slice,
  both packed strides, the column split's interleave, the row and column
  mapping of the MFMA result.  N >= 64: one seed selects every column of every
  head.  N < 64: one seed has only N non-zeros per head, and the seeds
  k*C .. k*C + C - 1, C = ceil(64 / N), select all 64 columns between them
  (selector_seeds; 2 seeds at N = 48, 4 at N = 16).
  Where the selected `out` element is an fp16 subnormal, 0 is accepted as well
  as the exact product (whether the MFMA flushes subnormal inputs is recorded,
  not assumed); Tally.finish asserts that such elements stay under 0.1 % of
  those compared.

Dense weights: Wo ~ fp16(0.05 N(0, 1)).  Against ref = the float64 sum,
  |slab - ref| <= 64 * 2^-24 * sum_k |out * Wo| per element: the first-order
  worst case of any-order fp32 summation of 64 exact products.  Not a fitted
  number: tests/test_oproj_cpu.py shows that sequential, reversed and pairwise
  float32 sums stay well inside it and that a dropped term does not.

The slab buffer of the GPU tests (slab_buffer / split_buffer): heads * max_T *
N floats between two guards of 64, prefilled with a non-NaN sentinel bit
pattern; everything outside [heads][T][N] -- the guards and the rows between
T and max_T -- must come back unchanged.
"""
import numpy as np

D = 64  # head size of the folded projection
# (heads, N) of tests/test_gpu_oproj.py.  112: 7 tiles, fewer than the 8
# waves; 144: 9 tiles, an odd count under the column split; 1024: 64 tiles, 8
# per wave; N != heads * 64 in most: the packed pitch differs from the K extent
TILE_GRID = ((1, 16), (3, 48), (2, 112), (3, 144), (12, 768), (16, 1024), (5, 1024))
RAGGED, MODES, PACKED = (3, 144), (12, 768), (4, 256)
SLAB_SOURCE = ((3, 144), (12, 768))
COMPOSED = ((12, 768), (16, 1024))
GPU_SHAPES = tuple(sorted(set(TILE_GRID + (RAGGED, MODES, PACKED) + SLAB_SOURCE + COMPOSED)))

SENTINEL = 0xC2ABCDEF  # float32 -85.9: finite, never a product of the data here
GUARD = 64
BOUND_FACTOR = D * 2.0 ** -24
SUBNORMAL_CAP = 1e-3


def selector_seeds(N, k=0):
    """the seeds that together select all 64 columns of every head"""
    C = -(-D // N) if N < D else 1
    return tuple(range(k * C, k * C + C))


class Tally:
    """what the checks of one test saw: elements compared by the selector
    check, fp16-subnormal sources among them and what the hardware gave for
    those, and the dense check's largest error / bound"""

    def __init__(self):
        self.compared = self.subnormal = self.flushed = self.kept = 0
        self.max_ratio = 0.0

    def finish(self):
        assert self.subnormal <= SUBNORMAL_CAP * self.compared, (self.subnormal, self.compared)
        return dict(compared=self.compared, subnormal_sources=self.subnormal,
                    subnormal_flushed=self.flushed, subnormal_kept=self.kept,
                    dense_max_err_over_bound=self.max_ratio)


class Selector:
    def __init__(self, heads, N, seed):
        assert heads >= 1 and N >= 16 and N % 16 == 0 and seed >= 0
        self.heads, self.N = heads, N
        C = len(selector_seeds(N))
        fam, shift = seed // C, (seed % C) * N
        n = np.arange(N)
        self.kappa = np.empty((N, heads), np.int64)
        for h in range(heads):
            for blk in range((N + D - 1) // D):
                perm = np.random.default_rng([fam, h, blk, N, heads]).permutation(D)
                rows = n[blk * D:(blk + 1) * D]
                self.kappa[rows, h] = perm[(rows - blk * D + shift) % D]
        rng = np.random.default_rng([seed, N, heads, 1])
        e = rng.integers(-3, 4, size=(N, heads))
        sign = rng.choice([-1.0, 1.0], size=(N, heads))
        self.coef = (sign * 2.0 ** e).astype(np.float32)
        self.Wo = np.zeros((N, heads * D), np.float16)
        for h in range(heads):
            self.Wo[n, h * D + self.kappa[:, h]] = self.coef[:, h]

    def check(self, slab, out, tally=None):
        """slab [heads][T][N] float32 == coef * out[t][h*64 + kappa], exactly"""
        heads, N = self.heads, self.N
        slab = np.asarray(slab)
        T = slab.shape[1]
        assert slab.dtype == np.float32 and slab.shape == (heads, T, N)
        o = np.asarray(out)
        assert o.dtype == np.float16
        o = o.reshape(T, heads, D)
        for h in range(heads):
            src = o[:, h, :][:, self.kappa[:, h]]  # [T][N] fp16
            want = self.coef[None, :, h] * src.astype(np.float32)
            assert want.dtype == np.float32
            sub = (src != 0) & (np.abs(src.astype(np.float32)) < 2.0 ** -14)
            exact = slab[h] == want
            zero = sub & (slab[h] == 0)
            bad = ~(exact | zero)
            assert not bad.any(), (f"head {h}: {int(bad.sum())} of {bad.size} wrong, first at "
                                   f"(t, n) = {tuple(np.argwhere(bad)[0])}")
            if tally is not None:
                tally.compared += sub.size
                tally.subnormal += int(sub.sum())
                tally.flushed += int(zero.sum())
                tally.kept += int((sub & exact).sum())


class Dense:
    def __init__(self, heads, N, rng):
        self.heads, self.N = heads, N
        self.Wo = (rng.standard_normal((N, heads * D)) * 0.05).astype(np.float32).astype(np.float16)

    def ref_and_bound(self, out):
        """float64 [heads][T][N]: the exact sum, and 64 * 2^-24 * sum |out * Wo|"""
        o = np.asarray(out)
        assert o.dtype == np.float16
        T = o.shape[0]
        o = o.astype(np.float64).reshape(T, self.heads, D)
        W = self.Wo.astype(np.float64).reshape(self.N, self.heads, D)
        ref = np.einsum("thk,nhk->htn", o, W)
        mag = np.einsum("thk,nhk->htn", np.abs(o), np.abs(W))
        return ref, BOUND_FACTOR * mag

    def check(self, slab, out, tally=None):
        slab = np.asarray(slab)
        ref, bound = self.ref_and_bound(out)
        assert slab.dtype == np.float32 and slab.shape == ref.shape, (slab.shape, ref.shape)
        err = np.abs(slab.astype(np.float64) - ref)
        bad = ~(err <= bound)  # (a NaN is bad)
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        if tally is not None:
            tally.max_ratio = max(tally.max_ratio, ratio)
        assert not bad.any(), (f"{int(bad.sum())} of {bad.size} beyond the bound, largest "
                               f"error / bound {ratio:.3g}, first at (h, t, n) = "
                               f"{tuple(np.argwhere(bad)[0])}")
        return ratio


def reference_slab(out, Wo, heads, ksteps=(0, 1), head_shift=0):
    """float32 [heads][T][N] of the rule; the faults of the negative controls:
    ksteps: which 32-column k-steps are summed; head_shift: head h's weight
    slice taken at head (h + head_shift) % heads"""
    o = np.asarray(out)
    assert o.dtype == np.float16
    T, N = o.shape[0], Wo.shape[0]
    o = o.astype(np.float64).reshape(T, heads, D)
    W = np.roll(np.asarray(Wo).astype(np.float64).reshape(N, heads, D), -head_shift, axis=1)
    cols = np.concatenate([np.arange(32 * k, 32 * k + 32) for k in ksteps])
    return np.einsum("thk,nhk->htn", o[:, :, cols], W[:, :, cols]).astype(np.float32)


def fake_out(T, heads, rng, keys=8):
    """fp16 [T][heads * 64] like an attention output: softmax-weighted
    averages of N(0, 1) values"""
    s = rng.standard_normal((T, heads, keys))
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    v = rng.standard_normal((heads, keys, D))
    return np.einsum("thl,hld->thd", p, v).reshape(T, heads * D).astype(np.float32).astype(np.float16)


# ---------------------------------------------------------------- the slab buffer
def slab_buffer(heads, max_T, N):
    """uint32 bits of the device buffer: guard, heads * max_T * N, guard"""
    return np.full(heads * max_T * N + 2 * GUARD, SENTINEL, np.uint32)


def split_buffer(buf, heads, T, N, projected=True):
    """The slab [heads][T][N] (row stride T, not the capacity) of a buffer read
    back, after asserting that every word outside it still holds the sentinel
    (projected false: every word of the buffer)."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint32
    used = heads * T * N if projected else 0
    assert GUARD + used <= buf.size - GUARD, "the step's rows exceed the buffer"
    assert (buf[:GUARD] == SENTINEL).all(), "guard before the slab written"
    rest = buf[GUARD + used:]
    assert (rest == SENTINEL).all(), (f"{int((rest != SENTINEL).sum())} words behind "
                                      f"[heads][T][N] written")
    if not projected:
        return None
    return buf[GUARD:GUARD + used].view(np.float32).reshape(heads, T, N).copy()
