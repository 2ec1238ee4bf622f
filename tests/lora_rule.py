"""The LoRA update of down_proj, in numpy (include/ffmi.h ffmi_lora_apply,
kernels/lora.hip; the reference's lora_linear_kernels.cu:174-278).

For a row t whose request uses adapter a -- A [r][F], B [H][r], s16 =
fp16(alpha / r) -- with x the row of the SiLU output the down GEMM reads and y
that row of the down projection, already fp16:

    h[j]  = fp16( sum_k x[k] * A[j][k] )          fp32 accumulation
    d[n]  =       sum_j h[j] * B[n][j]            fp32
    y'[n] = fp16( float(y[n]) + float(s16) * d[n] )

The reference's rounding points (the low-rank activation held in the
activation type, the scaling cast to it, the update in place); it accumulates
in fp16 through cuBLAS where this project, as in every GEMM, uses fp32.  Rows
without an adapter are not written.  fp16 x fp16 is exact in fp32, so only the
order of the fp32 additions is the kernel's own, and two kinds of adapter turn
that into two checks:

Selector adapters: A has one +-2^e (e in -3..3) per row j at column kappa(j),
  a random injection into F; B one +-2^e per row n at column pi(n) < r; alpha /
  r a power of two.  One exact product added to exact zeros is exact in any
  order: h[j] == fp16(+-2^e x[kappa(j)]) and, from the kernel's own h,
  y'[n] == fp16(float(y[n]) + s * (+-2^e h[pi(n)])) with the float32 operations
  done as written -- equal bit for bit, which pins every index.  Where the
  selected product of the h check is an fp16 subnormal (or its source is), 0
  is accepted too; Tally.finish caps such elements at 0.1 % of those compared
  (N(0, 1)-scale x stays near 0.01 %, tests/test_lora_cpu.py).

Dense adapters: against the float64 sums, any-order fp32 summation of exact
  products stays within the first-order bounds

    e_h[j]  = F * 2^-24 * sum_k |x[k] A[j][k]|
    e_y[n]  = |s| * r * 2^-24 * sum_j |h[j] B[n][j]|            (d, any order)
              + 2^-24 * |s d[n]| + 2^-24 * |y[n] + s d[n]|      (two roundings)

  and rounding is monotone, so fp16(ref - e) <= value <= fp16(ref + e) for h
  (from x) and for y' (from the kernel's own h).  Derived, not fitted:
  tests/test_lora_cpu.py shows that sequential, reversed and pairwise float32
  sums stay inside and that a dropped k-slice or a swapped adapter does not.
"""
import numpy as np

R_MAX = 64           # FFMI_LORA_MAX_RANK: h rows are [64], zero beyond the rank
MAX_ADAPTERS = 8     # FFMI_LORA_MAX_ADAPTERS
CHUNK = 256          # columns of F per part of the shrink (fixed by F alone)
U = 2.0 ** -24
SUBNORMAL_CAP = 1e-3
GUARD = 64
SENTINEL = 0xCAFE    # fp16 -13.98: finite, overwritten by any update

# (F, H) of tests/test_gpu_lora.py: 352 = 1 part + 96 columns; 1376 = 43 k-steps,
# an odd count; 2752 = 11 parts, the last one short; H = 64 < one column block
SHAPES = ((352, 64), (1024, 768), (1376, 1024), (2752, 4096))
RANKS = (1, 12, 16, 64)
TS = (1, 5, 17, 64, 65, 168)
# runs of several adapters and gaps: (rows, adapter) in order, 40 rows
MIXED_40 = ((3, 0), (1, -1), (17, 1), (2, 0), (16, -1), (1, 2))


def slots_of(runs):
    return np.concatenate([np.full(n, a, np.int32) for n, a in runs])


def f16(v):
    return np.asarray(v).astype(np.float32).astype(np.float16)


class Adapter:
    """A [r][F], B [H][r] fp16 and the scaling fp16(alpha / r)"""

    def __init__(self, A, B, alpha):
        self.A, self.B = np.asarray(A), np.asarray(B)
        assert self.A.dtype == np.float16 and self.B.dtype == np.float16
        self.r, self.F = self.A.shape
        self.H = self.B.shape[0]
        assert self.B.shape == (self.H, self.r) and 1 <= self.r <= R_MAX
        self.alpha = float(alpha)
        self.s16 = np.float16(np.float32(alpha) / np.float32(self.r))

    # ---- the rule in float64, with the first-order bounds
    def h_ref(self, x):
        """float64 [T][r]: the exact sums and e_h"""
        x64, A64 = np.asarray(x).astype(np.float64), self.A.astype(np.float64)
        return x64 @ A64.T, self.F * U * (np.abs(x64) @ np.abs(A64).T)

    def y_ref(self, y, h):
        """float64 [T][H] from fp16 y and fp16 h [T][r]: the exact value and e_y"""
        assert np.asarray(h).dtype == np.float16 and np.asarray(y).dtype == np.float16
        h64, B64 = np.asarray(h).astype(np.float64), self.B.astype(np.float64)
        s = float(self.s16)
        d = h64 @ B64.T
        ref = np.asarray(y).astype(np.float64) + s * d
        e = abs(s) * self.r * U * (np.abs(h64) @ np.abs(B64).T) + U * np.abs(s * d) + U * np.abs(ref)
        return ref, e

    # ---- the rule as float32 operations in one fixed order (sequential in k, j)
    def h_f32(self, x, order="seq", cols=None):
        return f16(sum_f32(products(x, self.A, cols), order))

    def y_f32(self, y, h, order="seq"):
        d = sum_f32(products(h, self.B), order)
        return (np.asarray(y).astype(np.float32) + np.float32(self.s16) * d).astype(np.float16)


def products(x, W, cols=None):
    """float32 [T][N][K] of x[t][k] * W[n][k] (exact); cols: the k kept"""
    x32, W32 = np.asarray(x).astype(np.float32), np.asarray(W).astype(np.float32)
    if cols is not None:
        x32, W32 = x32[:, cols], W32[:, cols]
    return x32[:, None, :] * W32[None, :, :]


def sum_f32(p, order="seq"):
    """float32 sum over the last axis in the given order, every add rounded"""
    p = np.asarray(p, np.float32)
    if order == "pairwise":
        while p.shape[-1] > 1:
            if p.shape[-1] % 2:
                p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], -1)
            p = p[..., 0::2] + p[..., 1::2]
        return p[..., 0]
    ks = range(p.shape[-1]) if order == "seq" else range(p.shape[-1] - 1, -1, -1)
    acc = np.zeros(p.shape[:-1], np.float32)
    for k in ks:
        acc = acc + p[..., k]
    return acc


def in_interval(val, ref, e):
    """fp16(ref - e) <= val <= fp16(ref + e), elementwise; val fp16"""
    val = np.asarray(val)
    assert val.dtype == np.float16
    lo, hi = (ref - e).astype(np.float16), (ref + e).astype(np.float16)
    with np.errstate(invalid="ignore"):
        return (val >= lo) & (val <= hi)


class Tally:
    """what the selector checks of one test saw (tests/oproj_rule.py Tally)"""

    def __init__(self):
        self.compared = self.subnormal = self.flushed = self.kept = 0

    def finish(self):
        assert self.compared > 0
        assert self.subnormal <= SUBNORMAL_CAP * self.compared, (self.subnormal, self.compared)
        return dict(compared=self.compared, subnormal_sources=self.subnormal,
                    subnormal_flushed=self.flushed, subnormal_kept=self.kept)


def _coef(rng, n):
    return (rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.integers(-3, 4, size=n)).astype(np.float32)


class Selector(Adapter):
    def __init__(self, r, F, H, seed, log2_scale=-1):
        rng = np.random.default_rng([seed, r, F, H])
        self.kappa = rng.permutation(F)[:r]                       # column of A's row j
        self.pi = np.concatenate([rng.permutation(r) for _ in range(-(-H // r))])[:H]
        self.ca, self.cb = _coef(rng, r), _coef(rng, H)
        A = np.zeros((r, F), np.float16)
        A[np.arange(r), self.kappa] = self.ca
        B = np.zeros((H, r), np.float16)
        B[np.arange(H), self.pi] = self.cb
        super().__init__(A, B, r * 2.0 ** log2_scale)
        assert float(self.s16) == 2.0 ** log2_scale

    def check_h(self, h, x, tally):
        """h [T][r] fp16 == fp16(ca * x[:, kappa]) exactly (0 also where subnormal)"""
        h, src = np.asarray(h), np.asarray(x)[:, self.kappa]
        assert h.dtype == np.float16 and src.dtype == np.float16
        want = (self.ca[None, :] * src.astype(np.float32)).astype(np.float16)
        tiny = 2.0 ** -14
        sub = (src != 0) & ((np.abs(src.astype(np.float32)) < tiny) |
                            (np.abs(want.astype(np.float32)) < tiny))
        exact = h == want
        zero = sub & (h == 0)
        bad = ~(exact | zero)
        assert not bad.any(), (f"h: {int(bad.sum())} of {bad.size} wrong, first at (t, j) = "
                               f"{tuple(np.argwhere(bad)[0])}")
        tally.compared += sub.size
        tally.subnormal += int(sub.sum())
        tally.flushed += int((zero & ~exact).sum())
        tally.kept += int((sub & exact).sum())

    def want_y(self, y, h):
        """fp16 [T][H]: the rule's float32 operations on the kernel's own h"""
        d = self.cb[None, :] * np.asarray(h)[:, self.pi].astype(np.float32)
        return (np.asarray(y).astype(np.float32) + np.float32(self.s16) * d).astype(np.float16)


def dense(r, F, H, rng, alpha=None, b_scale=0.05):
    """A ~ fp16(N(0, 1) / sqrt(F)) (h of N(0, 1) rows is then N(0, 1)-scale),
    B ~ fp16(b_scale N(0, 1))"""
    A = f16(rng.standard_normal((r, F)) / np.sqrt(F))
    B = f16(rng.standard_normal((H, r)) * b_scale)
    return Adapter(A, B, 2.0 * r if alpha is None else alpha)


def apply_rows(x, y, slots, adapters, order="seq"):
    """The whole rule over a batch, float32 operations in `order`: (h [T][64]
    fp16, zero beyond each rank and on rows without an adapter; y' fp16)"""
    x, y = np.asarray(x), np.asarray(y)
    T = x.shape[0]
    h = np.zeros((T, R_MAX), np.float16)
    out = y.copy()
    for a, ad in adapters.items():
        rows = np.nonzero(np.asarray(slots) == a)[0]
        if rows.size == 0:
            continue
        hr = ad.h_f32(x[rows], order)
        h[rows, :ad.r] = hr
        out[rows] = ad.y_f32(y[rows], hr, order)
    return h, out
