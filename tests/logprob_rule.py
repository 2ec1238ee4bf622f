"""The per-token log-probability rule (include/ffmi.h ffmi_token_logprobs) in
float64 numpy on the same fp16 row, for the kernel and model tests.

    z  = x                                        (temperature == 0)
    z  = R16(float(x) / float(R16(temperature)))  (temperature > 0: sampling_rule.scaled_logits)
    M  = max z;  S = sum exp(z - M);  lp = (z_s - M) - log(S)

The bar |lp - ref| <= 2^-16 + 2^-21 |ref| is derived, not measured: about ten
times the error of the same formula in fp32 with 4096-element chunks combined
in order (1.6e-6 at worst over V 1 .. 128256, N(0, 1.28), N(0, 8) clipped to
+-32, one-hot +-32 and +-65504 rows), which leaves room for the hardware exp
and log.  A wrong rule lands far outside it: a missing R16 on the scaled logit
moves z by its fp16 quantum, >= 1e-3 at |z| ~ 4.
"""
import numpy as np

from sampling_rule import scaled_logits


def z_rows(x16, temperature):
    """The rows the rule runs on, fp16."""
    x16 = np.asarray(x16, np.float16)
    return x16 if temperature == 0 else scaled_logits(x16, temperature)


def logprobs(x16, temperature, ids):
    """float64 lp of ids[t] in row t of x16 [T][V]."""
    z = z_rows(x16, temperature).astype(np.float64)
    ids = np.asarray(ids, np.int64)
    M = z.max(axis=1)
    S = np.exp(z - M[:, None]).sum(axis=1)
    return (z[np.arange(z.shape[0]), ids] - M) - np.log(S)


def bar(ref):
    return 2.0 ** -16 + 2.0 ** -21 * np.abs(np.asarray(ref, np.float64))


def assert_within_bar(lp, ref, what=None):
    lp, ref = np.asarray(lp, np.float64), np.asarray(ref, np.float64)
    err = np.abs(lp - ref)
    bad = np.nonzero(~(err <= bar(ref)))[0]  # (a NaN fails)
    assert bad.size == 0, (what, bad[:8], lp[bad[:8]], ref[bad[:8]], err[bad[:8]])
