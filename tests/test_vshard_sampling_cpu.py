"""Host side of vocab-sharded top-p sampling (no GPU): the two entry points,
the scratch size, the argument checks (all decided before any HIP call) and the
numpy twin of the kernel's phase algorithm (tests/vshard_sampling_rule.py)
against the rule (tests/sampling_rule.py pick) on fp16 probability rows.
"""
import ctypes

import numpy as np
import pytest

import flexflow_amd.ffmi as F
import sampling_rule as R
import vshard_sampling_rule as VR

INVALID, UNSUPPORTED = 1, 5


def test_entry_points_exist_and_are_bound():
    for name in ("ffmi_vocab_shard_sample_scratch_bytes", "ffmi_vocab_shard_sample_topp"):
        assert name in F.SIGNATURES, name
        raw = ctypes.CDLL(F.LIB_PATH)
        assert getattr(raw, name) is not None
        assert getattr(F.lib(), name).argtypes == F.SIGNATURES[name][1]
    assert F.lib().ffmi_version() == b"ffmi 0.4 (gfx950)"


def test_scratch_bytes():
    n = F.lib().ffmi_vocab_shard_sample_scratch_bytes
    for bad in ((0, 4, 100), (-1, 4, 100), (2, 0, 100), (2, -3, 100), (2, 4, 0), (2, 4, -1)):
        assert n(*bad) == 0, bad
    for P in (1, 2, 4, 8):
        prev_t = 0
        for T in (1, 2, 3, 31, 32, 33, 64, 257, 1024):
            prev_v = 0
            for Vl in (1, 2, 127, 128, 4000, 32000, 983040):
                b = n(P, T, Vl)
                assert b >= T * Vl * 2 and b >= prev_v, (P, T, Vl)
                prev_v = b
            assert n(P, T, 4000) > prev_t
            prev_t = n(P, T, 4000)
        # the exchange records stop growing at the chunk: 256 KiB per exchange
        assert n(P, 4096, 16) - n(P, 2048, 16) <= 2048 * (16 * 2 + 32) + 512


@pytest.fixture(scope="module")
def comm():
    h = ctypes.c_void_p()
    F.check(F.lib().ffmi_comm_create_peer(8, 7, ctypes.byref(h)))
    yield h
    F.lib().ffmi_comm_destroy(h)


def test_argument_checks_need_no_device(comm):
    """Every refusal is decided before the first HIP call: null or dangling
    device pointers are never touched."""
    L = F.lib()
    T, Vl = 4, 100
    nb = L.ffmi_vocab_shard_sample_scratch_bytes(8, T, Vl)
    p = ctypes.c_void_p(0x1000)  # never dereferenced

    def call(c=comm, logits=p, T=T, Vl=Vl, temperature=0.9, topp=0.8, u=p, ids=p, probs=None,
             scratch=p, nbytes=nb):
        return L.ffmi_vocab_shard_sample_topp(c, logits, T, Vl, temperature, topp, u, ids, probs,
                                              scratch, nbytes, None)

    for bad in (dict(c=None), dict(logits=None), dict(u=None), dict(ids=None), dict(T=-1),
                dict(Vl=0), dict(Vl=-5), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float("nan")), dict(topp=0.0), dict(topp=-0.5), dict(topp=1.5),
                dict(topp=float("nan")), dict(scratch=None), dict(nbytes=nb - 1), dict(nbytes=0)):
        assert call(**bad) == INVALID, bad
    big = 1 << 62
    assert call(Vl=983041, nbytes=big) == UNSUPPORTED
    assert call(Vl=1 << 30, nbytes=big) == UNSUPPORTED  # also (rank + 1) * Vl > 2^31 - 1
    # T == 0: nothing to do, no scratch needed
    assert call(T=0, scratch=None, nbytes=0) == F.FFMI_OK


# --- the numpy twin against the rule ----------------------------------------


def prob_rows(rng, V):
    """fp16 probability rows whose mass stays below 2^24 units, so that every
    integer target up to the mass + 1 is a float32 u: random softmax, flat,
    two-value ties, peaked."""
    z = rng.standard_normal(V) * rng.choice([0.05, 1.28, 3.0])
    e = np.exp(z - z.max())
    rows = [(e / e.sum() * 0.98).astype(np.float16),
            np.full(V, np.float16(0.9 / V)),
            rng.choice(np.array([0.9 / V, 0.45 / V], np.float16), V),
            np.where(np.arange(V) == rng.integers(V), np.float16(0.97), np.float16(0.02 / V))]
    if V >= 4:  # zeros (the -inf logits) at random places
        r = rows[0].copy()
        r[rng.random(V) < 0.3] = 0
        rows.append(r)
    return [np.asarray(r, np.float16) for r in rows]


def rule_pick(p16, target):
    """R.pick on the row sorted (p desc, index asc) with topp = 1 and
    u = target * 2^-24 (exact in float32 for target <= 2^24)."""
    assert target <= 1 << 24
    u = np.float32(target * 2.0 ** -24)
    assert VR.target_of(1.0, u) == target
    p = p16.astype(np.float32)
    order = np.lexsort((np.arange(p.size), -p))
    ids, pr = R.pick(order[None].astype(np.int32), p[order][None], 1.0, [u])
    return int(ids[0]), np.float32(pr[0])


@pytest.mark.parametrize("P", [1, 2, 4, 8])
def test_phase_algorithm_is_the_rule(P):
    rng = np.random.default_rng(90 + P)
    n = 0
    for Vl in (1, 2, 3, 17, 128, 500):
        for p16 in prob_rows(rng, P * Vl):
            keys = p16.view(np.uint16)
            total = int(VR.p_mass(keys).sum())
            assert 0 < total < (1 << 24) - 1
            targets = {1, total - 1, total, total + 1} | {int(x) for x in rng.integers(1, total + 1, 12)}
            for target in sorted(t for t in targets if t >= 1):
                gid, key = VR.pick_keys(keys, P, target)
                rid, rp = rule_pick(p16, target)
                assert gid == rid, (P, Vl, target, total, gid, rid)
                assert np.uint16(key).view(np.float16).astype(np.float32) == rp
                n += 1
    assert n > 300


def test_target_is_the_kernels_expression():
    """ceil(t * 2^24) with the clamps of sample_topp_kernel."""
    assert VR.target_of(1.0, 2.0 ** -24) == 1
    assert VR.target_of(1.0, 1.0) == 1 << 24
    assert VR.target_of(0.5, 1.0) == 1 << 22
    assert VR.target_of(2.0 ** -6, 2.0 ** -24) == 1  # t * 2^24 = 2^-12 rounds up to 1
    tp = np.float64(np.float32(0.8))
    assert VR.target_of(0.8, 0.3) == int(np.ceil(np.float64(np.float32(0.3)) * tp * tp * 2 ** 24))
