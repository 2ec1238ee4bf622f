"""The phase algorithm of ffmi_vocab_shard_sample_topp (sampling.hip
vshard_sample_kernel) restated in numpy on the fp16 keys of p: what each rank
sends in the last three exchanges and what every rank derives from the sums.
The integer arithmetic here is the kernel's; tests/sampling_rule.py is the rule
it must reproduce.

    mass(key) = p / 2^-24 (an integer: every fp16 p <= 1 is a multiple of 2^-24)
    target    = ceil(t * 2^24), t = (double(u) * topp) * topp, clamped to [1, 4e9]
    coarse    : per rank, the mass of each of the 121 buckets key >> 7, and the
                rank's last token of the order (lowest key, highest index)
      -> B, the first bucket from the top at which the cumulative mass over the
         ranks reaches target, c = the mass above B; none: the fallback, the
         lowest key over the ranks, then the highest global index
    fine      : per rank, the tokens per key for the 128 keys of B
      -> K, the first key from the top of B at which c + (count over ranks) *
         mass(key) reaches target; r = ceil((target - c_K) / mass(K)) - 1, the
         rank of the pick among K's tokens in global index order; the owner is
         the first rank whose prefix of counts exceeds r
    owner     : its (r - prefix)-th local token holding K
"""
import numpy as np

KEYS = 0x3C00 + 1
BUCKETS = (KEYS + 127) // 128  # 121


def p_mass(key):
    key = np.asarray(key, np.int64)
    e, m = key >> 10, key & 1023
    return np.where(e > 0, (1024 + m) << np.maximum(e - 1, 0), m)


def target_of(topp, u):
    tp = np.float64(np.float32(topp))
    t = (np.float64(np.float32(u)) * tp) * tp
    return int(min(max(np.ceil(t * 16777216.0), 1.0), 4.0e9))


def pick_keys(keys, P, target):
    """(global id, key) of the pick of one row; keys [P * Vl] uint16 (fp16 bits
    of p, every p in [0, 1]), rank r holding [r * Vl, (r + 1) * Vl)."""
    keys = np.asarray(keys, np.uint16).astype(np.int64)
    Vl = keys.size // P
    assert Vl * P == keys.size and keys.max() < KEYS
    shard = keys.reshape(P, Vl)
    mass = p_mass(shard)
    # exchange 3: coarse histograms + fallback candidates
    coarse = np.zeros((P, BUCKETS), np.int64)
    for r in range(P):
        np.add.at(coarse[r], shard[r] >> 7, mass[r])
    low = shard.min(axis=1)
    last = np.array([np.nonzero(shard[r] == low[r])[0][-1] + r * Vl for r in range(P)])
    tot, c, B = coarse.sum(axis=0), 0, -1
    for b in range(BUCKETS - 1, -1, -1):
        if c + tot[b] >= target:
            B = b
            break
        c += tot[b]
    if B < 0:
        r = max(range(P), key=lambda q: (-low[q], q))
        return int(last[r]), int(low[r])
    # exchange 4: token counts of bucket B's 128 keys
    cnt = np.zeros((P, 128), np.int64)
    for r in range(P):
        sel = shard[r][(shard[r] >> 7) == B]
        np.add.at(cnt[r], sel & 127, 1)
    ctot = cnt.sum(axis=0)
    for j in range(127, -1, -1):
        K = B * 128 + j
        m = int(ctot[j]) * int(p_mass(K)) if K < KEYS else 0
        if m and c + m >= target:
            break
        c += m
    else:
        raise AssertionError("bucket B does not reach the target")
    pm = int(p_mass(K))
    rk = (target - c + pm - 1) // pm - 1
    pre = 0
    for r in range(P):
        if rk - pre < cnt[r, j]:
            # exchange 5: the owner's id
            return int(np.nonzero(shard[r] == K)[0][rk - pre] + r * Vl), K
        pre += int(cnt[r, j])
    raise AssertionError("no owner")
