"""Host side of top-p sampling (no GPU): the per-token draw
ffmi_sampling_counter (include/ffmi.h) and the GenerationConfig defaults.
"""
import numpy as np

import flexflow_amd as fa
import flexflow_amd.ffmi as F

MASK = 2 ** 64 - 1


def splitmix_counter(seed, guid, pos):
    """The header's definition, restated."""
    x = (seed ^ ((guid & MASK) * 0x9E3779B97F4A7C15) ^ ((pos & MASK) * 0xD1342543DE82EF95)) & MASK
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return (x ^ (x >> 31)) >> 40


def test_sampling_counter_golden_values():
    golden = {(0, 0, 0): 14819496, (1, 1000000, 0): 1628165, (1, 1000000, 1): 4459075,
              (2, 1000000, 0): 10949382, (1, 1000001, 0): 15293861,
              (MASK, -1, 2047): 6366426, (20250117, 1000063, 1023): 16357410}
    for args, want in golden.items():
        assert F.sampling_counter(*args) == want == splitmix_counter(*args), args
    # seed, guid and pos each change the draw
    assert len({golden[k] for k in [(1, 1000000, 0), (1, 1000000, 1), (2, 1000000, 0),
                                    (1, 1000001, 0)]}) == 4


def test_sampling_counter_is_24_bits_and_matches_the_header_formula():
    rng = np.random.default_rng(1)
    for _ in range(2000):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
        guid = int(rng.integers(-2 ** 62, 2 ** 62))
        pos = int(rng.integers(0, 2 ** 20))
        c = F.sampling_counter(seed, guid, pos)
        assert 0 <= c < 2 ** 24 and c == splitmix_counter(seed, guid, pos), (seed, guid, pos)


def test_sampling_uniforms_pass_kolmogorov_smirnov():
    """65536 draws (guids 1000000..1000063 x positions 0..1023, seed 1): the
    Kolmogorov-Smirnov distance of u = (counter + 1) * 2^-24 from the uniform
    distribution is below 1.95 / sqrt(n), the 0.1% critical value.  The draws
    are fixed, so this is a property of the generator, not a flaky test."""
    u = np.sort(np.array([(F.sampling_counter(1, g, p) + 1) * 2.0 ** -24
                          for g in range(1000000, 1000064) for p in range(1024)]))
    n = len(u)
    assert n == 65536 and u[0] > 0.0 and u[-1] <= 1.0
    i = np.arange(1, n + 1)
    d = max((i / n - u).max(), (u - (i - 1) / n).max())
    print("KS distance", d, "bound", 1.95 / np.sqrt(n))
    assert d < 1.95 / np.sqrt(n), d


def test_generation_config_defaults():
    gc = fa.GenerationConfig()
    assert (gc.do_sample, gc.temperature, gc.topp, gc.topk) == (False, 0.9, 0.8, 1)
    gc = fa.GenerationConfig(True, 0.7, 0.95, 4)
    assert (gc.do_sample, gc.temperature, gc.topp, gc.topk) == (True, 0.7, 0.95, 4)
    assert fa.serve.GenerationConfig is fa.GenerationConfig
    assert F.lib().ffmi_version() == b"ffmi 0.4 (gfx950)"
