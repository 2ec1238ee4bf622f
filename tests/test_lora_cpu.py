"""The LoRA rule's bounds are derived, not fitted (tests/lora_rule.py), and the
PEFT adapter converter round-trips.  No GPU."""
import json
import os

import numpy as np
import pytest

import lora_rule as LR
from flexflow_amd import checkpoint

ORDERS = ("seq", "rev", "pairwise")


def _case(seed, T=6, F=352, H=48, r=12):
    rng = np.random.default_rng(seed)
    x = LR.f16(rng.standard_normal((T, F)))
    y = LR.f16(rng.standard_normal((T, H)))
    return rng, x, y, LR.dense(r, F, H, rng)


@pytest.mark.parametrize("F,r", [(352, 12), (1376, 16), (2752, 64)])
def test_h_bound_holds_for_any_order(F, r):
    rng, x, _, ad = _case(F + r, T=4, F=F, H=16, r=r)
    ref, e = ad.h_ref(x)
    ratios = []
    for order in ORDERS:
        s = LR.sum_f32(LR.products(x, ad.A), order).astype(np.float64)
        err = np.abs(s - ref)
        assert (err <= e).all(), order
        ratios.append(float((err / e).max()))
        assert LR.in_interval(ad.h_f32(x, order), ref, e).all(), order
    # far inside: the worst case needs every rounding to go the same way
    assert max(ratios) < 0.05, ratios


def test_y_bound_holds_for_any_order():
    for seed in range(3):
        rng, x, y, ad = _case(seed, r=(12, 16, 64)[seed])
        h = ad.h_f32(x)
        ref, e = ad.y_ref(y, h)
        for order in ORDERS:
            d = LR.sum_f32(LR.products(h, ad.B), order)
            v = y.astype(np.float32) + np.float32(ad.s16) * d  # the two fp32 roundings
            assert (np.abs(v.astype(np.float64) - ref) <= e).all(), order
            assert LR.in_interval(ad.y_f32(y, h, order), ref, e).all(), order


def test_a_dropped_k_slice_leaves_the_h_interval():
    rng, x, _, ad = _case(7, T=8, F=1024, r=16)
    ref, e = ad.h_ref(x)
    keep = np.r_[0:512, 544:1024]  # one 32-column k-step of 32 missing
    ok = LR.in_interval(ad.h_f32(x, cols=keep), ref, e)
    assert ok.mean() < 0.2, ok.mean()


def test_a_swapped_adapter_leaves_both_intervals():
    rng, x, y, ad = _case(8)
    other = LR.dense(ad.r, ad.F, ad.H, rng)
    ref, e = ad.h_ref(x)
    assert LR.in_interval(other.h_f32(x), ref, e).mean() < 0.05
    h = ad.h_f32(x)
    ref, e = ad.y_ref(y, h)
    assert LR.in_interval(other.y_f32(y, h), ref, e).mean() < 0.2
    # and an update that is not applied at all
    assert LR.in_interval(y, ref, e).mean() < 0.2


def test_rows_without_adapter_are_untouched_and_rows_are_independent():
    rng, x, y, a0 = _case(9, T=40)
    a1, a2 = LR.dense(16, a0.F, a0.H, rng), LR.dense(1, a0.F, a0.H, rng)
    ads = {0: a0, 1: a1, 2: a2}
    slots = LR.slots_of(LR.MIXED_40)
    h, out = LR.apply_rows(x, y, slots, ads)
    none = slots < 0
    assert (out[none].view(np.uint16) == y[none].view(np.uint16)).all() and not h[none].any()
    assert (out[~none] != y[~none]).mean() > 0.5
    for t in (0, 4, 21, 39):
        h1, o1 = LR.apply_rows(x[t:t + 1], y[t:t + 1], slots[t:t + 1], ads)
        assert (h1.view(np.uint16) == h[t].view(np.uint16)).all()
        assert (o1.view(np.uint16) == out[t].view(np.uint16)).all()


def test_selector_is_exact_and_subnormal_sources_stay_under_the_cap():
    tally = LR.Tally()
    for seed, (F, H) in enumerate(LR.SHAPES):
        for r in LR.RANKS:
            rng = np.random.default_rng([seed, r])
            sel = LR.Selector(r, F, H, seed)
            assert (np.count_nonzero(sel.A, axis=1) == 1).all()
            assert (np.count_nonzero(sel.B, axis=1) == 1).all()
            x = LR.f16(rng.standard_normal((64, F)))
            y = LR.f16(rng.standard_normal((64, H)))
            for order in ORDERS:  # one exact product among zeros: any order, the same bits
                h = sel.h_f32(x, order)
                sel.check_h(h, x, tally)
                assert (sel.y_f32(y, h, order).view(np.uint16) ==
                        sel.want_y(y, h).view(np.uint16)).all()
            # a wrong index is seen: a row of h moved by one
            with pytest.raises(AssertionError):
                sel.check_h(np.roll(sel.h_f32(x), 1, axis=0), x, LR.Tally())
    seen = tally.finish()
    # N(0, 1)-scale inputs: far under the 0.1 % cap the GPU test applies
    assert seen["subnormal_sources"] <= 0.3 * LR.SUBNORMAL_CAP * seen["compared"], seen


def _peft_state(L, r, F, H, rng, name=""):
    sd = {}
    for i in range(L):
        p = f"base_model.model.model.layers.{i}.mlp.down_proj."
        sd[p + f"lora_A.{name}weight"] = rng.standard_normal((r, F)).astype(np.float32)
        sd[p + f"lora_B.{name}weight"] = rng.standard_normal((H, r)).astype(np.float32)
    return sd


@pytest.mark.parametrize("name,dtype", [("", np.float16), ("default.", np.float32)])
def test_convert_peft_adapter_round_trip(tmp_path, name, dtype):
    L, r, F, H = 3, 12, 96, 64
    sd = _peft_state(L, r, F, H, np.random.default_rng(3), name)
    cfg = dict(peft_type="LORA", r=r, lora_alpha=24, target_modules=["down_proj"])
    dst = str(tmp_path / "adapter")
    assert checkpoint.convert_peft_adapter(sd, cfg, dst, dtype=dtype) == (r, 24.0)
    files = sorted(f for f in os.listdir(dst) if f != "adapter_config.json")
    assert files == sorted(f"layers.{i}.mlp.down_proj.lora_{ab}.weight"
                           for i in range(L) for ab in "AB")
    for i in range(L):
        for ab, shape in (("A", (r, F)), ("B", (H, r))):
            got = np.fromfile(os.path.join(dst, f"layers.{i}.mlp.down_proj.lora_{ab}.weight"),
                              dtype).reshape(shape)
            src = sd[f"base_model.model.model.layers.{i}.mlp.down_proj.lora_{ab}.{name}weight"]
            assert (got == src.astype(dtype)).all()
    with open(os.path.join(dst, "adapter_config.json")) as f:
        assert json.load(f)["r"] == r


def test_convert_peft_adapter_refuses_other_targets(tmp_path):
    sd = _peft_state(1, 4, 32, 32, np.random.default_rng(4))
    for targets in (["down_proj", "q_proj"], ["up_proj"], []):
        with pytest.raises(ValueError):
            checkpoint.convert_peft_adapter(sd, dict(r=4, lora_alpha=8, target_modules=targets),
                                            str(tmp_path / "x"))
    sd["base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"] = np.zeros((4, 32))
    with pytest.raises(ValueError):
        checkpoint.convert_peft_adapter(sd, dict(r=4, lora_alpha=8, target_modules=["down_proj"]),
                                        str(tmp_path / "y"))
