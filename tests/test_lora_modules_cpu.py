"""LoRA on the attention projections, the parts that need no GPU: the PEFT
converter for q / k / v / o / down, the segmented rule of the fused qkv row
(tests/lora_qkv_rule.py) with the mistakes the GPU checks must be able to see,
and the new entry points of the C ABI."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F
import lora_qkv_rule as QR
import lora_rule as LR
from flexflow_amd import checkpoint

INVALID, UNSUPPORTED = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")
BLOCK = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
         "down_proj": "mlp"}
# a GQA shape: hidden 64, 4 heads of 16, 2 K/V heads, intermediate 96
L_, R_, HID, KV, FF = 3, 12, 64, 32, 96
DIMS = {"q_proj": (HID, HID), "k_proj": (HID, KV), "v_proj": (HID, KV), "o_proj": (HID, HID),
        "down_proj": (FF, HID)}


def peft_state(mods, rng, name="", layers=L_, r=R_):
    sd = {}
    for i in range(layers):
        for m in mods:
            p = f"base_model.model.model.layers.{i}.{BLOCK[m]}.{m}."
            sd[p + f"lora_A.{name}weight"] = rng.standard_normal((r, DIMS[m][0])).astype(np.float32)
            sd[p + f"lora_B.{name}weight"] = rng.standard_normal((DIMS[m][1], r)).astype(np.float32)
    return sd


@pytest.mark.parametrize("mods", [("q_proj", "v_proj"), ALL], ids=["q_v", "all_five"])
@pytest.mark.parametrize("name,dtype", [("", np.float16), ("default.", np.float32)])
def test_convert_peft_adapter_round_trip(tmp_path, mods, name, dtype):
    sd = peft_state(mods, np.random.default_rng(3), name)
    cfg = dict(peft_type="LORA", r=R_, lora_alpha=24, target_modules=list(mods))
    dst = str(tmp_path / "adapter")
    assert checkpoint.convert_peft_adapter(sd, cfg, dst, dtype=dtype) == (R_, 24.0)
    files = sorted(f for f in os.listdir(dst) if f != "adapter_config.json")
    assert files == sorted(f"layers.{i}.{BLOCK[m]}.{m}.lora_{ab}.weight"
                           for i in range(L_) for m in mods for ab in "AB")
    for i in range(L_):
        for m in mods:
            for ab, shape in (("A", (R_, DIMS[m][0])), ("B", (DIMS[m][1], R_))):
                fn = f"layers.{i}.{BLOCK[m]}.{m}.lora_{ab}.weight"
                assert os.path.getsize(os.path.join(dst, fn)) == shape[0] * shape[1] * np.dtype(dtype).itemsize
                got = np.fromfile(os.path.join(dst, fn), dtype).reshape(shape)
                src = sd[f"base_model.model.model.layers.{i}.{BLOCK[m]}.{m}.lora_{ab}.{name}weight"]
                assert (got == src.astype(dtype)).all()
    with open(os.path.join(dst, "adapter_config.json")) as f:
        assert json.load(f) == cfg


def test_convert_peft_adapter_refusals(tmp_path):
    rng = np.random.default_rng(4)
    conv = checkpoint.convert_peft_adapter
    cfg = lambda t, **kw: dict(r=R_, lora_alpha=8, target_modules=t, **kw)
    dst = str(tmp_path / "x")
    qv = peft_state(("q_proj", "v_proj"), rng)
    for targets in (["gate_proj"], ["q_proj", "up_proj"], [], None):
        with pytest.raises(ValueError):
            conv(peft_state(("q_proj",), rng), cfg(targets), dst)
    # a target without tensors, or with some of them
    with pytest.raises(ValueError):
        conv(qv, cfg(["q_proj", "v_proj", "o_proj"]), dst)
    with pytest.raises(ValueError):
        conv(peft_state(("down_proj",), rng), cfg(["down_proj", "q_proj"]), dst)
    part = dict(qv)
    del part["base_model.model.model.layers.1.self_attn.v_proj.lora_B.weight"]
    with pytest.raises(ValueError):
        conv(part, cfg(["q_proj", "v_proj"]), dst)
    # a tensor of a module that is not a target; a module in the wrong block
    with pytest.raises(ValueError):
        conv(qv, cfg(["q_proj"]), dst)
    with pytest.raises(ValueError):
        conv({k.replace("self_attn", "mlp"): v for k, v in qv.items()}, cfg(["q_proj", "v_proj"]), dst)
    for kw in (dict(rank_pattern={"q_proj": 4}), dict(alpha_pattern={"v_proj": 2.0})):
        with pytest.raises(ValueError):
            conv(qv, cfg(["q_proj", "v_proj"], **kw), dst)
    assert not os.path.exists(dst)  # nothing was written on the way to a refusal
    assert conv(qv, cfg(["q_proj", "v_proj"]), dst) == (R_, 8.0)


# ---------------------------------------------------------------- the segmented rule
WIDTHS = (256, 64, 64)  # boundaries at 256 and 320: inside the second 256-column block


def _qkv_case(seed, T=8, in_dim=352, r=12):
    rng = np.random.default_rng(seed)
    x = LR.f16(rng.standard_normal((T, in_dim)))
    y = LR.f16(rng.standard_normal((T, sum(WIDTHS) + LR.GUARD)))
    segs = [{0: LR.dense(r, in_dim, w, rng, b_scale=0.5)} for w in WIDTHS]
    return rng, x, y, segs


def _inside(out, x, y, slots, segs):
    """fraction of each segment's elements inside the dense intervals around the
    rule with the adapters `segs`, h taken from the rule itself"""
    frac = []
    for s, (c0, c1) in enumerate(QR.bounds(WIDTHS)):
        ad = segs[s][0]
        rows = slots == 0
        ref, e = ad.y_ref(np.ascontiguousarray(y[rows, c0:c1]), ad.h_f32(x[rows]))
        frac.append(float(LR.in_interval(np.ascontiguousarray(out[rows, c0:c1]), ref, e).mean()))
    return frac


def test_segmented_rule_is_the_rule_per_segment_and_sees_a_swapped_segment():
    rng, x, y, segs = _qkv_case(1)
    slots = np.array([0, 0, -1, 0, 0, -1, 0, 0], np.int32)
    h, out = QR.apply_qkv(x, y, slots, WIDTHS, segs)
    assert _inside(out, x, y, slots, segs) == [1.0, 1.0, 1.0]
    for order in ("rev", "pairwise"):  # any summation order stays inside
        assert _inside(QR.apply_qkv(x, y, slots, WIDTHS, segs, order)[1], x, y, slots, segs) == [1.0] * 3
    none = slots < 0
    assert (out[none].view(np.uint16) == y[none].view(np.uint16)).all() and not h[:, none].any()
    assert (out[:, sum(WIDTHS):].view(np.uint16) == y[:, sum(WIDTHS):].view(np.uint16)).all()
    # k's and v's adapters swapped (same shapes): both segments leave their intervals
    swapped = QR.apply_qkv(x, y, slots, WIDTHS, [segs[0], segs[2], segs[1]])[1]
    f = _inside(swapped, x, y, slots, segs)
    assert f[0] == 1.0 and f[1] < 0.2 and f[2] < 0.2, f
    # a segment's update written one segment further (the boundary ignored)
    shifted = y.copy()
    shifted[:, 64:320] = out[:, 0:256]
    assert max(_inside(shifted, x, y, slots, segs)[:2]) < 0.2
    # an adapter without a module: that segment's columns keep the input's bits
    h2, out2 = QR.apply_qkv(x, y, slots, WIDTHS, [segs[0], {}, segs[2]])
    assert (out2[:, 256:320].view(np.uint16) == y[:, 256:320].view(np.uint16)).all() and not h2[1].any()
    assert (out2[:, :256].view(np.uint16) == out[:, :256].view(np.uint16)).all()
    assert _inside(out2, x, y, slots, segs)[1] < 0.2


def test_a_kv_b_that_was_not_replicated_leaves_the_interval():
    heads, kvh, d, in_dim, r, T = 4, 2, 16, 352, 12, 6
    rng = np.random.default_rng(2)
    x = LR.f16(rng.standard_normal((T, in_dim)))
    y = LR.f16(rng.standard_normal((T, heads * d)))
    hf = LR.dense(r, in_dim, kvh * d, rng, b_scale=0.5)  # the adapter as PEFT stores it
    rep = QR.replicate_kv(hf.B, heads, kvh, d)
    assert rep.shape == (heads * d, r)
    for h in range(heads):
        assert (rep[h * d:(h + 1) * d] == hf.B[(h // 2) * d:(h // 2 + 1) * d]).all()
    good = LR.Adapter(hf.A, rep, hf.alpha)
    hh = good.h_f32(x)
    ref, e = good.y_ref(y, hh)
    assert LR.in_interval(good.y_f32(y, hh), ref, e).all()
    # the B tiled instead (row n of the replicated K takes row n % (kvh * d)): heads 1 and 2 wrong
    tiled = LR.Adapter(hf.A, np.ascontiguousarray(np.tile(hf.B, (heads // kvh, 1))), hf.alpha)
    ok = LR.in_interval(tiled.y_f32(y, hh), ref, e)
    assert ok[:, :d].all() and ok[:, 3 * d:].all() and ok[:, d:3 * d].mean() < 0.2
    # MHA: nothing to replicate
    assert (QR.replicate_kv(hf.B, kvh, kvh, d) == hf.B).all()


# ---------------------------------------------------------------- the C ABI
NEW = ("ffmi_model_lora_load_modules", "ffmi_model_lora_load_folder_ex", "ffmi_lora_apply_qkv",
       "ffmi_lora_qkv_workspace_bytes")


@pytest.mark.parametrize("name", NEW)
def test_new_functions_are_declared_bound_and_exported(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ffmi.h")).read(), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", src) and name in F.SIGNATURES and hasattr(F.lib(), name)


def test_module_ids_match_the_header():
    src = open(os.path.join(ROOT, "include", "ffmi.h")).read()
    for hf, macro in (("q_proj", "Q"), ("k_proj", "K"), ("v_proj", "V"), ("o_proj", "O"),
                      ("down_proj", "DOWN"), ("gate_proj", "GATE"), ("up_proj", "UP")):
        m = re.search(rf"#define FFMI_LORA_{macro} (\d+)\s", src)
        assert m and int(m.group(1)) == F.LORA_MODULES[hf], hf
    assert ctypes.sizeof(F.LoraModule) == 24
    assert F.lib().ffmi_version().decode() == "ffmi 0.4 (gfx950)"  # by addition only


def test_a_model_without_the_flag_refuses_modules_and_argument_checks():
    """(the BEAM hash model stands for any model that serves no adapters)"""
    L = F.lib()
    ssm = fa.HashModel(1000, "beam")
    out = ctypes.c_int(-1)
    mods = (F.LoraModule * 1)(F.LoraModule(F.LORA_MODULES["q_proj"], None, None))
    assert L.ffmi_model_lora_load_modules(ssm.handle, 8, 16.0, 1, mods, ctypes.byref(out)) == UNSUPPORTED
    assert "lora" in L.ffmi_last_error().decode()
    assert L.ffmi_model_lora_load_folder_ex(ssm.handle, b"/nonexistent", 8, 16.0, 1 | 4,
                                            ctypes.byref(out)) == UNSUPPORTED
    assert "lora" in L.ffmi_last_error().decode()
    assert L.ffmi_model_lora_load_modules(None, 8, 16.0, 1, mods, ctypes.byref(out)) == INVALID
    assert L.ffmi_model_lora_load_folder_ex(None, b"/nonexistent", 8, 16.0, 1, ctypes.byref(out)) == INVALID
    assert L.ffmi_lora_qkv_workspace_bytes(5, 352) == 3 * 2 * 5 * 64 * 4
    assert L.ffmi_lora_qkv_workspace_bytes(0, 352) == 0
    assert L.ffmi_lora_apply_qkv(None, 1, 32, None, None, None, None, 0, 0, None, 0, None, None) == INVALID


def test_one_module_down_is_lora_load_on_every_model():
    """ffmi_model_lora_load_modules with down_proj alone answers as
    ffmi_model_lora_load does, also on a model that only overrides that one
    (the INC hash model); an attention module there is refused."""
    L = F.lib()
    llm = fa.HashModel(1000, "inc")
    out = ctypes.c_int(-1)
    down = (F.LoraModule * 1)(F.LoraModule(F.LORA_MODULES["down_proj"], None, None))
    assert L.ffmi_model_lora_load_modules(llm.handle, 65, 16.0, 1, down, ctypes.byref(out)) == \
        L.ffmi_model_lora_load(llm.handle, 65, 16.0, None, None, ctypes.byref(out)) == UNSUPPORTED
    assert "rank" in L.ffmi_last_error().decode()
    q = (F.LoraModule * 1)(F.LoraModule(F.LORA_MODULES["q_proj"], None, None))
    assert L.ffmi_model_lora_load_modules(llm.handle, 8, 16.0, 1, q, ctypes.byref(out)) == UNSUPPORTED
    assert "lora" in L.ffmi_last_error().decode()
