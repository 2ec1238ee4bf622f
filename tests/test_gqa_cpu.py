"""Native GQA entry points without a device: the three refusals of
ffmi_attn_create_gqa are decided before any HIP call, and the new functions
are declared, bound and exported."""
import ctypes
import os
import re

import pytest

import flexflow_amd.ffmi as F

INVALID, UNSUPPORTED = 1, 5
NEW = ["ffmi_attn_create_gqa", "ffmi_attn_cache_bytes", "ffmi_attn_set_gqa_route",
       "ffmi_model_create_ex", "ffmi_model_kv_cache_bytes"]


def cfg(heads=8, d=128, full_precision=0, mode=None):
    return F.AttnCfg(F.ATTN_INC if mode is None else mode, heads, d, 2, 64, 0, 16, 0.125, 10000.0,
                     0, 0, 1.0, 1.0, 4.0, 8192, full_precision)


def create(c, kvh):
    h = ctypes.c_void_p()
    st = F.lib().ffmi_attn_create_gqa(ctypes.byref(c), kvh, ctypes.byref(h))
    assert st != 0 and not h.value
    return st, F.lib().ffmi_last_error().decode()


def test_status_codes_are_the_headers():
    assert F.STATUS[INVALID] == "invalid argument" and F.STATUS[UNSUPPORTED] == "unsupported"


def test_kv_heads_must_divide_heads():
    for kvh in (3, 5, 7, 16):
        assert create(cfg(heads=8), kvh)[0] == INVALID


def test_full_precision_gqa_is_refused_by_name():
    st, msg = create(cfg(full_precision=1), 2)
    assert st == UNSUPPORTED and "gqa" in msg


def test_head_dim_32_gqa_is_refused_by_name():
    st, msg = create(cfg(d=32), 2)
    assert st == UNSUPPORTED and "gqa" in msg


def test_null_arguments():
    L = F.lib()
    h = ctypes.c_void_p()
    assert L.ffmi_attn_create_gqa(None, 2, ctypes.byref(h)) == INVALID
    assert L.ffmi_attn_create_gqa(ctypes.byref(cfg()), 2, None) == INVALID
    assert L.ffmi_attn_cache_bytes(None) == 0
    assert L.ffmi_attn_set_gqa_route(None, 0) == INVALID
    m = ctypes.c_void_p()
    assert L.ffmi_model_create_ex(None, None, 1, ctypes.byref(m)) == INVALID


def test_model_flag_refusals_before_the_device():
    L = F.lib()
    c = F.LlamaConfig.from_dict(dict(num_layers=1, vocab_size=1000, num_heads=8, num_kv_heads=2,
                                     hidden=512, intermediate=1024, rms_eps=1e-6,
                                     rope_theta=10000.0))
    m = ctypes.c_void_p()
    o = F.ModelOpts(F.MODEL_INC, 0, 1, None, 2, 16, 64, 0, 1, 0, None, 0, 1)  # full_precision
    assert L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(o), F.MODEL_NATIVE_GQA,
                                  ctypes.byref(m)) == UNSUPPORTED
    assert "native_gqa" in L.ffmi_last_error().decode()
    o = F.ModelOpts(F.MODEL_INC, 0, 1, None, 2, 16, 64, 0, 1, 0, None, 0, 0)
    assert L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(o), 2, ctypes.byref(m)) == INVALID


@pytest.mark.parametrize("name", NEW)
def test_new_functions_are_declared_bound_and_exported(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ffmi.h")).read(), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", src) and name in F.SIGNATURES and hasattr(F.lib(), name)


def test_version_string_is_unchanged():
    assert F.lib().ffmi_version().decode() == "ffmi 0.4 (gfx950)"
