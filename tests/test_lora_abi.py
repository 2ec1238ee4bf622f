"""The LoRA additions to the C ABI (include/ffmi.h): declared, bound, exported,
and the refusals that need no GPU."""
import ctypes
import os
import re

import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F

INVALID, UNSUPPORTED = 1, 5
NEW = ("ffmi_model_lora_load", "ffmi_model_lora_load_folder", "ffmi_model_lora_unload",
       "ffmi_lora_apply", "ffmi_lora_workspace_bytes", "ffmi_rm_register_request_ex")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "ffmi.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_new_functions_are_declared_bound_and_exported(name):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(rf"\b{name}\s*\(", src) and name in F.SIGNATURES and hasattr(F.lib(), name)


def test_constants_match_the_header():
    src = header()
    for name, val in (("FFMI_MODEL_LORA", F.MODEL_LORA), ("FFMI_LORA_MAX_ADAPTERS", F.LORA_MAX_ADAPTERS),
                      ("FFMI_LORA_MAX_RANK", F.LORA_MAX_RANK)):
        m = re.search(rf"#define {name} (\d+)u?\s", src)
        assert m and int(m.group(1)) == val, name
    assert (F.MODEL_LORA, F.LORA_MAX_ADAPTERS, F.LORA_MAX_RANK) == (4, 8, 64)
    assert ctypes.sizeof(F.LoraEntry) == 24
    assert F.lib().ffmi_version().decode() == "ffmi 0.4 (gfx950)"  # by addition only


def _opts(mode=F.MODEL_INC, tp_size=1, full_precision=0):
    return F.ModelOpts(mode, 0, tp_size, None, 2, 16, 64, 0, 1, 0, None, 0, full_precision)


def test_model_flag_refusals_before_the_device():
    L = F.lib()
    c = F.LlamaConfig.from_dict(dict(num_layers=1, vocab_size=1000, num_heads=8, hidden=512,
                                     intermediate=1024))
    m = ctypes.c_void_p()
    for o in (_opts(mode=F.MODEL_BEAM), _opts(full_precision=1), _opts(tp_size=2)):
        for flags in (F.MODEL_LORA, F.MODEL_LORA | F.MODEL_NATIVE_GQA):
            assert L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(o), flags,
                                          ctypes.byref(m)) == UNSUPPORTED
            assert "lora" in L.ffmi_last_error().decode()
    for unknown in (2, 8):  # (2 is left unassigned between the two flags)
        assert L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(_opts()), F.MODEL_LORA | unknown,
                                      ctypes.byref(m)) == INVALID


def test_a_model_without_the_flag_refuses_adapters():
    """(the BEAM hash model stands for any model that serves no adapters)"""
    L = F.lib()
    ssm = fa.HashModel(1000, "beam")
    out = ctypes.c_int(-1)
    for st in (L.ffmi_model_lora_load(ssm.handle, 8, 16.0, None, None, ctypes.byref(out)),
               L.ffmi_model_lora_load_folder(ssm.handle, b"/nonexistent", 8, 16.0, ctypes.byref(out)),
               L.ffmi_model_lora_unload(ssm.handle, 0)):
        assert st == UNSUPPORTED and "lora" in L.ffmi_last_error().decode()
    assert L.ffmi_model_lora_load(None, 8, 16.0, None, None, ctypes.byref(out)) == INVALID
    assert L.ffmi_model_lora_unload(None, 0) == INVALID
    llm = fa.HashModel(1000, "inc")
    assert L.ffmi_model_lora_load(llm.handle, 65, 16.0, None, None, ctypes.byref(out)) == UNSUPPORTED
    assert "lora" in L.ffmi_last_error().decode()


def test_register_request_ex_and_kernel_entry_argument_checks():
    L = F.lib()
    rm = fa.RequestManager(max_sequence_length=64)
    arr = F.int_array([5, 6, 7])
    assert L.ffmi_rm_register_request_ex(rm.handle, arr, 3, 20, -1, 1, -1) > 0  # == the old entry
    assert L.ffmi_rm_register_request_ex(rm.handle, arr, 3, 20, -1, 1, 3) == 0   # not loaded
    assert L.ffmi_rm_register_request_ex(None, arr, 3, 20, -1, 1, -1) == 0
    assert L.ffmi_lora_workspace_bytes(5, 352) == 2 * 5 * 64 * 4
    assert L.ffmi_lora_workspace_bytes(0, 352) == 0
    assert L.ffmi_lora_apply(None, 1, 32, 64, None, None, None, 0, None, 0, None, None) == INVALID
