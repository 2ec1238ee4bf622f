"""The W4A8 additions to the C ABI that need no GPU: workspace size, refusals
(naming "w4a8") and the rules of FFMI_MODEL_W4 | FFMI_MODEL_A8."""
import ctypes

import pytest

import flexflow_amd as fa
import flexflow_amd.ffmi as F

INVALID, UNSUPPORTED = 1, 5


def refused(fn, st, *args):
    assert fn(*args) == st and "w4a8" in F.lib().ffmi_last_error().decode(), args


def test_linear_w4a8_refusals_and_the_one_pass_workspace():
    L = F.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # (never dereferenced: every call below is refused first)
    for T in (1, 64, 168, 300):  # S = 8 slabs of min(T, 256) rows x 16 padded columns
        assert L.ffmi_linear_w4a8_workspace_bytes(T, 16, 4096, 0) == 8 * min(T, 256) * 16 * 4
        assert L.ffmi_linear_w4a8_workspace_bytes(T, 16, 4096, F.EPI_SILU_MUL) == 0
    gemm = L.ffmi_linear_w4a8
    for i in range(5):  # X8, row scales, W4, scale bytes, Y
        ptrs = [None if j == i else p for j in range(5)]
        refused(gemm, INVALID, *ptrs, 8, 16, 128, 0, None, 0, None)
    refused(gemm, INVALID, p, p, p, p, p, -1, 16, 128, 0, None, 0, None)
    refused(gemm, UNSUPPORTED, p, p, p, p, p, 8, 16, 192, 0, None, 0, None)
    for flag in (F.X_PACKED, F.Y_PACKED):
        refused(gemm, UNSUPPORTED, p, p, p, p, p, 8, 64, 128, flag, None, 0, None)
    need = L.ffmi_linear_w4a8_workspace_bytes(8, 16, 4096, 0)
    refused(gemm, INVALID, p, p, p, p, p, 8, 16, 4096, 0, p, need - 4, None)
    refused(gemm, INVALID, p, p, p, p, p, 8, 16, 4096, 0, None, need, None)


def test_model_flags_w4_a8_rules_before_the_device():
    L = F.lib()
    c = F.LlamaConfig.from_dict(dict(num_layers=1, vocab_size=1000, num_heads=8, hidden=512,
                                     intermediate=1024))
    m = ctypes.c_void_p()

    def opts(tp_size=1, full_precision=0):
        return F.ModelOpts(F.MODEL_INC, 0, tp_size, None, 2, 16, 64, 0, 1, 0, None, 0, full_precision)

    both = F.MODEL_W4 | F.MODEL_A8
    for o, flags in ((opts(full_precision=1), both), (opts(tp_size=2), both),
                     (opts(), both | F.MODEL_LORA)):
        st = L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(o), flags, ctypes.byref(m))
        assert st == UNSUPPORTED and "w4" in L.ffmi_last_error().decode()
    cfg = dict(num_layers=1, vocab_size=100, num_heads=2, hidden=128, intermediate=256)
    with pytest.raises(ValueError, match="activation_dtype"):
        fa.Model(cfg, "inc", activation_dtype="fp8")
