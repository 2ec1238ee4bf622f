"""The MXFP4 weight-only additions to the C ABI (include/ffmi.h): the size
functions against the layout arithmetic and the refusals that need no GPU."""
import ctypes

import pytest

import flexflow_amd.ffmi as F

INVALID, UNSUPPORTED = 1, 5
EPI = {"none": F.EPI_NONE, "silu": F.EPI_SILU_MUL}


@pytest.mark.parametrize("N,K", [(16, 128), (40, 256), (144, 1408), (4096, 4096), (32000, 4096)])
def test_sizes_follow_the_layout(N, K):
    L, tiles = F.lib(), (N + 15) // 16
    assert L.ffmi_linear_w4_packed_bytes(N, K) == tiles * (K // 128) * 1024  # 16 x 128 nibbles
    assert L.ffmi_linear_w4_scale_bytes(N, K) == tiles * (K // 128) * 64     # 16 rows x 4 blocks
    assert L.ffmi_linear_w4_packed_bytes(N, K + 64) == L.ffmi_linear_w4_scale_bytes(N, K + 64) == 0
    # k-slices: until about 256 workgroups of 8 tiles, at most 8, >= 2 quad steps each, none empty
    groups, steps = (tiles + 7) // 8, K // 128
    S = max(1, min(256 // groups, 8, steps // 2))
    S = -(-steps // -(-steps // S))
    for T in (1, 64, 168):  # (a launch covers at most 64 rows; S does not depend on T)
        want = S * min(T, 64) * tiles * 16 * 4 if S > 1 else 0
        assert L.ffmi_linear_w4_workspace_bytes(T, N, K, EPI["none"]) == want
        assert L.ffmi_linear_w4_workspace_bytes(T, N, K, EPI["silu"] | F.W_STREAM) == 0


def test_linear_w4_refusals_name_w4():
    L = F.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # (never dereferenced: every call below is refused first)

    def refused(st, *args):
        assert L.ffmi_linear_w4(*args) == st and "w4" in L.ffmi_last_error().decode()
    for i in range(4):  # X, W4, scales, Y
        ptrs = [None if j == i else p for j in range(4)]
        refused(INVALID, *ptrs, 8, 16, 128, 0, None, 0, None)
    refused(INVALID, p, p, p, p, -1, 16, 128, 0, None, 0, None)
    refused(UNSUPPORTED, p, p, p, p, 8, 16, 192, 0, None, 0, None)
    for flag in (F.X_PACKED, F.Y_PACKED):
        refused(UNSUPPORTED, p, p, p, p, 8, 64, 128, flag, None, 0, None)
    need = L.ffmi_linear_w4_workspace_bytes(8, 16, 4096, 0)
    assert need > 0
    refused(INVALID, p, p, p, p, 8, 16, 4096, 0, p, need - 4, None)
    refused(INVALID, p, p, p, p, 8, 16, 4096, 0, None, need, None)
    for st, args in ((INVALID, (None, 16, 128, p, p, None)), (UNSUPPORTED, (p, 16, 192, p, p, None))):
        assert L.ffmi_linear_w4_quantize_pack(*args) == st and "w4" in L.ffmi_last_error().decode()
    assert L.ffmi_linear_w4_quantize_pack_gate_up(p, None, 16, 128, p, p, None) == INVALID
    assert L.ffmi_debug_linear_w4_unpack(None, p, 16, 128, 0, p, p, None) == INVALID


def test_model_flag_refusals_before_the_device():
    L = F.lib()
    c = F.LlamaConfig.from_dict(dict(num_layers=1, vocab_size=1000, num_heads=8, hidden=512,
                                     intermediate=1024))
    m = ctypes.c_void_p()

    def opts(tp_size=1, full_precision=0):
        return F.ModelOpts(F.MODEL_INC, 0, tp_size, None, 2, 16, 64, 0, 1, 0, None, 0, full_precision)

    def create(o, flags):
        return L.ffmi_model_create_ex(ctypes.byref(c), ctypes.byref(o), flags, ctypes.byref(m))
    assert F.MODEL_W4 == 256
    for unknown in (2, 8, 64, 512):
        assert create(opts(), F.MODEL_W4 | unknown) == INVALID
    for o, flags in ((opts(), F.MODEL_W4 | F.MODEL_W8), (opts(), F.MODEL_W4 | F.MODEL_W8 | F.MODEL_A8),
                     (opts(full_precision=1), F.MODEL_W4), (opts(tp_size=2), F.MODEL_W4),
                     (opts(), F.MODEL_W4 | F.MODEL_LORA)):
        assert create(o, flags) == UNSUPPORTED and "w4" in L.ffmi_last_error().decode()
