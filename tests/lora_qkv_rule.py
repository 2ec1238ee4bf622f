"""The LoRA update of the fused qkv row (include/ffmi.h ffmi_lora_apply_qkv),
in numpy: the rule of tests/lora_rule.py per segment.

y [T][ldy] holds [Q | K | V], the segments widths[0..2] columns wide; each
segment s has its own adapters {id: lora_rule.Adapter} with A [r][in] and B
[widths[s]][r], and a row whose adapter is not in a segment's dict is not
written in that segment's columns.  Under the default replicated load of a
GQA checkpoint the k / v B [num_kv_heads * d][r] of HF PEFT is replicated to
the query heads as the loader replicates the k / v weights: query head h uses
K/V head h // G (replicate_kv).
"""
import numpy as np

import lora_rule as LR


def bounds(widths):
    """[(first column, one past the last)] of the three segments"""
    c = np.concatenate([[0], np.cumsum(widths)])
    return [(int(c[s]), int(c[s + 1])) for s in range(3)]


def apply_qkv(x, y, slots, widths, seg_adapters, order="seq"):
    """(h [3][T][64] fp16, y' fp16): lora_rule.apply_rows on every segment's
    column slice; columns past the last segment are not touched"""
    y = np.asarray(y)
    out = y.copy()
    h = np.zeros((3, y.shape[0], LR.R_MAX), np.float16)
    for s, (c0, c1) in enumerate(bounds(widths)):
        h[s], out[:, c0:c1] = LR.apply_rows(x, np.ascontiguousarray(y[:, c0:c1]), slots,
                                            seg_adapters[s], order)
    return h, out


def replicate_kv(B, num_heads, num_kv_heads, d):
    """B [num_kv_heads * d][r] -> [num_heads * d][r]: query head h takes the
    rows of K/V head h // G"""
    B = np.asarray(B)
    G = num_heads // num_kv_heads
    assert B.shape[0] == num_kv_heads * d and num_heads == G * num_kv_heads
    rows = np.arange(num_heads * d)
    return np.ascontiguousarray(B[(rows // d // G) * d + rows % d])
