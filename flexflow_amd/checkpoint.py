"""Checkpoints in the reference's on-disk format.

The reference serves LLaMA from a folder of raw tensors, one file per HF
parameter, written by FlexFlowLLAMA.convert_hf_model
(python/flexflow/serve/models/llama.py:274-285: the HF name without "model.",
numpy ``tofile`` of the tensor, plus ``lm_head.weight``) and read by
FileDataLoader (src/runtime/file_loader.cc:217-361, 363-389).  The model
config comes from the HF ``config.json`` (inference/models/llama.h:30-79).
``Model(..., weights_folder=...)`` loads such a folder in the C++ runtime.
"""
import json
import os
from typing import Mapping, Union

import numpy as np


def convert_hf_weight_name(name: str) -> str:
    """llama.py:274-275."""
    return name.replace("model.", "")


def convert_hf_model(model_or_state_dict, dst_folder: str, dtype=np.float16) -> list:
    """Write every parameter as one raw file (llama.py:277-285).

    Accepts an HF ``LlamaForCausalLM`` (anything with ``named_parameters``
    and an ``lm_head``) or a mapping name -> array.  ``dtype`` is the file
    element type (fp16 as the reference's half-precision serving uses, or
    fp32; the loader takes either).  Returns the written file names."""
    os.makedirs(dst_folder, exist_ok=True)
    if hasattr(model_or_state_dict, "named_parameters"):
        items = [(n, p.detach().cpu().float().numpy())
                 for n, p in model_or_state_dict.named_parameters()]
        lm = getattr(model_or_state_dict, "lm_head", None)
        if lm is not None:
            items.append(("lm_head.weight", lm.weight.detach().cpu().float().numpy()))
    else:
        items = [(n, np.asarray(v)) for n, v in model_or_state_dict.items()]
    written = []
    for name, arr in dict(items).items():  # (lm_head may appear twice)
        fname = convert_hf_weight_name(name)
        np.ascontiguousarray(arr, dtype=dtype).tofile(os.path.join(dst_folder, fname))
        written.append(fname)
    return written


def llama_config_from_hf(src: Union[str, Mapping]) -> dict:
    """LLAMAConfig (llama.h:30-79) from an HF config.json path, a folder
    holding one, or an already-parsed dict."""
    if isinstance(src, str):
        path = os.path.join(src, "config.json") if os.path.isdir(src) else src
        with open(path) as f:
            src = json.load(f)
    c = dict(src)
    heads = int(c["num_attention_heads"])
    # newer HF configs keep theta and the scaling under "rope_parameters"
    rp = c.get("rope_parameters") if isinstance(c.get("rope_parameters"), Mapping) else {}
    theta = c.get("rope_theta", rp.get("rope_theta", 10000.0))
    cfg = dict(num_layers=int(c["num_hidden_layers"]), vocab_size=int(c["vocab_size"]),
               num_heads=heads, num_kv_heads=int(c.get("num_key_value_heads") or heads),
               hidden=int(c["hidden_size"]), intermediate=int(c["intermediate_size"]),
               rms_eps=float(c["rms_norm_eps"]), rope_theta=float(theta))
    # llama3 RoPE scaling: the reference reads it under "scaling_factor",
    # HF configs under "rope_scaling" or "rope_parameters"
    sc = c.get("scaling_factor") or c.get("rope_scaling") or rp
    kind = sc.get("rope_type", sc.get("type")) if isinstance(sc, Mapping) else None
    if kind not in (None, "default", "llama3"):
        # the reference applies only plain and llama3 RoPE (inc_multihead_self_attention.cu:
        # 703-722); loading another scaling (linear, dynamic, yarn, ...) unscaled would
        # decode wrongly without any error
        raise ValueError(f"unsupported rope scaling type {kind!r} (supported: default, llama3)")
    if kind == "llama3":
        cfg.update(rope_llama3=1, rope_factor=float(sc["factor"]),
                   rope_low_freq_factor=float(sc["low_freq_factor"]),
                   rope_high_freq_factor=float(sc["high_freq_factor"]),
                   rope_original_max_pos=int(sc["original_max_position_embeddings"]))
    return cfg


_PEFT_PREFIX = "base_model.model.model."
# the served target modules and the block each lives in
_PEFT_SERVED = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn",
                "o_proj": "self_attn", "down_proj": "mlp"}


def convert_peft_adapter(state_dict: Mapping, adapter_config: Mapping, dst_folder: str,
                         dtype=np.float16):
    """Write an HF PEFT LoRA adapter in the reference's per-tensor format and
    return ``(rank, alpha)``.

    ``state_dict`` maps the PEFT keys
    ``base_model.model.model.layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight``
    and ``...layers.{i}.mlp.down_proj.lora_{A,B}.weight`` (an adapter name
    between ``lora_A`` and ``weight``, as in ``lora_A.default.weight``, is
    dropped) to arrays or tensors; ``adapter_config`` is the parsed
    ``adapter_config.json`` (``r``, ``lora_alpha``, ``target_modules``).  The
    files are named as the reference's loader reads them
    (``layers.{i}.self_attn.q_proj.lora_A.weight``, ``layers.{i}.mlp.down_proj.
    lora_A.weight``, peft_weight_allocator.cc:171-240), raw ``tofile`` of the
    HF row-major tensor, and the config is copied next to them as
    ``adapter_config.json`` (``Model.load_lora(folder)`` takes the target
    modules, rank and alpha from it).  Served: any non-empty subset of
    ``q_proj, k_proj, v_proj, o_proj, down_proj``.  ``ValueError``: another
    target module (``gate_proj``, ``up_proj``, ...) or none, a target whose
    tensors are missing or incomplete, a tensor of a module that is not a
    target, ``rank_pattern`` / ``alpha_pattern`` (one rank and one alpha per
    adapter).  Needs no ``peft`` package."""
    targets = adapter_config.get("target_modules") or []
    if isinstance(targets, str):
        targets = [targets]
    targets = [t.split(".")[-1] for t in targets]
    bad = sorted(t for t in targets if t not in _PEFT_SERVED)
    if bad or not targets:
        raise ValueError("convert_peft_adapter: adapters on q_proj, k_proj, v_proj, o_proj and "
                         f"down_proj are served, got {targets}")
    if adapter_config.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"convert_peft_adapter: peft_type {adapter_config.get('peft_type')}")
    if adapter_config.get("rank_pattern") or adapter_config.get("alpha_pattern"):
        raise ValueError("convert_peft_adapter: rank_pattern / alpha_pattern are not served")
    rank, alpha = int(adapter_config["r"]), float(adapter_config["lora_alpha"])
    tensors = {}
    for key, val in state_dict.items():
        if ".lora_" not in key:
            continue
        name = key[len(_PEFT_PREFIX):] if key.startswith(_PEFT_PREFIX) else key
        parts = name.split(".")
        # layers.{i}.{self_attn,mlp}.{module}.lora_A[.adapter].weight
        if (len(parts) not in (6, 7) or parts[0] != "layers" or parts[3] not in targets
                or _PEFT_SERVED[parts[3]] != parts[2]
                or parts[4] not in ("lora_A", "lora_B") or parts[-1] != "weight"):
            raise ValueError(f"convert_peft_adapter: cannot serve adapter tensor {key}")
        arr = val.detach().cpu().float().numpy() if hasattr(val, "detach") else np.asarray(val)
        want = 0 if parts[4] == "lora_A" else 1
        if arr.ndim != 2 or arr.shape[want] != rank:
            raise ValueError(f"convert_peft_adapter: {key} has shape {arr.shape}, rank {rank}")
        tensors[".".join(parts[:5] + ["weight"])] = arr
    layers = {n.split(".")[1] for n in tensors}
    missing = [f"layers.{i}.{_PEFT_SERVED[t]}.{t}.lora_{ab}.weight"
               for t in sorted(set(targets)) for i in sorted(layers) for ab in "AB"
               if f"layers.{i}.{_PEFT_SERVED[t]}.{t}.lora_{ab}.weight" not in tensors]
    if not tensors or missing:
        raise ValueError(f"convert_peft_adapter: lora_A / lora_B missing: {missing[:4]}")
    os.makedirs(dst_folder, exist_ok=True)
    for name, arr in tensors.items():
        np.ascontiguousarray(arr, dtype=dtype).tofile(os.path.join(dst_folder, name))
    with open(os.path.join(dst_folder, "adapter_config.json"), "w") as f:
        json.dump(dict(adapter_config), f)
    return rank, alpha
