"""The one seeded weight recipe of the Qwen3 baseline fixtures (tests/golden/qwen3_*.npz, decode_qwen3_small.npz).

Both the fixture generator (tools/make_golden_qwen3.py, which loads the weights into the reference's
``Qwen3WithTemperature``) and the tests (which load them into ``gamer_amd``'s) build the weights here; the fixtures pin
them with per-tensor fp64 checksums.  HF's initialisation: normal(0, initializer_range) for matrices, ones for the
RMSNorm weights, the padding row of the embedding zero.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import numpy as np
import torch


def _get(cfg, k):
    return cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)


def state_dict_shapes(cfg) -> "OrderedDict[str, tuple]":
    """HF Qwen3ForCausalLM's parameter names and shapes (without the tied ``lm_head.weight``), in module order."""
    H, dh, I = _get(cfg, "hidden_size"), _get(cfg, "head_dim"), _get(cfg, "intermediate_size")
    nq, nkv = _get(cfg, "num_attention_heads"), _get(cfg, "num_key_value_heads")
    out = OrderedDict([("model.embed_tokens.weight", (_get(cfg, "vocab_size"), H))])
    for l in range(_get(cfg, "num_hidden_layers")):
        p = f"model.layers.{l}."
        out.update([(p + "self_attn.q_proj.weight", (nq * dh, H)), (p + "self_attn.k_proj.weight", (nkv * dh, H)),
                    (p + "self_attn.v_proj.weight", (nkv * dh, H)), (p + "self_attn.o_proj.weight", (H, nq * dh)),
                    (p + "self_attn.q_norm.weight", (dh,)), (p + "self_attn.k_norm.weight", (dh,)),
                    (p + "mlp.gate_proj.weight", (I, H)), (p + "mlp.up_proj.weight", (I, H)), (p + "mlp.down_proj.weight", (H, I)),
                    (p + "input_layernorm.weight", (H,)), (p + "post_attention_layernorm.weight", (H,))])
    out["model.norm.weight"] = (H,)
    return out


def init_state_dict(cfg, seed: int, scale: float = 1.0) -> "OrderedDict[str, torch.Tensor]":
    """fp32 CPU tensors; ``scale`` multiplies every matrix (the decode fixture peaks the next-token distributions)."""
    g = torch.Generator().manual_seed(int(seed))
    std = float(_get(cfg, "initializer_range")) if (isinstance(cfg, dict) and "initializer_range" in cfg) or \
        hasattr(cfg, "initializer_range") else 0.02
    sd = OrderedDict()
    for k, shp in state_dict_shapes(cfg).items():
        if len(shp) == 1:
            sd[k] = torch.ones(shp, dtype=torch.float32)
        else:
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float32) * (std * scale)
    sd["model.embed_tokens.weight"][int(_get(cfg, "pad_token_id"))] = 0.0
    return sd


def fp64_checksums(sd):
    """(sorted keys, [n, 2] array of fp64 sum and absolute sum per tensor)."""
    keys = sorted(sd)
    return keys, np.array([[float(sd[k].double().sum()), float(sd[k].double().abs().sum())] for k in keys])
