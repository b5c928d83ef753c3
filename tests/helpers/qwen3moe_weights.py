"""The seeded weight recipe of the Qwen3Moe fixtures (tests/golden/moe_*.npz, decode_moe_small.npz).

Qwen3MoeWithTemperature's parameters are Qwen3Multi's without the cross attention, with the FFN norm named
``post_attention_layernorm`` (ref:SeqRec/models/generative/Qwen3Moe/model.py:39-63).  The fixture generator
(tools/make_golden_qwen3moe.py) checks that the reference model's state dict has exactly these names and shapes; the tests load
the same weights into ``gamer_amd``'s model.  HF's initialisation as in ``ffn_ablation_weights``.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import torch

import ffn_ablation_weights as fw

fp64_checksums = fw.fp64_checksums


def state_dict_shapes(cfg) -> "OrderedDict[str, tuple]":
    """Parameter names and shapes (without the tied ``lm_head.weight``), sorted by name."""
    d = dict(cfg) if isinstance(cfg, dict) else {k: getattr(cfg, k) for k in dir(cfg) if not k.startswith("_")}
    d["cross_attention_decoder"] = []
    out = {k.replace("post_cross_attention_layernorm", "post_attention_layernorm"): v
           for k, v in fw.state_dict_shapes(d).items()}
    return OrderedDict(sorted(out.items()))


def init_state_dict(cfg, seed: int, scale: float = 1.0) -> "OrderedDict[str, torch.Tensor]":
    """fp32 CPU tensors drawn in sorted-name order; ``scale`` multiplies every matrix."""
    g = torch.Generator().manual_seed(int(seed))
    std = float(fw._get(cfg, "initializer_range", 0.02))
    sd = OrderedDict()
    for k, shp in state_dict_shapes(cfg).items():
        if len(shp) == 1:
            sd[k] = torch.ones(shp, dtype=torch.float32)
        else:
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float32) * (std * scale)
    sd["model.embed_tokens.weight"][int(fw._get(cfg, "pad_token_id"))] = 0.0
    return sd
