"""The one seeded weight recipe of the FFN ablation fixtures (tests/golden/ablate_*.npz, decode_ablate_small.npz).

Qwen3Multi with the switches of the reference's config.json that select its FFN: ``mlp_type`` ("Qwen3" = MyQwen3SparseMLP's
SwiGLU experts, "PBATransformer" = T5DenseActDense experts wi / wo), ``sparse_layers_decoder`` (the other layers run one dense
MLP, ``mlp.mlp.*``) and ``Moe_behavior_only`` (num_experts = 2).  Both the fixture generator (tools/make_golden_ffn_ablation.py,
which loads the weights into the reference's model and checks that its state dict has exactly these names and shapes) and the
tests (which load them into ``gamer_amd``'s) build the weights here; the fixtures pin them with per-tensor fp64 checksums.
HF's initialisation: normal(0, initializer_range) for matrices, ones for the RMSNorm weights, the padding row of the embedding
zero; tensors drawn in sorted-name order.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import numpy as np
import torch


def _get(cfg, k, default=None):
    if isinstance(cfg, dict):
        return cfg.get(k, default)
    return getattr(cfg, k, default)


def state_dict_shapes(cfg) -> "OrderedDict[str, tuple]":
    """Qwen3MultiWithTemperature's parameter names and shapes (without the tied ``lm_head.weight``), sorted by name."""
    H, dh, I = _get(cfg, "hidden_size"), _get(cfg, "head_dim"), _get(cfg, "intermediate_size")
    nq, nkv, L = _get(cfg, "num_attention_heads"), _get(cfg, "num_key_value_heads"), _get(cfg, "num_hidden_layers")
    Eb, NB1, E = _get(cfg, "behavior_embedding_dim"), _get(cfg, "num_behavior") + 1, _get(cfg, "num_experts")
    gated = _get(cfg, "mlp_type", "PBATransformer") == "Qwen3"
    out = {"model.embed_tokens.weight": (_get(cfg, "vocab_size"), H), "model.norm.weight": (H,)}
    for l in range(L):
        p = f"model.layers.{l}."
        cross = l in _get(cfg, "cross_attention_decoder")
        inject = l in _get(cfg, "behavior_injection_decoder")
        for a in (["self_attn", "cross_attn"] if cross else ["self_attn"]):
            ap = p + a + "."
            out.update({ap + "q_proj.weight": (nq * dh, H), ap + "k_proj.weight": (nkv * dh, H),
                        ap + "v_proj.weight": (nkv * dh, H), ap + "o_proj.weight": (H, nq * dh),
                        ap + "q_norm.weight": (dh,), ap + "k_norm.weight": (dh,)})
            if a == "cross_attn":
                out.update({ap + "gating.weight": (H, H), ap + "q_behavior_embedding.weight": (NB1, nq * Eb),
                            ap + "k_behavior_embedding.weight": (NB1, nkv * Eb),
                            ap + "v_behavior_embedding.weight": (NB1, nkv * Eb)})
        din = H + (Eb if inject else 0)
        mlps = [f"{p}mlp.experts.expert_{e}." for e in range(E)] if l in _get(cfg, "sparse_layers_decoder") else [f"{p}mlp.mlp."]
        for m in mlps:
            if gated:
                out.update({m + "gate_proj.weight": (I, din), m + "up_proj.weight": (I, din), m + "down_proj.weight": (H, I)})
            else:
                out.update({m + "wi.weight": (I, din), m + "wo.weight": (H, I)})
        if inject:
            out[p + "mlp.behavior_embedding.weight"] = (NB1, Eb)
        out[p + "input_layernorm.weight"] = (H,)
        if cross:
            out[p + "post_self_attention_layernorm.weight"] = (H,)
        out[p + "post_cross_attention_layernorm.weight"] = (H,)
    return OrderedDict(sorted(out.items()))


def init_state_dict(cfg, seed: int, scale: float = 1.0) -> "OrderedDict[str, torch.Tensor]":
    """fp32 CPU tensors; ``scale`` multiplies every matrix (the decode fixture peaks the next-token distributions)."""
    g = torch.Generator().manual_seed(int(seed))
    std = float(_get(cfg, "initializer_range", 0.02))
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
