"""The seeded weight recipe of the Qwen3MoeAction fixtures (tests/golden/moe_action_*.npz, decode_moe_action_small.npz).

Qwen3ActionMoeWithTemperature's parameters are Qwen3Moe's with ``(num_experts - 1) * num_behavior + 1`` experts in a sparse layer
(ref:SeqRec/models/generative/Qwen3MoeAction/FFN.py:21) where Qwen3Moe has ``num_experts``: the recipe is
``qwen3moe_weights``' over a config whose expert count is the FFN's.  The fixture generator (tools/make_golden_moe_action.py)
checks that the reference model's state dict has exactly these names and shapes.  CPU only, no gamer_amd import."""
import ffn_ablation_weights as fw
import qwen3moe_weights as mw

fp64_checksums = mw.fp64_checksums


def num_ffn_experts(cfg) -> int:
    return (int(fw._get(cfg, "num_experts")) - 1) * int(fw._get(cfg, "num_behavior")) + 1


def _ffn_config(cfg) -> dict:
    d = dict(cfg) if isinstance(cfg, dict) else {k: getattr(cfg, k) for k in dir(cfg) if not k.startswith("_")}
    d["num_experts"] = num_ffn_experts(cfg)
    return d


def state_dict_shapes(cfg):
    """Parameter names and shapes (without the tied ``lm_head.weight``), sorted by name."""
    return mw.state_dict_shapes(_ffn_config(cfg))


def init_state_dict(cfg, seed: int, scale: float = 1.0):
    """fp32 CPU tensors drawn in sorted-name order; ``scale`` multiplies every matrix."""
    return mw.init_state_dict(_ffn_config(cfg), seed, scale)
