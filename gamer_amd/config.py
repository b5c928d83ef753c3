"""Configuration object with the reference's config.json schema.

Mirrors what ``Qwen3MoeConfig.from_pretrained(config_dir)`` + the run-time mutation in
ref:SeqRec/tasks/train_SMB_decoder.py:321-360 give the model: the same keys
(ref:config/s2s-models/Qwen3Multi/config.json), attribute access, ``in`` tests and
``save_pretrained`` / ``from_pretrained`` round trips, without needing ``transformers``.
"""
from __future__ import annotations

import copy
import json
import os
from typing import Any, Dict

_DEFAULTS: Dict[str, Any] = {
    # ref:config/s2s-models/Qwen3Multi/config.json
    "architectures": ["Qwen3ForCausalLM"],
    "mlp_type": "Qwen3",
    "Moe_behavior_only": False,
    "moe_intermediate_size": 256,
    "behavior_injection": True,
    "behavior_embedding_dim": 64,
    "sparse_layers_decoder": [0, 1, 2, 3, 4, 5, 6, 7],
    "behavior_injection_decoder": [0, 1, 2, 3],
    "cross_attention_decoder": [4, 5, 6, 7],
    "dropout_rate": 0.2,
    "attention_bias": False,
    "attention_dropout": 0.2,
    "bos_token_id": 4,
    "pad_token_id": 4,
    "eos_token_id": 8,
    "head_dim": 64,
    "hidden_act": "silu",
    "hidden_size": 256,
    "initializer_range": 0.02,
    "intermediate_size": 512,
    "max_position_embeddings": 40960,
    "max_window_layers": 8,
    "model_type": "qwen3",
    "num_attention_heads": 6,
    "num_hidden_layers": 8,
    "num_key_value_heads": 3,
    "rms_norm_eps": 1e-6,
    "rope_scaling": None,
    "rope_theta": 1000000,
    "sliding_window": None,
    "tie_word_embeddings": True,
    "torch_dtype": "float32",
    "use_cache": True,
    "use_sliding_window": False,
    "vocab_size": 14,
    # run-time fields (train_SMB_decoder.py:335-360)
    "num_behavior": 0,
    "behavior_maps": {},
    "use_behavior_token": True,
    "num_positions": 5,
    "num_experts": 6,
    "n_positions": 101,
    "use_user_token": False,
    "model_max_length": 1024,
}


MLP_TYPES = ("Qwen3", "PBATransformer")


def expected_num_experts(config) -> int:
    """num_experts as train_SMB_decoder.py:344-351 sets it at run time: 2 under Moe_behavior_only (one expert for the
    behaviour tokens, one for pad / eos), else num_positions + 1."""
    return 2 if getattr(config, "Moe_behavior_only", False) else int(config.num_positions) + 1


def apply_runtime_fields(config, num_behavior: int, behavior_maps: dict, num_positions: int = 5,
                         n_positions: int = 101, model_max_length: int = 1024):
    """The run-time mutation of a config read from config.json (train_SMB_decoder.py:321-360): the dataset's behaviours,
    a behaviour token per item, no user token, and the expert count of the routing mode (``expected_num_experts``).
    Works on this class and on any attribute bag (a transformers config); returns ``config``."""
    config.num_behavior = int(num_behavior)
    config.behavior_maps = {str(k): int(v) for k, v in behavior_maps.items()}
    config.use_behavior_token = True
    config.use_user_token = False
    config.num_positions = int(num_positions)
    config.n_positions = int(n_positions)
    config.model_max_length = int(model_max_length)
    config.num_experts = expected_num_experts(config)
    return config


class Qwen3MultiConfig:
    """Plain attribute bag with dict semantics (``'num_positions' in config`` works as in HF)."""

    def __init__(self, **kwargs):
        d = copy.deepcopy(_DEFAULTS)
        d.update(kwargs)
        # transformers 5.x stores rope_theta inside `rope_parameters` (config.json written by its save_pretrained)
        rp = kwargs.get("rope_parameters")
        if "rope_theta" not in kwargs and isinstance(rp, dict) and "rope_theta" in rp:
            d["rope_theta"] = rp["rope_theta"]
        if "sparse_layers_decoder" not in kwargs:
            d["sparse_layers_decoder"] = list(range(int(d["num_hidden_layers"])))
        self.__dict__.update(d)

    # --- HF-like surface ---------------------------------------------------------------------
    def __contains__(self, key):
        return key in self.__dict__

    def to_dict(self) -> Dict[str, Any]:
        d = copy.deepcopy(self.__dict__)
        d["behavior_maps"] = {str(k): int(v) for k, v in d.get("behavior_maps", {}).items()}
        return d

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "Qwen3MultiConfig":
        return cls(**d)

    @classmethod
    def coerce(cls, config) -> "Qwen3MultiConfig":
        """Accepts what the reference hands its model (ref:SeqRec/tasks/train_SMB_decoder.py:231, 335-368): a
        ``transformers`` ``Qwen3MoeConfig`` read from config.json and mutated at run time - or an instance of this
        class, or a plain dict.  Every field of the schema is read by ATTRIBUTE (the run-time fields the task sets are
        attributes, not constructor arguments); ``rope_theta`` also from transformers 5.x's ``rope_parameters``."""
        if isinstance(config, cls):
            return config
        if isinstance(config, dict):
            return cls(**config)
        d = {}
        for key in _DEFAULTS:
            if hasattr(config, key):
                d[key] = copy.deepcopy(getattr(config, key))
        if "rope_theta" not in d:
            rp = getattr(config, "rope_parameters", None)
            if isinstance(rp, dict) and "rope_theta" in rp:
                d["rope_theta"] = rp["rope_theta"]
        missing = [k for k in ("num_positions", "model_max_length", "num_behavior", "behavior_maps") if k not in d]
        if missing:
            raise ValueError(f"config object lacks the run-time fields {missing} (train_SMB_decoder.py:335-360 sets them "
                             "before the model is constructed)")
        return cls(**d)

    @classmethod
    def from_pretrained(cls, path: str) -> "Qwen3MultiConfig":
        f = os.path.join(path, "config.json") if os.path.isdir(path) else path
        with open(f) as fh:
            return cls(**json.load(fh))

    def save_pretrained(self, path: str):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as fh:
            json.dump(self.to_dict(), fh, indent=2, sort_keys=True)

    # --- validation of what the HIP kernels are built for --------------------------------------
    def validate(self):
        if self.head_dim != 64:
            raise ValueError("the attention kernels are built for head_dim=64")
        if self.behavior_embedding_dim != self.head_dim:
            raise ValueError("behavior_embedding_dim must equal head_dim (q/k/v bias tables are viewed per head)")
        if self.moe_intermediate_size != self.hidden_size:
            raise ValueError("moe_intermediate_size must equal hidden_size (expert input/output is the hidden state)")
        if self.num_attention_heads // self.num_key_value_heads not in (1, 2) or \
                self.num_attention_heads % self.num_key_value_heads:
            raise ValueError("GQA group (num_attention_heads / num_key_value_heads) must be 1 or 2")
        if self.hidden_size % 4 or self.hidden_size > 1024 or self.intermediate_size % 4:
            raise ValueError("hidden_size must be a multiple of 4 and <= 1024")
        if self.num_behavior + 1 > 8:
            raise ValueError("at most 7 behaviours are supported by the bias-gradient kernels")
        if self.mlp_type not in MLP_TYPES:
            raise ValueError(f"mlp_type must be one of {MLP_TYPES} (MyQwen3SparseMLP / PBATransformerSparseMLP)")
        if self.hidden_act != "silu":
            raise ValueError("only hidden_act='silu' is implemented")
        if any(int(l) not in range(self.num_hidden_layers) for l in self.sparse_layers_decoder):
            raise ValueError("sparse_layers_decoder must be a subset of range(num_hidden_layers)")
        self._check_routing_mode()
        if self.num_experts != expected_num_experts(self):
            raise ValueError("num_experts must be num_positions + 1, or 2 with Moe_behavior_only "
                             "(train_SMB_decoder.py:344-351)")
        if not self.tie_word_embeddings:
            raise ValueError("lm_head is tied to embed_tokens in this model")

    def _check_routing_mode(self):
        """The router modes the model runs (Qwen3Multi: a behaviour token per item, no user token)."""
        if self.use_user_token or not self.use_behavior_token:
            raise ValueError("only the routing modes with a behaviour token and without a user token are implemented "
                             "(use_user_token=False, use_behavior_token=True)")

    # --- the FFN ablation switches (mlp_type, sparse_layers_decoder, Moe_behavior_only) -------------------
    def is_sparse(self, layer: int) -> bool:
        """Whether decoder layer ``layer`` runs position-routed experts (else one dense MLP over every token)."""
        return layer in self.sparse_layers_decoder

    @property
    def gated_mlp(self) -> bool:
        """mlp_type "Qwen3": SwiGLU experts (gate / up / down); "PBATransformer": wo(dropout(silu(wi(x))))."""
        return self.mlp_type == "Qwen3"

    @property
    def shipped_ffn(self) -> bool:
        """The FFN configuration of the shipped config.json: SwiGLU experts in every layer, one expert per position."""
        return (self.gated_mlp and not self.Moe_behavior_only and
                sorted(self.sparse_layers_decoder) == list(range(self.num_hidden_layers)))

    @property
    def num_ffn_experts(self) -> int:
        """Experts of a sparse layer's FFN.  Here the router's count ``num_experts``; Qwen3MoeAction has more."""
        return int(self.num_experts)

    def position_experts(self):
        """Expert index of each position inside an item (router.py:28-54): 1..num_positions, or with
        Moe_behavior_only 1 for the behaviour token and 2 for every semantic token.  Pad and eos go to expert 0.
        With Moe_behavior_only and num_experts = 2 the semantic tokens' index names no expert: the reference's
        MyQwen3SparseMLP / PBATransformerSparseMLP leave their FFN output at zero (only the residual passes)."""
        P = int(self.num_positions)
        if self.Moe_behavior_only:
            return [1] + [2] * (P - 1)
        return list(range(1, P + 1))

    def behavior_lut(self):
        """int32 table token id -> behaviour index (or -1), what the router kernel consumes."""
        import torch
        lut = torch.full((int(self.vocab_size),), -1, dtype=torch.int32)
        for tok, idx in self.behavior_maps.items():
            if 0 <= int(tok) < self.vocab_size:
                lut[int(tok)] = int(idx)
        return lut


def base_model_config(path: str, vocab_size: int, num_behavior: int, behavior_maps: dict, num_positions: int,
                      n_positions: int, pad_token_id: int = None, model_max_length: int = 1024) -> Qwen3MultiConfig:
    """``--base_model DIR`` of train_SMB_decoder.py: DIR/config.json (any of the shipped Qwen3Multi configs, with its FFN
    ablation switches mlp_type / sparse_layers_decoder / Moe_behavior_only as written there), the vocabulary resized to the
    tokenizer's, then the run-time fields of train_SMB_decoder.py:321-360 (``apply_runtime_fields``).  A config.json without
    ``mlp_type`` gets this class's default "Qwen3" - the reference's decoder layer falls back to "PBATransformer" then
    (model.py:166-169)."""
    cfg = Qwen3MultiConfig.from_pretrained(path)
    cfg.vocab_size = int(vocab_size)
    if pad_token_id is not None:
        cfg.pad_token_id = int(pad_token_id)
    return apply_runtime_fields(cfg, num_behavior, behavior_maps, num_positions, n_positions, model_max_length)


def synthetic_config(codebook: int = 256, num_behavior: int = 3, **overrides) -> Qwen3MultiConfig:
    """The shipped architecture with the vocabulary of ``gamer_amd.synthetic``."""
    from . import synthetic
    cfg = Qwen3MultiConfig(
        vocab_size=synthetic.vocab_size(codebook, num_behavior),
        num_behavior=num_behavior,
        behavior_maps={str(k): v for k, v in synthetic.behavior_maps(codebook, num_behavior).items()},
        **overrides,
    )
    return cfg


_QWEN3_DEFAULTS: Dict[str, Any] = {
    # the Qwen3-Light backbone of the SMB decoder harness (--backbone Qwen3): HF Qwen3ForCausalLM, no run-time fields
    "architectures": ["Qwen3ForCausalLM"],
    "attention_bias": False,
    "attention_dropout": 0.1,
    "bos_token_id": 4,
    "pad_token_id": 4,
    "eos_token_id": 8,
    "head_dim": 64,
    "hidden_act": "silu",
    "hidden_size": 256,
    "initializer_range": 0.02,
    "intermediate_size": 512,
    "max_position_embeddings": 40960,
    "max_window_layers": 8,
    "model_type": "qwen3",
    "num_attention_heads": 6,
    "num_hidden_layers": 8,
    "num_key_value_heads": 3,
    "rms_norm_eps": 1e-6,
    "rope_scaling": None,
    "rope_theta": 1000000,
    "sliding_window": None,
    "tie_word_embeddings": True,
    "torch_dtype": "float32",
    "use_cache": True,
    "use_sliding_window": False,
    "vocab_size": 14,
}


class Qwen3Config:
    """Configuration of the plain Qwen3 baseline (train_SMB_decoder.py:317-320 builds ``Qwen3WithTemperature`` from it):
    the keys of HF ``Qwen3Config`` with the Qwen3-Light defaults, and the dict / json surface of ``Qwen3MultiConfig``.
    None of Qwen3Multi's routing, injection or cross-attention fields exist here."""

    def __init__(self, **kwargs):
        d = copy.deepcopy(_QWEN3_DEFAULTS)
        d.update(kwargs)
        rp = kwargs.get("rope_parameters")
        if "rope_theta" not in kwargs and isinstance(rp, dict) and "rope_theta" in rp:
            d["rope_theta"] = rp["rope_theta"]
        self.__dict__.update(d)

    def __contains__(self, key):
        return key in self.__dict__

    def to_dict(self) -> Dict[str, Any]:
        return copy.deepcopy(self.__dict__)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "Qwen3Config":
        return cls(**d)

    @classmethod
    def from_pretrained(cls, path: str) -> "Qwen3Config":
        f = os.path.join(path, "config.json") if os.path.isdir(path) else path
        with open(f) as fh:
            return cls(**json.load(fh))

    def save_pretrained(self, path: str):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as fh:
            json.dump(self.to_dict(), fh, indent=2, sort_keys=True)

    @classmethod
    def coerce(cls, config) -> "Qwen3Config":
        """An instance of this class, a dict, or what the reference hands its model: a transformers ``Qwen3Config`` read
        from config.json (every field of the schema is read by attribute; ``rope_theta`` also from transformers 5.x's
        ``rope_parameters``)."""
        if isinstance(config, cls):
            return config
        if isinstance(config, dict):
            return cls(**config)
        d = {}
        for key in _QWEN3_DEFAULTS:
            if hasattr(config, key):
                d[key] = copy.deepcopy(getattr(config, key))
        if "rope_theta" not in d:
            rp = getattr(config, "rope_parameters", None)
            if isinstance(rp, dict) and "rope_theta" in rp:
                d["rope_theta"] = rp["rope_theta"]
        return cls(**d)

    # the layer sets the shared engine code asks about: no cross attention, no behaviour injection
    cross_attention_decoder: tuple = ()
    behavior_injection_decoder: tuple = ()

    def validate(self):
        if self.head_dim != 64:
            raise ValueError("the attention kernels are built for head_dim=64")
        if self.num_attention_heads // self.num_key_value_heads not in (1, 2) or \
                self.num_attention_heads % self.num_key_value_heads:
            raise ValueError("GQA group (num_attention_heads / num_key_value_heads) must be 1 or 2")
        if self.hidden_size % 4 or self.hidden_size > 1024 or self.intermediate_size % 4:
            raise ValueError("hidden_size must be a multiple of 4 and <= 1024")
        if not self.tie_word_embeddings:
            raise ValueError("lm_head is tied to embed_tokens in this model")
        if self.hidden_act != "silu" or self.attention_bias:
            raise ValueError("only hidden_act='silu' without attention bias is implemented")


class Qwen3SessionConfig(Qwen3Config):
    """Configuration of the Qwen3Session baseline (ref:SeqRec/models/generative/Qwen3Session/model.py: HF
    ``Qwen3ForCausalLM`` with session-wise masks): ``Qwen3Config`` plus the two integer fields its model asserts
    (model.py:16-17) and train_SMB_decoder.py:369-378 sets on the HF config - ``num_positions`` (tokens per item) and
    ``model_max_length`` (the in-item mask covers ``(model_max_length // num_positions) * num_positions`` tokens)."""

    REQUIRED = (("num_positions", "Config must have 'num_positions' attribute for Qwen3SessionModel."),
                ("model_max_length", "Config must have 'model_max_length' attribute for Qwen3SessionModel."))

    def __init__(self, **kwargs):
        for key, msg in self.REQUIRED:
            if not isinstance(kwargs.get(key), int) or isinstance(kwargs.get(key), bool):
                raise ValueError(msg)
        super().__init__(**kwargs)

    @classmethod
    def coerce(cls, config) -> "Qwen3SessionConfig":
        """As ``Qwen3Config.coerce``; an HF config object must carry both run-time fields as attributes."""
        if isinstance(config, cls) or isinstance(config, dict):
            return super().coerce(config)
        base = Qwen3Config.coerce(config).to_dict()
        for key, _ in cls.REQUIRED:
            if hasattr(config, key):
                base[key] = getattr(config, key)
        return cls(**base)

    @property
    def max_item_tokens(self) -> int:
        """Length of the reference's in-item mask: the longest sequence its forward accepts."""
        return (self.model_max_length // self.num_positions) * self.num_positions

    def validate(self):
        super().validate()
        if self.num_positions <= 0:
            raise ValueError("num_positions must be positive")


_QWEN3MOE_DEFAULTS: Dict[str, Any] = {
    # ref:config/s2s-models/Qwen3Moe/config.json: Qwen3Multi's schema without cross attention (no cross_attention_decoder key),
    # residual and attention dropout 0.1, the router's auxiliary-loss coefficient (multiplied by an aux loss of 0)
    "architectures": ["Qwen3MoeForCausalLM"],
    "model_type": "qwen3_moe",
    "router_aux_loss_coef": 0.001,
    "cross_attention_decoder": [],
    "dropout_rate": 0.1,
    "attention_dropout": 0.1,
}


class Qwen3MoeConfig(Qwen3MultiConfig):
    """Configuration of the Qwen3Moe model (ref:SeqRec/models/generative/Qwen3Moe/model.py; train_MB_decoder.py:317-364 builds
    ``Qwen3MoeWithTemperature`` from it): Qwen3Multi's schema and FFN switches, no cross attention, and besides the shipped
    routing mode the one of a dataset without behaviour tokens (task ``mb``): ``use_behavior_token = False``, no behaviours,
    no injection, behaviour index 0 everywhere.  ``mlp_type`` absent from a config.json or an HF config object falls back to
    "PBATransformer", as the reference's decoder layer does (model.py:50-53); keyword construction takes config.json's values."""

    def __init__(self, **kwargs):
        d = copy.deepcopy(_QWEN3MOE_DEFAULTS)
        d.update(kwargs)
        super().__init__(**d)

    @classmethod
    def from_pretrained(cls, path: str) -> "Qwen3MoeConfig":
        f = os.path.join(path, "config.json") if os.path.isdir(path) else path
        with open(f) as fh:
            d = json.load(fh)
        d.setdefault("mlp_type", "PBATransformer")
        return cls(**d)

    @classmethod
    def coerce(cls, config) -> "Qwen3MoeConfig":
        """As ``Qwen3MultiConfig.coerce``; an HF config object without ``mlp_type`` gets "PBATransformer" (model.py:50-53)."""
        if isinstance(config, cls):
            return config
        if isinstance(config, dict):
            return cls(**config)
        d = {key: copy.deepcopy(getattr(config, key)) for key in _DEFAULTS if hasattr(config, key)}
        if "rope_theta" not in d:
            rp = getattr(config, "rope_parameters", None)
            if isinstance(rp, dict) and "rope_theta" in rp:
                d["rope_theta"] = rp["rope_theta"]
        missing = [k for k in ("num_positions", "num_behavior", "behavior_maps", "n_positions") if k not in d]
        if missing:
            raise ValueError(f"config object lacks the run-time fields {missing} (train_MB_decoder.py:319-362 sets them "
                             "before the model is constructed)")
        d["router_aux_loss_coef"] = getattr(config, "router_aux_loss_coef", _QWEN3MOE_DEFAULTS["router_aux_loss_coef"])
        d["cross_attention_decoder"] = list(getattr(config, "cross_attention_decoder", []) or [])
        if not hasattr(config, "mlp_type"):
            d["mlp_type"] = "PBATransformer"
        return cls(**d)

    def expected_num_experts(self) -> int:
        """train_MB_decoder.py:354-361: num_positions + 1, or 2 under Moe_behavior_only."""
        return 2 if self.Moe_behavior_only else int(self.num_positions) + 1

    def validate(self):
        if self.cross_attention_decoder:
            raise ValueError("Qwen3Moe has no cross attention (cross_attention_decoder must be empty)")
        if not self.use_behavior_token:
            # task "mb" (train_MB_decoder.py:343-350): no behaviour tokens, no behaviours, no injection
            if self.num_behavior or self.behavior_maps:
                raise ValueError("use_behavior_token=False: num_behavior must be 0 and behavior_maps empty "
                                 "(train_MB_decoder.py:343-344)")
            if self.behavior_injection_decoder:
                raise ValueError("use_behavior_token=False: behavior_injection_decoder must be empty "
                                 "(train_MB_decoder.py:346-350)")
        super().validate()
        if int(self.n_positions) < 1:
            raise ValueError("n_positions (the router's item count, max_his_len + 1) must be positive")

    def _check_routing_mode(self):
        """Qwen3Moe's router also runs without behaviour tokens (task "mb", checked in ``validate``); no user token."""
        if self.use_user_token:
            raise ValueError("the routing modes with a user token are not implemented (use_user_token=False)")

    def position_experts(self):
        """Expert index of each position inside an item (router.py:29-54): 1..num_positions; Moe_behavior_only: [1, 2, .., 2]
        with a behaviour token, [1, .., 1] without one (no +1 there)."""
        P = int(self.num_positions)
        if self.Moe_behavior_only and not self.use_behavior_token:
            return [1] * P
        return super().position_experts()


def apply_mb_runtime_fields(config, num_behavior: int, behavior_maps: dict, use_behavior_token: bool, num_positions: int,
                            max_his_len: int = 20):
    """The run-time mutation train_MB_decoder.py:319-362 applies to a Qwen3Moe config read from config.json: the dataset's
    behaviours (none without behaviour tokens, and then no injection), the item's token count, the expert count of the
    routing mode, ``n_positions = max_his_len + 1`` and no user token.  Returns ``config``."""
    config.use_behavior_token = bool(use_behavior_token)
    if config.use_behavior_token:
        config.num_behavior = int(num_behavior)
        config.behavior_maps = {str(k): int(v) for k, v in behavior_maps.items()}
    else:
        config.num_behavior = 0
        config.behavior_maps = {}
        config.behavior_injection = False
        config.behavior_injection_decoder = []
    config.num_positions = int(num_positions)
    config.num_experts = 2 if config.Moe_behavior_only else config.num_positions + 1
    config.n_positions = int(max_his_len) + 1
    config.use_user_token = False
    return config


def base_model_config_moe(path: str, vocab_size: int, num_behavior: int, behavior_maps: dict, use_behavior_token: bool,
                          num_positions: int, max_his_len: int = 20, pad_token_id: int = None) -> Qwen3MoeConfig:
    """``--base_model DIR`` of train_MB_decoder.py for ``--backbone Qwen3Moe``: DIR/config.json (mlp_type absent -> the
    reference's "PBATransformer"), the vocabulary resized to the tokenizer's, then ``apply_mb_runtime_fields``."""
    cfg = Qwen3MoeConfig.from_pretrained(path)
    cfg.vocab_size = int(vocab_size)
    if pad_token_id is not None:
        cfg.pad_token_id = int(pad_token_id)
    return apply_mb_runtime_fields(cfg, num_behavior, behavior_maps, use_behavior_token, num_positions, max_his_len)


class Qwen3SessionMoeConfig(Qwen3MoeConfig):
    """Configuration of the Qwen3SessionMoe model (ref:SeqRec/models/generative/Qwen3SessionMoe/model.py: Qwen3Moe's layers
    and router under Qwen3Session's session-wise self mask): ``Qwen3MoeConfig`` plus the two integer fields its model asserts
    (model.py:404-405) - ``num_positions`` (tokens per item) and ``model_max_length`` (the in-item mask covers
    ``(model_max_length // num_positions) * num_positions`` tokens).  The reference constructs this class in no task; the
    harness sets the run-time fields of the Qwen3SessionMulti branch (train_SMB_decoder.py:321-367)."""

    REQUIRED = Qwen3SessionConfig.REQUIRED

    def __init__(self, **kwargs):
        for key, msg in self.REQUIRED:
            if not isinstance(kwargs.get(key), int) or isinstance(kwargs.get(key), bool):
                raise ValueError(msg)
        super().__init__(**kwargs)

    @classmethod
    def coerce(cls, config) -> "Qwen3SessionMoeConfig":
        """As ``Qwen3MoeConfig.coerce``; an HF config object must carry both run-time fields as attributes."""
        if isinstance(config, cls):
            return config
        if isinstance(config, dict):
            return cls(**config)
        for key, msg in cls.REQUIRED:
            if not hasattr(config, key):
                raise ValueError(msg)
        base = Qwen3MoeConfig.coerce(config).to_dict()
        for key, _ in cls.REQUIRED:
            base[key] = getattr(config, key)
        return cls(**base)

    @property
    def max_item_tokens(self) -> int:
        """Length of the reference's in-item mask: the longest sequence its forward accepts."""
        return (self.model_max_length // self.num_positions) * self.num_positions

    def validate(self):
        super().validate()
        if self.num_positions <= 0:
            raise ValueError("num_positions must be positive")


def base_model_config_session_moe(path: str, vocab_size: int, num_behavior: int, behavior_maps: dict, num_positions: int,
                                  n_positions: int, pad_token_id: int = None,
                                  model_max_length: int = 1024) -> Qwen3SessionMoeConfig:
    """``--base_model DIR`` for ``--backbone Qwen3SessionMoe``: DIR/config.json is a Qwen3Moe base config (mlp_type absent ->
    the reference's "PBATransformer"), the vocabulary resized to the tokenizer's, then the run-time fields the reference's
    Qwen3SessionMulti branch sets (train_SMB_decoder.py:321-367, ``apply_runtime_fields``) with ``model_max_length``.  The
    reference has no branch of its own for this backbone."""
    f = os.path.join(path, "config.json") if os.path.isdir(path) else path
    with open(f) as fh:
        d = json.load(fh)
    d.setdefault("mlp_type", "PBATransformer")
    d.update(vocab_size=int(vocab_size), num_positions=int(num_positions), model_max_length=int(model_max_length))
    if pad_token_id is not None:
        d["pad_token_id"] = int(pad_token_id)
    cfg = Qwen3SessionMoeConfig(**d)
    return apply_runtime_fields(cfg, num_behavior, behavior_maps, num_positions, n_positions, model_max_length)


class Qwen3MoeActionConfig(Qwen3MoeConfig):
    """Configuration of the Qwen3MoeAction model (ref:SeqRec/models/generative/Qwen3MoeAction/{model,FFN}.py: Qwen3Moe whose FFN
    expert is chosen by the pair (behaviour of the token's item, position inside the item)).  ``num_experts`` stays the
    router's count (num_positions + 1, or 2 under Moe_behavior_only); a sparse layer has ``num_ffn_experts`` =
    (num_experts - 1) * num_behavior + 1 experts (FFN.py:21).  Only ``mlp_type == "Qwen3"`` can run: with "PBATransformer" -
    the value an absent field falls back to (model.py:49-52) - the reference's decoder layer calls
    ``PBATransformerSparseMLP.forward`` with four arguments and raises TypeError, so construction refuses it.  The reference
    constructs this class in no task; the harness sets Qwen3Moe's run-time fields (``apply_mb_runtime_fields``)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._check_mlp_type()

    def _check_mlp_type(self):
        if self.mlp_type != "Qwen3":
            raise ValueError(f"Qwen3MoeAction runs mlp_type 'Qwen3' only, not {self.mlp_type!r}: the reference's decoder layer "
                             "calls PBATransformerSparseMLP.forward with four arguments (hidden states, position, behaviour "
                             "and action index) and raises TypeError; 'PBATransformer' is also what a config.json without "
                             "mlp_type falls back to (Qwen3MoeAction/model.py:49-52)")

    @classmethod
    def coerce(cls, config) -> "Qwen3MoeActionConfig":
        """As ``Qwen3MoeConfig.coerce`` (an HF config object without ``mlp_type`` is refused, as its "PBATransformer")."""
        if isinstance(config, cls):
            return config
        if isinstance(config, dict):
            return cls(**config)
        return cls(**Qwen3MoeConfig.coerce(config).to_dict())

    @property
    def num_ffn_experts(self) -> int:
        """(num_experts - 1) * num_behavior + 1 (FFN.py:21): expert 0 for pad / eos and tokens without an action, then
        num_experts - 1 position experts per behaviour."""
        return (int(self.num_experts) - 1) * int(self.num_behavior) + 1

    def validate(self):
        self._check_mlp_type()
        if not self.use_behavior_token:
            raise ValueError("Qwen3MoeAction needs behaviour tokens (use_behavior_token=True): without them every action "
                             "index is 0 and the model collapses to one expert")
        super().validate()
        if self.num_ffn_experts > 64:
            raise ValueError(f"num_ffn_experts = (num_experts - 1) * num_behavior + 1 = {self.num_ffn_experts}: the expert "
                             "lists (gamer_expert_lists) hold at most 64 groups")


def base_model_config_moe_action(path: str, vocab_size: int, num_behavior: int, behavior_maps: dict, num_positions: int,
                                 max_his_len: int = 20, pad_token_id: int = None) -> Qwen3MoeActionConfig:
    """``--base_model DIR`` for ``--backbone Qwen3MoeAction``: DIR/config.json (a file without mlp_type is refused, see the
    class), the vocabulary resized to the tokenizer's, then ``apply_mb_runtime_fields`` with behaviour tokens."""
    cfg = Qwen3MoeActionConfig.from_pretrained(path)
    cfg.vocab_size = int(vocab_size)
    if pad_token_id is not None:
        cfg.pad_token_id = int(pad_token_id)
    return apply_mb_runtime_fields(cfg, num_behavior, behavior_maps, True, num_positions, max_his_len)
