"""Train-step engine of the Qwen3Moe model (``--backbone Qwen3Moe`` of the MB decoder harness).

ref:SeqRec/models/generative/Qwen3Moe/model.py is Qwen3Multi without the behaviour-level cross attention: per decoder layer
  x = x + dropout(o_proj(attn(q/k-norm + RoPE of q|k|v(input_layernorm(x)))))          causal + key-padding mask, GQA
  x = x + dropout(mlp(post_attention_layernorm(x), position index, behaviour index))   position-routed experts
with the router of Qwen3Multi minus the action indices (router.py), the same FFN switches (``mlp_type``,
``sparse_layers_decoder``, ``Moe_behavior_only``, injection layers) and the temperature loss (plus ``router_aux_loss_coef``
times an aux loss of 0).  The layers are exactly Qwen3Multi's layers without a cross block, so the forward and backward
are ``Engine``'s (self attention, fused shipped FFN or ``_ffn_fwd_plain`` / ``_ffn_bwd_plain``, head, update, accumulation
window, data parallelism).  What this engine changes:
  - the parameter layout: the FFN norm is ``post_attention_layernorm`` (Qwen3Multi: ``post_cross_attention_layernorm``);
  - the router: ``gamer_moe_router_prep`` builds the expert and behaviour indices, the causal + key-padding mask and, for a
    generation's prompt pass, the per-row RoPE positions in one launch - in every routing mode, including the one without
    behaviour tokens (task ``mb``: behaviour index 0, no injection) and ``Moe_behavior_only`` without a behaviour token
    (every semantic token in expert 1);
  - training sequences need not be a whole number of items (the router covers ``n_positions * num_positions + 1`` tokens).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .config import Qwen3MoeConfig
from .engine import Engine, ParamLayout


class Qwen3MoeLayout(ParamLayout):
    """``ParamLayout`` under Qwen3Moe's names: no cross attention, the FFN norm is ``post_attention_layernorm``."""

    FFN_NORM = "post_attention_layernorm.weight"


class Qwen3MoeEngine(Engine):
    """``Engine(cfg, variant="qwen3moe")``; ``dtype`` / ``matmul`` / ``deterministic`` / ``share_buffers_of`` as in ``Engine``."""

    _VARIANTS = ("qwen3moe",)
    _item_aligned = False
    _layout_cls = Qwen3MoeLayout

    def __init__(self, cfg: Qwen3MoeConfig, device="cuda", temperature: float = 1.0, variant: str = "qwen3moe",
                 dtype: str = "f32", matmul: Optional[str] = None, share_buffers_of: Optional["Qwen3MoeEngine"] = None,
                 deterministic: Optional[bool] = None):
        cfg = Qwen3MoeConfig.coerce(cfg)
        super().__init__(cfg, device, temperature, variant, dtype, matmul, share_buffers_of, deterministic)
        # the router's table per position inside an item (router.py:29-54); None = the kernel's own p + 1
        P = int(cfg.num_positions)
        tbl = cfg.position_experts()
        self.position_table = None
        self.moe_table = (None if tbl == list(range(1, P + 1))
                          else torch.tensor(tbl, dtype=torch.int32, device=self.device))

    def max_len(self) -> int:
        """The longest sequence the router's table covers: n_positions * num_positions + 1 (router.py:46-60)."""
        return int(self.cfg.n_positions) * int(self.cfg.num_positions) + 1

    def _route(self, c, actions, act_zero_col, rope_from_mask: bool):
        """gamer_moe_router_prep: expert and behaviour indices, the causal + key-padding mask, and with ``rope_from_mask``
        generate()'s positions ``cumsum(attention_mask) - 1`` (the prompt pass of a generation).  ``actions`` and
        ``act_zero_col`` do not exist in this model and are ignored."""
        cfg, ws = self.cfg, c.ws
        r = ws.router
        pos = None
        if rope_from_mask:
            pos = ws._buf("moe_pos_ids", (c.B, c.S), torch.int32)
            self.next_pos = ws._buf("moe_next_pos", (c.B,), torch.int32)
        if c.S > self.max_len():
            raise ValueError(f"sequence length {c.S} exceeds the router's table, n_positions * num_positions + 1 = "
                             f"{self.max_len()} (router.py:46-60)")
        ops.moe_router_prep(c.ids, c.am, self.lut, self.moe_table, cfg.num_positions, cfg.n_positions,
                            cfg.use_behavior_token, cfg.pad_token_id, cfg.eos_token_id, r, pos_ids=pos,
                            next_pos=self.next_pos if rope_from_mask else None)
        return pos

    def forward(self, input_ids, attention_mask=None, actions=None, labels=None, num_items_in_batch=None,
                train: bool = False, dropout: Optional[bool] = None, kv_sink=None, kv_dest=None, session_ids=None,
                extended_session_ids=None, last_row_logits: bool = False, hidden_sink: Optional[list] = None,
                rope_from_mask: bool = False):
        """``Engine.forward`` of this model; ``actions`` and the session ids are accepted and ignored (the collators emit
        them for every backbone, the reference's forward takes them in ``**kwargs``)."""
        return super().forward(input_ids, attention_mask, None, labels, num_items_in_batch, train=train, dropout=dropout,
                               kv_sink=kv_sink, kv_dest=kv_dest, last_row_logits=last_row_logits, hidden_sink=hidden_sink,
                               rope_from_mask=rope_from_mask)
