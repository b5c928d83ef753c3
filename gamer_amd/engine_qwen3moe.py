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

``Engine(cfg, variant="qwen3_session_moe")`` constructs ``Qwen3SessionMoeEngine``, the Qwen3SessionMoe model
(ref:SeqRec/models/generative/Qwen3SessionMoe/model.py): the same layers, router and loops under Qwen3Session's session-wise
self mask and RoPE positions.  ``gamer_session_moe_prep`` builds the router outputs and the mask in one launch; that launch,
its buffers and the argument checks are all the class adds.

``Engine(cfg, variant="qwen3moe_action")`` constructs ``Qwen3MoeActionEngine``, the Qwen3MoeAction model
(ref:SeqRec/models/generative/Qwen3MoeAction/{model,FFN}.py): Qwen3Moe whose FFN expert is chosen by the pair (behaviour of
the token's item, position inside the item) among ``cfg.num_ffn_experts`` = (num_experts - 1) * num_behavior + 1 experts.
``gamer_moe_action_router_prep`` writes that index where Qwen3Moe's launch writes the position's; the layout, the expert
lists and the grouped GEMMs take their count from ``cfg.num_ffn_experts``, so the class adds only the launch - and the FFN
of rows that sit at one position but in several experts (a generation's last prompt row and decode step).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .config import Qwen3MoeActionConfig, Qwen3MoeConfig, Qwen3SessionMoeConfig
from .engine import Engine, ParamLayout


class Qwen3MoeLayout(ParamLayout):
    """``ParamLayout`` under Qwen3Moe's names: no cross attention, the FFN norm is ``post_attention_layernorm``."""

    FFN_NORM = "post_attention_layernorm.weight"


class Qwen3MoeEngine(Engine):
    """``Engine(cfg, variant="qwen3moe")``; ``dtype`` / ``matmul`` / ``deterministic`` / ``share_buffers_of`` as in ``Engine``."""

    _VARIANTS = ("qwen3moe",)
    _item_aligned = False
    _layout_cls = Qwen3MoeLayout
    _config_cls = Qwen3MoeConfig

    def __init__(self, cfg: Qwen3MoeConfig, device="cuda", temperature: float = 1.0, variant: str = "qwen3moe",
                 dtype: str = "f32", matmul: Optional[str] = None, share_buffers_of: Optional["Qwen3MoeEngine"] = None,
                 deterministic: Optional[bool] = None):
        cfg = self._config_cls.coerce(cfg)
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


class Qwen3SessionMoeEngine(Qwen3MoeEngine):
    """The Qwen3SessionMoe model (``--backbone Qwen3SessionMoe``): Qwen3Moe's parameters, router tables, FFN switches and
    loops with Qwen3Session's self mask (a token sees its own item up to itself and every kept token of a strictly earlier
    session, model.py:402-468) and RoPE positions ``extended_session_ids`` (model.py:680-703).  ``gamer_session_moe_prep``
    writes the router outputs and the mask - as per-query key spans, which the attention kernels take in every form (split3,
    split6, f32, bf16) - in the pass's one prep launch."""

    _VARIANTS = ("qwen3_session_moe",)
    _config_cls = Qwen3SessionMoeConfig
    key_spans = True
    _session_in = None          # (session ids, extended ids) of the forward in progress, on the device: ``_route`` reads them

    @staticmethod
    def _bind_masks(ws, B: int, S: int):
        """The router buffers of ``Engine._bind_masks`` plus the session buffers of ``Qwen3SessionEngine._bind_masks``: key
        spans, RoPE positions and the violation count (key levels and empty rows / tiles are the router's ``*_self``)."""
        Qwen3MoeEngine._bind_masks(ws, B, S)
        i32 = torch.int32
        if "s_violations" not in ws._store:
            ws._store["s_violations"] = torch.zeros(1, dtype=i32, device=ws.device)
        ws.session = dict(span_self=ws._buf("s_span_self", (B, S, 4), i32), span_cross=None,
                          pos_ids=ws._buf("s_pos_ids", (B, S), i32), violations=ws._store["s_violations"])

    def forward(self, input_ids, attention_mask=None, actions=None, labels=None, num_items_in_batch=None,
                train: bool = False, dropout: Optional[bool] = None, kv_sink=None, kv_dest=None, session_ids=None,
                extended_session_ids=None, last_row_logits: bool = False, hidden_sink: Optional[list] = None):
        """``Qwen3MoeEngine.forward`` with the session-wise mask: ``session_ids`` [B,S] are required (the reference asserts
        the same), ``extended_session_ids`` [B,S] are the RoPE positions (None: 0..S-1).  ``actions`` are ignored."""
        if session_ids is None:
            raise ValueError("Session IDs must be provided to generate session-wise causal mask.")
        S = input_ids.shape[1]
        # the reference's in-item mask has (model_max_length // num_positions) * num_positions rows: a longer sequence fails
        # there; the mask kernel keeps a row's session ids in LDS up to 2048 tokens; the router's table ends at max_len()
        if S > self.cfg.max_item_tokens:
            raise ValueError(f"sequence length {S} exceeds the reference's in-item mask, (model_max_length // "
                             f"num_positions) * num_positions = {self.cfg.max_item_tokens}")
        if S > 2048:
            raise ValueError(f"sequence length {S} > 2048: the session mask kernel (gamer_session_moe_prep) is built for "
                             "S <= 2048")
        if S > self.max_len():
            raise ValueError(f"sequence length {S} exceeds the router's table, n_positions * num_positions + 1 = "
                             f"{self.max_len()} (router.py:46-60)")
        # (ops.session_moe_prep checks both shapes against input_ids)
        self._session_in = (session_ids.to(self.device, torch.int64).contiguous(),
                            None if extended_session_ids is None else
                            extended_session_ids.to(self.device, torch.int64).contiguous())
        try:
            return super().forward(input_ids, attention_mask, None, labels, num_items_in_batch, train=train, dropout=dropout,
                                   kv_sink=kv_sink, kv_dest=kv_dest, last_row_logits=last_row_logits, hidden_sink=hidden_sink)
        finally:
            self._session_in = None

    def _route(self, c, actions, act_zero_col, rope_from_mask: bool):
        """gamer_session_moe_prep: the expert and behaviour indices into ``ws.router``, the session mask's key levels and
        empty rows there too, its key spans, positions and violation count into ``ws.session``.  Returns the positions."""
        if rope_from_mask:
            raise ValueError("rope_from_mask is not an option of a session model (its positions are extended_session_ids)")
        cfg, ws = self.cfg, c.ws
        sid, ext = self._session_in
        ws.session["violations"].zero_()
        ops.session_moe_prep(c.ids, c.am, sid, ext, self.lut, self.moe_table, cfg.num_positions, cfg.n_positions,
                             cfg.use_behavior_token, cfg.pad_token_id, cfg.eos_token_id, c.S, {**ws.router, **ws.session})
        return ws.session["pos_ids"]

    def check_inputs(self):
        """``Engine.check_inputs`` (behaviour tokens, labels) and rows whose session ids cannot be expressed as key spans
        (``forward`` has already refused sequences past the in-item mask, 2048 tokens or the router's table)."""
        super().check_inputs()
        n = int(self.ws.session["violations"].item())
        if n:
            raise ValueError(f"{n} row(s) with session ids that decrease along the sequence or RoPE positions "
                             "outside [0, S): the session masks are built as causal key spans "
                             "(gamer_session_moe_prep), which needs the dataset's layout (SMB_dataset.py:194-222)")


class Qwen3MoeActionEngine(Qwen3MoeEngine):
    """The Qwen3MoeAction model (``--backbone Qwen3MoeAction``): Qwen3Moe's layers, mask, positions and loops; the router's
    one launch also writes the action index and routes every token to expert max(0, (num_experts - 1) * (action - 1) +
    position expert) of ``cfg.num_ffn_experts`` (FFN.py:43-44).  With the shipped five positions and four behaviours the 21
    experts times 5 behaviour indices exceed the 64 groups of the (expert, behaviour) inject table, so ``split_inject`` is
    off and the fp32 forms take the concatenated [T, H + Eb] input, as the bf16 form always does."""

    _VARIANTS = ("qwen3moe_action",)
    _config_cls = Qwen3MoeActionConfig

    def _route(self, c, actions, act_zero_col, rope_from_mask: bool):
        """gamer_moe_action_router_prep: ``Qwen3MoeEngine._route`` with the action index and the FFN's expert index.
        ``act_zero_col`` (a generation's re-run): the column whose action stays 0, as in the reference's cache."""
        cfg, ws = self.cfg, c.ws
        pos = None
        if rope_from_mask:
            pos = ws._buf("moe_pos_ids", (c.B, c.S), torch.int32)
            self.next_pos = ws._buf("moe_next_pos", (c.B,), torch.int32)
        if c.S > self.max_len():
            raise ValueError(f"sequence length {c.S} exceeds the router's table, n_positions * num_positions + 1 = "
                             f"{self.max_len()} (router.py:46-60)")
        ops.moe_action_router_prep(c.ids, c.am, self.lut, self.moe_table, cfg.num_positions, cfg.n_positions,
                                   cfg.use_behavior_token, cfg.pad_token_id, cfg.eos_token_id, cfg.num_experts - 1,
                                   cfg.num_ffn_experts, ws.router, pos_ids=pos, next_pos=self.next_pos if rope_from_mask else None,
                                   act_zero_col=act_zero_col)
        return pos

    def forward(self, input_ids, attention_mask=None, actions=None, labels=None, num_items_in_batch=None,
                train: bool = False, dropout: Optional[bool] = None, kv_sink=None, kv_dest=None, session_ids=None,
                extended_session_ids=None, last_row_logits: bool = False, hidden_sink: Optional[list] = None,
                rope_from_mask: bool = False, act_zero_col: Optional[int] = None):
        """``Qwen3MoeEngine.forward``; ``act_zero_col`` (evaluation only) as in ``Engine.forward``."""
        return Engine.forward(self, input_ids, attention_mask, None, labels, num_items_in_batch, train=train, dropout=dropout,
                              act_zero_col=act_zero_col, kv_sink=kv_sink, kv_dest=kv_dest, last_row_logits=last_row_logits,
                              hidden_sink=hidden_sink, rope_from_mask=rope_from_mask)

    def row_lists(self, expert: torch.Tensor) -> tuple:
        """(perm, slot, offsets) of gamer_expert_lists over ``expert`` [B, n] int32 on the device: the FFN index of B * n
        rows, which ``ffn_rows_grouped`` takes."""
        B, n = expert.shape
        E = self.cfg.num_ffn_experts
        i32 = dict(dtype=torch.int32, device=self.device)
        perm, slot = torch.empty(B * n, **i32), torch.empty(B * n, **i32)
        offsets = torch.empty(E + 1, **i32)
        ops.expert_lists(expert.contiguous(), E, perm, slot, offsets, torch.empty((B + 1) * E, **i32))
        return perm, slot, offsets

    def ffn_rows_grouped(self, W, lists: tuple, x, beh, out, bufs: Optional[dict] = None):
        """The FFN of a sparse layer W on rows in several experts (no dropout): out = x + FFN(x), with the rows sorted by
        expert (``lists`` of ``row_lists``) for the grouped GEMMs exactly as in the forward pass - the norm writes sorted rows,
        the down projection's epilogue adds the residual and scatters back.  A row in no group (behaviour-only routing) keeps
        out = x.  ``bufs``: hin / gu / hm buffers at fixed addresses (a decode step); fp32 operands only."""
        cfg = self.cfg
        perm, slot, offsets = lists
        N, H, I, din, nI = x.shape[0], cfg.hidden_size, cfg.intermediate_size, W.din, W.nI
        f32 = dict(dtype=torch.float32, device=self.device)
        hin = (bufs["hin"] if bufs else torch.empty(N, din, **f32)).view(-1)[:N * din].view(N, din)
        gu = bufs["gu"] if bufs else torch.empty(N, nI, **f32)
        hm = bufs["hm"] if bufs else torch.empty(N, I, **f32)
        grp = dict(groups=W.ne, group_offsets=offsets)
        ops.rmsnorm_fwd(x, W.ln3, float(cfg.rms_norm_eps), hin, din, slot)
        if W.inject:
            ops.rowtable_fwd(W.beh, beh, hin, din, H, slot)
        if cfg.Moe_behavior_only:
            gu.zero_()          # (rows in no group are never written by the GEMM)
            out.copy_(x)
        ops.linear_fwd(hin, din, W.gu, din, gu, nI, N, nI, din, strideB=nI * din, **grp)
        ops.swiglu_fwd_ld(gu, nI, N, I, 0.0, 0, hm)
        ops.gemm(hm, I, 1, W.down, I, 1, out, H, N, H, I, strideB=H * I, resid=x, row_map=perm, **grp)

    def _ffn_last_rows(self, W, S: int, rows, x, beh, out, Wm):
        """The last prompt position of every sample in its own row's expert (a prompt of n P + 1 tokens: expert 0, the action
        table's eos slot)."""
        if not W.sparse:
            return super()._ffn_last_rows(W, S, rows, x, beh, out, Wm)
        e = self.ws.router["expert"].view(-1).index_select(0, rows).view(-1, 1)
        self.ffn_rows_grouped(W, self.row_lists(e), x, beh, out)
