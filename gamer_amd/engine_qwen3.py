"""Train-step engine for the plain Qwen3 baseline of the SMB decoder harness (``--backbone Qwen3``).

ref:SeqRec/models/generative/Qwen3/model.py is HF ``Qwen3ForCausalLM`` plus the temperature loss of the Multi
variants (train_SMB_decoder.py:317-320 builds it from the Qwen3-Light config).  Per decoder layer:
  x = x + o_proj(attn(q/k-norm + RoPE of q|k|v(input_layernorm(x))))          causal + key-padding mask, GQA
  x = x + down(silu(gate h) * up h),  h = post_attention_layernorm(x)          one dense SwiGLU over every token
No router, no experts, no behaviour injection, no cross attention, no residual dropout; attention dropout in training
mode only.  The kernels are the Multi engine's (gamer_amd/engine.py): the same fused q|k|v, attention, SwiGLU-epilogue,
residual-epilogue, head / temperature-CE and clip+AdamW launches, the FFN GEMMs in their ungrouped form (all T rows in
token order, no ``row_map``, no group offsets).  The mask comes from ``gamer_causal_prep`` instead of the router; with
``rope_from_mask=True`` (the prompt pass of a generation) the same kernel builds transformers' per-row positions
``cumsum(attention_mask) - 1`` for left-padded prompts on the device.

``Engine(cfg, variant="qwen3_session")`` constructs ``Qwen3SessionEngine``, the Qwen3Session baseline: the same model
with session-wise masks and RoPE positions from ``extended_session_ids``, built by ``gamer_session_prep`` instead of
``gamer_causal_prep``: besides its argument checks, the ``_self_mask`` hook is all it changes of the forward and backward
loops.

``Engine(cfg, variant="qwen3")`` constructs ``Qwen3Engine``.  It brings its parameter layout, masks and per-layer loops with
the dense MLP; the construction, workspace, bf16 shadow, the shared forward / backward blocks and the update, accumulation-
window and data-parallel surface are ``Engine``'s.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch

from . import ops
from .config import Qwen3Config, Qwen3SessionConfig
from .engine import Engine, _check_dtype, _check_split_dtype, _FlatLayout, _matmul_arg


class Qwen3Layout(_FlatLayout):
    """Flat fp32 layout under HF Qwen3's state-dict names (see ``_FlatLayout``); a layer's q/k/v projections are adjacent
    (one [768, 256] operand) and so are its gate and up projections (one [2 I, H] operand: the fused gate|up GEMM)."""

    VERSION = 1

    def __init__(self, cfg: Qwen3Config, version: int = 1):
        H, dh = cfg.hidden_size, cfg.head_dim
        nq, nkv, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size
        self.version = version
        decay, nodecay = [("model.embed_tokens.weight", (cfg.vocab_size, H))], []
        for l in range(cfg.num_hidden_layers):
            lp = f"model.layers.{l}."
            ap = lp + "self_attn."
            decay += [(ap + "q_proj.weight", (nq * dh, H)), (ap + "k_proj.weight", (nkv * dh, H)),
                      (ap + "v_proj.weight", (nkv * dh, H)), (ap + "o_proj.weight", (H, nq * dh)),
                      (lp + "mlp.gate_proj.weight", (I, H)), (lp + "mlp.up_proj.weight", (I, H)),
                      (lp + "mlp.down_proj.weight", (H, I))]
            nodecay += [(ap + "q_norm.weight", (dh,)), (ap + "k_norm.weight", (dh,)),
                        (lp + "input_layernorm.weight", (H,)), (lp + "post_attention_layernorm.weight", (H,))]
        nodecay.append(("model.norm.weight", (H,)))
        super().__init__(decay, nodecay)

    def adopt(self, flat: torch.Tensor, cfg, version) -> torch.Tensor:
        version = 1 if version is None else int(version)
        if version != self.VERSION:
            raise ValueError(f"flat optimizer state was written under Qwen3 parameter layout {version}; this build knows layout 1")
        if flat.numel() != self.numel:
            raise ValueError(f"flat optimizer state has {flat.numel()} elements, this model {self.numel}")
        return flat


class _Qwen3LayerW:
    """Fused weight views of one decoder layer over a flat buffer (parameters, gradients or their bf16 copies)."""

    def __init__(self, cfg, layout: Qwen3Layout, flat: torch.Tensor, l: int):
        H, dh, I = cfg.hidden_size, cfg.head_dim, cfg.intermediate_size
        QKV = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * dh
        v = layout.views(flat)
        lp = f"model.layers.{l}."
        ap = lp + "self_attn."
        self.self_attn = dict(qkv=layout.span(flat, ap + "q_proj.weight", QKV, H), o=v[ap + "o_proj.weight"],
                              qn=v[ap + "q_norm.weight"], kn=v[ap + "k_norm.weight"])
        self.ln1 = v[lp + "input_layernorm.weight"]
        self.ln2 = v[lp + "post_attention_layernorm.weight"]
        self.gu = layout.span(flat, lp + "mlp.gate_proj.weight", 2 * I, H)      # rows [0, I) gate, [I, 2 I) up
        self.down = v[lp + "mlp.down_proj.weight"]


class _Qwen3LayerWT:
    """Transposed bf16 weight views of one layer (dgrad operands of the bf16 step)."""

    def __init__(self, cfg, sh, l: int):
        lp = f"model.layers.{l}."
        self.self_attn = dict(qkv=sh.t(lp + "self_attn.qkv"), o=sh.t(lp + "self_attn.o_proj.weight"))
        self.gu, self.down = sh.t(lp + "mlp.gu"), sh.t(lp + "mlp.down_proj.weight")


class Qwen3Engine(Engine):
    """Flat parameter / gradient / optimizer buffers of the baseline and its forward / backward chains (see the module
    docstring).  ``dtype`` / ``matmul`` / ``deterministic`` / ``share_buffers_of`` as in ``Engine``."""

    _layout_cls = Qwen3Layout
    _layer_cls = _Qwen3LayerW
    _layer_t_cls = _Qwen3LayerWT
    VARIANT = "qwen3"
    _config_cls = Qwen3Config

    def __init__(self, cfg: Qwen3Config, device="cuda", temperature: float = 1.0, variant: Optional[str] = None,
                 dtype: str = "f32", matmul: Optional[str] = None, share_buffers_of: Optional["Qwen3Engine"] = None,
                 deterministic: Optional[bool] = None):
        variant = self.VARIANT if variant is None else variant
        if variant != self.VARIANT:
            raise ValueError(f"{type(self).__name__} is the {self.VARIANT!r} variant, not {variant!r}")
        cfg = self._config_cls.coerce(cfg)
        cfg.validate()
        matmul = _matmul_arg(dtype, matmul)
        _check_dtype(dtype)
        _check_split_dtype(dtype, matmul)
        self._init_core(cfg, device, temperature, variant, dtype, matmul, share_buffers_of, deterministic)

    @staticmethod
    def _bind_masks(ws, B: int, S: int):
        """gamer_causal_prep's outputs: the causal + key-padding mask and the RoPE positions of a generation's prompt."""
        i32 = torch.int32
        ws.mask = dict(kl_self=ws._buf("m_kl_self", (B, S), i32), empty_self=ws._buf("m_empty_self", (B, S), i32),
                       tile_empty_self=ws._buf("m_tile_empty_self", (B, (S + 31) // 32), i32),
                       pos_ids=ws._buf("m_pos_ids", (B, S), i32), next_pos=ws._buf("m_next_pos", (B,), i32))

    # ------------------------------------------------------------------------------------------
    @ops.scoped_f32_matmul(lambda self, *a: self.matmul, lambda self, *a: self._planes())
    @ops.scoped_amax(lambda self, *a: self._amax)
    def forward(self, input_ids, attention_mask=None, actions=None, labels=None, num_items_in_batch=None,
                train: bool = False, dropout: Optional[bool] = None, kv_sink=None, kv_dest=None,
                session_ids=None, extended_session_ids=None, last_row_logits: bool = False,
                hidden_sink: Optional[list] = None, rope_from_mask: bool = False):
        """Returns (loss or None, logits view [B,S,V]) as ``Engine.forward``.  ``actions`` / ``session_ids`` /
        ``extended_session_ids`` are accepted and ignored (the SMB collator emits them for every backbone; the reference's
        forward takes them in ``**kwargs``).  RoPE positions are 0..S-1 (the training and scoring forward), or with
        ``rope_from_mask`` transformers' generate() positions ``cumsum(attention_mask) - 1`` (0 at pads) - the prompt pass
        of a generation.  ``kv_dest`` / ``kv_sink`` / ``last_row_logits`` / ``hidden_sink``: see ``Engine.forward``
        (kinds "self" only)."""
        del actions
        c = self._prologue(input_ids, attention_mask, labels, train, dropout, 0.0, kv_dest, hidden_sink, last_row_logits, 0,
                           eval_only=("last_row_logits / rope_from_mask are evaluation-only options"
                                      if last_row_logits or rope_from_mask else None),
                           f32_only=(f"generation (cached decode) of variant {self.variant!r} is built for dtype='f32' only"
                                     if last_row_logits else None))
        cfg, ws, m = self.cfg, c.ws, c.ws.mask
        B, S, T, H, I, L, eps = c.B, c.S, c.T, c.H, c.I, cfg.num_hidden_layers, c.eps
        span, pos_ids = ws.self_span = self._self_mask(c, rope_from_mask, session_ids, extended_session_ids)
        ops.embedding_fwd(c.ids, self.params["model.embed_tokens.weight"], ws.x[0][0])
        # the q|k|v projection with per-head RMSNorm + RoPE in its epilogue: opt-in in the train step (Engine.__init__), always
        # in a generation's prompt pass when its tiles are whole (it writes q and the rotated keys with the prompt's positions)
        fuse_qkv = (((self.fuse_qkv_bf16 if c.bf16 else self.fuse_qkv) or last_row_logits) and
                    ops.qkv_fused_ok(ws.layers[0]["h1"], T, c.QKV))
        x_last = None
        for l in range(L):
            W, Wm, A, xs = self.W[l], self.Wm[l], ws.layers[l], ws.x[l]
            if hidden_sink is not None:
                hidden_sink.append(xs[0].view(B, S, H).clone())
            # ---- self attention, o_proj with the residual add (no residual dropout in this model) ----
            self._self_attention(c, l, m, span, pos_ids, fuse_qkv, kv_dest, kv_sink)
            # ---- dense SwiGLU MLP ----
            if last_row_logits and l == L - 1:
                # prompt pass of a generation: the last layer's K/V are cached; of its MLP only the last position of every
                # sample is still needed
                f32 = dict(dtype=torch.float32, device=self.device)
                rows = torch.arange(B, device=self.device) * S + (S - 1)
                xl = xs[1].index_select(0, rows).contiguous()
                hin, gu, hm = torch.empty(B, H, **f32), torch.empty(B, 2 * I, **f32), torch.empty(B, I, **f32)
                ops.rmsnorm_fwd(xl, W.ln2, eps, hin)
                ops.linear_fwd(hin, H, W.gu, H, gu, 2 * I, B, 2 * I, H)
                ops.swiglu_fwd_ld(gu, 2 * I, B, I, 0.0, 0, hm)
                x_last = torch.empty(B, H, **f32)
                ops.gemm(hm, I, 1, W.down, I, 1, x_last, H, B, H, I, resid=xl)
                break
            ops.rmsnorm_fwd(xs[1], W.ln2, eps, A["hin"])
            if c.fuse_swiglu_fwd:
                # gate|up AND hm = silu(gate) * up from one call (the SwiGLU forward as the projection's epilogue), all T rows
                ops.gemm(A["hin"], H, 1, Wm.gu, H, 1, A["gu"], 2 * I, T, 2 * I, H, swiglu_fwd=(A["hm"], None, None))
            else:
                ops.linear_fwd(A["hin"], H, Wm.gu, H, A["gu"], 2 * I, T, 2 * I, H)
                ops.swiglu_fwd_ld(A["gu"], 2 * I, T, I, 0.0, 0, A["hm"])
            xnext = ws.x[l + 1][0] if l + 1 < L else ws.x_final
            ops.gemm(A["hm"], I, 1, Wm.down, I, 1, xnext, H, T, H, I, resid=xs[1])
        # ---- final norm, tied head, temperature CE ----
        return self._head(c, x_last, num_items_in_batch, hidden_sink)

    def _self_mask(self, c, rope_from_mask: bool, session_ids, extended_session_ids):
        """Builds the pass's self-attention mask into ``ws.mask`` and returns (per-query key spans, RoPE positions) for the
        forward and the backward: the causal + key-padding mask, no spans, positions 0..S-1 or, with ``rope_from_mask``,
        generate()'s ``cumsum(attention_mask) - 1``.  The session ids are not used here."""
        m = c.ws.mask
        ops.causal_prep(c.am, c.B, c.S, m["kl_self"], m["empty_self"], m["tile_empty_self"],
                        pos_ids=m["pos_ids"] if rope_from_mask else None, next_pos=m["next_pos"])
        return None, (m["pos_ids"] if rope_from_mask else None)

    def check_inputs(self):
        """Host-synchronising validation: labels outside the vocabulary (nn.CrossEntropyLoss raises on them)."""
        n = int(self.ws.bad_label.item())
        if n:
            raise IndexError(f"{n} label(s) outside [0, vocab_size={self.cfg.vocab_size}) that are not -100 "
                             "(nn.CrossEntropyLoss raises 'Target out of bounds' in the reference)")

    # ------------------------------------------------------------------------------------------
    def _backward(self, dloss: float = 1.0, layer_done=None, dloss_dev: Optional[torch.Tensor] = None):
        """See ``Engine._backward``."""
        c = self._backward_head(dloss, dloss_dev, rows=None)
        ws, T, H, I = c.ws, c.T, c.H, c.I
        dgrad, hold = functools.partial(self._dgrad, c), c.hold
        t0 = ws.tmpH[0]
        for l in reversed(range(self.cfg.num_hidden_layers)):
            W, G, A, xs = self.W[l], self.G[l], ws.layers[l], ws.x[l]
            WT = self.WT[l] if c.bf16 else None
            # ---- MLP ----   (t0 = d layer output)
            with hold(t0):
                ops.linear_wgrad(t0, H, A["hm"], I, G.down, I, T, H, I)
                if c.fuse_swiglu_bwd:
                    # the down projection's input gradient with the SwiGLU backward in its epilogue: A["gu"] <- d gate | d up
                    if c.bf16:
                        ops.linear_dgrad_t(t0, H, WT.down, WT.down.shape[1], ws.dhm, I, T, H, I, swiglu_bwd=(A["gu"], 2 * I))
                    else:
                        ops.gemm(t0, H, 1, W.down, 1, I, ws.dhm, I, T, I, H, swiglu_bwd=(A["gu"], 2 * I))
                else:
                    dgrad(t0, H, W.down, WT.down if c.bf16 else None, I, ws.dhm, I, H, I)
            if not c.fuse_swiglu_bwd:
                ops.swiglu_bwd_ld(A["gu"], 2 * I, T, I, ws.dhm, 0.0, 0)
            with hold(A["gu"]):
                ops.linear_wgrad(A["gu"], 2 * I, A["hin"], H, G.gu, H, T, 2 * I, H)
                dgrad(A["gu"], 2 * I, W.gu, WT.gu if c.bf16 else None, H, ws.dhin, H, 2 * I, H)
            # (t0 = dx for the attention block's output: the dropout-mask pass with p = 0)
            self._norm_bwd(c, xs[1], W.ln2, ws.dhin, H, G.ln2, True, branch=(self._seed(l, 1), None))
            self._self_attention_bwd(c, l, ws.mask, *ws.self_span, rows=None)
            if layer_done is not None:
                layer_done(l)
        self._backward_tail(c)


class Qwen3SessionEngine(Qwen3Engine):
    """The Qwen3Session baseline (``--backbone Qwen3Session``; ref:SeqRec/models/generative/Qwen3Session/model.py): HF
    ``Qwen3ForCausalLM`` - the parameters, layers and loops of ``Qwen3Engine`` - with Qwen3SessionMulti's self mask (a token
    sees its own item up to itself and every kept token of a strictly earlier session, model.py:28-80) and RoPE positions
    ``extended_session_ids`` (model.py:293-309).  ``gamer_session_prep`` builds both on the device, without a router, as
    per-query key spans; the attention kernels take them in every form (split3, split6, f32, bf16)."""

    VARIANT = "qwen3_session"
    _config_cls = Qwen3SessionConfig
    key_spans = True

    @staticmethod
    def _bind_masks(ws, B: int, S: int):
        """gamer_session_prep's outputs: key-padding levels, key spans, RoPE positions, empty rows / tiles, violations."""
        i32 = torch.int32
        if "m_violations" not in ws._store:
            ws._store["m_violations"] = torch.zeros(1, dtype=i32, device=ws.device)
        ws.mask = dict(kl_self=ws._buf("m_kl_self", (B, S), i32), empty_self=ws._buf("m_empty_self", (B, S), i32),
                       tile_empty_self=ws._buf("m_tile_empty_self", (B, (S + 31) // 32), i32),
                       span_self=ws._buf("m_span_self", (B, S, 4), i32), pos_ids=ws._buf("m_pos_ids", (B, S), i32),
                       violations=ws._store["m_violations"])

    def forward(self, input_ids, attention_mask=None, actions=None, labels=None, num_items_in_batch=None,
                train: bool = False, dropout: Optional[bool] = None, kv_sink=None, kv_dest=None,
                session_ids=None, extended_session_ids=None, last_row_logits: bool = False,
                hidden_sink: Optional[list] = None):
        """``Qwen3Engine.forward`` with the session-wise mask: ``session_ids`` [B,S] are required (the reference asserts
        the same), ``extended_session_ids`` [B,S] are the RoPE positions (None: 0..S-1).  ``actions`` are ignored."""
        if session_ids is None:
            raise ValueError("Session IDs must be provided to generate session-wise causal mask.")
        S = input_ids.shape[1]
        # the reference's in-item mask has (model_max_length // num_positions) * num_positions rows: a longer sequence
        # fails there; the mask kernel keeps a row's session ids in LDS up to 2048 tokens
        if S > self.cfg.max_item_tokens:
            raise ValueError(f"sequence length {S} exceeds the reference's in-item mask, (model_max_length // "
                             f"num_positions) * num_positions = {self.cfg.max_item_tokens}")
        if S > 2048:
            raise ValueError(f"sequence length {S} > 2048: the session mask kernel (gamer_session_prep) is built for S <= 2048")
        return super().forward(input_ids, attention_mask, labels=labels, num_items_in_batch=num_items_in_batch,
                               train=train, dropout=dropout, kv_sink=kv_sink, kv_dest=kv_dest, session_ids=session_ids,
                               extended_session_ids=extended_session_ids, last_row_logits=last_row_logits,
                               hidden_sink=hidden_sink)

    def _self_mask(self, c, rope_from_mask: bool, session_ids, extended_session_ids):
        """The session-wise mask as key spans and the extended ids as positions (gamer_session_prep, one launch)."""
        m = c.ws.mask
        sid = session_ids.to(self.device, torch.int64).contiguous()
        if tuple(sid.shape) != (c.B, c.S):
            raise ValueError(f"session_ids has shape {tuple(sid.shape)}, input_ids {(c.B, c.S)}")
        ext = None
        if extended_session_ids is not None:
            ext = extended_session_ids.to(self.device, torch.int64).contiguous()
            if tuple(ext.shape) != (c.B, c.S):
                raise ValueError(f"extended_session_ids has shape {tuple(ext.shape)}, input_ids {(c.B, c.S)}")
        m["violations"].zero_()
        ops.session_prep(sid, ext, c.am, self.cfg.num_positions, c.S, m)
        return m["span_self"], m["pos_ids"]

    def check_inputs(self):
        """Labels outside the vocabulary, and rows whose session ids cannot be expressed as key spans (``forward`` has
        already refused sequences longer than the reference's in-item mask or 2048 tokens)."""
        super().check_inputs()
        n = int(self.ws.mask["violations"].item())
        if n:
            raise ValueError(f"{n} row(s) with session ids that decrease along the sequence or RoPE positions "
                             "outside [0, S): the session masks are built as causal key spans "
                             "(gamer_session_prep), which needs the dataset's layout (SMB_dataset.py:194-222)")
