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

``Engine(cfg, variant="qwen3")`` constructs this class; it shares the Multi engine's update, accumulation-window and
data-parallel surface (``optimizer_step``, ``train_step``, ``train_window``, ``backward(layer_done=...)``).
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .config import Qwen3Config
from .engine import IGNORE_INDEX, Bf16Shadow, Engine, _Workspace, _round_up


class Qwen3Layout:
    """Flat fp32 layout under HF Qwen3's state-dict names.  Decayed matrices first, RMSNorm weights (no weight decay
    under HF Trainer) last; a layer's q/k/v projections are adjacent (one [768, 256] operand) and so are its gate and
    up projections (one [2 I, H] operand: the fused gate|up GEMM)."""

    VERSION = 1

    def __init__(self, cfg: Qwen3Config, version: int = 1):
        H, dh = cfg.hidden_size, cfg.head_dim
        nq, nkv, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size
        self.version = version
        decay: List[Tuple[str, tuple]] = [("model.embed_tokens.weight", (cfg.vocab_size, H))]
        nodecay: List[Tuple[str, tuple]] = []
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
        self.entries: Dict[str, Tuple[int, tuple]] = {}
        off = 0
        for i, (name, shp) in enumerate(decay + nodecay):
            if i == len(decay):
                self.n_decay = off
            n = math.prod(shp)
            assert n % 4 == 0, f"{name}: size {n} is not a multiple of 4"
            self.entries[name] = (off, shp)
            off += n
        self.numel = off

    def views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {k: flat[o:o + math.prod(s)].view(s) for k, (o, s) in self.entries.items()}

    def adopt(self, flat: torch.Tensor, cfg, version) -> torch.Tensor:
        version = 1 if version is None else int(version)
        if version != self.VERSION:
            raise ValueError(f"flat optimizer state was written under Qwen3 parameter layout {version}; this build knows layout 1")
        if flat.numel() != self.numel:
            raise ValueError(f"flat optimizer state has {flat.numel()} elements, this model {self.numel}")
        return flat

    def span(self, flat: torch.Tensor, first: str, rows: int, cols: int) -> torch.Tensor:
        o = self.entries[first][0]
        return flat[o:o + rows * cols].view(rows, cols)


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


class _Qwen3Shadow(Bf16Shadow):
    """bf16 operand copies (same offsets) and transposed copies of the baseline's matrices (see ``Bf16Shadow``)."""

    def __init__(self, cfg: Qwen3Config, layout: Qwen3Layout, flat_p: torch.Tensor):
        dev = flat_p.device
        H, dh, I = cfg.hidden_size, cfg.head_dim, cfg.intermediate_size
        nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        QKV = (nq + 2 * nkv) * dh
        self.layout, self.flat_p = layout, flat_p
        self.flat16 = torch.zeros(layout.numel, dtype=torch.bfloat16, device=dev)
        self.ldv = _round_up(cfg.vocab_size, 64)
        entries = []
        toff = 0
        self.t_views: Dict[str, Tuple[int, tuple]] = {}

        def add(first: str, rows: int, cols: int, ldt: Optional[int] = None, tkey: Optional[str] = None):
            nonlocal toff
            ldt = ldt or rows
            entries.append((layout.entries[first][0], rows, cols, ldt, toff))
            self.t_views[tkey or first] = (toff, (cols, ldt))
            toff += _round_up(cols * ldt, 8)
        add("model.embed_tokens.weight", cfg.vocab_size, H, ldt=self.ldv)
        for l in range(cfg.num_hidden_layers):
            lp = f"model.layers.{l}."
            add(lp + "self_attn.q_proj.weight", QKV, H, tkey=lp + "self_attn.qkv")
            add(lp + "self_attn.o_proj.weight", H, nq * dh)
            add(lp + "mlp.gate_proj.weight", 2 * I, H, tkey=lp + "mlp.gu")
            add(lp + "mlp.down_proj.weight", H, I)
        self.flatT = torch.zeros(toff, dtype=torch.bfloat16, device=dev)
        tab, tile0 = [], 0
        for src, rows, cols, ldt, dst_t in entries:
            tab += [src, src, dst_t, rows | (cols << 32), ldt | (tile0 << 32)]
            tile0 += ((rows + 31) // 32) * ((cols + 31) // 32)
        self.n_entries, self.n_tiles = len(entries), tile0
        self.table = torch.tensor(tab, dtype=torch.int64, device=dev)
        self.params16 = layout.views(self.flat16)


class _Qwen3LayerWT:
    """Transposed bf16 weight views of one layer (dgrad operands of the bf16 step)."""

    def __init__(self, sh: _Qwen3Shadow, l: int):
        lp = f"model.layers.{l}."
        self.self_attn = dict(qkv=sh.t(lp + "self_attn.qkv"), o=sh.t(lp + "self_attn.o_proj.weight"))
        self.gu = sh.t(lp + "mlp.gu")
        self.down = sh.t(lp + "mlp.down_proj.weight")


class _Qwen3Workspace:
    """Activation / scratch buffers of the baseline's train step (``train=True``) or scoring forward; grow-only storage
    viewed at the batch's shape by ``bind`` (as the Multi engine's ``_Workspace``)."""

    def __init__(self, cfg: Qwen3Config, device, train: bool, act: torch.dtype = torch.float32, spill: bool = True):
        self.cfg, self.device, self.train, self.act, self.spill = cfg, device, train, act, spill
        self._store: Dict[str, torch.Tensor] = {}
        self.B = self.S = self.T = 0
        self.loss_sum = torch.zeros(1, dtype=torch.float32, device=device)
        self.count = torch.zeros(1, dtype=torch.float32, device=device)
        self.bad_label = torch.zeros(1, dtype=torch.int32, device=device)

    _buf = _Workspace._buf
    allocated_bytes = _Workspace.allocated_bytes

    def bind(self, B: int, S: int):
        if (B, S) == (self.B, self.S):
            return self
        cfg, train, act = self.cfg, self.train, self.act
        f32, i32 = torch.float32, torch.int32
        self.B, self.S, self.T = B, S, B * S
        T, H = self.T, cfg.hidden_size
        nq, nkv, dh, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size
        NQ, NKV = nq * dh, nkv * dh
        QKV = NQ + 2 * NKV
        L = cfg.num_hidden_layers
        buf = self._buf
        self.mask = dict(kl_self=buf("m_kl_self", (B, S), i32), empty_self=buf("m_empty_self", (B, S), i32),
                         tile_empty_self=buf("m_tile_empty_self", (B, (S + 31) // 32), i32),
                         pos_ids=buf("m_pos_ids", (B, S), i32), next_pos=buf("m_next_pos", (B,), i32))
        self.ldl = _round_up(cfg.vocab_size, 32 if act == f32 else 64)
        self.logits = buf("logits", (T, self.ldl), act)
        if act != f32:
            self.logits[:, cfg.vocab_size:].zero_()
        self.lse_ce = buf("lse_ce", (T,), f32)
        self.row_loss = buf("row_loss", (T,), f32)
        self.xn = buf("xn", (T, H), act)
        # residual stream snapshots: x[l][0] layer input, [1] after the attention block
        self.x: List[List[torch.Tensor]] = []
        self.layers: List[dict] = []
        for l in range(L):
            tag = f"l{l}_" if train else "l_"          # evaluation keeps one set of buffers and reuses it for every layer
            if train or l == 0:
                self.layers.append(dict(
                    h1=buf(tag + "h1", (T, H), act), qkv=buf(tag + "qkv", (T, QKV), act), q=buf(tag + "q", (T, NQ), act),
                    k=buf(tag + "k", (T, NKV), act), ao=buf(tag + "ao", (T, NQ), act), lse=buf(tag + "lse", (B, nq, S), f32),
                    hin=buf(tag + "hin", (T, H), act), gu=buf(tag + "gu", (T, 2 * I), act), hm=buf(tag + "hm", (T, I), act)))
                self.x.append([buf(tag + "x0", (T, H), f32), buf(tag + "x1", (T, H), f32)])
            else:
                self.layers.append(self.layers[0])
                self.x.append(self.x[0])
        self.x_final = buf("x_final", (T, H), f32) if train else self.x[0][0]
        self.tmpH = [buf(f"tmpH{i}", (T, H), act) for i in range(4)]
        if train:
            self.dx = buf("dx", (T, H), f32)
            self.dhm = buf("dhm", (T, I), act)
            self.dhin = buf("dhin", (T, H), act)
            self.dqkv = buf("dqkv", (T, QKV), act)
            self.dq = buf("dq", (T, NQ), act)
            self.dk = buf("dk", (T, NKV), act)
            self.dao = buf("dao", (T, NQ), act)
            self.delta = buf("delta", (B, nq, S), f32)
            self.norm_partial = buf("norm_partial", (2 * L + 1, 2048, H), f32)
            self.qk_partial = buf("qk_partial", (ops.qknorm_partial_numel(0),), f32)
            self.ds_work = (buf("ds_work", (ops.attn_ds_work_numel(B, S, nq),), f32)
                            if (os.environ.get("GAMER_ATTN_SPILL", "1") != "0" and act == torch.float32 and self.spill)
                            else None)
        return self


class Qwen3Engine(Engine):
    """Flat parameter / gradient / optimizer buffers of the baseline and its forward / backward chains (see the module
    docstring).  ``dtype`` / ``matmul`` / ``deterministic`` / ``share_buffers_of`` as in ``Engine``."""

    def __init__(self, cfg: Qwen3Config, device="cuda", temperature: float = 1.0, variant: str = "qwen3",
                 dtype: str = "f32", matmul: Optional[str] = None, share_buffers_of: Optional["Qwen3Engine"] = None,
                 deterministic: Optional[bool] = None):
        if variant != "qwen3":
            raise ValueError(f"Qwen3Engine is the 'qwen3' variant, not {variant!r}")
        cfg = Qwen3Config.coerce(cfg)
        cfg.validate()
        if matmul is None:
            matmul = "split3" if dtype == "f32" else "f32"
        if matmul not in ops.MATMUL_MODES:
            raise ValueError(f"unknown matmul {matmul!r} ({sorted(ops.MATMUL_MODES)})")
        if dtype not in ("f32", "bf16"):
            raise ValueError(f"unknown dtype {dtype!r} (f32 or bf16; the reference's --fp16 is not built)")
        if dtype != "f32" and matmul != "f32":
            raise ValueError("matmul='split3'/'split6'/'split9' is a form of the fp32 path; dtype='bf16' has its own GEMM")
        if not torch.cuda.is_available():
            raise RuntimeError("gamer_amd.Engine needs a HIP device (there is no CPU fallback)")
        from . import _lib
        _lib.load()
        self.matmul, self.variant, self.dtype = matmul, variant, dtype
        self.deterministic = (os.environ.get("GAMER_DETERMINISTIC", "0") == "1") if deterministic is None else bool(deterministic)
        # the same A/B switches as the Multi engine (Engine.__init__ documents the measurements behind their defaults)
        self.fuse_qkv = False
        self.fuse_qkv_bf16 = os.environ.get("GAMER_FUSE_QKV_BF16", "0") == "1"
        self.split_attention = True
        self.h2_attention = os.environ.get("GAMER_H2_ATTENTION", "1") != "0"
        self.gemm_c_amax = os.environ.get("GAMER_GEMM_CAMAX", "1") != "0"
        self.fuse_swiglu_bwd = os.environ.get("GAMER_FUSE_SWIGLU_BWD", "1") != "0"
        self.ordered_embedding_grad = os.environ.get("GAMER_EMBEDDING_ATOMICS", "0") == "0"
        self.act_dtype = torch.float32 if dtype == "f32" else torch.bfloat16
        self.cfg = cfg
        self.device = torch.device(device)
        self.temperature = float(temperature)
        self.layout = Qwen3Layout(cfg)
        n = self.layout.numel
        if share_buffers_of is not None:
            if share_buffers_of.layout.numel != n or share_buffers_of.device != self.device:
                raise ValueError("share_buffers_of: the other engine has another parameter layout or device")
            self.flat_p, self.flat_g = share_buffers_of.flat_p, share_buffers_of.flat_g
        else:
            self.flat_p = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.flat_g = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.flat_m: Optional[torch.Tensor] = None
        self.flat_v: Optional[torch.Tensor] = None
        self.params = self.layout.views(self.flat_p)
        self.grads = self.layout.views(self.flat_g)
        L = cfg.num_hidden_layers
        self.W = [_Qwen3LayerW(cfg, self.layout, self.flat_p, l) for l in range(L)]
        self.G = [_Qwen3LayerW(cfg, self.layout, self.flat_g, l) for l in range(L)]
        self.shadow: Optional[_Qwen3Shadow] = None
        self.Wm, self.WT = self.W, None
        if dtype == "bf16":
            self.shadow = _Qwen3Shadow(cfg, self.layout, self.flat_p)
            self.Wm = [_Qwen3LayerW(cfg, self.layout, self.shadow.flat16, l) for l in range(L)]
            self.WT = [_Qwen3LayerWT(self.shadow, l) for l in range(L)]
        self.weight_planes: Optional[torch.Tensor] = None
        if dtype == "f32" and matmul != "f32" and os.environ.get("GAMER_SPLIT_PLANES", "0") == "1":
            self.weight_planes = torch.zeros(3, _round_up(n, 4), dtype=torch.bfloat16, device=self.device)
        self._amax = None
        if dtype == "f32" and matmul == "split3":
            self._amax = ops.amax_reuse()
            self._amax.stable_range(self.flat_p.data_ptr(), self.flat_p.numel() * 4)
            if os.environ.get("GAMER_SPLIT3_PLANES", "1") != "0":
                self._amax.planes = torch.zeros(_round_up(n, 4), dtype=torch.float32, device=self.device)
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._ws: Dict[bool, _Qwen3Workspace] = {}
        self.ws: Optional[_Qwen3Workspace] = None
        self.opt_step = 0
        self.dropout_step = 0
        self.base_seed = 0x5EED
        self.sumsq_partial = torch.empty(self.N_SUMSQ_PARTIAL, dtype=torch.float32, device=self.device)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._norm_out_table = None
        self._check_deterministic_embedding()
        self._saved = None

    def workspace(self, B: int, S: int, train: bool) -> _Qwen3Workspace:
        if train not in self._ws:
            # the dS-spill scratch is the fp32-MFMA attention backward's; the split forms recompute instead
            spill = not (self.split_attention and self.matmul != "f32")
            self._ws[train] = _Qwen3Workspace(self.cfg, self.device, train, self.act_dtype, spill=spill)
        return self._ws[train].bind(B, S)

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
        del actions, session_ids, extended_session_ids
        cfg = self.cfg
        B, S = input_ids.shape
        if kv_dest is not None and train:
            raise ValueError("kv_dest is an evaluation-only option (the backward reads the workspace's q|k|v and keys)")
        if (last_row_logits or rope_from_mask) and (train or labels is not None):
            raise ValueError("last_row_logits / rope_from_mask are evaluation-only options")
        if hidden_sink is not None and last_row_logits:
            raise ValueError("hidden_sink needs the full-sequence forward")
        bf16 = self.dtype == "bf16"
        if bf16:
            if last_row_logits:
                raise NotImplementedError("generation (cached decode) is built for dtype='f32' only")
            self.shadow.refresh()
        if self.weight_planes is not None:
            ops.split3_planes(self.flat_p, self.weight_planes)
        T, H = B * S, cfg.hidden_size
        nq, nkv, dh, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size
        NQ, NKV = nq * dh, nkv * dh
        QKV = NQ + 2 * NKV
        L = cfg.num_hidden_layers
        eps = float(cfg.rms_norm_eps)
        use_drop = train if dropout is None else dropout
        p_att = float(cfg.attention_dropout) if use_drop else 0.0
        if use_drop:
            self.dropout_step += 1
        ws = self.workspace(B, S, train)
        self.ws = ws
        if self._amax is not None:
            self._amax.reset()
            if train:
                self._amax.stable(ws.xn, *[A[k] for A in ws.layers for k in ("h1", "ao", "hin", "hm")])
                if self.h2_attention:
                    self._amax.stable(*[A[k] for A in ws.layers for k in ("q", "k")],
                                      *[A["qkv"][:, NQ + NKV:] for A in ws.layers])
        ids = input_ids.to(self.device, torch.int64).contiguous()
        am = attention_mask.to(self.device, torch.int64).contiguous() if attention_mask is not None else None
        lab = labels.to(self.device, torch.int64).contiguous() if labels is not None else None
        if lab is not None:
            ws.bad_label.zero_()
            ops.check_labels(lab, cfg.vocab_size, IGNORE_INDEX, ws.bad_label)
        m = ws.mask
        ops.causal_prep(am, B, S, m["kl_self"], m["empty_self"], m["tile_empty_self"],
                        pos_ids=m["pos_ids"] if rope_from_mask else None, next_pos=m["next_pos"])
        pos_ids = m["pos_ids"] if rope_from_mask else None
        cos, sin = self.rope(S)
        scale = float(dh) ** -0.5
        x = ws.x[0][0]
        ops.embedding_fwd(ids, self.params["model.embed_tokens.weight"], x)
        emb_m = self.shadow.params16["model.embed_tokens.weight"] if bf16 else self.params["model.embed_tokens.weight"]
        # the q|k|v projection with per-head RMSNorm + RoPE in its epilogue: opt-in in the train step (Engine.__init__), always
        # in a generation's prompt pass when its tiles are whole (it writes q and the rotated keys with the prompt's positions)
        fuse_qkv = (((self.fuse_qkv_bf16 if bf16 else self.fuse_qkv) or last_row_logits) and
                    ops.qkv_fused_ok(ws.layers[0]["h1"], T, QKV))
        split_attn = self.split_attention and self.matmul != "f32" and not bf16
        h2_now = split_attn and self.h2_attention and self.matmul == "split3" and p_att < 0.75
        fuse_swiglu_fwd = not bf16 and self.matmul == "split3" and os.environ.get("GAMER_FUSE_SWIGLU_FWD", "1") != "0"
        kl, empty, tile_empty = m["kl_self"], m["empty_self"], m["tile_empty_self"]

        for l in range(L):
            W, Wm, A, xs = self.W[l], self.Wm[l], ws.layers[l], ws.x[l]
            if hidden_sink is not None:
                hidden_sink.append(xs[0].view(B, S, H).clone())
            # ---- self attention ----
            ops.rmsnorm_fwd(xs[0], W.ln1, eps, A["h1"])
            qkv_s, k_s = kv_dest(l, "self") if kv_dest is not None else (A["qkv"], A["k"])
            if fuse_qkv:
                ops.gemm(A["h1"], H, 1, Wm.self_attn["qkv"], H, 1, qkv_s, QKV, T, QKV, H,
                         qknorm=dict(wq=W.self_attn["qn"], wk=W.self_attn["kn"], eps=eps, cos=cos, sin=sin, q_rot=A["q"],
                                     k_rot=k_s, pos_ids=pos_ids, S=S, nq=nq, nkv=nkv))
            else:
                c_amax = (dict(c_amax=(qkv_s[:, NQ + NKV:], NQ + NKV)) if (h2_now and self.gemm_c_amax) else {})
                ops.linear_fwd(A["h1"], H, Wm.self_attn["qkv"], H, qkv_s, QKV, T, QKV, H, **c_amax)
                ops.qknorm_rope_fwd(qkv_s, S, nq, nkv, W.self_attn["qn"], W.self_attn["kn"], eps, cos, sin, A["q"], k_s,
                                    pos_ids=pos_ids)
            v_s = qkv_s[:, NQ + NKV:]
            if kv_sink is not None:
                kv_sink(l, "self", k_s, v_s)
            seed = self._seed(l, 0)
            if split_attn:
                ops.attn_fwd_split(A["q"], NQ, k_s, NKV, v_s, QKV, kl, None, empty, B, S, nq, nkv, scale, p_att, seed,
                                   A["ao"], A["lse"], h2=h2_now)
            elif bf16:
                ops.attn_fwd_bf16(A["q"], NQ, k_s, NKV, v_s, QKV, kl, None, B, S, nq, nkv, scale, p_att, seed, A["ao"], A["lse"])
            else:
                ops.attn_fwd(A["q"], NQ, k_s, NKV, v_s, QKV, kl, None, empty, tile_empty, B, S, nq, nkv, scale, p_att, seed,
                             A["ao"], A["lse"])
            # o_proj with the residual add in the GEMM epilogue (no residual dropout in this model)
            ops.gemm(A["ao"], NQ, 1, Wm.self_attn["o"], NQ, 1, xs[1], H, T, H, NQ, resid=xs[0])
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
            if fuse_swiglu_fwd:
                # gate|up AND hm = silu(gate) * up from one call (the SwiGLU forward as the projection's epilogue), all T rows
                ops.gemm(A["hin"], H, 1, Wm.gu, H, 1, A["gu"], 2 * I, T, 2 * I, H, swiglu_fwd=(A["hm"], None, None))
            else:
                ops.linear_fwd(A["hin"], H, Wm.gu, H, A["gu"], 2 * I, T, 2 * I, H)
                ops.swiglu_fwd_ld(A["gu"], 2 * I, T, I, 0.0, 0, A["hm"])
            xnext = ws.x[l + 1][0] if l + 1 < L else ws.x_final
            ops.gemm(A["hm"], I, 1, Wm.down, I, 1, xnext, H, T, H, I, resid=xs[1])
        # ---- final norm, tied head, temperature CE ----
        V = cfg.vocab_size
        if last_row_logits:
            xn = torch.empty_like(x_last)
            ops.rmsnorm_fwd(x_last, self.params["model.norm.weight"], eps, xn)
            small = torch.empty(B, ws.ldl, dtype=torch.float32, device=self.device)
            ops.linear_fwd(xn, H, self.params["model.embed_tokens.weight"], H, small, ws.ldl, B, V, H)
            self._saved = None
            self.last_logits_buf = small
            return None, small.view(B, 1, ws.ldl)[:, :, :V]
        ops.rmsnorm_fwd(ws.x_final, self.params["model.norm.weight"], eps, ws.xn)
        if hidden_sink is not None:
            hidden_sink.append(ws.xn.view(B, S, H).clone())
        head_alpha = (1.0 / self.temperature) if (lab is not None and ws.logits.dtype == torch.float32) else 1.0
        ops.linear_fwd(ws.xn, H, emb_m, H, ws.logits, ws.ldl, T, V, H, alpha=head_alpha)
        loss = None
        if lab is not None:
            ops.ce_fwd(ws.logits, ws.ldl, lab, V, 1.0 if head_alpha != 1.0 else self.temperature, IGNORE_INDEX, ws.lse_ce,
                       ws.row_loss, ws.loss_sum, ws.count)
            if torch.is_tensor(num_items_in_batch):
                num_items_in_batch = num_items_in_batch.to(self.device, torch.float32).reshape(1)
                loss = ws.loss_sum[0] / num_items_in_batch[0]
            elif num_items_in_batch is not None:
                loss = ws.loss_sum[0] / float(num_items_in_batch)
            else:
                loss = ws.loss_sum[0] / ws.count[0]
        self._saved = dict(ids=ids, labels=lab, num_items=num_items_in_batch, train=train, p_att=p_att, B=B, S=S,
                           dropout_step=self.dropout_step)
        return loss, ws.logits.view(B, S, ws.ldl)[:, :, :V]

    def check_inputs(self):
        """Host-synchronising validation: labels outside the vocabulary (nn.CrossEntropyLoss raises on them)."""
        n = int(self.ws.bad_label.item())
        if n:
            raise IndexError(f"{n} label(s) outside [0, vocab_size={self.cfg.vocab_size}) that are not -100 "
                             "(nn.CrossEntropyLoss raises 'Target out of bounds' in the reference)")

    # ------------------------------------------------------------------------------------------
    @ops.scoped_f32_matmul(lambda self, *a: self.matmul, lambda self, *a: self._planes())
    @ops.scoped_amax(lambda self, *a: self._amax)
    def _backward(self, dloss: float = 1.0, layer_done=None, dloss_dev: Optional[torch.Tensor] = None):
        """See ``Engine._backward``."""
        sv = self._saved
        if sv is None or not sv["train"] or sv["labels"] is None:
            raise RuntimeError("backward() needs forward(train=True, labels=...) first")
        cfg, ws = self.cfg, self.ws
        B, S = sv["B"], sv["S"]
        T, H = B * S, cfg.hidden_size
        nq, nkv, dh, I = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size
        NQ, NKV = nq * dh, nkv * dh
        QKV = NQ + 2 * NKV
        eps = float(cfg.rms_norm_eps)
        p_att = sv["p_att"]
        saved_step = self.dropout_step
        self.dropout_step = sv["dropout_step"]          # regenerate exactly the forward's masks
        m = ws.mask
        cos, sin = self.rope(S)
        scale = float(dh) ** -0.5
        V = cfg.vocab_size
        emb = self.params["model.embed_tokens.weight"]
        demb = self.grads["model.embed_tokens.weight"]
        norm_dws: List[torch.Tensor] = []
        bf16 = self.dtype == "bf16"
        split_attn = self.split_attention and self.matmul != "f32" and not bf16
        fuse_delta = (ws.ds_work is not None or bf16 or split_attn) and T % 128 == 0 and NQ % 128 == 0
        h2_bwd = split_attn and self.h2_attention and self.matmul == "split3" and p_att < 0.75
        do_amax = dict(c_amax=(ws.dao, 0)) if (h2_bwd and self.gemm_c_amax) else {}
        fuse_swiglu_bwd = (bf16 or self.matmul == "split3") and self.fuse_swiglu_bwd

        def dgrad(dy, lddy, Wf, Wt, ldw, dx, lddx, n_out, k_in, **kw):
            if bf16:
                ops.linear_dgrad_t(dy, lddy, Wt, Wt.shape[1], dx, lddx, T, n_out if Wt.shape[1] == n_out else Wt.shape[1],
                                   k_in, **kw)
            else:
                ops.linear_dgrad(dy, lddy, Wf, ldw, dx, lddx, T, n_out, k_in, **kw)

        def norm_bwd(xin, w, dy, dw, accumulate_dx, branch: bool):
            """dx (+)= the RMSNorm's input gradient; ``branch``: also t0 = dx in the activation dtype (the output gradient
            of the residual branch that reads dx next - the Multi engine's dropout-mask pass with p = 0)."""
            part = ws.norm_partial[len(norm_dws)]
            norm_dws.append(dw)
            if branch:
                ops.rmsnorm_bwd(xin, w, dy, H, eps, ws.dx, part, accumulate_dx, mask_out=ws.tmpH[0], p=0.0, seed=0)
            else:
                ops.rmsnorm_bwd(xin, w, dy, H, eps, ws.dx, part, accumulate_dx)

        # ---- loss -> logits -> final norm ----
        if torch.is_tensor(sv["num_items"]):
            ops.ce_bwd(ws.logits, ws.ldl, sv["labels"], V, self.temperature, IGNORE_INDEX, ws.lse_ce, sv["num_items"], 0.0,
                       dloss, dloss_dev)
        elif sv["num_items"] is not None:
            ops.ce_bwd(ws.logits, ws.ldl, sv["labels"], V, self.temperature, IGNORE_INDEX, ws.lse_ce, None,
                       float(sv["num_items"]), dloss, dloss_dev)
        else:
            ops.ce_bwd(ws.logits, ws.ldl, sv["labels"], V, self.temperature, IGNORE_INDEX, ws.lse_ce, ws.count, 0.0,
                       dloss, dloss_dev)
        hold = self._amax.hold if self._amax is not None else (lambda *t: contextlib.nullcontext())
        t0, t1, t2, t3 = ws.tmpH
        with hold(ws.logits):
            ops.linear_wgrad(ws.logits, ws.ldl, ws.xn, H, demb, H, T, V, H)
            dgrad(ws.logits, ws.ldl, emb, self.shadow.t("model.embed_tokens.weight") if bf16 else None, H, t3, H, V, H)
        norm_bwd(ws.x_final, self.params["model.norm.weight"], t3, self.grads["model.norm.weight"], False, True)

        for l in reversed(range(cfg.num_hidden_layers)):
            W, G, A, xs = self.W[l], self.G[l], ws.layers[l], ws.x[l]
            WT = self.WT[l] if bf16 else None
            # ---- MLP ----   (t0 = d layer output)
            with hold(t0):
                ops.linear_wgrad(t0, H, A["hm"], I, G.down, I, T, H, I)
                if fuse_swiglu_bwd:
                    # the down projection's input gradient with the SwiGLU backward in its epilogue: A["gu"] <- d gate | d up
                    if bf16:
                        ops.linear_dgrad_t(t0, H, WT.down, WT.down.shape[1], ws.dhm, I, T, H, I, swiglu_bwd=(A["gu"], 2 * I))
                    else:
                        ops.gemm(t0, H, 1, W.down, 1, I, ws.dhm, I, T, I, H, swiglu_bwd=(A["gu"], 2 * I))
                else:
                    dgrad(t0, H, W.down, WT.down if bf16 else None, I, ws.dhm, I, H, I)
            if not fuse_swiglu_bwd:
                ops.swiglu_bwd_ld(A["gu"], 2 * I, T, I, ws.dhm, 0.0, 0)
            with hold(A["gu"]):
                ops.linear_wgrad(A["gu"], 2 * I, A["hin"], H, G.gu, H, T, 2 * I, H)
                dgrad(A["gu"], 2 * I, W.gu, WT.gu if bf16 else None, H, ws.dhin, H, 2 * I, H)
            norm_bwd(xs[1], W.ln2, ws.dhin, G.ln2, True, True)
            # ---- self attention ----   (t0 = d(x after the attention block))
            SA, GS = W.self_attn, G.self_attn
            ST = WT.self_attn if bf16 else dict(o=None, qkv=None)
            with hold(t0):
                ops.linear_wgrad(t0, H, A["ao"], NQ, GS["o"], NQ, T, H, NQ)
                dgrad(t0, H, SA["o"], ST["o"], NQ, ws.dao, NQ, H, NQ, rowdot=(A["ao"], ws.delta, S) if fuse_delta else None,
                      **do_amax)
            q, k, v, seed = A["q"], A["k"], A["qkv"][:, NQ + NKV:], self._seed(l, 0)
            dv = ws.dqkv[:, NQ + NKV:]
            if split_attn:
                ops.attn_bwd_split(q, NQ, k, NKV, v, QKV, A["ao"], ws.dao, A["lse"], m["kl_self"], None, m["empty_self"],
                                   m["tile_empty_self"], B, S, nq, nkv, scale, p_att, seed, ws.delta, ws.dq, NQ, ws.dk, NKV, dv,
                                   QKV, delta_ready=fuse_delta, dv_of=ws.dqkv, h2=h2_bwd)
            elif bf16:
                ops.attn_bwd_bf16(q, NQ, k, NKV, v, QKV, A["ao"], ws.dao, A["lse"], m["kl_self"], None, B, S, nq, nkv, scale,
                                  p_att, seed, ws.delta, ws.dq, NQ, ws.dk, NKV, dv, QKV, delta_ready=fuse_delta)
            else:
                ops.attn_bwd(q, NQ, k, NKV, v, QKV, A["ao"], ws.dao, A["lse"], m["kl_self"], None, m["empty_self"],
                             m["tile_empty_self"], B, S, nq, nkv, scale, p_att, seed, ws.delta, ws.dq, NQ, ws.dk, NKV, dv, QKV,
                             ds_work=ws.ds_work, delta_ready=fuse_delta and ws.ds_work is not None)
            ops.qknorm_rope_bwd(A["qkv"], ws.dq, ws.dk, S, nq, nkv, SA["qn"], SA["kn"], eps, cos, sin, ws.dqkv, GS["qn"],
                                GS["kn"], partial=ws.qk_partial)
            with hold(ws.dqkv):
                ops.linear_wgrad(ws.dqkv, QKV, A["h1"], H, GS["qkv"], H, T, QKV, H)
                dgrad(ws.dqkv, QKV, SA["qkv"], ST["qkv"], H, t3, H, QKV, H)
            norm_bwd(xs[0], W.ln1, t3, G.ln1, True, l > 0)
            if layer_done is not None:
                layer_done(l)
        self._check_deterministic_embedding()
        if self.ordered_embedding_grad and V <= 8191:
            ops.embedding_bwd_ordered(sv["ids"], ws.dx, cfg.pad_token_id, demb)
        else:
            ops.embedding_bwd(sv["ids"], ws.dx, cfg.pad_token_id, demb)
        key = tuple(d.data_ptr() for d in norm_dws)
        if self._norm_out_table is None or self._norm_out_table[0] != key:
            self._norm_out_table = (key, torch.tensor(key, dtype=torch.int64, device=self.device))
        ops.colsum_reduce_batched(ws.norm_partial, len(norm_dws), self._norm_out_table[1], accumulate=True)
        self.dropout_step = saved_step
