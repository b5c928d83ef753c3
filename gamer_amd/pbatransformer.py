"""PBATransformer, the position- and behaviour-aware T5 backbone of the decoder tasks, on the HIP path.

Same nn.Module surface, state-dict names and shapes as the reference (ref:SeqRec/models/generative/PBATransformer/model.py, a
Switch-Transformers T5 with a temperature): TIGER's names for the tied table, the attention layers and the layer norms, and in the
last layer of every block ``mlp.mlp.{wi,wo}.weight`` (a dense layer) or ``mlp.experts.expert_{e}.{wi,wo}.weight`` (a sparse one),
with ``mlp.behavior_embedding.weight`` and ``wi`` of d_model + behavior_embedding_dim columns where the layer injects the
behaviour.  A reference checkpoint loads here and one saved here loads there.

What differs from gamer_amd.tiger is the feed-forward layer of a block; the attention half of the block, the stacks' input and
final norm, the loss and the beam search are TIGER's code (``tiger.attn_half_fwd / _bwd``, ``TIGER._stack``, ``TIGER.forward``,
``tiger.beam_search``).  Every step runs as HIP kernels, with no PyTorch fallback:
  routers       gamer_pba_router, one launch per stack call: the expert (= position) and the behaviour index of every token from the
                ids alone (ref:.../router.py), and expert * (num_behavior + 1) + behaviour as the row's group key
  rows          gamer_expert_lists sorts the rows by that key once per stack call and kind of layer; rows that no expert owns
                (Moe_behavior_only with behaviour tokens routes the item tokens to position 2 of 2 experts) lie behind the last
                group and keep the zero output the reference gives them
  feed forward  wi on the d_model columns as one grouped fp32 GEMM over the experts' row ranges; the behaviour columns' share,
                behavior_embedding[b] @ wi_e[:, d_model:]^T, as a table row per (expert, behaviour) (gamer_inject_table_fwd) that
                gamer_relu_tbl_fwd adds while it applies ReLU and dropout - the [T, d_model + behavior_embedding_dim] concatenation
                never exists; wo as a second grouped GEMM.  Backward: gamer_relu_tbl_bwd in place, the grouped input and weight
                gradients, and gamer_segment_colsum + gamer_inject_table_bwd for the behaviour columns and the embedding
A dense layer is the one-expert case; a dense layer without injection runs without sorting.

Not the reference's: an unmapped behaviour token at a position whose behaviour is used indexes ``behavior_embedding`` out of range
there; here the router counts such positions and ``check_inputs()`` raises ValueError (the commands call it after a step).  The
z and auxiliary router losses of the reference are literally 0 and are not formed.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch
from torch import nn

from . import modules, ops, tiger
from .layer_blocks import _dropout_bwd, add_dropout
from .tiger import T5LayerCrossAttention, T5LayerNorm, T5LayerSelfAttention, _f32, _linear, _linear_bwd, _rms, _rms_bwd

MAX_GROUPS = 64          # gamer_expert_lists: num_experts * (num_behavior + 1) row groups at most
MAX_NB1, MAX_EB = 16, 256  # gamer_inject_table_fwd


@dataclasses.dataclass(init=False)
class PBATransformerConfig(tiger.TigerConfig):
    """TIGER's keys with SwitchTransformersConfig's defaults, and the keys of ref:.../PBATransformer/configuration.py; every other
    key is dropped without a word.  ``num_experts`` is derived as the reference derives it."""
    d_model: int = 768
    d_ff: int = 2048
    num_layers: int = 12
    num_heads: int = 12
    dense_act_fn: str = "relu"
    behavior_injection: bool = False
    behavior_embedding_dim: int = 64
    num_positions: int = 4
    num_behavior: int = 4
    n_positions: int = 50
    sparse_layers_encoder: list = dataclasses.field(default_factory=list)
    sparse_layers_decoder: list = dataclasses.field(default_factory=list)
    behavior_injection_encoder: list = dataclasses.field(default_factory=list)
    behavior_injection_decoder: list = dataclasses.field(default_factory=list)
    Moe_behavior_only: bool = False
    shared_expert: bool = False
    use_behavior_token: bool = True
    behavior_maps: dict = dataclasses.field(default_factory=dict)
    use_user_token: bool = False
    num_experts: int = 5

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        for name in ("sparse_layers_encoder", "sparse_layers_decoder", "behavior_injection_encoder", "behavior_injection_decoder"):
            setattr(self, name, [int(i) for i in kwargs.get(name) or []])
        self.behavior_maps = {int(k): int(v) for k, v in (kwargs.get("behavior_maps") or {}).items()}
        self.derive_num_experts()

    def derive_num_experts(self):
        """configuration.py:57-60: one expert per position and one for <s>, </s> and padding, or two"""
        self.num_experts = 2 if self.Moe_behavior_only else self.num_positions + 1
        return self.num_experts


# ---- parameter holders with the reference's names ----------------------------------------------------------------------------------
class PBATransformerDenseActDense(nn.Module):
    def __init__(self, config: PBATransformerConfig, behavior_injection: bool):
        super().__init__()
        self.wi = nn.Linear(config.d_model + (config.behavior_embedding_dim if behavior_injection else 0), config.d_ff, bias=False)
        self.wo = nn.Linear(config.d_ff, config.d_model, bias=False)


class PBATransformerSparseMLP(nn.Module):
    def __init__(self, config: PBATransformerConfig, is_sparse: bool, behavior_injection: bool):
        super().__init__()
        self.is_sparse, self.behavior_injection = is_sparse, behavior_injection
        if is_sparse:
            self.experts = nn.ModuleDict({f"expert_{e}": PBATransformerDenseActDense(config, behavior_injection)
                                          for e in range(config.num_experts)})
        else:
            self.mlp = PBATransformerDenseActDense(config, behavior_injection)
        if behavior_injection:
            self.behavior_embedding = nn.Embedding(config.num_behavior + 1, config.behavior_embedding_dim)

    def expert_list(self):
        return list(self.experts.values()) if self.is_sparse else [self.mlp]


class PBATransformerLayerFF(nn.Module):
    def __init__(self, config: PBATransformerConfig, is_sparse: bool, behavior_injection: bool):
        super().__init__()
        self.is_sparse = is_sparse
        self.mlp = PBATransformerSparseMLP(config, is_sparse, behavior_injection)
        self.layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


class PBATransformerBlock(nn.Module):
    def __init__(self, config, is_decoder: bool, has_relative_attention_bias: bool, is_sparse: bool, behavior_injection: bool):
        super().__init__()
        self.layer = nn.ModuleList([T5LayerSelfAttention(config, has_relative_attention_bias)])
        if is_decoder:
            self.layer.append(T5LayerCrossAttention(config))
        self.layer.append(PBATransformerLayerFF(config, is_sparse, behavior_injection))


class PBATransformerStack(nn.Module):
    def __init__(self, config: PBATransformerConfig, embed_tokens: nn.Embedding, is_decoder: bool):
        super().__init__()
        self.is_decoder = is_decoder
        self.embed_tokens = embed_tokens
        n = config.num_decoder_layers if is_decoder else config.num_layers
        sparse = config.sparse_layers_decoder if is_decoder else config.sparse_layers_encoder
        inject = config.behavior_injection_decoder if is_decoder else config.behavior_injection_encoder
        self.block = nn.ModuleList([PBATransformerBlock(config, is_decoder, i == 0, i in sparse, i in inject) for i in range(n)])
        self.final_layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


# ---- routing ---------------------------------------------------------------------------------------------------------------------
class _Lists:
    """The rows of one stack call ordered by a group key: ``perm`` int64 [T] (sorted slot -> flat row), ``offsets`` int32 [G + 1],
    ``eoffs`` int32 [E + 1] the experts' ranges (every ``per`` groups one expert), ``gid`` int32 [T] the group of every sorted row
    (outside [0, G) for the rows behind the last group)."""

    def __init__(self, keys: torch.Tensor, G: int, per: int):
        B, S = keys.shape
        dev = keys.device
        i32 = dict(dtype=torch.int32, device=dev)
        perm, slot = torch.empty(B * S, **i32), torch.empty(B * S, **i32)
        self.offsets = torch.empty(G + 1, **i32)
        ops.expert_lists(keys, G, perm, slot, self.offsets, torch.empty((B + 1) * G, **i32))
        self.perm = perm.long()
        self.gid = keys.reshape(-1).index_select(0, self.perm).contiguous()
        self.eoffs = self.offsets[::per].contiguous()
        self.G, self.E = G, G // per


class _Route:
    """The router outputs of one stack call and, per kind of layer, the sorted row lists (built on first use, shared by the
    layers of that kind)."""

    def __init__(self, expert, beh, key, E, NB1):
        self.expert, self.beh, self.key, self.E, self.NB1 = expert, beh, key, E, NB1
        self._lists = {}

    def lists(self, sparse: bool, inject: bool) -> Optional[_Lists]:
        if not sparse and not inject:
            return None
        if (sparse, inject) not in self._lists:
            if sparse and inject:
                made = _Lists(self.key, self.E * self.NB1, self.NB1)
            elif sparse:
                made = _Lists(self.expert, self.E, 1)
            else:
                made = _Lists(self.beh, self.NB1, self.NB1)
            self._lists[sparse, inject] = made
        return self._lists[sparse, inject]


# ---- the feed-forward layer ----------------------------------------------------------------------------------------------------------
def _grp(lists: _Lists) -> dict:
    """the experts' row ranges as the grouped GEMM takes them; a single expert holds every row and runs ungrouped"""
    return dict(groups=lists.E, group_offsets=lists.eoffs) if lists.E > 1 else {}


def ffn_fwd(n2, W1, W2, Eb, lists: Optional[_Lists], p: float, seed: int):
    """wo_e(dropout(relu(wi_e(cat(n2, Eb[b]))))) of every row's expert e and behaviour b.  n2 [T, D]; W1 [E, dff, D (+ EB)], W2
    [E, D, dff] the experts' stacked weights; Eb [NB1, EB] or None (no injection); ``lists`` None: one expert, no injection, no
    sorting.  Returns (out [T, D] in row order, the tensors the backward needs)."""
    T, D = n2.shape
    E, dff, Kw = W1.shape
    dev = n2.device
    act = torch.empty(T, dff, **_f32(dev))
    if lists is None:
        pre = _linear(n2, W1[0])
        ops.relu_tbl_fwd(pre, dff, T, dff, p, seed, act)
        return _linear(act, W2[0]), (n2, pre, act, None)
    grp = _grp(lists)
    xs = n2.index_select(0, lists.perm)
    pre = torch.zeros(T, dff, **_f32(dev))
    ops.linear_fwd(xs, D, W1, Kw, pre, dff, T, dff, D, strideB=dff * Kw, **grp)
    tbl = None
    if Eb is not None:
        tbl = torch.empty(lists.G, dff, **_f32(dev))
        ops.inject_table_fwd(Eb, W1, Kw, D, E, dff, tbl)
    ops.relu_tbl_fwd(pre, dff, T, dff, p, seed, act, tbl, None if tbl is None else lists.gid, lists.G if tbl is not None else 0)
    outs = torch.zeros(T, D, **_f32(dev))
    ops.linear_fwd(act, dff, W2, dff, outs, D, T, D, dff, strideB=D * dff, **grp)
    out = torch.empty(T, D, **_f32(dev))
    out.index_copy_(0, lists.perm, outs)
    return out, (xs, pre, act, tbl)


def ffn_bwd(df, saved, W1, W2, Eb, lists: Optional[_Lists], p: float, seed: int):
    """(dn2 [T, D] in row order, dW1, dW2, dEb or None) from df [T, D] in row order; ``pre`` of ``saved`` is overwritten"""
    xs, pre, act, tbl = saved
    T, D = df.shape
    E, dff, Kw = W1.shape
    dev = df.device
    if lists is None:
        dact, dW2 = _linear_bwd(df, act, W2[0])
        ops.relu_tbl_bwd(pre, dff, T, dff, dact, p, seed)
        dn2, dW1 = _linear_bwd(pre, xs, W1[0])
        return dn2, dW1[None], dW2[None], None
    grp = _grp(lists)
    dfs = df.index_select(0, lists.perm)
    dW1, dW2 = torch.zeros_like(W1), torch.zeros_like(W2)
    ops.linear_wgrad(dfs, D, act, dff, dW2, dff, T, D, dff, strideC=D * dff, **grp)
    dact = torch.zeros(T, dff, **_f32(dev))
    ops.linear_dgrad(dfs, D, W2, dff, dact, dff, T, D, dff, strideB=D * dff, **grp)
    ops.relu_tbl_bwd(pre, dff, T, dff, dact, p, seed, tbl, None if tbl is None else lists.gid, lists.G if tbl is not None else 0)
    ops.linear_wgrad(pre, dff, xs, D, dW1, Kw, T, dff, D, strideC=dff * Kw, **grp)
    dEb = None
    if Eb is not None:
        # the behaviour columns: the column sums of d pre over the rows of every (expert, behaviour) group
        seg = torch.empty(lists.G, dff, **_f32(dev))
        ws = torch.empty(ops.segment_colsum_ws_floats(T, dff, lists.G), **_f32(dev))
        ops.segment_colsum(pre, dff, T, dff, lists.offsets, lists.G, ws, seg)
        dEb = torch.zeros_like(Eb)
        ops.inject_table_bwd(seg, Eb, W1, Kw, D, E, dff, dW1, dEb, torch.empty(Eb.shape[0] * E * Eb.shape[1], **_f32(dev)))
    dxs = torch.zeros(T, D, **_f32(dev))
    ops.linear_dgrad(pre, dff, W1, Kw, dxs, D, T, dff, D, strideB=dff * Kw, **grp)
    dn2 = torch.empty(T, D, **_f32(dev))
    dn2.index_copy_(0, lists.perm, dxs)
    return dn2, dW1, dW2, dEb


def _stacked(ws):
    """[E, N, K] from E weights [N, K] (one weight: a view)"""
    return ws[0][None] if len(ws) == 1 else torch.stack(list(ws)).contiguous()


class _BlockFn(torch.autograd.Function):
    """One PBATransformerBlock: tiger's attention half, then x + dropout(ffn(norm(x))).  params: the attention half's (ln0, q, k,
    v, o, [ln1, cq, ck, cv, co]), block 0's bias table or None, lnf, [behavior_embedding,] then wi, wo of every expert.
    meta["lists"]: the _Lists of this kind of layer or None; meta["inject"]."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, enc, meta, *params):
        na = 10 if enc is not None else 5
        table, lnf = params[na], params[na + 1]
        ffp = params[na + 2:]
        Eb = ffp[0] if meta["inject"] else None
        experts = ffp[1:] if meta["inject"] else ffp
        seeds = [modules._SeedCounter.next() for _ in range(6)]
        x2, saved, info = tiger.attn_half_fwd(x, enc, meta, params[:na], seeds)
        p = info["p"]
        n2 = _rms(x2, lnf, meta["eps"])
        W1, W2 = _stacked(experts[0::2]), _stacked(experts[1::2])
        out, fs = ffn_fwd(n2, W1, W2, Eb, meta["lists"], p, seeds[4])
        x3 = add_dropout(x2, out, p, seeds[5])
        ctx.n_attn = len(saved)
        ctx.save_for_backward(*saved, lnf, W1, W2, Eb, *fs, meta["keep"])
        ctx.meta = dict(meta, table=table, **info)
        return x3.view(x.shape)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        sv = list(ctx.saved_tensors)
        mt = ctx.meta
        B, S, D = mt["shape"]
        p, seeds = mt["p"], mt["seeds"]
        keep_mask = sv.pop()
        attn_sv = sv[:ctx.n_attn]
        lnf, W1, W2, Eb = sv[ctx.n_attn:ctx.n_attn + 4]
        fs = sv[ctx.n_attn + 4:]
        x2 = attn_sv[19] if mt["dec"] else attn_sv[7]
        T = x2.shape[0]
        dx = dout.reshape(T, D).contiguous().float().clone()                      # the gradient of the residual stream, added to in place
        df = _dropout_bwd(dx, D, p, seeds[5])
        dn2, dW1, dW2, dEb = ffn_bwd(df, fs, W1, W2, Eb, mt["lists"], p, seeds[4])
        dlnf = _rms_bwd(x2, lnf, mt["eps"], dn2, dx)
        denc, agrads, dtable = tiger.attn_half_bwd(attn_sv, mt, dx, keep_mask)
        fgrads = [dEb] if mt["inject"] else []
        for e in range(W1.shape[0]):
            fgrads += [dW1[e], dW2[e]]
        return (dx.view(dout.shape), denc, None, *agrads, dtable, dlnf, *fgrads)


class PBATransformerForConditionalGeneration(tiger.TIGER):
    """The model of ``--backbone PBATransformer``.  ``forward``, ``encode``, ``decode``, ``logits``, ``set_hyper``,
    ``resize_token_embeddings`` and ``_shift_right`` are TIGER's; the blocks' last layer and the routers are this module's."""

    def __init__(self, config: PBATransformerConfig):
        nn.Module.__init__(self)
        c = config
        name = "PBATransformer on the HIP path"
        if c.shared_expert:
            raise NotImplementedError(f"{name}: shared_expert=True is not built (the half-width experts next to a shared one)")
        if c.use_user_token:
            raise NotImplementedError(f"{name}: use_user_token=True is not built (no task sets it)")
        if c.feed_forward_proj != "relu" or c.dense_act_fn != "relu":
            raise NotImplementedError(f"{name}: the relu feed-forward layer only (got feed_forward_proj={c.feed_forward_proj!r}, "
                                      f"dense_act_fn={c.dense_act_fn!r})")
        if not c.tie_word_embeddings:
            raise NotImplementedError(f"{name}: tie_word_embeddings=False is not built (the head is the shared table)")
        if c.d_kv not in ops.T5_HEAD_DIMS or c.num_heads > ops.T5_MAX_H or c.num_heads < 1:
            raise NotImplementedError(f"{name}: d_kv in {ops.T5_HEAD_DIMS}, num_heads <= {ops.T5_MAX_H} (got d_kv={c.d_kv}, "
                                      f"num_heads={c.num_heads})")
        if c.d_model % 4 or c.d_model > 256 or c.d_ff % 4:
            raise NotImplementedError(f"{name}: d_model <= 256, d_model and d_ff divisible by 4 (got {c.d_model}, {c.d_ff})")
        c.derive_num_experts()
        injects = bool(c.behavior_injection_encoder or c.behavior_injection_decoder)
        if c.num_positions < 1 or c.num_experts * (c.num_behavior + 1 if injects else 1) > MAX_GROUPS:
            raise NotImplementedError(f"{name}: num_positions >= 1 and at most {MAX_GROUPS} (expert, behaviour) row groups (got "
                                      f"{c.num_experts} experts x {c.num_behavior + 1} behaviour indices)")
        if injects and (c.num_behavior + 1 > MAX_NB1 or c.behavior_embedding_dim % 4 or not 0 < c.behavior_embedding_dim <= MAX_EB):
            raise NotImplementedError(f"{name}: injection with num_behavior < {MAX_NB1} and behavior_embedding_dim a multiple of 4 up "
                                      f"to {MAX_EB} (got {c.num_behavior}, {c.behavior_embedding_dim})")
        self.config = c
        self.model_dim = c.d_model
        self.temperature = 1.0
        self.shared = nn.Embedding(c.vocab_size, c.d_model)
        self.encoder = PBATransformerStack(c, self.shared, False)
        self.decoder = PBATransformerStack(c, self.shared, True)
        self.lm_head = nn.Linear(c.d_model, c.vocab_size, bias=False)
        self.lm_head.weight = self.shared.weight
        self.register_buffer("_zero_bias", torch.zeros(c.d_ff), persistent=False)
        self.register_buffer("_bad_token", torch.zeros(1, dtype=torch.int32), persistent=False)
        self._buckets = {}
        self._lut = None
        self.apply(self._init_weights)

    def _init_weights(self, m: nn.Module):
        """the per-tensor standard deviations of the reference's ``_init_weights`` (model.py:69-137; not its random stream).  Its
        PBATransformerSparseMLP branch runs after the experts' own and leaves wi AND wo at d_model ** -0.5; it does not touch
        ``behavior_embedding``, which keeps nn.Embedding's normal(0, 1)."""
        c = self.config
        f = c.initializer_factor
        if isinstance(m, PBATransformerForConditionalGeneration):
            m.shared.weight.data.normal_(mean=0.0, std=f * 1.0)
        elif isinstance(m, PBATransformerSparseMLP):
            for ex in m.expert_list():
                ex.wi.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)
                ex.wo.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)
        else:
            super()._init_weights(m)

    def resize_token_embeddings(self, n: int) -> nn.Embedding:
        self._lut = None
        return super().resize_token_embeddings(n)

    # ---- the routers -------------------------------------------------------------------------------------------------------------
    def _behavior_lut(self, device) -> Optional[torch.Tensor]:
        """int32 [vocab] on the device: the behaviour index of a behaviour token, -1 elsewhere"""
        c = self.config
        if not c.use_behavior_token:
            return None
        V = self.shared.weight.shape[0]
        if self._lut is None or self._lut.device != device or self._lut.numel() != V:
            lut = torch.full((V,), -1, dtype=torch.int32)
            for tok, idx in c.behavior_maps.items():
                if not 0 <= int(tok) < V or not 0 <= int(idx) < c.num_behavior:
                    raise ValueError(f"behavior_maps: token {tok} -> {idx} outside the vocabulary of {V} / the {c.num_behavior} behaviours")
                lut[int(tok)] = int(idx)
            self._lut = lut.to(device)
        return self._lut

    def route(self, ids: torch.Tensor, decoder: bool) -> _Route:
        """the router of a stack on ids int64 [B, S] (gamer_pba_router); refuses the shapes the reference's routers fail on"""
        c = self.config
        B, S = ids.shape
        P = c.num_positions
        if decoder:
            if S > P + 2:
                raise ValueError(f"PBATransformer: decoder rows of at most num_positions + 2 = {P + 2} tokens (got {S})")
        else:
            if c.use_behavior_token and (S - 1) % P != 0:
                raise ValueError(f"PBATransformer: encoder rows of k x num_positions + 1 tokens with behaviour tokens (got {S}, "
                                 f"num_positions {P})")
            if S > c.n_positions * P + 1:
                raise ValueError(f"PBATransformer: encoder rows of at most n_positions x num_positions + 1 = {c.n_positions * P + 1} "
                                 f"tokens (got {S})")
        i32 = dict(dtype=torch.int32, device=ids.device)
        expert, beh, key = torch.empty(B, S, **i32), torch.empty(B, S, **i32), torch.empty(B, S, **i32)
        NB1 = c.num_behavior + 1
        ops.pba_router(ids.long().contiguous(), decoder, P, c.n_positions, c.Moe_behavior_only, c.use_behavior_token,
                       self._behavior_lut(ids.device), NB1, c.num_experts, c.pad_token_id, c.eos_token_id, expert, beh, key,
                       self._bad_token)
        return _Route(expert, beh, key, c.num_experts, NB1)

    def check_inputs(self):
        """raises ValueError when a router since the last call met a position whose behaviour is used and whose behaviour slot
        holds no token of ``behavior_maps`` (one copy of an integer from the device)"""
        n = int(self._bad_token)
        if n:
            self._bad_token.zero_()
            raise ValueError(f"PBATransformer: {n} positions follow a behaviour slot whose token is not in behavior_maps "
                             f"(the reference indexes behavior_embedding out of range there)")

    # ---- TIGER's hooks -----------------------------------------------------------------------------------------------------------
    def _route(self, stack, ids):
        return self.route(ids, stack.is_decoder)

    @staticmethod
    def _ff_params(ff: PBATransformerLayerFF):
        mlp = ff.mlp
        params = [mlp.behavior_embedding.weight] if mlp.behavior_injection else []
        for ex in mlp.expert_list():
            params += [ex.wi.weight, ex.wo.weight]
        return params

    def _block(self, stack, l, x, enc, meta, attn_params, table, route):
        if meta.get("pack") is not None:
            raise NotImplementedError("PBATransformer on the HIP path: packed rows are not built")
        ff = stack.block[l].layer[-1]
        mlp = ff.mlp
        meta = dict(meta, inject=mlp.behavior_injection, lists=route.lists(mlp.is_sparse, mlp.behavior_injection))
        return _BlockFn.apply(x, enc, meta, *attn_params, table, ff.layer_norm.weight, *self._ff_params(ff))

    def _eval_ffn_weights(self, stack, l) -> dict:
        ff = stack.block[l].layer[-1]
        mlp = ff.mlp
        ws = [ex for ex in mlp.expert_list()]
        return dict(lnf=ff.layer_norm.weight.detach(), W1=_stacked([ex.wi.weight.detach() for ex in ws]),
                    W2=_stacked([ex.wo.weight.detach() for ex in ws]), sparse=mlp.is_sparse, inject=mlp.behavior_injection,
                    Eb=mlp.behavior_embedding.weight.detach() if mlp.behavior_injection else None)

    def _eval_ffn(self, x, L, route):
        n2 = _rms(x, L["lnf"], self.config.layer_norm_epsilon)
        out, _ = ffn_fwd(n2, L["W1"], L["W2"], L["Eb"], route.lists(L["sparse"], L["inject"]), 0.0, 0)
        return add_dropout(x, out, 0.0, 0)

    def forward(self, input_ids, attention_mask=None, labels=None, decoder_input_ids=None, want_logits=None, packed=False, **kwargs):
        """(loss, logits) as TIGER.forward; the z and auxiliary router losses of the reference are 0"""
        if packed:
            raise NotImplementedError("PBATransformer on the HIP path: packed=True is not built (the routers read the padded rows)")
        kwargs.pop("output_router_logits", None)
        return super().forward(input_ids, attention_mask, labels=labels, decoder_input_ids=decoder_input_ids, want_logits=want_logits,
                               **kwargs)

    def encode(self, input_ids, attention_mask=None, packed=False, lengths=None):
        if packed:
            raise NotImplementedError("PBATransformer on the HIP path: packed=True is not built (the routers read the padded rows)")
        return super().encode(input_ids, attention_mask)


@torch.no_grad()
def beam_search(model: PBATransformerForConditionalGeneration, input_ids, attention_mask, trie, num_beams: int, max_new_tokens: int,
                decoder_prefix=None):
    """Trie-constrained beam search, ``tiger.beam_search`` with this model's feed-forward step: routed and injected, every
    hypothesis routed by its OWN tokens (the behaviour of a hypothesis is the token at its position 1).  The semantics are those
    of the reference's ``generate(..., use_cache=False)``.  The reference's cached decoder router keeps
    ``cached_input_id_sequence`` without reordering it when the beams are reordered, so that with ``use_cache=True`` a hypothesis
    can be routed by another hypothesis' behaviour token; that is not reproduced.  Arguments and result as tiger.beam_search;
    raises ValueError afterwards when a router met an unmapped behaviour token at a used slot."""
    out = tiger.beam_search(model, input_ids, attention_mask, trie, num_beams, max_new_tokens, decoder_prefix=decoder_prefix)
    model.check_inputs()
    return out


@torch.no_grad()
def score_items(model: PBATransformerForConditionalGeneration, input_ids, attention_mask, items, decoder_prefix=None, packed=False,
                lengths=None, max_rows: int = 65536):
    """``tiger.score_items`` with this model's feed-forward step: every candidate is routed by its OWN tokens (its behaviour is the
    token at position 1 of its row, from ``decoder_prefix`` [B, 2]).  Arguments and result as tiger.score_items; ``packed=True`` is
    refused (the routers read the padded rows); raises ValueError afterwards when a router met an unmapped behaviour token at a
    used slot."""
    out = tiger.score_items(model, input_ids, attention_mask, items, decoder_prefix=decoder_prefix, packed=packed, lengths=lengths,
                            max_rows=max_rows)
    model.check_inputs()
    return out
