"""MBSTR, the first behaviour-aware baseline of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface, parameter and state-dict names as the reference (ref:SeqRec/models/discriminative/MBSTR/model.py,
ref:SeqRec/modules/layers/mbs_transformer.py): ``item_embedding`` [n_items + 2, H] (row 0 pads, row n_items + 1 is ``<MASK>``; no
position table, no input LayerNorm), ``trm_encoder.layer.{l}.multi_head_attention.{W1, alpha1, W2, alpha2, query, key, value,
relative_position_bias.{c}.relative_attention_bias, LayerNorm}``, ``trm_encoder.layer.{l}.feed_forward.{FFN.{i}.*, LayerNorm}``,
``head.{shared_experts, specific_experts, w_gates, ln}`` and ``head.token_embeddings``, the item table again (two state-dict
keys, one parameter).  A reference ``best_model.pth`` loads here and one saved here loads into the reference class.

With b behaviours a token has a type t in [0, b] (0 = padding) and a (query, key) pair the index c = 0 if either type is 0,
else (t_q - 1) b + t_k.  Every step runs as HIP kernels, with no PyTorch fallback:
  masking       gamer_cloze_mask at ft_ratio = 0, which is exactly the reference's rule (rand < mask_ratio and item != 0)
  input         gamer_embedding_fwd + dropout; backward gamer_embedding_bwd_large into the gradient buffer shared with the head
  projections   Q / K / V = x_i . {query, key, value}[t_i]: ONE grouped fp32 GEMM over the rows sorted by type (gamer_expert_lists),
                a row multiplied by its own behaviour's weights only
  attention     gamer_mbs_mix_fwd (W1m, W2m), gamer_mbs_attn_fwd / _bwd: the [B, h, L, L, b b + 1] tensors of the reference are
                never formed, nothing of size L^2 reaches memory (csrc/mbs_attention.hip)
  FFN           dense_2[t](act(dense_1[t](x))) as two grouped GEMMs over the same sorted rows (the bias rides as one more input
                column), zero for padding; the experts' own LayerNorms are never used (no gradient), as in the reference
  head          CGC on the M masked rows only: the shared experts as one GEMM, the specific experts and the gates grouped by type,
                gamer_mbs_gate_mix_fwd / _bwd, LayerNorm, then gamer_catalog_ce_fwd / _bwd on items [0, n_items]; ranking:
                gamer_catalog_topk.  behavior_head=False: BERT4Rec's DotProductPredictionHead on the biased catalogue kernels.
                The cloze task around it is rec_common.ClozeMixin, which BERT4Rec uses too; the types ride along as its ``extra``.

Reference behaviour kept on purpose:
  * ``apply(_init_weights)`` redraws Linear / Embedding weights and ``query`` / ``key`` / ``value`` with normal(0,
    initializer_range); ``W1``, ``W2``, ``alpha1``, ``alpha2`` and ``w_gates`` keep their ``torch.randn`` draw; the item table is
    visited twice (``head.token_embeddings``).
  * ``behavior_moe=False`` and ``n_behaviors < 2`` cannot run in the reference (AttributeError) and are refused here.
  * No masked position (M = 0): the loss is NaN and every parameter of the graph gets an all-zero gradient.
  * A type outside [0, n_behaviors] raises (the reference's one_hot does).
Not the reference's: keys are masked by their TYPE (0 = padding), which is the item mask on every batch the collator emits; masks
(cloze and dropout) come from the project's counter-based hash.  ``behavior_attention=False`` is not built yet.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import nn

from . import modules, ops
from .layer_blocks import (_TypeLists, _aug_weights, _with_ones, colsum, grouped_ffn_bwd, grouped_ffn_fwd, layernorm_bwd,
                           post_ln_bwd, post_ln_fwd, split_aug_grads)
from .rec_common import ClozeMixin, DotProductPredictionHead, DropUnknownConfig, EmbedDropoutFn, GatherLinearFn, _next_seed

_REF_FFN_ERROR = "'FeedForward' object has no attribute 'dropout'"


@dataclasses.dataclass(init=False)
class MBSTRConfig(DropUnknownConfig):
    """The fields and defaults of the reference's MBSTRConfig (ref:SeqRec/models/discriminative/MBSTR/config.py); unknown keys are
    dropped, as the reference's pydantic model does."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 64
    inner_size: int = 256
    dropout_prob: float = 0.2
    hidden_act: str = "relu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    mask_ratio: float = 0.2
    loss_type: str = "CE"
    num_buckets: int = 32
    max_distance: int = 40
    behavior_head: bool = True
    behavior_attention: bool = True
    behavior_moe: bool = True
    behavior_position_bias: bool = True
    n_shared_experts: int = 3
    n_specific_experts: int = 1


def relative_position_buckets(L: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    """int32 [2 L - 1] on the CPU: the bucket of the offset k - q at index k - q + L - 1 (T5's bidirectional rule, as
    ref:SeqRec/modules/layers/mbs_transformer.py RelativePositionBias buckets it).  Each direction has num_buckets / 2 buckets, keys
    after the query in the upper half; a distance below a quarter of num_buckets has a bucket of its own, larger ones share
    logarithmic buckets up to max_distance.  The logarithmic index is the reference's fp32 torch expression term for term, so the
    floor at a bucket boundary cannot differ (tests/golden/mbstr_small.npz holds the reference's tables)."""
    offset = torch.arange(-(L - 1), L, dtype=torch.long)
    per_side = num_buckets // 2
    max_exact = per_side // 2
    dist = offset.abs()
    log_index = max_exact + (
        torch.log(dist.float() / max_exact) / math.log(max_distance / max_exact) * (per_side - max_exact)
    ).long()
    bucket = torch.where(dist < max_exact, dist, log_index.clamp(max=per_side - 1))
    return (bucket + per_side * (offset > 0).long()).to(torch.int32)


# ---- parameter holders with the reference's names ------------------------------------------------------------------------------
class RelativePositionBias(nn.Module):
    def __init__(self, num_buckets: int = 32, max_distance: int = 128, n_heads: int = 2):
        super().__init__()
        self.num_buckets = num_buckets
        self.max_distance = max_distance
        self.relative_attention_bias = nn.Embedding(num_buckets, n_heads)


class MBSMultiHeadAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout, layer_norm_eps, n_behaviors, behavior_position_bias, num_buckets=32,
                 max_distance=40):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)" % (embed_dim, num_heads))
        h, d, b = num_heads, embed_dim // num_heads, n_behaviors
        self.num_attention_heads, self.attention_head_size, self.all_head_size = h, d, embed_dim
        self.n_behaviors = b
        self.behavior_attention, self.behavior_position_bias = True, behavior_position_bias
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        self.W1 = nn.Parameter(torch.randn(b, h, d, d))
        self.alpha1 = nn.Parameter(torch.randn(b * b + 1, b, h))
        self.W2 = nn.Parameter(torch.randn(b, h, d, d))
        self.alpha2 = nn.Parameter(torch.randn(b * b + 1, b, h))
        self.query = nn.Parameter(torch.randn(b + 1, embed_dim, h, d))
        self.key = nn.Parameter(torch.randn(b + 1, embed_dim, h, d))
        self.value = nn.Parameter(torch.randn(b + 1, embed_dim, h, d))
        self.attn_dropout = nn.Dropout(dropout)
        if behavior_position_bias:
            self.relative_position_bias = nn.ModuleList([
                RelativePositionBias(num_buckets=num_buckets, max_distance=max_distance, n_heads=h) for _ in range(b * b + 1)])
        self.LayerNorm = nn.LayerNorm(embed_dim, eps=layer_norm_eps)
        self.out_dropout = nn.Dropout(dropout)


class MBSFeedForward(nn.Module):
    def __init__(self, d_model, dim_feedforward, dropout, activation, layer_norm_eps, n_behaviors):
        super().__init__()
        self.n_behaviors = n_behaviors
        self.behavior_moe = True
        self.FFN = nn.ModuleList([modules.FeedForward(d_model, dim_feedforward, dropout, activation, layer_norm_eps)
                                  for _ in range(n_behaviors)])
        self.LayerNorm = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.dropout = nn.Dropout(dropout)
        # (outside the state dict: the zero bias of the activation kernel, whose real bias rides in the grouped GEMM)
        self.register_buffer("_zero_bias", torch.zeros(dim_feedforward), persistent=False)


class _MBSLayerFn(torch.autograd.Function):
    """One MBSTransformerEncoderLayer.  params: W1, alpha1, W2, alpha2, query, key, value, ln1w, ln1b, ln2w, ln2b, then
    (dense_1.weight, dense_1.bias, dense_2.weight, dense_2.bias) of each behaviour's expert, then the b b + 1 bias tables."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, lists, meta, *params):
        B, L, H = x.shape
        T = B * L
        h, b, act, eps, bucket = meta["heads"], meta["b"], meta["act"], meta["eps"], meta["bucket"]
        p = meta["dropout"] if meta["training"] else 0.0
        d = H // h
        C_ = b * b + 1
        f32 = dict(dtype=torch.float32, device=x.device)
        W1, alpha1, W2, alpha2, query, key, value, ln1w, ln1b, ln2w, ln2b = params[:11]
        ffn = params[11:11 + 4 * b]
        rel = params[11 + 4 * b:]
        seeds = [modules._SeedCounter.next() for _ in range(3)]
        perm, offs = lists.perm, lists.offsets
        xf = x.reshape(T, H).contiguous().float()
        # q | k | v of every row from its own type's weights: one grouped GEMM over the rows sorted by type
        xs = xf.index_select(0, perm)
        wqkv = torch.cat([query.reshape(b + 1, H, H), key.reshape(b + 1, H, H), value.reshape(b + 1, H, H)], 2).contiguous()
        qkv_s = torch.empty(T, 3 * H, **f32)
        ops.gemm(xs, H, 1, wqkv, 1, 3 * H, qkv_s, 3 * H, T, 3 * H, H, groups=b + 1, group_offsets=offs, strideB=3 * H * H)
        qkv = torch.empty(T, 3 * H, **f32)
        qkv.index_copy_(0, perm, qkv_s)
        del qkv_s
        w1m, w2m = torch.empty(C_, h, d, d, **f32), torch.empty(C_, h, d, d, **f32)
        ops.mbs_mix_fwd(W1.contiguous(), alpha1.contiguous(), w1m)
        ops.mbs_mix_fwd(W2.contiguous(), alpha2.contiguous(), w2m)
        relt = torch.stack(list(rel)).contiguous() if rel else None
        ctxv, lse = torch.empty(T, H, **f32), torch.empty(B, h, L, **f32)
        scale = math.sqrt(1.0 / float(d))
        ops.mbs_attn_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], lists.types, w1m, w2m, relt, bucket, B, L, h, d, b, scale, p,
                         seeds[0], ctxv, lse)
        y1, ln1 = post_ln_fwd(xf, ctxv, ln1w, ln1b, eps, p, seeds[1])            # x + dropout(context): no output projection
        # the behaviour FFN: groups 1 .. b of the sorted rows; padding rows (group 0) stay zero
        w1a, w2a = _aug_weights(ffn[0::4], ffn[1::4]), _aug_weights(ffn[2::4], ffn[3::4])
        f2, fsv = grouped_ffn_fwd(y1, perm, dict(groups=b, group_offsets=offs[1:]), w1a, w2a, act, meta["zero_bias"])
        out, ln2 = post_ln_fwd(y1, f2, ln2w, ln2b, eps, p, seeds[2])
        ctx.meta = dict(meta, p=p, seeds=seeds, scale=scale, shape=(B, L, H), n_rel=len(rel))
        ctx.lists = lists
        ctx.save_for_backward(xs, wqkv, qkv, W1, alpha1, W2, alpha2, w1m, w2m, relt, ctxv, lse, *ln1, ln1w, *fsv, w1a, w2a, *ln2, ln2w)
        return out.view(B, L, H)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        (xs, wqkv, qkv, W1, alpha1, W2, alpha2, w1m, w2m, relt, ctxv, lse, v1, mean1, rstd1, ln1w, y1a, pre1, a1a, w1a, w2a, v2,
         mean2, rstd2, ln2w) = ctx.saved_tensors
        mt, lists = ctx.meta, ctx.lists
        B, L, H = mt["shape"]
        T, h, b, act, p, seeds, bucket = B * L, mt["heads"], mt["b"], mt["act"], mt["p"], mt["seeds"], mt["bucket"]
        d = H // h
        C_ = b * b + 1
        f32 = dict(dtype=torch.float32, device=xs.device)
        perm, offs = lists.perm, lists.offsets
        g = dout.reshape(T, H).contiguous().float()
        # LayerNorm(y1 + dropout(ffn)), the behaviour FFN, LayerNorm(x + dropout(context))
        dy1, df2, dln2w, dln2b = post_ln_bwd(g, (v2, mean2, rstd2), ln2w, p, seeds[2])
        dw1a, dw2a = torch.zeros_like(w1a), torch.zeros_like(w2a)
        dy1s = grouped_ffn_bwd(df2, (y1a, pre1, a1a), perm, dict(groups=b, group_offsets=offs[1:]), w1a, w2a, act, dw1a, dw2a)
        dy1.index_add_(0, perm, dy1s)                                             # (perm is a permutation: one addend per row)
        dv1, dctx, dln1w, dln1b = post_ln_bwd(dy1, (v1, mean1, rstd1), ln1w, p, seeds[1])
        n = ops.mbs_n_partial(B, h, d, b)
        dqkv = torch.zeros(T, 3 * H, **f32)
        p1, p2 = torch.zeros(n, C_, h, d, d, **f32), torch.zeros(n, C_, h, d, d, **f32)
        pr = torch.zeros(n, C_, 2 * L - 1, h, **f32) if relt is not None else None
        ops.mbs_attn_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], lists.types, w1m, w2m, relt, bucket, B, L, h, d, b, mt["scale"],
                         p, seeds[0], ctxv, dctx, lse, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], p1, p2, pr)
        dw1m, dw2m = colsum(p1.view(n, -1)).view(C_, h, d, d), colsum(p2.view(n, -1)).view(C_, h, d, d)
        dW1, dal1, dW2, dal2 = torch.empty_like(W1), torch.empty_like(alpha1), torch.empty_like(W2), torch.empty_like(alpha2)
        ops.mbs_mix_bwd(W1.contiguous(), alpha1.contiguous(), dw1m, dW1, dal1)
        ops.mbs_mix_bwd(W2.contiguous(), alpha2.contiguous(), dw2m, dW2, dal2)
        drel = ()
        if relt is not None:
            dr = torch.empty_like(relt)
            ops.mbs_bias_fold(colsum(pr.view(n, -1)).view(C_, 2 * L - 1, h), bucket, dr)
            drel = tuple(dr[c] for c in range(C_))
        del p1, p2, pr
        dqkv_s = dqkv.index_select(0, perm)
        dwqkv = torch.zeros_like(wqkv)
        ops.linear_wgrad(xs, H, dqkv_s, 3 * H, dwqkv, 3 * H, T, H, 3 * H, groups=b + 1, group_offsets=offs, strideC=3 * H * H)
        dxs = torch.empty(T, H, **f32)
        ops.linear_fwd(dqkv_s, 3 * H, wqkv, 3 * H, dxs, H, T, H, 3 * H, groups=b + 1, group_offsets=offs, strideB=3 * H * H)
        dx = dv1
        dx.index_add_(0, perm, dxs)
        shp = (b + 1, H, h, d)
        return (dx.view(B, L, H), None, None, dW1, dal1, dW2, dal2, dwqkv[:, :, :H].reshape(shp), dwqkv[:, :, H:2 * H].reshape(shp),
                dwqkv[:, :, 2 * H:].reshape(shp), dln1w, dln1b, dln2w, dln2b, *split_aug_grads(dw1a, dw2a), *drel)


class MBSTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, n_behaviors, dim_feedforward=2048, dropout=0.1, activation="relu", layer_norm_eps=1e-12,
                 num_buckets=32, max_distance=40, behavior_position_bias=True):
        super().__init__()
        self.multi_head_attention = MBSMultiHeadAttention(d_model, nhead, dropout, layer_norm_eps, n_behaviors,
                                                          behavior_position_bias, num_buckets, max_distance)
        self.feed_forward = MBSFeedForward(d_model, dim_feedforward, dropout, activation, layer_norm_eps, n_behaviors)
        self.dropout_p, self.eps = float(dropout), float(layer_norm_eps)
        self.num_buckets, self.max_distance = num_buckets, max_distance

    def forward(self, hidden_states, attention_mask=None, type_seq=None, bucket=None):
        """``type_seq``: the _TypeLists of the batch; ``bucket``: int32 [2 L - 1] on the device (position bias on)."""
        a, f = self.multi_head_attention, self.feed_forward
        meta = dict(heads=a.num_attention_heads, b=a.n_behaviors, act=f.FFN[0].act_code, dropout=self.dropout_p, eps=self.eps,
                    training=self.training, bucket=bucket, zero_bias=f._zero_bias)
        params = [a.W1, a.alpha1, a.W2, a.alpha2, a.query, a.key, a.value, a.LayerNorm.weight, a.LayerNorm.bias, f.LayerNorm.weight,
                  f.LayerNorm.bias]
        for e in f.FFN:
            params += [e.dense_1.weight, e.dense_1.bias, e.dense_2.weight, e.dense_2.bias]
        if a.behavior_position_bias:
            params += [m.relative_attention_bias.weight for m in a.relative_position_bias]
        return _MBSLayerFn.apply(hidden_states, type_seq, meta, *params)


class CGCDotProductPredictionHead(nn.Module):
    """Parameter holder with the reference's names: shared and behaviour-specific experts, the gates and the shared table."""

    def __init__(self, d_model, n_items, token_embeddings, layer_norm_eps, n_behaviors, n_shared_experts, n_specific_experts):
        super().__init__()
        self.n_behaviors, self.n_shared_experts, self.n_specific_experts = n_behaviors, n_shared_experts, n_specific_experts
        self.vocab_size = n_items + 1
        self.softmax = nn.Softmax(dim=-1)
        self.shared_experts = nn.ModuleList([nn.Sequential(nn.Linear(d_model, d_model)) for _ in range(n_shared_experts)])
        self.specific_experts = nn.ModuleList([nn.Sequential(nn.Linear(d_model, d_model))
                                               for _ in range(n_behaviors * n_specific_experts)])
        self.w_gates = nn.Parameter(torch.randn(n_behaviors, d_model, n_shared_experts + n_specific_experts), requires_grad=True)
        self.token_embeddings = token_embeddings
        self.ln = nn.LayerNorm(d_model, eps=layer_norm_eps)


class _CGCHeadFn(torch.autograd.Function):
    """y = x[rows] + ln(sum_e gates_e expert_e(x[rows])) for the rows of x's [B L, H] view, types [M] int32: [M, H] in the order of
    ``rows``; dx is zero elsewhere.  params: w_gates, ln.weight, ln.bias, then (weight, bias) of the shared experts, then of the
    specific ones."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, rows, types, meta, w_gates, lnw, lnb, *experts):
        H = x.shape[-1]
        b, ns, nsp, eps = meta["b"], meta["ns"], meta["nsp"], meta["eps"]
        E = ns + nsp
        E4 = (E + 3) // 4 * 4
        f32 = dict(dtype=torch.float32, device=x.device)
        M = rows.numel()
        # rows sorted by type (padded to whole 64-row blocks of gamer_expert_lists; the padding is in no group)
        Mp = (M + 63) // 64 * 64
        tp = torch.full((Mp,), b + 1, dtype=torch.int32, device=x.device)
        tp[:M] = types
        lists = _TypeLists(tp.view(Mp // 64, 64), b)
        perm = lists.perm[:M]                                       # (the M real rows come first: the rest is behind the last group)
        offs = lists.offsets
        ts = types.index_select(0, perm).contiguous()
        xg = x.reshape(-1, H).index_select(0, rows.index_select(0, perm))
        xa = _with_ones(xg)
        wsh = _aug_weights(experts[0:2 * ns:2], experts[1:2 * ns:2]).view(ns * H, H + 4)
        wsp = _aug_weights(experts[2 * ns::2], experts[2 * ns + 1::2]).view(b, nsp * H, H + 4)
        outs = torch.zeros(M, E * H, **f32)
        grp = dict(groups=b, group_offsets=offs[1:])
        ops.linear_fwd(xa, H + 4, wsh, H + 4, outs, E * H, M, ns * H, H + 4)
        ops.linear_fwd(xa, H + 4, wsp, H + 4, outs[:, ns * H:], E * H, M, nsp * H, H + 4, strideB=nsp * H * (H + 4), **grp)
        wg = torch.zeros(b, H, E4, **f32)
        wg[:, :, :E] = w_gates
        logits = torch.zeros(M, E4, **f32)
        ops.gemm(xa, H + 4, 1, wg, 1, E4, logits, E4, M, E4, H, strideB=H * E4, **grp)
        gates, mix = torch.empty(M, E, **f32), torch.empty(M, H, **f32)
        ops.mbs_gate_mix_fwd(logits, outs.view(M, E, H), ts, gates, mix)
        ln = torch.empty(M, H, **f32)
        mean, rstd = torch.empty(M, **f32), torch.empty(M, **f32)
        ops.layernorm_fwd(mix, None, lnw, lnb, eps, None, ln, mean, rstd)
        ys = xg + ln
        y = torch.empty(M, H, **f32)
        y.index_copy_(0, perm, ys)
        ctx.meta = dict(meta, x_shape=x.shape, E4=E4)
        ctx.save_for_backward(rows, perm, offs, xa, wsh, wsp, wg, outs, gates, mix, lnw, mean, rstd)
        return y

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dy):
        rows, perm, offs, xa, wsh, wsp, wg, outs, gates, mix, lnw, mean, rstd = ctx.saved_tensors
        mt = ctx.meta
        b, ns, nsp, E4 = mt["b"], mt["ns"], mt["nsp"], mt["E4"]
        E = ns + nsp
        M, H = mix.shape
        f32 = dict(dtype=torch.float32, device=mix.device)
        grp = dict(groups=b, group_offsets=offs[1:])
        g = dy.contiguous().float().index_select(0, perm)
        dmix, dlnw, dlnb = layernorm_bwd(mix, lnw, mean, rstd, g)
        douts, dlogits = torch.empty(M, E * H, **f32), torch.zeros(M, E4, **f32)
        ops.mbs_gate_mix_bwd(gates, outs.view(M, E, H), dmix, douts.view(M, E, H), dlogits)
        dwsh, dwsp, dwg = torch.zeros_like(wsh), torch.zeros_like(wsp), torch.zeros_like(wg)
        dsh, dsp = douts[:, :ns * H], douts[:, ns * H:]
        ops.linear_wgrad(dsh, E * H, xa, H + 4, dwsh, H + 4, M, ns * H, H + 4)
        ops.linear_wgrad(dsp, E * H, xa, H + 4, dwsp, H + 4, M, nsp * H, H + 4, strideC=nsp * H * (H + 4), **grp)
        ops.linear_wgrad(xa, H + 4, dlogits, E4, dwg, E4, M, H, E4, strideC=H * E4, **grp)
        dxg = torch.zeros(M, H, **f32)
        ops.gemm(dsh, E * H, 1, wsh, 1, H + 4, dxg, H, M, H, ns * H)
        ops.gemm(dsp, E * H, 1, wsp, 1, H + 4, dxg, H, M, H, nsp * H, accumulate=True, strideB=nsp * H * (H + 4), **grp)
        ops.linear_fwd(dlogits, E4, wg, E4, dxg, H, M, H, E4, accumulate=True, strideB=H * E4, **grp)
        dxg += g
        dx = torch.zeros(mt["x_shape"], **f32)
        dx.view(-1, H)[rows.index_select(0, perm)] = dxg             # (rows are distinct positions)
        dsh_w = dwsh.view(ns, H, H + 4)
        dexp = []
        for i in range(ns):
            dexp += [dsh_w[i, :, :H], dsh_w[i, :, H]]
        dsp_w = dwsp.view(b * nsp, H, H + 4)
        for i in range(b * nsp):
            dexp += [dsp_w[i, :, :H], dsp_w[i, :, H]]
        return (dx, None, None, None, dwg[:, :, :E], dlnw, dlnb, *dexp)


class MBSTR(ClozeMixin, nn.Module):
    def __init__(self, config: MBSTRConfig, n_items: int, max_his_len: int, n_behaviors: int, **kwargs):
        super().__init__()
        if config.loss_type != "CE":
            raise NotImplementedError("MBSTR: only loss_type 'CE' is supported (as the reference: 'Only support CE loss now')")
        if not config.behavior_moe or n_behaviors < 2:
            raise NotImplementedError("MBSTR: behavior_moe=False and n_behaviors < 2 build FeedForward(residual=False), which cannot "
                                      f"run in the reference (AttributeError: {_REF_FFN_ERROR})")
        if not config.behavior_attention:
            raise NotImplementedError("MBSTR on the HIP path: behavior_attention=False (plain attention with the behaviour position "
                                      "bias) is not built yet")
        if config.hidden_size % config.n_heads:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.n_heads))
        ops.mbs_check_limits(1, config.hidden_size, config.hidden_size // config.n_heads, n_behaviors)
        if config.behavior_head and config.n_shared_experts + config.n_specific_experts > ops.MBS_MAX_E:
            raise NotImplementedError(f"MBSTR on the HIP path: n_shared_experts + n_specific_experts <= {ops.MBS_MAX_E}")
        self.config = config
        self.n_items = n_items
        self.n_layers, self.n_heads = config.n_layers, config.n_heads
        self.hidden_size, self.inner_size = config.hidden_size, config.inner_size
        self.dropout_prob, self.hidden_act = config.dropout_prob, config.hidden_act
        self.layer_norm_eps, self.initializer_range = config.layer_norm_eps, config.initializer_range
        self.mask_ratio = config.mask_ratio
        self.num_buckets, self.max_distance = config.num_buckets, config.max_distance
        self.behavior_head, self.behavior_attention = config.behavior_head, config.behavior_attention
        self.behavior_moe, self.behavior_position_bias = config.behavior_moe, config.behavior_position_bias
        self.n_shared_experts, self.n_specific_experts = config.n_shared_experts, config.n_specific_experts
        self.max_seq_length = max_his_len
        self.n_behaviors = n_behaviors
        self.mask_token = n_items + 1
        self.loss_type = config.loss_type
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        H = self.hidden_size
        self.item_embedding = nn.Embedding(n_items + 2, H, padding_idx=0)          # 0: <PAD>, n_items + 1: <MASK>
        self.dropout = nn.Dropout(self.dropout_prob)
        layer = MBSTransformerEncoderLayer(d_model=H, nhead=self.n_heads, n_behaviors=n_behaviors, dim_feedforward=self.inner_size,
                                           dropout=self.dropout_prob, activation=self.hidden_act, layer_norm_eps=self.layer_norm_eps,
                                           num_buckets=self.num_buckets, max_distance=self.max_distance,
                                           behavior_position_bias=self.behavior_position_bias)
        self.trm_encoder = modules.TransformerEncoder(layer, self.n_layers)
        if self.behavior_head:
            self.head = CGCDotProductPredictionHead(d_model=H, n_items=n_items, token_embeddings=self.item_embedding,
                                                    layer_norm_eps=self.layer_norm_eps, n_behaviors=n_behaviors,
                                                    n_shared_experts=self.n_shared_experts,
                                                    n_specific_experts=self.n_specific_experts)
        else:
            self.head = DotProductPredictionHead(d_model=H, n_items=n_items, token_embeddings=self.item_embedding)
        self.apply(self._init_weights)
        self._buckets = {}

    def _init_weights(self, module: nn.Module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()
        if isinstance(module, MBSMultiHeadAttention):
            module.query.data.normal_(mean=0.0, std=self.initializer_range)
            module.key.data.normal_(mean=0.0, std=self.initializer_range)
            module.value.data.normal_(mean=0.0, std=self.initializer_range)

    # ---- masking ---------------------------------------------------------------------------------------------------------------
    def _cloze(self, item_seq: torch.Tensor, seed=None):
        self._require_device(item_seq)
        seed = _next_seed() if seed is None else int(seed)
        ones = torch.ones(item_seq.shape[0], dtype=torch.int64, device=item_seq.device)     # (read by the fine-tuning rows only)
        return ops.cloze_mask(item_seq.long().contiguous(), ones, self.mask_ratio, 0.0, self.mask_token, self.max_seq_length, seed)

    def reconstruct_train_data(self, item_seq: torch.Tensor, seed=None):
        """(masked_item_seq, labels) of the cloze task; ``seed`` fixes the masks (default: the module's running counter)."""
        masked, labels = self._cloze(item_seq, seed)[:2]
        return masked, labels

    # ---- encoder ---------------------------------------------------------------------------------------------------------------
    def _bucket(self, L: int, device) -> torch.Tensor:
        key = (L, str(device))
        if key not in self._buckets:
            t = relative_position_buckets(L, self.num_buckets, self.max_distance)
            if int(t.min()) < 0 or int(t.max()) >= self.num_buckets:
                raise IndexError(f"relative position buckets outside [0, {self.num_buckets}) for num_buckets={self.num_buckets}, "
                                 f"max_distance={self.max_distance}")
            self._buckets[key] = t.to(device)
        return self._buckets[key]

    def _types(self, item_seq, type_seq, extra=None):
        """int32 [B, L] types after ONE host read that checks their range (and fetches ``extra``, a device scalar, with it)"""
        self._require_device(item_seq)
        B, L = item_seq.shape
        if L > self.max_seq_length:
            raise ValueError(f"sequence length {L} > max_his_len {self.max_seq_length}")
        ops.mbs_check_limits(L, self.hidden_size, self.hidden_size // self.n_heads, self.n_behaviors)
        t = type_seq.to(item_seq.device)
        if t.shape != item_seq.shape:
            raise RuntimeError(f"behaviors must be [{B}, {L}], got {tuple(t.shape)}")
        bad = ((t < 0) | (t > self.n_behaviors)).any().long().reshape(1)
        vals = torch.cat([bad, extra.long().reshape(1)] if extra is not None else [bad]).tolist()
        if vals[0]:
            raise RuntimeError(f"Class values must be smaller than num_classes. (behaviors outside [0, {self.n_behaviors}])")
        return t.to(torch.int32).contiguous(), (vals[1] if extra is not None else None)

    def _encode(self, item_seq: torch.Tensor, types: torch.Tensor, shared=None) -> torch.Tensor:
        p = self.dropout_prob if self.training else 0.0
        x = EmbedDropoutFn.apply(item_seq.long().contiguous(), self.item_embedding.weight, p, _next_seed(), shared)
        lists = _TypeLists(types, self.n_behaviors)
        bucket = self._bucket(item_seq.shape[1], item_seq.device) if self.behavior_position_bias else None
        return self.trm_encoder(x, None, type_seq=lists, bucket=bucket)

    def _head_input(self, item_seq, types, rows, shared=None) -> torch.Tensor:
        """the head's hidden state on the rows (flat positions) given: [M, H]"""
        x = self._encode(item_seq, types, shared)
        if not self.behavior_head:
            lin = self.head.out[0]
            return GatherLinearFn.apply(x, rows, lin.weight, lin.bias, ops.ACTIVATIONS["relu"])
        hd = self.head
        meta = dict(b=self.n_behaviors, ns=self.n_shared_experts, nsp=self.n_specific_experts, eps=self.layer_norm_eps)
        experts = []
        for e in list(hd.shared_experts) + list(hd.specific_experts):
            experts += [e[0].weight, e[0].bias]
        rt = types.flatten().index_select(0, rows).contiguous()
        return _CGCHeadFn.apply(x, rows, rt, meta, hd.w_gates, hd.ln.weight, hd.ln.bias, *experts)

    # ---- the cloze task (ClozeMixin: _loss, calculate_loss, full_sort_predict, full_sort_topk) -----------------------------------
    def forward(self, item_seq: torch.Tensor, type_seq: torch.Tensor, labels: torch.Tensor, candidates=None):
        """(valid_logits [M, n_items + 1], valid_labels [M]) of the positions with labels != 0, the scores materialised (tests and
        small catalogues; no gradient flows through the scores: training goes through calculate_loss)."""
        self._refuse_candidates(candidates)
        return self._scores_at_labels(item_seq, labels, self._types(item_seq, type_seq)[:1])

    def sample_sort_predict(self, interaction: dict):
        raise NotImplementedError("MBSTR.sample_sort_predict: candidates (the negative-sampling tasks) are not supported on the HIP path")

    def _extra(self, item_seq, interaction):
        return self._types(item_seq, interaction["behaviors"])[:1]

    def _draw_cloze(self, interaction: dict):
        masked, _, rows, targets, count = self._cloze(interaction["inputs"])
        types, M = self._types(masked, interaction["behaviors"], count)          # (the step's host read)
        return masked, (types,), rows[:M], targets[:M]

    @staticmethod
    def _in_graph(name: str) -> bool:
        return not (".FFN." in name and ".LayerNorm." in name)
