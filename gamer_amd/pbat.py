"""PBAT, the personalized behaviour-aware baseline of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface, parameter and state-dict names as the reference (ref:SeqRec/models/discriminative/PBAT/model.py,
ref:SeqRec/modules/layers/pbat.py): ten embeddings - ``{item, type, user, type_relation}_embedding_{m, c}`` are ``SimpleEmbedding``s
(``.embedding``, ``.LayerNorm``; ELU(dropout(LayerNorm(E[ids])))), ``position_embedding_{m, c}`` plain tables -, ``Wub``, ``WPub``,
``trm_encoder.layer.{l}.multi_head_attention.{xm, xc, bm, bc}.{q, k, v}``, ``.{mean_dense, cov_dense, LayerNorm, Wq1, Wq2, Wk1,
Wk2}``, ``trm_encoder.layer.{l}.feed_forward.FFN.{i}.*``, ``head.out.0`` and ``head.token_embeddings_{m, c}``, the two item tables
again (two state-dict keys, one parameter each).  A reference ``best_model.pth`` loads here and one saved here loads there.

Every token is a Gaussian: a mean stream and a covariance stream (ELU + 1 keeps it positive).  What runs where:
  masking       gamer_cloze_mask at ft_ratio = 0 (rand < mask_ratio and item != 0)
  embeddings    gamer_embedding_fwd, gamer_layernorm_fwd, dropout, gamer_bias_act_fwd (elu); the item tables' gradients take the
                head's and the input gather's contributions in one buffer each
  pre-encoder   the user x behaviour SAGP, the (b + 1)^2 pairwise distances and the relation scaling - all of size B (b + 1)^2 H -
                are device torch ops under autograd, and so is the final SAGP with ``WPub`` on the M masked rows
  projections   one [q | k | v] fp32 GEMM per stream on [x | type embedding]
  attention     gamer_pbat_attn_fwd / _bwd (csrc/pbat.hip): a score depends on the key through its type alone, so the reference's
                [B, h, L, L, d] tensors are never formed and only [B, h, L, b + 1] scores are kept for backward
  FFN           dense_2[t](act(dense_1[t](x))) as grouped GEMMs over the rows sorted by type, once per stream, zero for type 0
  head          distance(r, v) = a_r + c_v + x'_r . E'_v: gamer_wass_rows_*, gamer_wass_table_*, then the biased catalogue kernels
                at width 2 H (gamer_catalog_ce_bias_fwd / _bwd, gamer_catalog_topk_bias); the [M, V] distances are never written

Reference behaviour kept on purpose ("PBAT", lists the seven facts):
  * both fused Gaussians of a pair (i, j) are built from token i's projections; the relation entry is R[t_i, t_j];
  * the head's "logits" are the distances themselves (no minus sign): the cross entropy and ``argsort(-scores)`` see them as is;
  * the head applies one ``out`` (Linear + ELU) to both streams, the covariance stream gets no + 1 and may be negative;
  * the experts' LayerNorms and dropouts are never used (``FeedForward(residual=True)``): their parameters get no gradient;
  * ``behavior_emb_c`` passes ELU twice; relation index 0 is (0, ELU(1) + 1).
Not the reference's: B = 1 runs (the reference's ``.squeeze()`` drops the batch axis and raises IndexError); masks (cloze and
dropout) come from the project's counter-based hash; ``candidates`` / ``sample_sort_predict`` are refused; the kernels' limits
(L <= 128, head size <= 64, hidden size <= 128, both multiples of 4, at most 8 behaviours) are refused with NotImplementedError.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import nn
from torch.nn import functional as F

from . import modules, ops
from .layer_blocks import (_N_PARTIAL, _TypeLists, _aug_weights, _dropout_bwd, colsum, dropout_fwd, grouped_ffn_bwd, grouped_ffn_fwd,
                           layernorm_bwd, linear_act_bwd, linear_act_fwd, post_ln_bwd, post_ln_fwd, split_aug_grads)
from .rec_common import ClozeMixin, DropUnknownConfig, _GatherRowsFn, _next_seed, _SharedGrad

_EPS = 1e-24
_ELU = ops.ACTIVATIONS["elu"]


@dataclasses.dataclass(init=False)
class PBATConfig(DropUnknownConfig):
    """The fields and defaults of the reference's PBATConfig (ref:SeqRec/models/discriminative/PBAT/config.py); unknown keys are
    dropped, as the reference's pydantic model does."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 64
    inner_size: int = 256
    dropout_prob: float = 0.2
    hidden_act: str = "elu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    mask_ratio: float = 0.2
    loss_type: str = "CE"


def sagp(mean1, mean2, cov1, cov2):
    """Self-adaptive Gaussian production of two Gaussians (ref:SeqRec/modules/layers/pbat.py SAGP)."""
    cov1, cov2 = torch.clamp(cov1, min=_EPS), torch.clamp(cov2, min=_EPS)
    return (cov1 * mean2 + cov2 * mean1) / (cov1 + cov2), 2 * (cov1 * cov2) / (cov1 + cov2)


def pairwise_wasserstein(mean, cov):
    """[B, n, n] distances between the n Gaussians of every row, as sums of squared differences (the reference expands the
    squares and cancels)."""
    s = torch.sqrt(torch.clamp(cov, min=_EPS))
    dm = mean[:, :, None, :] - mean[:, None, :, :]
    cv = cov[:, :, None, :] + cov[:, None, :, :] - 2 * s[:, :, None, :] * s[:, None, :, :]
    return (dm * dm + cv).sum(-1)


# ---- parameter holders with the reference's names ------------------------------------------------------------------------------
class SimpleEmbedding(nn.Module):
    def __init__(self, vocab_size: int, embed_dim: int, dropout: float, layer_norm_eps: float = 1e-12, padding_idx: int = 0):
        super().__init__()
        self.embedding = nn.Embedding(vocab_size, embed_dim, padding_idx=padding_idx)
        self.dropout = nn.Dropout(dropout)
        self.LayerNorm = nn.LayerNorm(embed_dim, eps=layer_norm_eps)
        self.activation = nn.ELU()

    def forward(self, ids: torch.Tensor, shared=None) -> torch.Tensor:
        p = float(self.dropout.p) if self.training else 0.0
        return _SimpleEmbedFn.apply(ids.long().contiguous(), self.embedding.weight, self.LayerNorm.weight, self.LayerNorm.bias,
                                    float(self.LayerNorm.eps), p, _next_seed(), shared)


class _SimpleEmbedFn(torch.autograd.Function):
    """ELU(dropout(LayerNorm(E[ids]))) for ids of any shape: [*ids.shape, H]; E's gradient (padding row 0 skipped) goes into the
    shared buffer when there is one."""

    @staticmethod
    def forward(ctx, ids, E, w, b, eps, p, seed, shared=None):
        H = E.shape[1]
        T = ids.numel()
        f32 = dict(dtype=torch.float32, device=E.device)
        x = torch.empty(T, H, **f32)
        ops.embedding_fwd(ids, E, x)
        y, mean, rstd = torch.empty(T, H, **f32), torch.empty(T, **f32), torch.empty(T, **f32)
        ops.layernorm_fwd(x, None, w, b, eps, None, y, mean, rstd)
        y = dropout_fwd(y, p, seed)
        out = torch.empty(T, H, **f32)
        ops.bias_act_fwd(y, torch.zeros(H, **f32), _ELU, out)
        ctx.meta = (p, seed, E.shape, tuple(ids.shape))
        ctx.shared = shared
        ctx.save_for_backward(ids, x, w, mean, rstd, y)
        return out.view(*ids.shape, H)

    @staticmethod
    def backward(ctx, dout):
        ids, x, w, mean, rstd, y = ctx.saved_tensors
        p, seed, e_shape, _ = ctx.meta
        T, H = x.shape
        f32 = dict(dtype=torch.float32, device=x.device)
        g = torch.empty(T, H, **f32)
        ops.bias_act_bwd(y, dout.reshape(T, H).contiguous().float(), _ELU, g, torch.empty(_N_PARTIAL, H, **f32))
        dx, dw, db = layernorm_bwd(x, w, mean, rstd, _dropout_bwd(g, H, p, seed))
        dE = _SharedGrad.take(ctx.shared, e_shape, x.device)
        ops.embedding_bwd_large(ids.reshape(-1), dx, 0, dE)
        return None, dE, dw, db, None, None, None, None


class FBAMultiHeadAttention(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, dropout: float, layer_norm_eps: float, n_behaviors: int):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)" % (embed_dim, num_heads))
        self.num_attention_heads = num_heads
        self.attention_head_size = embed_dim // num_heads
        self.all_head_size = embed_dim
        self.n_behaviors = n_behaviors

        def qkv():
            return nn.ModuleDict({n: nn.Linear(embed_dim, embed_dim) for n in ("q", "k", "v")})
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        self.xm, self.xc, self.bm, self.bc = qkv(), qkv(), qkv(), qkv()
        self.attn_dropout = nn.Dropout(dropout)
        self.activation = nn.ELU()
        self.mean_dense = nn.Linear(embed_dim, embed_dim)
        self.cov_dense = nn.Linear(embed_dim, embed_dim)
        self.LayerNorm = nn.LayerNorm(embed_dim, eps=layer_norm_eps)
        self.out_dropout = nn.Dropout(dropout)
        d = self.attention_head_size
        self.Wq1, self.Wq2, self.Wk1, self.Wk2 = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)


class BehaviorSpecificFeedForward(nn.Module):
    def __init__(self, d_model, dim_feedforward, dropout, activation, layer_norm_eps, n_behaviors):
        super().__init__()
        self.n_behaviors = n_behaviors
        self.FFN = nn.ModuleList([modules.FeedForward(d_model, dim_feedforward, dropout, activation, layer_norm_eps)
                                  for _ in range(n_behaviors)])
        # (outside the state dict: the zero biases of the activation kernel; the real biases ride in the grouped GEMMs)
        self.register_buffer("_zero_ff", torch.zeros(dim_feedforward), persistent=False)
        self.register_buffer("_zero_h", torch.zeros(d_model), persistent=False)


def _split_proj_grads(dW, db, H):
    """the twelve gradients of _proj_weights' inputs, in the order x.{q, k, v}.{weight, bias}, b.{q, k, v}.{weight, bias}"""
    out_x, out_b = [], []
    for i in range(3):
        out_x += [dW[i * H:(i + 1) * H, :H], db[i * H:(i + 1) * H]]
        out_b += [dW[i * H:(i + 1) * H, H:], db[i * H:(i + 1) * H]]
    return out_x + out_b


class _PBATLayerFn(torch.autograd.Function):
    """One PBATLayer on both streams.  params: xm.{q, k, v}.{weight, bias}, bm.*, xc.*, bc.* (24), mean_dense, cov_dense
    (weight, bias), LayerNorm (weight, bias), Wq1, Wq2, Wk1, Wk2 (weight, bias), then (dense_1.weight, dense_1.bias,
    dense_2.weight, dense_2.bias) of each behaviour's expert."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, xm, xc, tm, tc, rel_m, rel_c, pos_m, pos_c, lists, keep, meta, *params):
        B, L, H = xm.shape
        T = B * L
        h, b, act, eps = meta["heads"], meta["b"], meta["act"], meta["eps"]
        p = meta["dropout"] if meta["training"] else 0.0
        d = H // h
        f32 = dict(dtype=torch.float32, device=xm.device)
        pxm, pbm, pxc, pbc = params[0:6], params[6:12], params[12:18], params[18:24]
        mdw, mdb, cdw, cdb, lnw, lnb = params[24:30]
        attw = tuple(t.contiguous() for t in params[30:38])                  # Wq1, bq1, Wq2, bq2, Wk1, bk1, Wk2, bk2
        ffn = params[38:]
        seeds = [modules._SeedCounter.next() for _ in range(3)]

        def wcat(px, pb):
            W = torch.cat([torch.cat([px[2 * i], pb[2 * i]], 1) for i in range(3)], 0).contiguous()
            return W, torch.cat([px[2 * i + 1] + pb[2 * i + 1] for i in range(3)], 0).contiguous()
        Wm, bm_ = wcat(pxm, pbm)
        Wc, bc_ = wcat(pxc, pbc)
        Am = torch.cat([xm.reshape(T, H), tm.reshape(T, H)], 1).contiguous().float()
        Ac = torch.cat([xc.reshape(T, H), tc.reshape(T, H)], 1).contiguous().float()
        _, pm = linear_act_fwd(Am, Wm, bm_, 0)
        pre_c, pc = linear_act_fwd(Ac, Wc, bc_, _ELU)
        pc += 1.0
        proj = (pm[:, :H], pc[:, :H], pm[:, H:2 * H], pc[:, H:2 * H], pm[:, 2 * H:], pc[:, 2 * H:])
        rel_m, rel_c = rel_m.reshape(B, -1, H).contiguous().float(), rel_c.reshape(B, -1, H).contiguous().float()
        pos_m, pos_c = pos_m.contiguous().float(), pos_c.contiguous().float()
        o = torch.empty(2, T, H, **f32)
        S, lse = torch.empty(B, h, L, b + 1, **f32), torch.empty(B, h, L, **f32)
        scale = math.sqrt(1.0 / float(d))
        ops.pbat_attn_fwd(proj, rel_m, rel_c, pos_m, pos_c, attw, lists.types, keep, B, L, h, d, b, scale, p, seeds[0], o[0], o[1], S, lse)

        def dense_ln(ov, x, W, bias, seed):
            return post_ln_fwd(x, linear_act_fwd(ov, W, bias, 0)[1], lnw, lnb, eps, p, seed)
        ym, ln_m = dense_ln(o[0], Am[:, :H].contiguous(), mdw, mdb, seeds[1])
        yc, ln_c = dense_ln(o[1], Ac[:, :H].contiguous(), cdw, cdb, seeds[2])
        # the behaviour FFN, once per stream: groups 1 .. b of the sorted rows; padding rows (group 0) stay zero
        perm, grp = lists.perm, dict(groups=b, group_offsets=lists.offsets[1:])
        w1a, w2a = _aug_weights(ffn[0::4], ffn[1::4]), _aug_weights(ffn[2::4], ffn[3::4])
        fm, ffn_m = grouped_ffn_fwd(ym, perm, grp, w1a, w2a, act, meta["zero_ff"])
        fc, ffn_c = grouped_ffn_fwd(yc, perm, grp, w1a, w2a, act, meta["zero_ff"])
        out_c = torch.empty(T, H, **f32)
        ops.bias_act_fwd(fc, meta["zero_h"], _ELU, out_c)
        out_c += 1.0
        ctx.meta = dict(meta, p=p, seeds=seeds, scale=scale, shape=(B, L, H))
        ctx.lists, ctx.attw = lists, attw
        ctx.save_for_backward(Am, Ac, Wm, Wc, pm, pre_c, pc, rel_m, rel_c, pos_m, pos_c, keep, o, S, lse, mdw, cdw, lnw, *ln_m, *ln_c,
                              w1a, w2a, *ffn_m, *ffn_c, fc)
        return fm.view(B, L, H), out_c.view(B, L, H)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dfm, dout_c):
        (Am, Ac, Wm, Wc, pm, pre_c, pc, rel_m, rel_c, pos_m, pos_c, keep, o, S, lse, mdw, cdw, lnw, vm, mean_m, rstd_m, vc, mean_c,
         rstd_c, w1a, w2a, yam, pre1m, a1am, yac, pre1c, a1ac, fc) = ctx.saved_tensors
        mt, lists, attw = ctx.meta, ctx.lists, ctx.attw
        B, L, H = mt["shape"]
        T, h, b, act, p, seeds = B * L, mt["heads"], mt["b"], mt["act"], mt["p"], mt["seeds"]
        d = H // h
        f32 = dict(dtype=torch.float32, device=Am.device)
        perm, grp = lists.perm, dict(groups=b, group_offsets=lists.offsets[1:])
        dw1a, dw2a = torch.zeros_like(w1a), torch.zeros_like(w2a)              # both streams' FFN gradients add up here

        def ffn_bwd(df2, saved):
            dy = torch.empty(T, H, **f32)
            dy.index_copy_(0, perm, grouped_ffn_bwd(df2, saved, perm, grp, w1a, w2a, act, dw1a, dw2a))
            return dy
        dfc = torch.empty(T, H, **f32)
        ops.bias_act_bwd(fc, dout_c.reshape(T, H).contiguous().float(), _ELU, dfc, torch.empty(_N_PARTIAL, H, **f32))
        dym = ffn_bwd(dfm.reshape(T, H).contiguous().float(), (yam, pre1m, a1am))
        dyc = ffn_bwd(dfc, (yac, pre1c, a1ac))

        def dense_ln_bwd(dy, ln, ov, W, seed):
            dv, dd, dlw, dlb = post_ln_bwd(dy, ln, lnw, p, seed)
            do, dW, db = linear_act_bwd(dd, None, ov, W, 0)
            return dv, do, dW, db, dlw, dlb
        dxm_res, do_m, dmdw, dmdb, dlw1, dlb1 = dense_ln_bwd(dym, (vm, mean_m, rstd_m), o[0], mdw, seeds[1])
        dxc_res, do_c, dcdw, dcdb, dlw2, dlb2 = dense_ln_bwd(dyc, (vc, mean_c, rstd_c), o[1], cdw, seeds[2])
        proj = (pm[:, :H], pc[:, :H], pm[:, H:2 * H], pc[:, H:2 * H], pm[:, 2 * H:], pc[:, 2 * H:])
        dpm, dpc = torch.empty(T, 3 * H, **f32), torch.empty(T, 3 * H, **f32)
        dproj = (dpm[:, :H], dpc[:, :H], dpm[:, H:2 * H], dpc[:, H:2 * H], dpm[:, 2 * H:], dpc[:, 2 * H:])
        drel_m, drel_c = torch.empty_like(rel_m), torch.empty_like(rel_c)
        n = ops.pbat_n_partial(B, h)
        wpart, ppart = torch.zeros(n, h, 4 * (d * d + d), **f32), torch.zeros(n, h, 4, L, d, **f32)
        do = torch.stack([do_m, do_c])
        ops.pbat_attn_bwd(proj, rel_m, rel_c, pos_m, pos_c, attw, lists.types, keep, B, L, h, d, b, mt["scale"], p, seeds[0], S, lse,
                          do[0], do[1], dproj, drel_m, drel_c, wpart, ppart)
        dw = colsum(wpart.view(n * h, -1)).view(4, d * d + d)
        datt = []
        for i in (0, 2, 1, 3):                                                # slab order Wq1, Wk1, Wq2, Wk2 -> Wq1, Wq2, Wk1, Wk2
            datt += [dw[i, :d * d].reshape(d, d), dw[i, d * d:]]
        dpos = colsum(ppart.view(n, -1)).view(h, 4, L, d)
        dpos_m, dpos_c = dpos[:, 0].permute(1, 0, 2).reshape(L, H), dpos[:, 1].permute(1, 0, 2).reshape(L, H)
        dAm, dWm, dbm = linear_act_bwd(dpm, None, Am, Wm, 0)
        dAc, dWc, dbc = linear_act_bwd(dpc, pre_c, Ac, Wc, _ELU)
        dxm, dxc = dAm[:, :H] + dxm_res, dAc[:, :H] + dxc_res
        gm, gc = _split_proj_grads(dWm, dbm, H), _split_proj_grads(dWc, dbc, H)
        NT = b + 1
        return (dxm.view(B, L, H), dxc.view(B, L, H), dAm[:, H:].reshape(B, L, H), dAc[:, H:].reshape(B, L, H),
                drel_m.view(B, NT, NT, H), drel_c.view(B, NT, NT, H), dpos_m, dpos_c, None, None, None,
                *gm, *gc, dmdw, dmdb, dcdw, dcdb, dlw1 + dlw2, dlb1 + dlb2, *datt, *split_aug_grads(dw1a, dw2a))


class PBATLayer(nn.Module):
    def __init__(self, d_model, nhead, n_behaviors, dim_feedforward=2048, dropout=0.1, activation="relu", layer_norm_eps=1e-5):
        super().__init__()
        self.multi_head_attention = FBAMultiHeadAttention(d_model, nhead, dropout, layer_norm_eps, n_behaviors)
        self.feed_forward = BehaviorSpecificFeedForward(d_model, dim_feedforward, dropout, activation, layer_norm_eps, n_behaviors)
        self.dropout = nn.Dropout(p=dropout)
        self.activation_func = nn.ELU()
        self.dropout_p, self.eps = float(dropout), float(layer_norm_eps)

    def forward(self, hidden_states, attention_mask=None, type_seq=None, type_tensor=None, type_relation_tensor=None,
                position_tensor=None):
        """``hidden_states``: (mean, covariance) [B, L, H]; ``attention_mask``: int32 [B, L], != 0 where a key may be attended;
        ``type_seq``: the _TypeLists of the batch; relations [B, b + 1, b + 1, H] and positions [L, H] as (mean, covariance)."""
        a, f = self.multi_head_attention, self.feed_forward
        meta = dict(heads=a.num_attention_heads, b=a.n_behaviors, act=f.FFN[0].act_code, dropout=self.dropout_p, eps=self.eps,
                    training=self.training, zero_ff=f._zero_ff, zero_h=f._zero_h)
        params = []
        for dct in (a.xm, a.bm, a.xc, a.bc):
            for n in ("q", "k", "v"):
                params += [dct[n].weight, dct[n].bias]
        for lin in (a.mean_dense, a.cov_dense, a.LayerNorm, a.Wq1, a.Wq2, a.Wk1, a.Wk2):
            params += [lin.weight, lin.bias]
        for e in f.FFN:
            params += [e.dense_1.weight, e.dense_1.bias, e.dense_2.weight, e.dense_2.bias]
        return _PBATLayerFn.apply(hidden_states[0], hidden_states[1], type_tensor[0], type_tensor[1], type_relation_tensor[0],
                                  type_relation_tensor[1], position_tensor[0], position_tensor[1], type_seq, attention_mask, meta,
                                  *params)


class WassersteinPredictionHead(nn.Module):
    """Parameter holder with the reference's names: ``out.0`` (Linear + ELU, applied to both streams) and the two shared tables."""

    def __init__(self, d_model: int, n_items: int, token_embeddings_m: nn.Embedding, token_embeddings_c: nn.Embedding):
        super().__init__()
        self.token_embeddings_m = token_embeddings_m
        self.token_embeddings_c = token_embeddings_c
        self.vocab_size = n_items + 1
        self.out = nn.Sequential(nn.Linear(d_model, d_model), nn.ELU())
        self.activation = nn.ELU()


class _WassHeadFn(torch.autograd.Function):
    """(x' [M, 2 H], a [M]) of the head's rows: hm = ELU(out(om)), hc = ELU(out(oc)) as one GEMM on [om; oc], then
    gamer_wass_rows_fwd.  No gradient flows through a (it changes neither the cross entropy nor the ranking)."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, om, oc, W, bias):
        M, H = om.shape
        f32 = dict(dtype=torch.float32, device=om.device)
        x = torch.cat([om, oc], 0).contiguous().float()
        pre, hid = linear_act_fwd(x, W, bias, _ELU)
        xp, a = torch.empty(M, 2 * H, **f32), torch.empty(M, **f32)
        ops.wass_rows_fwd(hid[:M], hid[M:], xp, a)
        ctx.save_for_backward(x, W, pre, hid)
        ctx.mark_non_differentiable(a)
        return xp, a

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dxp, _da):
        x, W, pre, hid = ctx.saved_tensors
        M = x.shape[0] // 2
        dh = torch.empty_like(hid)
        ops.wass_rows_bwd(hid[:M], hid[M:], dxp.contiguous().float(), None, dh[:M], dh[M:])
        dx, dW, db = linear_act_bwd(dh, pre, x, W, _ELU)
        return dx[:M], dx[M:], dW, db


class _WassTableFn(torch.autograd.Function):
    """(E' [V, 2 H], c [V]) of the first V rows of the two item tables (gamer_wass_table_fwd).  With ``shared`` (one _SharedGrad per
    table) the tables' gradients are handed to the input gathers' backward, which add their rows and return them."""

    @staticmethod
    def forward(ctx, Em, Ec, V, shared=None):
        f32 = dict(dtype=torch.float32, device=Em.device)
        E2, c = torch.empty(V, 2 * Em.shape[1], **f32), torch.empty(V, **f32)
        ops.wass_table_fwd(Em, Ec, V, E2, c)
        ctx.save_for_backward(Em, Ec)
        ctx.V, ctx.shared = V, shared
        return E2, c

    @staticmethod
    def backward(ctx, dE2, dc):
        Em, Ec = ctx.saved_tensors
        dEm, dEc = torch.zeros_like(Em), torch.zeros_like(Ec)
        ops.wass_table_bwd(Em, Ec, ctx.V, dE2.contiguous().float(), None if dc is None else dc.contiguous().float(), dEm, dEc)
        if ctx.shared is not None:
            ctx.shared[0].dE, ctx.shared[1].dE = dEm, dEc
            return None, None, None, None
        return dEm, dEc, None, None


class PBAT(ClozeMixin, nn.Module):
    def __init__(self, config: PBATConfig, n_items: int, n_users: int, max_his_len: int, n_behaviors: int, **kwargs):
        super().__init__()
        if config.loss_type != "CE":
            raise NotImplementedError("PBAT: only loss_type 'CE' is supported (as the reference: 'Only support CE loss now')")
        if config.hidden_size % config.n_heads:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.n_heads))
        ops.pbat_check_limits(min(max_his_len, ops.PBAT_MAX_L) if max_his_len >= 1 else max_his_len, config.hidden_size,
                              config.hidden_size // config.n_heads, n_behaviors)
        self.config = config
        self.n_items = n_items
        self.n_layers, self.n_heads = config.n_layers, config.n_heads
        self.hidden_size, self.inner_size = config.hidden_size, config.inner_size
        self.dropout_prob, self.hidden_act = config.dropout_prob, config.hidden_act
        self.layer_norm_eps, self.initializer_range = config.layer_norm_eps, config.initializer_range
        self.mask_ratio = config.mask_ratio
        self.max_seq_length = max_his_len
        self.n_behaviors = n_behaviors
        self.n_users = n_users
        self.mask_token = n_items + 1
        self.loss_type = config.loss_type
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        H, b = self.hidden_size, n_behaviors
        se = dict(dropout=self.dropout_prob, layer_norm_eps=self.layer_norm_eps, padding_idx=0)
        self.item_embedding_m = SimpleEmbedding(n_items + 2, H, **se)              # 0: <PAD>, n_items + 1: <MASK>
        self.item_embedding_c = SimpleEmbedding(n_items + 2, H, **se)
        self.type_embedding_m = SimpleEmbedding(b + 1, H, **se)
        self.type_embedding_c = SimpleEmbedding(b + 1, H, **se)
        self.user_embedding_m = SimpleEmbedding(n_users + 1, H, **se)
        self.user_embedding_c = SimpleEmbedding(n_users + 1, H, **se)
        self.position_embedding_m = nn.Embedding(max_his_len, H)
        self.position_embedding_c = nn.Embedding(max_his_len, H)
        self.type_relation_embedding_m = SimpleEmbedding(b * b + 1, H, **se)
        self.type_relation_embedding_c = SimpleEmbedding(b * b + 1, H, **se)
        self.activation = nn.ELU()
        self.Wub = nn.Linear(H, H)
        self.WPub = nn.Linear(H, H)
        layer = PBATLayer(d_model=H, nhead=self.n_heads, n_behaviors=b, dim_feedforward=self.inner_size, dropout=self.dropout_prob,
                          activation=self.hidden_act, layer_norm_eps=self.layer_norm_eps)
        self.trm_encoder = modules.TransformerEncoder(layer, self.n_layers)
        self.head = WassersteinPredictionHead(d_model=H, n_items=n_items, token_embeddings_m=self.item_embedding_m.embedding,
                                              token_embeddings_c=self.item_embedding_c.embedding)
        self.apply(self._init_weights)
        self._row_offset = None

    def _init_weights(self, module: nn.Module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

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
    def _types(self, item_seq, type_seq, user_ids, extra=None):
        """(int32 [B, L] types, int64 [B] users) after ONE host read that checks their ranges (and fetches ``extra``, a device
        scalar, with it)"""
        self._require_device(item_seq)
        B, L = item_seq.shape
        if L > self.max_seq_length:
            raise ValueError(f"sequence length {L} > max_his_len {self.max_seq_length}")
        ops.pbat_check_limits(L, self.hidden_size, self.hidden_size // self.n_heads, self.n_behaviors)
        t, u = type_seq.to(item_seq.device), user_ids.to(item_seq.device).long().reshape(-1)
        if t.shape != item_seq.shape or u.shape != (B,):
            raise RuntimeError(f"behaviors must be [{B}, {L}] and uid [{B}], got {tuple(t.shape)} and {tuple(user_ids.shape)}")
        bad_t = ((t < 0) | (t > self.n_behaviors)).any().long().reshape(1)
        bad_u = ((u < 0) | (u > self.n_users)).any().long().reshape(1)
        vals = torch.cat([bad_t, bad_u] + ([extra.long().reshape(1)] if extra is not None else [])).tolist()
        if vals[0]:
            raise IndexError(f"index out of range in self (behaviors outside [0, {self.n_behaviors}])")
        if vals[1]:
            raise IndexError(f"index out of range in self (uid outside [0, {self.n_users}])")
        return t.to(torch.int32).contiguous(), u.contiguous(), (vals[2] if extra is not None else None)

    def _user_behavior(self, users: torch.Tensor):
        """(P_m, P_c) [B, b + 1, H], the user x behaviour Gaussians, and the relation tensors (R_m, R_c) [B, b + 1, b + 1, H]"""
        B, b, H = users.shape[0], self.n_behaviors, self.hidden_size
        dev = users.device
        user_m = self.user_embedding_m(users[:, None])                              # [B, 1, H]
        user_c = self.user_embedding_c(users[:, None]) + 1
        beh = torch.arange(b + 1, device=dev)[None, :].expand(B, -1)
        beh_m = self.type_embedding_m(beh)
        beh_c = F.elu(self.type_embedding_c(beh)) + 1                               # (ELU twice, as the reference)
        P_m, P_c = sagp(user_m, self.Wub(beh_m), user_c, beh_c)
        w = -pairwise_wasserstein(P_m, P_c)                                         # [B, b + 1, b + 1]
        rel_ids = torch.arange(1, b * b + 1, device=dev)[None, :]
        rel_m = self.type_relation_embedding_m(rel_ids).view(b, b, H)
        rel_c = self.type_relation_embedding_c(rel_ids).view(b, b, H)
        wi = w[:, 1:, 1:, None]
        R_m = F.pad(wi * rel_m, (0, 0, 1, 0, 1, 0))                                 # zeros at relation index 0
        R_c = F.elu(F.pad(wi * rel_c, (0, 0, 1, 0, 1, 0), value=1.0)) + 1           # ELU(1) + 1 there
        return P_m, P_c, R_m, R_c

    def _encode(self, item_seq, types, users, shared=None):
        ids = item_seq.long().contiguous()
        L = ids.shape[1]
        sm, sc = shared if shared is not None else (None, None)
        item_m = self.item_embedding_m(ids, sm)
        item_c = self.item_embedding_c(ids, sc) + 1
        tl = types.long()
        type_m = self.type_embedding_m(tl)
        type_c = self.type_embedding_c(tl) + 1
        pos_m = self.position_embedding_m.weight[:L]
        pos_c = self.position_embedding_c.weight[:L] + 1
        P_m, P_c, R_m, R_c = self._user_behavior(users)
        lists = _TypeLists(types, self.n_behaviors)
        keep = (ids != 0).to(torch.int32).contiguous()
        out_m, out_c = self.trm_encoder((item_m, item_c), keep, type_seq=lists, type_tensor=(type_m, type_c),
                                        type_relation_tensor=(R_m, R_c), position_tensor=(pos_m, pos_c))
        return out_m, out_c, P_m, P_c

    def _head_input(self, item_seq, types, users, rows, shared=None) -> torch.Tensor:
        """x' [M, 2 H] of the flat positions ``rows``; the rows' own term a_r is kept in ``_row_offset``"""
        out_m, out_c, P_m, P_c = self._encode(item_seq, types, users, shared)
        B, L = item_seq.shape
        H = self.hidden_size
        om, oc = out_m.reshape(-1, H).index_select(0, rows), out_c.reshape(-1, H).index_select(0, rows)
        pair = torch.div(rows, L, rounding_mode="floor") * (self.n_behaviors + 1) + types.reshape(-1).index_select(0, rows).long()
        # (many rows share one (batch row, type): the gather whose backward adds the repeats in slot order, without float atomics)
        pm, pc = _GatherRowsFn.apply(P_m.reshape(-1, H), pair.contiguous()), _GatherRowsFn.apply(P_c.reshape(-1, H), pair.contiguous())
        om, oc = sagp(om, self.WPub(pm), oc, pc)
        lin = self.head.out[0]
        xp, a = _WassHeadFn.apply(om, oc, lin.weight, lin.bias)
        self._row_offset = a.detach()
        return xp

    # ---- the cloze task (ClozeMixin: _loss, calculate_loss, full_sort_predict, full_sort_topk) -----------------------------------
    @property
    def item_embedding(self):
        """the mean table (ClozeMixin asks it whether the tables train)"""
        return self.item_embedding_m.embedding

    _head_bias = None

    def _shared_grad(self):
        on = torch.is_grad_enabled() and self.item_embedding_m.embedding.weight.requires_grad and \
            self.item_embedding_c.embedding.weight.requires_grad
        return (_SharedGrad(), _SharedGrad()) if on else None

    def _head_table(self, shared=None):
        """(E' [V, 2 H], c [V], V): the derived table the biased catalogue kernels score against; the two item tables' gradients
        leave through ``shared``, so the cross entropy keeps E''s own gradient to itself"""
        V = self.n_items + 1
        E2, c = _WassTableFn.apply(self.item_embedding_m.embedding.weight, self.item_embedding_c.embedding.weight, V, shared)
        return E2, c, V, None

    def _cloze_scores(self, y):
        return super()._cloze_scores(y) + self._row_offset[:, None]

    @torch.no_grad()
    def full_sort_topk(self, interaction: dict, k: int):
        idx, scores = super().full_sort_topk(interaction, k)
        return idx, scores + self._row_offset[:, None]

    def forward(self, item_seq: torch.Tensor, type_seq: torch.Tensor, user_ids: torch.Tensor, labels: torch.Tensor, candidates=None):
        """(valid_logits [M, n_items + 1], valid_labels [M]) of the positions with labels != 0: the Wasserstein distances
        themselves, a_r included, materialised (tests and small catalogues; no gradient flows through them: training goes
        through calculate_loss)."""
        self._refuse_candidates(candidates)
        return self._scores_at_labels(item_seq, labels, self._types(item_seq, type_seq, user_ids)[:2])

    def sample_sort_predict(self, interaction: dict):
        raise NotImplementedError("PBAT.sample_sort_predict: candidates (the negative-sampling tasks) are not supported on the HIP path")

    def _extra(self, item_seq, interaction):
        return self._types(item_seq, interaction["behaviors"], interaction["uid"])[:2]

    def _draw_cloze(self, interaction: dict):
        masked, _, rows, targets, count = self._cloze(interaction["inputs"])
        types, users, M = self._types(masked, interaction["behaviors"], interaction["uid"], count)     # (the step's host read)
        return masked, (types, users), rows[:M], targets[:M]

    @staticmethod
    def _in_graph(name: str) -> bool:
        return not (".FFN." in name and ".LayerNorm." in name)
