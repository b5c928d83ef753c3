"""MBHT, the multi-behaviour hypergraph transformer of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface, parameter and state-dict names, creation order and seeded initialisation as the reference
(ref:SeqRec/models/discriminative/MBHT/model.py, ref:SeqRec/modules/layers/multi_scale_transformer.py,
ref:SeqRec/modules/layers/HGNN.py): ``type_embedding`` [n_behaviors + 1, H], ``item_embedding`` [n_items + 2, H] (row 0 pads, row
n_items + 1 is ``<MASK>``), ``position_embedding`` [L, H] with L = max_his_len + 1 (the input is right-padded to max_his_len and one
column is appended), ``trm_encoder.layer.{l}.multi_head_attention.{out_fc, attention1.{E, F, W_V, W_K, W_Q, dense, LayerNorm},
attention2.{query, key, value, dense, LayerNorm}}``, ``trm_encoder.layer.{l}.feed_forward.{dense_1, dense_2, LayerNorm}``,
``hgnn_layer.hgc{1,2}.{weight, bias}``, ``LayerNorm``, ``hg_type_embedding``, ``metric_w1``, ``metric_w2``, ``gating_weight``,
``gating_bias``, ``attn_weights``, ``attn``.  A reference ``best_model.pth`` loads here and one saved here loads into the reference.

Every step runs as HIP kernels, with no PyTorch fallback:
  input       dropout(LayerNorm(E[item] + P[pos] + T[type])): gamer_embedding_fwd, gamer_layernorm_fwd, the dropout kernel;
              backward into the item-table gradient shared with the loss
  layer       (enable_ms) FeedForward(out_fc(cat(a1(x), a2(pool_s1 x), a2(pool_s2 x)))) with no residual and no LayerNorm around
              out_fc, one autograd.Function (_MSLayerFn):
                a1      q | k | v GEMM, gamer_msa_linear_fwd / _bwd (csrc/mbht.hip: key / value masking, the sequence-axis
                        projections F / E to c = scales[0] rows, softmax over those c columns, dropout, context in one launch),
                        dense, dropout, LayerNorm(h + x)
                pool_s  x.view(B, s, L / s, H).mean(1), a strided mean (device torch op)
                a2      the plain post-LN attention without a mask, the SAME module on both pooled inputs (its gradients add)
                out_fc  gamer_seq_mix_fwd / _bwd: Linear(L + L / s1 + L / s2, L) along the sequence axis, three base pointers
                        instead of a cat, no transposes
              (enable_ms=False) the plain layer of gamer_amd.modules with the additive key mask
  hypergraph  (enable_hg) one autograd.Function (_HGFn): the gate x_raw = e sigmoid(e Wg + bg) (e = E[item]; existing GEMM and
              activation kernels), x_m = (w1 + w2) / 2 x_raw, gamer_hg_build_fwd / _bwd (one workgroup per row: similarities, top-k,
              the hypergraph as per-position (edge, value) lists in LDS, G = Dv^-1 H De^-1 H^T padded to [B, L, L]: the reference's
              block-diagonal [sum n, sum n] matrix never exists), two layers G (x W + b) with gamer_hg_conv_fwd / _bwd and the
              HGNN's own 0.2 dropout, (x1 + x2) / 2, the sequential sliding-window readout gamer_hg_readout_fwd / _bwd (training
              and evaluation forms) and the two-source fusion gamer_hg_fuse_fwd / _bwd
  loss        the cross entropy over ALL n_items + 2 rows of the table (rec_common.CatalogCEFn: the scores are never written);
              ranking: gamer_catalog_topk over items [0, n_items + 1)

Reference behaviour kept on purpose:
  * ``hg_type_embedding`` and ``feed_forward.LayerNorm`` exist in the state dict, are never used and get no gradient.
  * ``pos_items`` / ``masked_index`` are left-padded with 0 and cut to the last int(mask_ratio max_his_len) entries.  The loss is
    the mean over ALL B m slots: ``nn.CrossEntropyLoss()`` reduces to the mean before the reference multiplies by ``targets =
    masked_index > 0`` and divides by their sum, so that weighting cancels and a padded slot counts position 0 against class 0.
  * ``F.normalize(x_m)`` of the similarity runs along dim 1 of [B, l, H], the sequence axis: every hidden column is divided by its
    norm over the l positions of the row (padding included), and the "similarity" is the dot product of those scaled rows.
  * A ``pos == 0`` readout is skipped in training; in evaluation a ``<MASK>`` at position 0 reads the mean of no rows, NaN.
  * ``loss_type != "CE"`` is refused (the reference asserts); L must be divisible by scales[1] and scales[2] (the reference asserts).
Not the reference's:
  * the mask draw uses the project's counter-based hash (gamer_cloze_mask), not Python's ``random``;
  * ``gating_bias`` is zero-initialised (the reference leaves it uninitialised memory);
  * the two ``assert not isnan`` host syncs are dropped;
  * among equal similarities the top-k takes the lower key position (the reference's ``topk(sorted=False)`` leaves it open);
  * int(mask_ratio max_his_len) = 0 cannot run in the reference (ragged lists) and is refused.
Limits (NotImplementedError on the host): L <= 128, head size <= 64, hidden size <= 256 and a multiple of 4, scales[0] <= 16,
hyper_len <= 8.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import nn

from . import modules, ops
from .layer_blocks import (_dropout_bwd, attn_block_bwd, attn_block_fwd, colsum, dense_core, dropout_fwd, ffn_bwd, ffn_fwd,
                           layernorm_bwd, linear_act_bwd, linear_act_fwd)
from .rec_common import CatalogCEFn, ClozeMixin, DropUnknownConfig, _GatherRowsFn, _SharedGrad, _next_seed


@dataclasses.dataclass(init=False)
class MBHTConfig(DropUnknownConfig):
    """The fields and defaults of the reference's MBHTConfig (ref:SeqRec/models/discriminative/MBHT/config.py); unknown keys are
    dropped, as the reference's pydantic model does."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 128
    inner_size: int = 256
    dropout_prob: float = 0.5
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    mask_ratio: float = 0.2
    loss_type: str = "CE"
    enable_hg: bool = True
    enable_ms: bool = True
    hyper_len: int = 6
    scales: tuple = (5, 8, 40)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.scales = list(self.scales)


# ---- parameter holders with the reference's names ------------------------------------------------------------------------------
class LinearAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout, layer_norm_eps, linear_size, max_len):
        super().__init__()
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        self.E = nn.Linear(max_len, linear_size)
        self.F = nn.Linear(max_len, linear_size)
        self.W_V = nn.Linear(embed_dim, embed_dim)
        self.W_K = nn.Linear(embed_dim, embed_dim)
        self.W_Q = nn.Linear(embed_dim, embed_dim)
        self.dense = nn.Linear(embed_dim, embed_dim)
        self.n_heads = num_heads
        self.d_k = embed_dim // num_heads
        self.attn_dropout = nn.Dropout(p=dropout)
        self.out_dropout = nn.Dropout(p=dropout)
        self.LayerNorm = nn.LayerNorm(embed_dim, eps=layer_norm_eps)


class MultiScaleAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout, layer_norm_eps, scales, max_len):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)" % (embed_dim, num_heads))
        self.d_k = embed_dim // num_heads
        self.num_heads = num_heads
        self.scale_1, self.scale_2 = scales[1], scales[2]
        self.max_len = max_len
        self.out_fc = nn.Linear(max_len + max_len // self.scale_1 + max_len // self.scale_2, max_len)
        self.attention1 = LinearAttention(embed_dim, num_heads, dropout, layer_norm_eps, scales[0], max_len)
        self.attention2 = modules.MultiHeadAttention(embed_dim, num_heads, dropout, layer_norm_eps)


class HGNN_conv(nn.Module):
    """Parameter holder with the reference's names; initialised in the constructor (``_init_weights`` does not touch it)."""

    def __init__(self, n_hid: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n_hid, n_hid))
        nn.init.normal_(self.weight, std=0.02)
        self.bias = nn.Parameter(torch.empty(n_hid))
        nn.init.normal_(self.bias, std=0.02)


class HGNN(nn.Module):
    def __init__(self, n_hid: int, dropout: float = 0.2):
        super().__init__()
        self.dropout = dropout                                   # (its own attribute, not the config's dropout_prob)
        self.hgc1 = HGNN_conv(n_hid)
        self.hgc2 = HGNN_conv(n_hid)


class _MSLayerFn(torch.autograd.Function):
    """One MultiScaleTransformerEncoderLayer with multiscale=True.  params: out_fc (w, b); attention1: E (w, b), F (w, b), W_Q, W_K,
    W_V, dense (w, b each), LayerNorm (w, b); attention2: query, key, value, dense (w, b each), LayerNorm (w, b); dense_1, dense_2
    (w, b each)."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, keep, meta, *params):
        if not x.is_cuda:
            raise RuntimeError("gamer_amd.mbht runs on the HIP device only (no CPU fallback)")
        (wo, bo, Ew, Eb, Fw, Fb, wq1, bq1, wk1, bk1, wv1, bv1, wd1, bd1, l1w, l1b,
         wq2, bq2, wk2, bk2, wv2, bv2, wd2, bd2, l2w, l2b, w1, b1, w2, b2) = params
        B, L, H = x.shape
        h, act, eps, (s1, s2) = meta["heads"], meta["act"], meta["eps"], meta["scales"]
        p = meta["dropout"] if meta["training"] else 0.0
        d = H // h
        f32 = dict(dtype=torch.float32, device=x.device)
        scale = math.sqrt(1.0 / float(d))
        seeds = [modules._SeedCounter.next() for _ in range(6)]
        x = x.contiguous().float()
        xf = x.view(B * L, H)

        def linear_core(qkv, ctxv):
            lse = torch.empty(B, h, L, **f32)
            ops.msa_linear_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, p, seeds[0], ctxv, lse)
            return lse
        wqkv1, bqkv1 = torch.cat([wq1, wk1, wv1], 0).contiguous(), torch.cat([bq1, bk1, bv1], 0).contiguous()
        wqkv2, bqkv2 = torch.cat([wq2, wk2, wv2], 0).contiguous(), torch.cat([bq2, bk2, bv2], 0).contiguous()
        y1, sv1 = attn_block_fwd(xf, wqkv1, bqkv1, wd1.contiguous(), bd1, l1w, l1b, eps, p, seeds[1], linear_core)
        ys, svs = [y1.view(B, L, H)], [sv1]
        for i, s in enumerate((s1, s2)):
            S = L // s
            xp = x.view(B, s, S, H).mean(1).reshape(B * S, H).contiguous()       # row j averages positions j, j + L / s, ...
            core, _ = dense_core(None, B, S, h, d, scale, p, seeds[2 + 2 * i])
            y, sv = attn_block_fwd(xp, wqkv2, bqkv2, wd2.contiguous(), bd2, l2w, l2b, eps, p, seeds[3 + 2 * i], core)
            ys.append(y.view(B, S, H))
            svs.append(sv)
        wo_ = wo.contiguous()
        m = torch.empty(B, L, H, **f32)
        ops.seq_mix_fwd(ys, wo_, bo, m)
        mf = m.view(B * L, H)
        f2, (_, pre1, a1) = ffn_fwd(mf, w1, b1, w2, b2, act)
        ctx.meta = dict(meta, p=p, seeds=seeds, scale=scale, shape=(B, L, H))
        flat = []
        for sv in svs:
            flat += list(sv)
        ctx.save_for_backward(keep, Ew, Eb, Fw, Fb, wo_, mf, w1, pre1, a1, w2, *flat)
        return f2.view(B, L, H)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        keep, Ew, Eb, Fw, Fb, wo, mf, w1, pre1, a1, w2, *flat = ctx.saved_tensors
        svs = [tuple(flat[11 * i:11 * i + 11]) for i in range(3)]
        mt = ctx.meta
        B, L, H = mt["shape"]
        h, act, p, seeds, scale, (s1, s2) = mt["heads"], mt["act"], mt["p"], mt["seeds"], mt["scale"], mt["scales"]
        d = H // h
        T = B * L
        c = Ew.shape[0]
        f32 = dict(dtype=torch.float32, device=mf.device)
        g = dout.reshape(T, H).contiguous().float().clone()
        dm, dw1, db1, dw2, db2 = ffn_bwd(g, (mf, pre1, a1), w1, w2, act)
        # out_fc
        lens = [L, L // s1, L // s2]
        youts = [sv[10].view(B, n, H) for sv, n in zip(svs, lens)]
        dys = [torch.empty(B, n, H, **f32) for n in lens]
        n_part = ops.seq_mix_n_partial(B, L, sum(lens))
        part = torch.zeros(n_part, L * sum(lens) + L, **f32)
        ops.seq_mix_bwd(youts, wo, dm.view(B, L, H), dys, part)
        dwo_b = colsum(part)
        dwo, dbo = dwo_b[:L * sum(lens)].view(L, sum(lens)), dwo_b[L * sum(lens):].clone()     # (clone: gradients start 16-byte aligned)

        def linear_core_bwd(qkv, ctxv, dctx, dqkv, lse):
            n = ops.msa_n_partial(B, h)
            pt = torch.zeros(n, 2 * c * L + 2 * c, **f32)
            ops.msa_linear_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, p, seeds[0], dctx,
                               lse, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], pt)
            s = colsum(pt)
            return (s[:c * L].view(c, L), s[2 * c * L:2 * c * L + c].clone(), s[c * L:2 * c * L].view(c, L).clone(),
                    s[2 * c * L + c:].clone())
        dx, dwqkv1, dbqkv1, dwd1, dbd1, dl1w, dl1b, (dEw, dEb, dFw, dFb) = attn_block_bwd(
            dys[0].view(T, H), svs[0], p, seeds[1], linear_core_bwd)
        dx = dx.view(B, L, H)
        acc2 = None
        for i, s in enumerate((s1, s2)):
            S = L // s
            _, core_bwd = dense_core(None, B, S, h, d, scale, p, seeds[2 + 2 * i])
            r = attn_block_bwd(dys[1 + i].view(B * S, H), svs[1 + i], p, seeds[3 + 2 * i], core_bwd)
            dx.view(B, s, S, H).add_(r[0].view(B, 1, S, H) / s)                  # the strided mean's backward
            acc2 = list(r[1:7]) if acc2 is None else [a + b for a, b in zip(acc2, r[1:7])]
        dwqkv2, dbqkv2, dwd2, dbd2, dl2w, dl2b = acc2
        return (dx, None, None, dwo, dbo, dEw, dEb, dFw, dFb,
                dwqkv1[:H], dbqkv1[:H], dwqkv1[H:2 * H], dbqkv1[H:2 * H], dwqkv1[2 * H:], dbqkv1[2 * H:], dwd1, dbd1, dl1w, dl1b,
                dwqkv2[:H], dbqkv2[:H], dwqkv2[H:2 * H], dbqkv2[H:2 * H], dwqkv2[2 * H:], dbqkv2[2 * H:], dwd2, dbd2, dl2w, dl2b,
                dw1, db1, dw2, db2)


class MultiScaleTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward, dropout, activation, layer_norm_eps, scales, max_len):
        super().__init__()
        self.multi_head_attention = MultiScaleAttention(d_model, nhead, dropout, layer_norm_eps, scales, max_len)
        self.feed_forward = modules.FeedForward(d_model, dim_feedforward, dropout, activation, layer_norm_eps)
        self.dropout_p, self.eps = float(dropout), float(layer_norm_eps)

    def forward(self, hidden_states, attention_mask=None, keep=None):
        """``keep``: int32 [B, L], non-zero where the position holds an item (the reference's 0 / 1 attention mask)."""
        a, f = self.multi_head_attention, self.feed_forward
        a1, a2 = a.attention1, a.attention2
        meta = dict(heads=a.num_heads, act=f.act_code, dropout=self.dropout_p, eps=self.eps, training=self.training,
                    scales=(a.scale_1, a.scale_2))
        params = [a.out_fc.weight, a.out_fc.bias, a1.E.weight, a1.E.bias, a1.F.weight, a1.F.bias]
        for m in (a1.W_Q, a1.W_K, a1.W_V, a1.dense, a1.LayerNorm, a2.query, a2.key, a2.value, a2.dense, a2.LayerNorm, f.dense_1, f.dense_2):
            params += [m.weight, m.bias]
        return _MSLayerFn.apply(hidden_states, keep, meta, *params)


class _InputFn(torch.autograd.Function):
    """(dropout(LayerNorm(E[ids] + P[s] + T[types])), E[ids]) for ids / types [B, L]; gradients of E (padding row 0 skipped, into
    the shared table gradient), P, T (row 0 skipped) and the LayerNorm.  The second output feeds the hypergraph branch."""

    @staticmethod
    def forward(ctx, ids, types, E, P, T, w, b, eps, p, seed, shared=None):
        B, L = ids.shape
        H = E.shape[1]
        f32 = dict(dtype=torch.float32, device=E.device)
        e, t = torch.empty(B * L, H, **f32), torch.empty(B * L, H, **f32)
        ops.embedding_fwd(ids, E, e)
        ops.embedding_fwd(types, T, t)
        v = (e.view(B, L, H) + P[:L] + t.view(B, L, H)).view(B * L, H)
        y = torch.empty(B * L, H, **f32)
        mean, rstd = torch.empty(B * L, **f32), torch.empty(B * L, **f32)
        ops.layernorm_fwd(v, None, w, b, eps, None, y, mean, rstd)
        y = dropout_fwd(y, p, seed)
        ctx.meta = (p, seed, E.shape, P.shape, T.shape)
        ctx.shared = shared
        ctx.save_for_backward(ids, types, v, w, mean, rstd)
        return y.view(B, L, H), e.view(B, L, H)

    @staticmethod
    def backward(ctx, dy, de):
        ids, types, v, w, mean, rstd = ctx.saved_tensors
        p, seed, e_shape, p_shape, t_shape = ctx.meta
        B, L = ids.shape
        H = v.shape[1]
        dv, dw, db = layernorm_bwd(v, w, mean, rstd, _dropout_bwd(dy, H, p, seed))
        dT = torch.zeros(t_shape, dtype=torch.float32, device=v.device)
        ops.embedding_bwd_large(types, dv, 0, dT)
        dP = torch.zeros(p_shape, dtype=torch.float32, device=v.device)
        ops.position_bwd(dv.view(B, L, H), dP[:L])
        if de is not None:
            dv = dv + de.reshape(B * L, H)
        dE = _SharedGrad.take(ctx.shared, e_shape, v.device)
        ops.embedding_bwd_large(ids, dv.contiguous(), 0, dE)
        return None, None, dE, dP, dT, dw, db, None, None, None, None


class _HGFn(torch.autograd.Function):
    """The hypergraph branch and the fusion with the encoder's output: fuse(trm, readout(HGNN(x_raw, G(x_m)))) with
    x_raw = e sigmoid(e Wg + bg), x_m = (w1 + w2) / 2 x_raw.  params: gating_weight, gating_bias, metric_w1, metric_w2,
    hgc1 (weight, bias), hgc2 (weight, bias), attn_weights, attn."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, trm, e, items, pos, n_obj, meta, gw, gb, w1, w2, W1, b1, W2, b2, A, a):
        B, L, H = e.shape
        T = B * L
        K, mask_token, evaluation = meta["hyper_len"], meta["mask_token"], meta["evaluation"]
        p = meta["dropout"] if meta["training"] else 0.0
        seeds = [modules._SeedCounter.next() for _ in range(2)]
        f32 = dict(dtype=torch.float32, device=e.device)
        sig = ops.ACTIVATIONS["sigmoid"]
        ef = e.reshape(T, H).contiguous().float()
        gwT = gw.t().contiguous()
        z, sg = linear_act_fwd(ef, gwT, gb.reshape(H).contiguous(), sig)          # z = e Wg + bg, sg = sigmoid(z)
        x_raw = ef * sg
        ms = (0.5 * (w1 + w2)).reshape(1, H)
        xm = (x_raw * ms).view(B, L, H)
        G, sel = torch.empty(B, L, L, **f32), torch.empty(B, L, K, dtype=torch.int32, device=e.device)
        ops.hg_build_fwd(xm, items, mask_token, K, G, sel)

        def layer(x, W, b, seed):
            WT = W.t().contiguous()
            _, t = linear_act_fwd(x, WT, b, 0)
            y = torch.empty(B, L, H, **f32)
            ops.hg_conv_fwd(G, t.view(B, L, H), y)
            return WT, t, dropout_fwd(y.view(T, H), p, seed)
        W1T, t1, x1 = layer(x_raw, W1, b1, seeds[0])
        W2T, t2, x2 = layer(x1, W2, b2, seeds[1])
        hg = ((x1 + x2) / 2).view(B, L, H)
        r = torch.empty(B, L, H, **f32)
        ops.hg_readout_fwd(hg, pos, n_obj, r, meta["before"], meta["follow"], evaluation)
        wvec = (A @ a.t()).reshape(H).contiguous()
        trmf = trm.reshape(T, H).contiguous().float()
        out, p0 = torch.empty(T, H, **f32), torch.empty(T, **f32)
        ops.hg_fuse_fwd(trmf, r.view(T, H), wvec, out, p0)
        ctx.meta = dict(meta, p=p, seeds=seeds, shape=(B, L, H))
        ctx.save_for_backward(ef, gwT, z, sg, x_raw, ms, xm, items, sel, G, W1T, t1, x1, W2T, t2, pos, n_obj, trmf, r, wvec, p0, A, a)
        return out.view(B, L, H)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        (ef, gwT, z, sg, x_raw, ms, xm, items, sel, G, W1T, t1, x1, W2T, t2, pos, n_obj, trmf, r, wvec, p0, A, a) = ctx.saved_tensors
        mt = ctx.meta
        B, L, H = mt["shape"]
        T, p, seeds = B * L, mt["p"], mt["seeds"]
        f32 = dict(dtype=torch.float32, device=ef.device)
        g = dout.reshape(T, H).contiguous().float()
        dtrm, dr = torch.empty(T, H, **f32), torch.empty(T, H, **f32)
        part = torch.empty(min(256, (T + 3) // 4), H, **f32)
        ops.hg_fuse_bwd(trmf, r.view(T, H), wvec, p0, g, dtrm, dr, part)
        dwvec = colsum(part)
        dA, da = dwvec[:, None] * a, dwvec[None, :] @ A
        dhg = torch.empty(B, L, H, **f32)
        ops.hg_readout_bwd(dr.view(B, L, H), pos, n_obj, dhg, mt["before"], mt["follow"], mt["evaluation"])
        dhalf = dhg.view(T, H) / 2

        def layer_bwd(dx_out, x_in, WT, t, seed):
            dy = _dropout_bwd(dx_out, H, p, seed)
            dt, dG = torch.empty(B, L, H, **f32), torch.empty(B, L, L, **f32)
            ops.hg_conv_bwd(G, t.view(B, L, H), dy.view(B, L, H), dt, dG)
            dx_in, dWT, db = linear_act_bwd(dt.view(T, H), None, x_in, WT, 0)
            return dx_in, dWT.t(), db, dG
        dx1, dW2, db2, dG2 = layer_bwd(dhalf, x1, W2T, t2, seeds[1])
        dx1 += dhalf
        dxr, dW1, db1, dG1 = layer_bwd(dx1, x_raw, W1T, t1, seeds[0])
        dxm = torch.empty(B, L, H, **f32)
        ops.hg_build_bwd(xm, items, sel, G, dG1 + dG2, mt["mask_token"], dxm)
        dxm = dxm.view(T, H)
        dxr += dxm * ms
        dms = 0.5 * (dxm * x_raw).sum(0, keepdim=True)
        de = dxr * sg
        dex, dgwT, dgb = linear_act_bwd(dxr * ef, z, ef, gwT, ops.ACTIVATIONS["sigmoid"])
        de += dex
        return (dtrm.view(B, L, H), de.view(B, L, H), None, None, None, None, dgwT.t(), dgb.view(1, H), dms, dms.clone(), dW1, db1,
                dW2, db2, dA, da)


class MBHT(ClozeMixin, nn.Module):
    def __init__(self, config: MBHTConfig, n_items: int, max_his_len: int, target_behavior_id: int, n_behaviors: int, **kwargs):
        super().__init__()
        if config.loss_type != "CE":
            raise NotImplementedError("MBHT: only loss_type 'CE' is supported (the reference asserts it)")
        if config.hidden_size % config.n_heads:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.n_heads))
        L = max_his_len + 1
        scales = list(config.scales)
        if config.enable_ms:
            if len(scales) != 3:
                raise NotImplementedError(f"MBHT: scales must hold three values (linear size, two pooling factors), got {scales}")
            if L % scales[1] or L % scales[2]:
                raise ValueError(f"MBHT: max_his_len + 1 = {L} must be divisible by scales[1] = {scales[1]} and scales[2] = "
                                 f"{scales[2]} (the reference asserts it): choose another max_his_len")
        ops.mbht_check_limits(L, config.hidden_size, config.hidden_size // config.n_heads, scales[0] if config.enable_ms else 1,
                              config.hyper_len if config.enable_hg else 1)
        if int(config.mask_ratio * max_his_len) < 1:
            raise ValueError(f"MBHT: int(mask_ratio * max_his_len) = int({config.mask_ratio} * {max_his_len}) must be >= 1 (the "
                             "reference builds ragged lists otherwise)")
        self.config = config
        self.n_items = n_items
        self.n_layers, self.n_heads = config.n_layers, config.n_heads
        self.hidden_size, self.inner_size = config.hidden_size, config.inner_size
        self.dropout_prob, self.hidden_act = config.dropout_prob, config.hidden_act
        self.layer_norm_eps, self.initializer_range = config.layer_norm_eps, config.initializer_range
        self.mask_ratio = config.mask_ratio
        self.hglen, self.enable_hg, self.enable_ms, self.scales = config.hyper_len, config.enable_hg, config.enable_ms, scales
        self.max_seq_length = max_his_len
        self.target_type = target_behavior_id
        self.n_behaviors = n_behaviors
        self.mask_token = n_items + 1
        self.mask_item_length = int(self.mask_ratio * self.max_seq_length)
        self.loss_type = config.loss_type
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        H = self.hidden_size
        self.type_embedding = nn.Embedding(n_behaviors + 1, H, padding_idx=0)
        self.item_embedding = nn.Embedding(n_items + 2, H, padding_idx=0)          # 0: <PAD>, n_items + 1: <MASK>
        self.position_embedding = nn.Embedding(L, H)
        if self.enable_ms:
            layer = MultiScaleTransformerEncoderLayer(H, self.n_heads, self.inner_size, self.dropout_prob, self.hidden_act,
                                                      self.layer_norm_eps, scales, L)
        else:
            layer = modules.TransformerEncoderLayer(H, self.n_heads, self.inner_size, self.dropout_prob, self.hidden_act,
                                                    self.layer_norm_eps)
        self.trm_encoder = modules.TransformerEncoder(layer, self.n_layers)
        self.hgnn_layer = HGNN(H)
        self.LayerNorm = nn.LayerNorm(H, eps=self.layer_norm_eps)
        self.dropout = nn.Dropout(self.dropout_prob)
        self.hg_type_embedding = nn.Embedding(n_behaviors, H, padding_idx=0)
        self.metric_w1 = nn.Parameter(torch.empty(1, H))
        self.metric_w2 = nn.Parameter(torch.empty(1, H))
        self.gating_weight = nn.Parameter(torch.empty(H, H))
        self.gating_bias = nn.Parameter(torch.zeros(1, H))                         # (the reference: uninitialised memory)
        self.attn_weights = nn.Parameter(torch.empty(H, H))
        self.attn = nn.Parameter(torch.empty(1, H))
        self.sw_before, self.sw_follow = 10, 6
        self.apply(self._init_weights)

    def _init_weights(self, module: nn.Module):
        if isinstance(module, MBHT):
            for t in (module.attn, module.attn_weights, module.gating_weight, module.metric_w1, module.metric_w2):
                nn.init.normal_(t, std=self.initializer_range)
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    # ---- data --------------------------------------------------------------------------------------------------------------------
    def _right_padding(self, seq: torch.Tensor) -> torch.Tensor:
        if seq.shape[1] > self.max_seq_length:
            raise ValueError(f"sequence length {seq.shape[1]} > max_his_len {self.max_seq_length}")
        out = torch.zeros(seq.shape[0], self.max_seq_length + 1, dtype=torch.long, device=seq.device)
        out[:, :seq.shape[1]] = seq
        return out

    def reconstruct_train_data(self, item_seq, type_seq, last_target, last_type, seed=None):
        """(masked_item_seq [B, L], pos_items [B, m], masked_index [B, m], item_type_seq [B, L]), m = int(mask_ratio max_his_len):
        the target and its type are appended at column n = count_nonzero; that position is always masked, earlier ones with
        probability mask_ratio (gamer_cloze_mask under ``seed``, default: the module's running counter); masked positions get type
        0; pos_items / masked_index are left-padded with 0 and hold the LAST m masked positions.  All on the device."""
        self._require_device(item_seq)
        seed = _next_seed() if seed is None else int(seed)
        items, types = self._right_padding(item_seq.long()), self._right_padding(type_seq.long())
        B, L = items.shape
        ar = torch.arange(B, device=items.device)
        n = torch.count_nonzero(items, dim=1)
        items[ar, n] = last_target.to(items.device).long()
        types[ar, n] = last_type.to(items.device).long()
        ones = torch.ones(B, dtype=torch.int64, device=items.device)              # (read by the fine-tuning rows only)
        _, labels = ops.cloze_mask(items, ones, self.mask_ratio, 0.0, self.mask_token, L, seed)[:2]
        labels[ar, n] = items[ar, n]
        m = labels != 0
        masked = torch.where(m, torch.full_like(items, self.mask_token), items)
        types = types * (~m)
        M = self.mask_item_length
        rank = m.flip(1).cumsum(1).flip(1)                                        # masked positions at or after this one
        take = m & (rank <= M)
        b_idx, pos = take.nonzero(as_tuple=True)
        slot = M - rank[b_idx, pos]
        pos_items = torch.zeros(B, M, dtype=torch.long, device=items.device)
        masked_index = torch.zeros(B, M, dtype=torch.long, device=items.device)
        pos_items[b_idx, slot] = labels[b_idx, pos]
        masked_index[b_idx, slot] = pos
        return masked, pos_items, masked_index, types

    def reconstruct_test_data(self, item_seq, item_seq_len, item_type):
        """(item_seq [B, L], item_type [B, L]) with ``<MASK>`` (type 0) written at column item_seq_len of every row"""
        items, types = self._right_padding(item_seq.long()), self._right_padding(item_type.long())
        items[torch.arange(items.shape[0], device=items.device), item_seq_len.to(items.device).long()] = self.mask_token
        return items, types

    # ---- encoder -----------------------------------------------------------------------------------------------------------------
    def forward(self, item_seq: torch.Tensor, type_seq: torch.Tensor, mask_positions_nums=None, shared=None) -> torch.Tensor:
        """[B, L, H] for item_seq / type_seq [B, L] (L = max_his_len + 1).  ``mask_positions_nums`` = (masked_index, mask_nums)
        selects the training readout of the hypergraph branch, None the evaluation one."""
        self._require_device(item_seq)
        B, L = item_seq.shape
        if L != self.max_seq_length + 1:
            raise ValueError(f"MBHT.forward: sequences of max_his_len + 1 = {self.max_seq_length + 1} columns, got {L}")
        ids = item_seq.long().contiguous()
        types = type_seq.to(ids.device).long().contiguous()
        p = self.dropout_prob if self.training else 0.0
        x, e = _InputFn.apply(ids, types, self.item_embedding.weight, self.position_embedding.weight, self.type_embedding.weight,
                              self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps, p, _next_seed(), shared)
        if self.enable_ms:
            out = self.trm_encoder(x, None, keep=(ids > 0).to(torch.int32).contiguous())
        else:
            fmin = torch.finfo(torch.float32).min
            out = self.trm_encoder(x, ((ids <= 0).float() * fmin)[:, None, None, :])
        if not self.enable_hg:
            return out
        if mask_positions_nums is None:
            pos = (ids == self.mask_token).int().argmax(1, keepdim=True)            # the first <MASK>
        else:
            index, nums = (t.to(ids.device).long() for t in mask_positions_nums)
            last = torch.arange(index.shape[1], device=ids.device)[None, :] >= (index.shape[1] - nums)[:, None]
            pos = index * (last | (nums == 0)[:, None])                              # the last mask_len entries (``[-0:]``: all)
        g, hc1, hc2 = self.hgnn_layer, self.hgnn_layer.hgc1, self.hgnn_layer.hgc2
        meta = dict(hyper_len=self.hglen, mask_token=self.mask_token, evaluation=mask_positions_nums is None, dropout=float(g.dropout),
                    training=self.training, before=self.sw_before, follow=self.sw_follow)
        return _HGFn.apply(out, e, ids.to(torch.int32).contiguous(), pos.to(torch.int32).contiguous(),
                           torch.count_nonzero(ids, dim=1).to(torch.int32).contiguous(), meta, self.gating_weight, self.gating_bias,
                           self.metric_w1, self.metric_w2, hc1.weight, hc1.bias, hc2.weight, hc2.bias, self.attn_weights, self.attn)

    # ---- the cloze task ----------------------------------------------------------------------------------------------------------
    _head_bias = None

    def calculate_loss(self, interaction: dict, masked=None) -> torch.Tensor:
        """The cloze loss of one batch, as the reference computes it: the cross entropy over all n_items + 2 rows of the item table,
        averaged over ALL B m slots of ``masked_index`` - the reference's ``nn.CrossEntropyLoss()`` already returns the mean over
        every slot, so its ``* targets / sum(targets)`` changes nothing; a padded slot scores position 0 against class 0.
        ``masked`` = (masked_item_seq, pos_items, masked_index, item_type_seq) injects the reference's masking (parity tests); by
        default reconstruct_train_data draws it on the device.  One host read per step (the target check of the loss kernel)."""
        if masked is None:
            masked = self.reconstruct_train_data(interaction["inputs"], interaction["behaviors"], interaction["target"],
                                                 interaction["behavior"])
        dev = masked[0].device
        masked_seq, pos_items, masked_index, types = (t.to(dev).long() for t in masked)
        B, L = masked_seq.shape
        # (the clamp: an index outside the row cannot read outside the batch)
        rows = (torch.arange(B, device=dev)[:, None] * L + masked_index.clamp(0, L - 1)).flatten().contiguous()
        targets = pos_items.flatten().contiguous()
        self.last_masked_count = int(rows.numel())
        shared = self._shared_grad()
        out = self.forward(masked_seq, types, (masked_index, torch.count_nonzero(pos_items, dim=1)), shared)
        y = _GatherRowsFn.apply(out, rows)
        return CatalogCEFn.apply(y, torch.arange(rows.numel(), device=dev), self.item_embedding.weight, targets, shared)

    def _last_hidden(self, interaction: dict) -> torch.Tensor:
        item_seq = interaction["inputs"]
        self._require_device(item_seq)
        n = torch.count_nonzero(item_seq, dim=1)
        items, types = self.reconstruct_test_data(item_seq, n, interaction["behaviors"].to(item_seq.device))
        out = self.forward(items, types)
        rows = torch.arange(items.shape[0], device=items.device) * items.shape[1] + n
        return out.reshape(-1, out.shape[-1]).index_select(0, rows)

    def sample_sort_predict(self, interaction: dict):
        raise NotImplementedError("MBHT.sample_sort_predict: candidates (the negative-sampling tasks) are not supported on the HIP path")

    def _in_graph(self, name: str) -> bool:
        if name.startswith("hg_type_embedding.") or ".feed_forward.LayerNorm." in name:
            return False
        hg = name.startswith(("hgnn_layer.", "metric_w", "gating_", "attn"))
        return self.enable_hg or not hg
