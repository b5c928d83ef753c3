"""The forward / backward sequences the recommender backbones' layers are built from, at the bottom of the import graph (``ops`` and
``torch`` only; ``modules`` and ``rec_common`` both import it).

Plain functions, each a named sequence of ``ops.*`` calls.  A forward returns its output and the tuple its backward needs:
  linear_act_fwd / _bwd     act(x w^T + b)
  dropout_fwd, add_dropout  drop(x), x + drop(delta); backward of both: ``_dropout_bwd``
  post_ln_fwd / _bwd        LayerNorm(x + dropout(h))
  ffn_fwd / _bwd            dense_2(act(dense_1(x)))
  attn_block_fwd / _bwd     LayerNorm(x + dropout(dense(core(x Wqkv^T + bqkv)))), the attention core a callback; ``dense_core``
                            is the plain softmax attention of gamer_amd.modules as such a callback pair
  grouped_ffn_fwd / _bwd    dense_2[t](act(dense_1[t](x))) of every row's own type t as two grouped GEMMs over the rows sorted by
                            type (``_TypeLists``), the biases riding as one more input column (``_with_ones``, ``_aug_weights``)
Call them under the "f32" matmul mode.
"""
from __future__ import annotations

import torch

from . import ops

_N_PARTIAL = 256


def _f32(t):
    return dict(dtype=torch.float32, device=t.device)


# ---- Linear + activation, LayerNorm, dropout -----------------------------------------------------------------------------------
def colsum(partial):
    """the column sums [N] of a [rows, N] table of partial sums (gamer_colsum_reduce)"""
    out = torch.empty(partial.shape[1], dtype=torch.float32, device=partial.device)
    ops.colsum_reduce(partial, out)
    return out


def linear_act_fwd(x, w, b, act):
    """(pre, out) of out = act(x w^T + b), ``act`` a code of ops.ACTIVATIONS: pre = x w^T + b; act 0: out is pre itself"""
    M, K = x.shape
    N = w.shape[0]
    pre = torch.empty(M, N, **_f32(x))
    ops.linear_fwd(x, K, w, K, pre, N, M, N, K)
    out = pre if act == 0 else torch.empty_like(pre)
    ops.bias_act_fwd(pre, b, act, None if act == 0 else out)              # (pre <- pre + b in place: act 0 needs no more)
    return pre, out


def linear_act_bwd(g, pre, x, w, act, dx=None):
    """(dx, dw, db) of y = act(x w^T + b) from g = dy [M, N], which is overwritten with d(x w^T + b); ``pre`` = x w^T + b (None
    for act 0), x [M, K], w [N, K].  ``dx`` given: the input gradient is added to it in the GEMM's epilogue.  Call it under the
    "f32" matmul mode."""
    M, K = x.shape
    N = w.shape[0]
    pb = torch.empty(_N_PARTIAL, N, **_f32(x))
    ops.bias_act_bwd(pre, g, act, g, pb)
    db = colsum(pb)
    dw = torch.zeros_like(w)
    ops.linear_wgrad(g, N, x, K, dw, K, M, N, K)
    accumulate = dx is not None
    if dx is None:
        dx = torch.empty(M, K, **_f32(x))
    ops.linear_dgrad(g, N, w, K, dx, K, M, N, K, accumulate=accumulate)
    return dx, dw, db


def layernorm_bwd(v, w, mean, rstd, dy):
    """(dv, dw, db) of y = LayerNorm(v) [T, H] from the saved mean and rstd"""
    T, H = v.shape
    dv = torch.empty(T, H, **_f32(v))
    pw, pb = torch.empty(_N_PARTIAL, H, **_f32(v)), torch.empty(_N_PARTIAL, H, **_f32(v))
    ops.layernorm_bwd(v, w, mean, rstd, dy, dv, pw, pb)
    return dv, colsum(pw), colsum(pb)


def dropout_fwd(x, p, seed):
    """drop(x) under the mask of (p, seed); x itself for p = 0"""
    if p > 0:
        y = torch.zeros_like(x)
        ops.residual_dropout_fwd(y, x, p, seed)                           # y = 0 + drop(x)
        x = y
    return x


def add_dropout(x, delta, p, seed):
    """x + drop(delta)"""
    out = torch.empty(x.shape, **_f32(x))
    ops.residual_dropout_fwd(x, delta, p, seed, None, out)
    return out


def _dropout_bwd(dy, width, p, seed):
    """dy as contiguous fp32 rows of ``width`` values (dy itself when it is that already), through the dropout mask of (p, seed)"""
    g = dy.reshape(-1, width).contiguous().float()
    if p > 0:
        gm = torch.empty_like(g)
        ops.residual_dropout_bwd(g, p, seed, gm)
        g = gm
    return g


def post_ln_fwd(x, h, lnw, lnb, eps, p, seed):
    """y = LayerNorm(x + dropout(h)) [T, H]: (y, (v, mean, rstd))"""
    T = x.shape[0]
    v = add_dropout(x, h, p, seed)
    y = torch.empty_like(v)
    mean, rstd = torch.empty(T, **_f32(x)), torch.empty(T, **_f32(x))
    ops.layernorm_fwd(v, None, lnw, lnb, eps, None, y, mean, rstd)
    return y, (v, mean, rstd)


def post_ln_bwd(dy, saved, lnw, p, seed):
    """(dx_residual, dh, dlnw, dlnb): the gradient of x through the residual branch alone, and of h"""
    v, mean, rstd = saved
    dv, dlnw, dlnb = layernorm_bwd(v, lnw, mean, rstd, dy)
    dh = torch.empty_like(dv)
    ops.residual_dropout_bwd(dv, p, seed, dh)                             # dv stays = d x (residual branch)
    return dv, dh, dlnw, dlnb


# ---- dense FFN -----------------------------------------------------------------------------------------------------------------
def ffn_fwd(x, w1, b1, w2, b2, act):
    """f = dense_2(act(dense_1(x))): (f, (x, pre1, a1))"""
    pre1, a1 = linear_act_fwd(x, w1, b1, act)
    _, f = linear_act_fwd(a1, w2, b2, 0)
    return f, (x, pre1, a1)


def ffn_bwd(g, saved, w1, w2, act):
    """(dx, dw1, db1, dw2, db2) from g = df, which is overwritten"""
    x, pre1, a1 = saved
    da1, dw2, db2 = linear_act_bwd(g, None, a1, w2, 0)
    dx, dw1, db1 = linear_act_bwd(da1, pre1, x, w1, act)
    return dx, dw1, db1, dw2, db2


# ---- one post-LN attention block, y = LayerNorm(x + dropout(dense(core(x Wqkv^T + bqkv)))) ---------------------------------------
def attn_block_fwd(xf, wqkv, bqkv, wd, bd, lnw, lnb, eps, p, seed, core):
    """``core(qkv [T, 3 H], ctx [T, H])`` fills the context and returns what its backward needs.  Returns (y, saved), saved a flat
    tuple of 11 with y last."""
    T, H = xf.shape
    _, qkv = linear_act_fwd(xf, wqkv, bqkv, 0)
    ctxv = torch.empty(T, H, **_f32(xf))
    kept = core(qkv, ctxv)
    _, h = linear_act_fwd(ctxv, wd, bd, 0)
    y, (v, mean, rstd) = post_ln_fwd(xf, h, lnw, lnb, eps, p, seed)
    return y, (xf, wqkv, qkv, ctxv, wd, v, mean, rstd, lnw, kept, y)


def attn_block_bwd(dy, saved, p, seed, core_bwd):
    """``core_bwd(qkv, ctx, dctx, dqkv, kept)`` fills dqkv [T, 3 H] and returns its own parameter gradients.  Returns
    (dx, dwqkv, dbqkv, dwd, dbd, dlnw, dlnb, core's)."""
    xf, wqkv, qkv, ctxv, wd, v, mean, rstd, lnw, kept, _ = saved
    dx, dh, dlnw, dlnb = post_ln_bwd(dy, (v, mean, rstd), lnw, p, seed)
    dctx, dwd, dbd = linear_act_bwd(dh, None, ctxv, wd, 0)
    dqkv = torch.empty_like(qkv)
    extra = core_bwd(qkv, ctxv, dctx, dqkv, kept)
    _, dwqkv, dbqkv = linear_act_bwd(dqkv, None, xf, wqkv, 0, dx=dx)      # dx = d x (residual branch) + dqkv Wqkv
    return dx, dwqkv, dbqkv, dwd, dbd, dlnw, dlnb, extra


def dense_core(mask, B, S, h, d, scale, p, seed):
    """(core, core_bwd) of attn_block_*: softmax(q k^T scale + mask) v with dropout on the probabilities, ``mask`` additive fp32
    (broadcastable to [B, h, S, S]) or None; keeps the log-sum-exp [B, h, S]"""
    def core(qkv, ctxv):
        H = h * d
        lse = torch.empty(B, h, S, **_f32(qkv))
        ops.attn_dense_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask, B, S, h, d, scale, p, seed, ctxv, lse)
        return lse

    def core_bwd(qkv, ctxv, dctx, dqkv, lse):
        H = h * d
        ops.attn_dense_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask, B, S, h, d, scale, p, seed, ctxv, dctx, lse,
                           dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:])
    return core, core_bwd


# ---- behaviour-grouped FFN -----------------------------------------------------------------------------------------------------
class _TypeLists:
    """The rows of one batch ordered by type: ``perm`` int64 [T] (sorted slot -> flat row), ``offsets`` int32 [b + 2] (type t's
    slots are offsets[t] .. offsets[t + 1]); shared by every layer of a pass."""

    def __init__(self, types: torch.Tensor, b: int):
        B, L = types.shape
        dev = types.device
        self.types = types
        perm = torch.empty(B * L, dtype=torch.int32, device=dev)
        slot = torch.empty(B * L, dtype=torch.int32, device=dev)
        self.offsets = torch.empty(b + 2, dtype=torch.int32, device=dev)
        work = torch.empty((B + 1) * (b + 1), dtype=torch.int32, device=dev)
        ops.expert_lists(types, b + 1, perm, slot, self.offsets, work)
        self.perm = perm.long()


def _with_ones(x, pad=4):
    """[x | 1 0 0 0]: the bias of a grouped Linear rides as one more input column (the GEMM wants leading dims % 4 == 0)"""
    T = x.shape[0]
    tail = torch.zeros(T, pad, dtype=torch.float32, device=x.device)
    tail[:, 0] = 1.0
    return torch.cat([x, tail], 1)


def _aug_weights(ws, bs, pad=4):
    """[G, N, K + 4] from G Linear weights [N, K] and biases [N]"""
    W, b = torch.stack(list(ws)), torch.stack(list(bs))
    G, N, _ = W.shape
    return torch.cat([W, b[:, :, None], torch.zeros(G, N, pad - 1, dtype=torch.float32, device=W.device)], 2).contiguous()


def split_aug_grads(dw1a, dw2a):
    """the gradients of (dense_1.weight, dense_1.bias, dense_2.weight, dense_2.bias) of each expert, from those of the
    _aug_weights tables"""
    H, dff = dw1a.shape[2] - 4, dw2a.shape[2] - 4
    out = []
    for i in range(dw1a.shape[0]):
        out += [dw1a[i, :, :H], dw1a[i, :, H], dw2a[i, :, :dff], dw2a[i, :, dff]]
    return out


def grouped_ffn_fwd(y, perm, grp, w1a, w2a, act, zero_bias):
    """f[r] = dense_2[t_r](act(dense_1[t_r](y[r]))) [T, H], zero for the rows outside every group (padding).  ``perm``: the
    _TypeLists order; ``grp``: the groups / group_offsets of the experts' slots; w1a [b, dff, H + 4], w2a [b, H, dff + 4]:
    _aug_weights tables; ``zero_bias`` [dff] zeros (the biases rode in the GEMM).  Returns (f, (ya, pre1, a1a))."""
    T, H = y.shape
    dff = w1a.shape[1]
    ya = _with_ones(y.index_select(0, perm))
    pre1 = torch.zeros(T, dff, **_f32(y))
    ops.linear_fwd(ya, H + 4, w1a, H + 4, pre1, dff, T, dff, H + 4, strideB=dff * (H + 4), **grp)
    a1 = torch.empty(T, dff, **_f32(y))
    ops.bias_act_fwd(pre1, zero_bias, act, a1)
    a1a = _with_ones(a1)
    del a1
    fs = torch.zeros(T, H, **_f32(y))
    ops.linear_fwd(a1a, dff + 4, w2a, dff + 4, fs, H, T, H, dff + 4, strideB=H * (dff + 4), **grp)
    f = torch.empty(T, H, **_f32(y))
    f.index_copy_(0, perm, fs)
    return f, (ya, pre1, a1a)


def grouped_ffn_bwd(df, saved, perm, grp, w1a, w2a, act, dw1a, dw2a):
    """dys [T, H], the gradient of y in SORTED row order (the caller scatters it through ``perm``), from df [T, H] in row order;
    the weight gradients are added to the caller's dw1a / dw2a (zeros before the first call)."""
    ya, pre1, a1a = saved
    T, H = df.shape
    dff = w1a.shape[1]
    dfs = df.index_select(0, perm)
    ops.linear_wgrad(dfs, H, a1a, dff + 4, dw2a, dff + 4, T, H, dff + 4, strideC=H * (dff + 4), **grp)
    da1 = torch.zeros(T, dff, **_f32(df))
    ops.gemm(dfs, H, 1, w2a, 1, dff + 4, da1, dff, T, dff, H, strideB=H * (dff + 4), **grp)
    ops.bias_act_bwd(pre1, da1, act, da1, torch.empty(_N_PARTIAL, dff, **_f32(df)))
    ops.linear_wgrad(da1, dff, ya, H + 4, dw1a, H + 4, T, dff, H + 4, strideC=dff * (H + 4), **grp)
    dys = torch.zeros(T, H, **_f32(df))
    ops.gemm(da1, dff, 1, w1a, 1, H + 4, dys, H, T, H, dff, strideB=dff * (H + 4), **grp)
    return dys
