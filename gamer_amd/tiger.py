"""TIGER, the T5 encoder-decoder backbone of ``train_decoder``, on the HIP path.

Same nn.Module surface, state-dict names and shapes as the reference (ref:SeqRec/models/generative/TIGER/model.py, a
``T5ForConditionalGeneration`` with a temperature): ``shared.weight`` = ``encoder.embed_tokens.weight`` =
``decoder.embed_tokens.weight`` = ``lm_head.weight`` (four keys, one parameter), ``{encoder,decoder}.block.{l}.layer.0.SelfAttention.
{q,k,v,o}.weight`` with ``relative_attention_bias.weight`` on block 0, ``decoder.block.{l}.layer.1.EncDecAttention.{q,k,v,o}.weight``,
``layer.{n}.layer_norm.weight``, ``DenseReluDense.{wi,wo}.weight`` and the two ``final_layer_norm.weight``.  A reference checkpoint
loads here and one saved here loads there.

Every step runs as HIP kernels, with no PyTorch fallback (a CPU tensor raises):
  input         gamer_embedding_fwd + dropout; backward gamer_embedding_bwd_large into ONE gradient buffer shared by the head and
                both input gathers (rec_common._SharedGrad with two gathers)
  a block       one autograd function: T5's RMS norm (gamer_rmsnorm_fwd / _bwd), ONE [q|k|v] GEMM for self attention, one [k|v]
                GEMM on the encoder output per decoder layer, gamer_t5_attn_fwd / _bwd, the Linear forward / dgrad / wgrad,
                ReLU through gamer_bias_act (zero bias), residual dropout
  attention     csrc/t5_attention.hip up to 128 tokens, csrc/t5_attention_long.hip (K / V streamed in key blocks) up to 512, picked
                per call by the shape: no 1 / sqrt(d), the bucketed relative bias of block 0 added in every layer of its stack,
                key padding mask and causality inside the kernel; nothing of size S x S reaches memory.  The bias table is
                expanded once per stack per step (gamer_t5_bias_expand) and its gradient folded once per stack, after block 0's
                backward, from the per-layer slabs in layer order (gamer_t5_bias_fold)
  loss          rec_common.CatalogCEFn on the rows with label != -100, the decoder rows scaled by d_model ** -0.5 / temperature:
                the [B T, V] logits are not formed in training.  ``forward(..., labels=None)`` or ``want_logits=True``
                materialises them (tests, decoding)

  packed rows   ``forward(..., packed=True, lengths=None)`` (also ``encode`` and ``beam_search``; default off): the encoder side runs on
                the T = sum of the rows' token counts of a right-padded batch instead of B x S_max - the kept ids gathered into
                [T], the same autograd functions on [T, D] (they are token-wise), attention through gamer_t5_attn_packed_* /
                gamer_t5_attn_long_packed_* with per-row offsets, the decoder dense with its cross attention reading the packed
                encoder output.  Bias offsets and dropout counters of the attention keep the dense geometry

Not the reference's: a query row with NO allowed key gives a zero context and zero gradients here; HF's additive finfo.min mask
gives a softmax over the bias alone in that case.  Real inputs cannot produce it: every row holds at least ``</s>``.  Dropout
masks come from the project's counter-based hash.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch
from torch import nn

from . import modules, ops
from .layer_blocks import _N_PARTIAL, _dropout_bwd, add_dropout, colsum, dropout_fwd
from .rec_common import CatalogCEFn, DropUnknownConfig, EmbedDropoutFn, _SharedGrad, _next_seed

# MAX_ENCODER_LEN: the bound of the resident attention kernels (K / V of a head in LDS); longer encoders, up to
# MAX_LONG_ENCODER_LEN, run on the key-streaming kernels.  The decoder's self attention always runs resident.
MAX_ENCODER_LEN, MAX_DECODER_LEN = 128, 8
MAX_LONG_ENCODER_LEN = 512


@dataclasses.dataclass(init=False)
class TigerConfig(DropUnknownConfig):
    """The keys of ref:config/s2s-models/TIGER/config.json that the model reads, with T5Config's defaults where the file is
    silent; every other key (``task_specific_params``, ``architectures``, ...) is dropped without a word."""
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: Optional[int] = None
    num_heads: int = 8
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    dropout_rate: float = 0.1
    layer_norm_epsilon: float = 1e-6
    initializer_factor: float = 1.0
    feed_forward_proj: str = "relu"
    tie_word_embeddings: bool = True
    pad_token_id: int = 0
    eos_token_id: int = 1
    decoder_start_token_id: int = 0

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.num_decoder_layers is None:
            self.num_decoder_layers = self.num_layers


def relative_position_bucket(relative_position: torch.Tensor, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """HF's ``T5Attention._relative_position_bucket`` expression for expression (torch float32 log, ``.to(long)``, ``min`` with
    num_buckets - 1), on the host: a kernel-side logf could round differently at a bucket edge."""
    relative_buckets = 0
    if bidirectional:
        num_buckets //= 2
        relative_buckets += (relative_position > 0).to(torch.long) * num_buckets
        relative_position = torch.abs(relative_position)
    else:
        relative_position = -torch.min(relative_position, torch.zeros_like(relative_position))
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    relative_position_if_large = max_exact + (
        torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    relative_position_if_large = torch.min(relative_position_if_large, torch.full_like(relative_position_if_large, num_buckets - 1))
    relative_buckets += torch.where(is_small, relative_position, relative_position_if_large)
    return relative_buckets


def bucket_vector(S: int, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """int32 [2 S - 1] on the CPU: the bucket of the offset j - i (key - query) at index j - i + S - 1."""
    return relative_position_bucket(torch.arange(-(S - 1), S, dtype=torch.long), bidirectional, num_buckets, max_distance).to(torch.int32)


# ---- parameter holders with HF's names ---------------------------------------------------------------------------------------------
class T5LayerNorm(nn.Module):
    def __init__(self, hidden_size: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps


class T5Attention(nn.Module):
    def __init__(self, config: TigerConfig, has_relative_attention_bias: bool):
        super().__init__()
        inner = config.num_heads * config.d_kv
        self.q = nn.Linear(config.d_model, inner, bias=False)
        self.k = nn.Linear(config.d_model, inner, bias=False)
        self.v = nn.Linear(config.d_model, inner, bias=False)
        self.o = nn.Linear(inner, config.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(config.relative_attention_num_buckets, config.num_heads)


class T5LayerSelfAttention(nn.Module):
    def __init__(self, config: TigerConfig, has_relative_attention_bias: bool):
        super().__init__()
        self.SelfAttention = T5Attention(config, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


class T5LayerCrossAttention(nn.Module):
    def __init__(self, config: TigerConfig):
        super().__init__()
        self.EncDecAttention = T5Attention(config, False)
        self.layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


class T5DenseActDense(nn.Module):
    def __init__(self, config: TigerConfig):
        super().__init__()
        self.wi = nn.Linear(config.d_model, config.d_ff, bias=False)
        self.wo = nn.Linear(config.d_ff, config.d_model, bias=False)


class T5LayerFF(nn.Module):
    def __init__(self, config: TigerConfig):
        super().__init__()
        self.DenseReluDense = T5DenseActDense(config)
        self.layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


class T5Block(nn.Module):
    def __init__(self, config: TigerConfig, is_decoder: bool, has_relative_attention_bias: bool):
        super().__init__()
        self.layer = nn.ModuleList([T5LayerSelfAttention(config, has_relative_attention_bias)])
        if is_decoder:
            self.layer.append(T5LayerCrossAttention(config))
        self.layer.append(T5LayerFF(config))


class T5Stack(nn.Module):
    def __init__(self, config: TigerConfig, embed_tokens: nn.Embedding, is_decoder: bool):
        super().__init__()
        self.is_decoder = is_decoder
        self.embed_tokens = embed_tokens
        n = config.num_decoder_layers if is_decoder else config.num_layers
        self.block = nn.ModuleList([T5Block(config, is_decoder, i == 0) for i in range(n)])
        self.final_layer_norm = T5LayerNorm(config.d_model, config.layer_norm_epsilon)


# ---- backward idioms ---------------------------------------------------------------------------------------------------------------
def _f32(dev):
    return dict(dtype=torch.float32, device=dev)


def _linear(x, W):
    """x [M, K] (row-strided) @ W [N, K]^T"""
    M, (N, K) = x.shape[0], W.shape
    y = torch.empty(M, N, **_f32(x.device))
    ops.linear_fwd(x, x.stride(0), W, K, y, N, M, N, K)
    return y


def _linear_bwd(dy, x, W, dx=None, accumulate=False, packed=False):
    """(dx [M, K], dW) of y = x W^T from dy [M, N] (row-strided views allowed); ``dx``: written (or added to) in place.  ``packed``:
    M changes from batch to batch, so the weight gradient's measured chunk is kept per bucket of M"""
    M, (N, K) = x.shape[0], W.shape
    dW = torch.zeros_like(W)
    ops.linear_wgrad(dy, dy.stride(0), x, x.stride(0), dW, K, M, N, K, tune_rows=ops.wgrad_rows_bucket(M) if packed else None)
    if dx is None:
        dx = torch.empty(M, K, **_f32(x.device))
    ops.linear_dgrad(dy, dy.stride(0), W, K, dx, dx.stride(0), M, N, K, accumulate=accumulate)
    return dx, dW


def _rms(x, w, eps):
    y = torch.empty_like(x)
    ops.rmsnorm_fwd(x, w, eps, y)
    return y


def _rms_bwd(x, w, eps, dy, dx):
    """dx += d RMSNorm(x) from dy; returns dw"""
    part = torch.empty(_N_PARTIAL, x.shape[1], **_f32(x.device))
    ops.rmsnorm_bwd(x, w, dy, dy.stride(0), eps, dx, part, accumulate_dx=True)
    return colsum(part)


def _attn_fwd(q, k, v, rel, keep, B, Sq, Sk, *rest, pack=None, **kw):
    """t5_attn_fwd on the kernel family that the shape needs: resident up to ops.T5_MAX_S, key-streaming above.  ``pack``: the
    (query, key) ops.T5Offsets of packed rows - (Sq, Sk) is then the shape of the dense run and ``keep`` is not read"""
    long = max(Sq, Sk) > ops.T5_MAX_S
    if pack is not None:
        return (ops.t5_attn_long_packed_fwd if long else ops.t5_attn_packed_fwd)(q, k, v, rel, *pack, B, Sq, Sk, *rest, **kw)
    (ops.t5_attn_long_fwd if long else ops.t5_attn_fwd)(q, k, v, rel, keep, B, Sq, Sk, *rest, **kw)


def _attn_bwd(q, k, v, rel, keep, B, Sq, Sk, *rest, pack=None):
    long = max(Sq, Sk) > ops.T5_MAX_S
    if pack is not None:
        return (ops.t5_attn_long_packed_bwd if long else ops.t5_attn_packed_bwd)(q, k, v, rel, *pack, B, Sq, Sk, *rest)
    (ops.t5_attn_long_bwd if long else ops.t5_attn_bwd)(q, k, v, rel, keep, B, Sq, Sk, *rest)


def packed_lengths(attention_mask: torch.Tensor) -> torch.Tensor:
    """int64 [B] on the CPU: the token counts of the rows of a right-padded mask (mask[b, j] != 0 exactly for j < len_b).  Any other
    form raises ValueError naming the row: the relative positions are the original ones, so a hole cannot be packed away."""
    m = attention_mask.detach() != 0
    if m.dim() != 2:
        raise ValueError(f"packed rows: attention_mask [B, S] (got {tuple(m.shape)})")
    lengths = m.sum(1)
    bad = (m != (torch.arange(m.shape[1], device=m.device)[None, :] < lengths[:, None])).any(1)
    code = torch.where(bad, -1 - lengths, lengths).to("cpu")                      # (the one copy: B integers, a bad row negative)
    if int(code.min()) < 0:
        b = int((code < 0).nonzero()[0, 0])
        raise ValueError(f"packed rows need right-padded masks: row {b} of attention_mask is not {-1 - int(code[b])} ones followed by zeros")
    return code


@dataclasses.dataclass
class PackedRows:
    """A packed encoder batch: ``off`` the rows' ops.T5Offsets, ``S`` the padded length of the dense run it replaces, ``rows`` int64
    [T] on the device, the flat [B S] indices of the kept tokens."""
    off: "ops.T5Offsets"
    S: int
    rows: torch.Tensor
    _dense: dict = dataclasses.field(default_factory=dict)

    def dense_offsets(self, B, S, device):
        """the offsets of B dense rows of S tokens (the decoder's queries in cross attention), built once per batch"""
        if (B, S) not in self._dense:
            self._dense[B, S] = ops.T5Offsets.uniform(B, S, device)
        return self._dense[B, S]

    @classmethod
    def build(cls, lengths, B, S, device):
        lengths = torch.as_tensor(lengths).detach()
        if lengths.is_cuda or lengths.dim() != 1 or lengths.numel() != B or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"packed rows: lengths is a CPU int tensor [{B}]")
        lengths = lengths.to(torch.int64)
        if int(lengths.min()) < 0 or int(lengths.max()) > S:
            b = int(((lengths < 0) | (lengths > S)).nonzero()[0, 0])
            raise ValueError(f"packed rows: row {b} holds {int(lengths[b])} tokens of {S}")
        if int(lengths.sum()) == 0:
            raise ValueError("packed rows: the batch holds no token")
        off = ops.T5Offsets.from_lengths(lengths, device)
        pos = torch.arange(off.total, dtype=torch.int64) - torch.repeat_interleave(off.host[:-1].long(), lengths)
        rows = torch.repeat_interleave(torch.arange(B, dtype=torch.int64) * S, lengths) + pos
        return cls(off, S, rows.to(device))


class _BiasStack:
    """The relative bias of one stack for one step: ``rel`` [h, 2 S - 1] expanded once from block 0's table; in the backward every
    block writes its slabs of the offset gradient into ``slabs`` [layers, n, h, 2 S - 1] and block 0, whose backward runs last,
    folds them into the table gradient."""

    def __init__(self, table, bucket, S, n_layers):
        h = table.shape[1]
        self.bucket, self.n_layers, self.S, self.h = bucket, n_layers, S, h
        self.rel = torch.empty(h, 2 * S - 1, **_f32(table.device))
        ops.t5_bias_expand(table.detach().contiguous(), bucket, self.rel)
        self.slabs = None

    def slab(self, layer, B):
        if self.slabs is None:
            self.slabs = torch.empty(self.n_layers, ops.t5_n_slab(B, self.h), self.h, 2 * self.S - 1, **_f32(self.rel.device))
        return self.slabs[layer]

    def fold(self, num_buckets):
        dtable = torch.empty(num_buckets, self.h, **_f32(self.rel.device))
        ops.t5_bias_fold(self.slabs, self.bucket, dtable)
        self.slabs = None
        return dtable


def attn_half_fwd(x, enc, meta, params, seeds):
    """The attention layers of one T5Block, shared by every model built on this stack: x + dropout(o(attn(norm(x)))) and, in a
    decoder block, the same over the encoder output.  ``params``: ln0, q, k, v, o, [ln1, cq, ck, cv, co]; ``seeds``: the block's
    six dropout seeds, of which this half takes the first four.  Returns (x2 [T, D], the tensors its backward needs, the entries
    of the block's ctx.meta)."""
    dec = enc is not None
    pk = meta.get("pack")
    if pk is not None and not dec:
        (T, D), B, S = x.shape, pk.off.n, pk.S
    else:
        B, S, D = x.shape
        T = B * S
    spack = (pk.off, pk.off) if pk is not None and not dec else None
    h, d, eps, bias = meta["heads"], meta["d_kv"], meta["eps"], meta["bias"]
    I = h * d
    p = meta["dropout"] if meta["training"] else 0.0
    ln0, wq, wk, wv, wo = params[:5]
    xf = x.reshape(T, D).contiguous().float()
    # self attention: x + dropout(o(attn(norm(x))))
    n0 = _rms(xf, ln0, eps)
    wqkv = torch.cat([wq, wk, wv], 0).contiguous()
    qkv = _linear(n0, wqkv)
    c0, lse0 = torch.empty(T, I, **_f32(x.device)), torch.empty(h * T, **_f32(x.device))
    keep = None if dec else meta["keep"]
    _attn_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], bias.rel, keep, B, S, S, h, d, dec, p, seeds[0], c0, lse0, pack=spack)
    x1 = add_dropout(xf, _linear(c0, wo), p, seeds[1])
    saved = [xf, n0, wqkv, qkv, c0, lse0, wo, x1, ln0]
    if dec:
        ln1, cq, ck, cv, co = params[5:10]
        Se = pk.S if pk is not None else enc.shape[1]
        xpack = (pk.dense_offsets(B, S, x.device), pk.off) if pk is not None else None
        ef = enc.reshape(-1, D).contiguous().float()
        n1 = _rms(x1, ln1, eps)
        q1 = _linear(n1, cq)
        wkv = torch.cat([ck, cv], 0).contiguous()
        kv = _linear(ef, wkv)
        c1, lse1 = torch.empty(T, I, **_f32(x.device)), torch.empty(h * T, **_f32(x.device))
        _attn_fwd(q1, kv[:, :I], kv[:, I:], None, meta["keep"], B, S, Se, h, d, False, p, seeds[2], c1, lse1, pack=xpack)
        x2 = add_dropout(x1, _linear(c1, co), p, seeds[3])
        saved += [ln1, cq, wkv, co, ef, n1, q1, kv, c1, lse1, x2]
    else:
        x2 = x1
    info = dict(p=p, seeds=seeds, shape=(B, S, D), dec=dec, spack=spack, xpack=xpack if dec else None, Se=Se if dec else None,
                enc_shape=enc.shape if dec else None)
    return x2, saved, info


def attn_half_bwd(sv, mt, dx, keep_mask):
    """The backward of attn_half_fwd, after the feed-forward layer's: ``sv`` the tensors it saved, ``mt`` the block's ctx.meta,
    ``dx`` [T, D] the gradient of the residual stream, added to in place.  Returns (denc or None, the gradients of ``params`` in
    their order, the folded gradient of the stack's bias table after block 0 or None)."""
    B, S, D = mt["shape"]
    T, h, d, eps, p, seeds, dec, bias = sv[0].shape[0], mt["heads"], mt["d_kv"], mt["eps"], mt["p"], mt["seeds"], mt["dec"], mt["bias"]
    pk = mt["spack"] is not None                                              # a packed encoder block: T differs in every batch
    I = h * d
    xf, n0, wqkv, qkv, c0, lse0, wo, x1, ln0 = sv[:9]
    dev = xf.device
    cross = [None] * 5
    denc = None
    if dec:
        ln1, cq, wkv, co, ef, n1, q1, kv, c1, lse1 = sv[9:19]
        Se = mt["Se"]
        da = _dropout_bwd(dx, D, p, seeds[3])
        dc1, dco = _linear_bwd(da, c1, co)
        dq1, dkv = torch.empty(T, I, **_f32(dev)), torch.empty(ef.shape[0], 2 * I, **_f32(dev))
        _attn_bwd(q1, kv[:, :I], kv[:, I:], None, keep_mask, B, S, Se, h, d, False, p, seeds[2], dc1, lse1, dq1,
                  dkv[:, :I], dkv[:, I:], None, pack=mt["xpack"])
        dn1, dcq = _linear_bwd(dq1, n1, cq)
        denc, dwkv = _linear_bwd(dkv, ef, wkv, packed=mt["xpack"] is not None)
        dln1 = _rms_bwd(x1, ln1, eps, dn1, dx)
        cross = [dln1, dcq, dwkv[:I], dwkv[I:], dco]
        denc = denc.view(mt["enc_shape"])
    # self attention
    da = _dropout_bwd(dx, D, p, seeds[1])
    dc0, dwo = _linear_bwd(da, c0, wo, packed=pk)
    dqkv = torch.empty(T, 3 * I, **_f32(dev))
    _attn_bwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], bias.rel, None if dec else keep_mask, B, S, S, h, d, dec, p,
              seeds[0], dc0, lse0, dqkv[:, :I], dqkv[:, I:2 * I], dqkv[:, 2 * I:], bias.slab(mt["layer"], B), pack=mt["spack"])
    dn0, dwqkv = _linear_bwd(dqkv, n0, wqkv, packed=pk)
    dln0 = _rms_bwd(xf, ln0, eps, dn0, dx)
    dtable = bias.fold(mt["table"].shape[0]) if mt["table"] is not None else None
    return denc, [dln0, dwqkv[:I], dwqkv[I:2 * I], dwqkv[2 * I:], dwo] + (cross if dec else []), dtable


class _BlockFn(torch.autograd.Function):
    """One T5Block.  x [B, S, D]; enc [B, Se, D] or None (encoder block).  Packed rows (meta["pack"], a PackedRows): an encoder
    block takes x [T, D], a decoder block enc [T, D] next to its dense x; every other step is token-wise.  params: ln0, q, k, v, o, [ln1, cq, ck, cv, co,] lnf, wi,
    wo, then block 0's bias table (or None: a later block, whose offset gradient block 0 folds)."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, enc, meta, *params):
        lnf, wi, wff = params[-4:-1]
        seeds = [modules._SeedCounter.next() for _ in range(6)]
        x2, saved, info = attn_half_fwd(x, enc, meta, params[:-4], seeds)
        p = info["p"]
        # feed forward: x + dropout(wo(dropout(relu(wi(norm(x))))))
        n2 = _rms(x2, lnf, meta["eps"])
        pre = _linear(n2, wi)
        act = torch.empty_like(pre)
        ops.bias_act_fwd(pre, meta["zero_bias"], ops.ACTIVATIONS["relu"], act)
        actd = dropout_fwd(act, p, seeds[4])
        x3 = add_dropout(x2, _linear(actd, wff), p, seeds[5])
        saved += [lnf, wi, wff, n2, pre, actd]
        ctx.save_for_backward(*saved, meta["keep"])
        ctx.meta = dict(meta, table=params[-1], **info)
        return x3.view(x.shape)

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        sv = list(ctx.saved_tensors)
        mt = ctx.meta
        B, S, D = mt["shape"]
        T, eps, p, seeds, dec = sv[0].shape[0], mt["eps"], mt["p"], mt["seeds"], mt["dec"]
        pk = mt["spack"] is not None                                              # a packed encoder block: T differs in every batch
        keep_mask = sv.pop()
        lnf, wi, wff, n2, pre, actd = sv[-6:]
        x2 = sv[19] if dec else sv[7]
        dev = sv[0].device
        dx = dout.reshape(T, D).contiguous().float().clone()                      # the gradient of the residual stream, added to in place
        # feed forward
        df = _dropout_bwd(dx, D, p, seeds[5])
        dactd, dwff = _linear_bwd(df, actd, wff, packed=pk)
        dact = _dropout_bwd(dactd, dactd.shape[1], p, seeds[4])
        ops.bias_act_bwd(pre, dact, ops.ACTIVATIONS["relu"], dact, torch.empty(_N_PARTIAL, pre.shape[1], **_f32(dev)))
        dn2, dwi = _linear_bwd(dact, n2, wi, packed=pk)
        dlnf = _rms_bwd(x2, lnf, eps, dn2, dx)
        denc, agrads, dtable = attn_half_bwd(sv[:-6], mt, dx, keep_mask)
        return (dx.view(dout.shape), denc, None, *agrads, dlnf, dwi, dwff, dtable)


class _FinalNormFn(torch.autograd.Function):
    """dropout(RMSNorm(x)) * scale"""

    @staticmethod
    def forward(ctx, x, w, eps, p, seed, scale):
        xf = x.reshape(-1, x.shape[-1]).contiguous().float()
        y = dropout_fwd(_rms(xf, w, eps), p, seed)
        ctx.meta = (eps, p, seed, scale, x.shape)
        ctx.save_for_backward(xf, w)
        return (y * scale if scale != 1.0 else y).view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        xf, w = ctx.saved_tensors
        eps, p, seed, scale, shape = ctx.meta
        g = dy.reshape(xf.shape).contiguous().float()
        g = _dropout_bwd(g * scale if scale != 1.0 else g, xf.shape[1], p, seed)
        dx = torch.zeros_like(xf)
        dw = _rms_bwd(xf, w, eps, g, dx)
        return dx.view(shape), dw, None, None, None, None


class TIGER(nn.Module):
    def __init__(self, config: TigerConfig):
        super().__init__()
        c = config
        if c.feed_forward_proj != "relu":
            raise NotImplementedError(f"TIGER on the HIP path: feed_forward_proj 'relu' only (got {c.feed_forward_proj!r})")
        if not c.tie_word_embeddings:
            raise NotImplementedError("TIGER on the HIP path: tie_word_embeddings=False is not built (the head is the shared table)")
        if c.d_kv not in ops.T5_HEAD_DIMS or c.num_heads > ops.T5_MAX_H or c.num_heads < 1:
            raise NotImplementedError(f"TIGER on the HIP path: d_kv in {ops.T5_HEAD_DIMS}, num_heads <= {ops.T5_MAX_H} "
                                      f"(got d_kv={c.d_kv}, num_heads={c.num_heads})")
        if c.d_model % 4 or c.d_model > 256 or c.d_ff % 4:
            raise NotImplementedError(f"TIGER on the HIP path: d_model <= 256, d_model and d_ff divisible by 4 (got {c.d_model}, {c.d_ff})")
        self.config = c
        self.model_dim = c.d_model
        self.temperature = 1.0
        self.shared = nn.Embedding(c.vocab_size, c.d_model)
        self.encoder = T5Stack(c, self.shared, False)
        self.decoder = T5Stack(c, self.shared, True)
        self.lm_head = nn.Linear(c.d_model, c.vocab_size, bias=False)
        self.lm_head.weight = self.shared.weight
        self.register_buffer("_zero_bias", torch.zeros(c.d_ff), persistent=False)
        self._buckets = {}
        self.apply(self._init_weights)

    def _init_weights(self, m: nn.Module):
        """HF T5PreTrainedModel._init_weights: the per-tensor standard deviations (not its random stream)"""
        c = self.config
        f = c.initializer_factor
        if isinstance(m, T5LayerNorm):
            m.weight.data.fill_(f * 1.0)
        elif isinstance(m, TIGER):
            m.shared.weight.data.normal_(mean=0.0, std=f * 1.0)
        elif isinstance(m, T5DenseActDense):
            m.wi.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)
            m.wo.weight.data.normal_(mean=0.0, std=f * c.d_ff ** -0.5)
        elif isinstance(m, T5Attention):
            m.q.weight.data.normal_(mean=0.0, std=f * (c.d_model * c.d_kv) ** -0.5)
            m.k.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)
            m.v.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)
            m.o.weight.data.normal_(mean=0.0, std=f * (c.num_heads * c.d_kv) ** -0.5)
            if hasattr(m, "relative_attention_bias"):
                m.relative_attention_bias.weight.data.normal_(mean=0.0, std=f * c.d_model ** -0.5)

    # ---- HF surface ------------------------------------------------------------------------------------------------------------
    def set_hyper(self, temperature: float):
        self.temperature = temperature

    def resize_token_embeddings(self, n: int) -> nn.Embedding:
        """A table of n rows that keeps the first min(n, old) rows; new rows are drawn as HF draws them (normal(0, factor))."""
        old = self.shared.weight
        if n != old.shape[0]:
            new = nn.Embedding(n, old.shape[1]).to(device=old.device, dtype=old.dtype)
            new.weight.data.normal_(mean=0.0, std=self.config.initializer_factor * 1.0)
            keep = min(n, old.shape[0])
            new.weight.data[:keep] = old.data[:keep]
            self.shared = new
            self.encoder.embed_tokens = self.decoder.embed_tokens = new
            self.lm_head = nn.Linear(old.shape[1], n, bias=False)
            self.lm_head.weight = new.weight
            self.config.vocab_size = n
        return self.shared

    def _shift_right(self, labels: torch.Tensor) -> torch.Tensor:
        c = self.config
        shifted = labels.new_zeros(labels.shape)
        shifted[..., 1:] = labels[..., :-1].clone()
        shifted[..., 0] = c.decoder_start_token_id
        shifted.masked_fill_(shifted == -100, c.pad_token_id)
        return shifted

    # ---- the stacks ------------------------------------------------------------------------------------------------------------
    def _bucket(self, S: int, bidirectional: bool, device) -> torch.Tensor:
        key = (S, bidirectional, str(device))
        if key not in self._buckets:
            c = self.config
            t = bucket_vector(S, bidirectional, c.relative_attention_num_buckets, c.relative_attention_max_distance)
            if int(t.min()) < 0 or int(t.max()) >= c.relative_attention_num_buckets:
                raise IndexError(f"relative position buckets outside [0, {c.relative_attention_num_buckets})")
            self._buckets[key] = t.to(device)
        return self._buckets[key]

    def _check(self, ids: torch.Tensor, limit: int, what: str):
        if not ids.is_cuda:
            raise RuntimeError("gamer_amd.tiger runs on the HIP device only (no CPU fallback)")
        if ids.dim() != 2 or ids.shape[1] < 1 or ids.shape[1] > limit:
            raise NotImplementedError(f"TIGER on the HIP path: {what} length in [1, {limit}] (got {tuple(ids.shape)})")

    # the feed-forward layer of a block is the model's own: a model built on this stack (gamer_amd.pbatransformer) overrides these
    def _route(self, stack, ids):
        """what the feed-forward layers of a stack call need to know about its ids [B, S] (here: nothing)"""
        return None

    def _block(self, stack, l, x, enc, meta, attn_params, table, route):
        ff = stack.block[l].layer[-1]
        return _BlockFn.apply(x, enc, meta, *attn_params, ff.layer_norm.weight, ff.DenseReluDense.wi.weight, ff.DenseReluDense.wo.weight,
                              table)

    def _eval_ffn_weights(self, stack, l) -> dict:
        """the feed-forward weights of decoder block l as _DecoderEval keeps them for a search"""
        ff = stack.block[l].layer[-1]
        return dict(lnf=ff.layer_norm.weight.detach(), wi=ff.DenseReluDense.wi.weight.detach(), wff=ff.DenseReluDense.wo.weight.detach())

    def _eval_ffn(self, x, L, route):
        """x + wo(relu(wi(norm(x)))) on the rows x [N S, D] of a search step; L: the layer's _DecoderEval entry"""
        pre = _linear(_rms(x, L["lnf"], self.config.layer_norm_epsilon), L["wi"])
        act = torch.empty_like(pre)
        ops.bias_act_fwd(pre, self._zero_bias, ops.ACTIVATIONS["relu"], act)
        return add_dropout(x, _linear(act, L["wff"]), 0.0, 0)

    def _stack(self, stack: T5Stack, ids, keep, enc=None, shared=None, pack=None):
        """keep: uint8 [B, Se] over the ENCODER tokens (the encoder's own keys, the decoder's cross-attention keys).  ``pack``
        (PackedRows, keep = None): the encoder runs on the [T] kept tokens of ids [B, S] and returns [T, D]; the decoder takes
        enc [T, D]"""
        c = self.config
        p = c.dropout_rate if self.training else 0.0
        B, S = ids.shape
        ids = ids.long().contiguous()
        if pack is not None and not stack.is_decoder:
            ids = ids.reshape(-1)[pack.rows][None, :].contiguous()
        x = EmbedDropoutFn.apply(ids, stack.embed_tokens.weight, p, _next_seed(), shared, -1)
        if pack is not None and not stack.is_decoder:
            x = x[0]
        blk0 = stack.block[0].layer[0].SelfAttention
        table = blk0.relative_attention_bias.weight
        bias = _BiasStack(table, self._bucket(S, not stack.is_decoder, ids.device), S, len(stack.block))
        route = self._route(stack, ids)
        for l, blk in enumerate(stack.block):
            meta = dict(heads=c.num_heads, d_kv=c.d_kv, eps=c.layer_norm_epsilon, dropout=c.dropout_rate, training=self.training,
                        bias=bias, keep=keep, layer=l, zero_bias=self._zero_bias, pack=pack)
            a = blk.layer[0]
            params = [a.layer_norm.weight, a.SelfAttention.q.weight, a.SelfAttention.k.weight, a.SelfAttention.v.weight,
                      a.SelfAttention.o.weight]
            if stack.is_decoder:
                x_ = blk.layer[1]
                e = x_.EncDecAttention
                params += [x_.layer_norm.weight, e.q.weight, e.k.weight, e.v.weight, e.o.weight]
            x = self._block(stack, l, x, enc, meta, params, table if l == 0 else None, route)
        scale = c.d_model ** -0.5 if stack.is_decoder else 1.0
        return _FinalNormFn.apply(x, stack.final_layer_norm.weight, c.layer_norm_epsilon, p, _next_seed(), scale)

    def _pack(self, input_ids, attention_mask, lengths) -> PackedRows:
        """the packed form of a batch: from ``lengths`` (CPU int [B]) without any copy from the device, else from the mask"""
        B, S = input_ids.shape
        if lengths is None:
            lengths = torch.full((B,), S, dtype=torch.int64) if attention_mask is None else packed_lengths(attention_mask)
        return PackedRows.build(lengths, B, S, input_ids.device)

    def encode(self, input_ids, attention_mask=None, packed=False, lengths=None):
        """(encoder output [B, Se, D], keep uint8 [B, Se]); ``packed=True``: (encoder output [T, D] without the padding tokens, the
        PackedRows of the batch, whose ``off`` holds k_start)"""
        self._check(input_ids, MAX_LONG_ENCODER_LEN, "encoder")
        if packed:
            pack = self._pack(input_ids, attention_mask, lengths)
            return self._stack(self.encoder, input_ids, None, pack=pack), pack
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        keep = (attention_mask.to(input_ids.device) != 0).to(torch.uint8).contiguous()
        return self._stack(self.encoder, input_ids, keep), keep

    def decode(self, decoder_input_ids, enc, keep, shared=None, pack=None):
        """the decoder's output rows, already scaled by d_model ** -0.5: [B, T, D]"""
        self._check(decoder_input_ids, MAX_DECODER_LEN, "decoder")
        return self._stack(self.decoder, decoder_input_ids, keep, enc, shared, pack)

    def logits(self, dec_out: torch.Tensor) -> torch.Tensor:
        """the materialised logits [B, T, V] of decoder rows (no gradient: tests and decoding)"""
        B, T, D = dec_out.shape
        V = self.shared.weight.shape[0]
        out = torch.empty(B * T, V, **_f32(dec_out.device))
        with ops.f32_matmul("f32"):
            ops.linear_fwd(dec_out.detach().reshape(B * T, D).contiguous(), D, self.shared.weight.detach(), D, out, V, B * T, V, D)
        return out.view(B, T, V)

    def forward(self, input_ids, attention_mask=None, labels=None, decoder_input_ids=None, want_logits=None, packed=False,
                lengths=None, **kwargs):
        """(loss, logits).  With labels the loss is the mean over the positions with label != -100 of CE(logits / temperature); the
        logits are formed only without labels or with ``want_logits=True`` (default: formed when no gradient is recorded).
        ``packed=True``: the encoder side runs on the sum of the rows' token counts, without the padding tokens (right-padded masks
        only); ``lengths`` (CPU int [B]) spares the one copy of B integers that reading them from the mask costs."""
        for name in ("head_mask", "decoder_head_mask", "cross_attn_head_mask", "inputs_embeds", "decoder_inputs_embeds",
                     "output_attentions", "output_hidden_states", "past_key_values", "encoder_outputs", "decoder_attention_mask"):
            if kwargs.pop(name, None) not in (None, False):
                raise NotImplementedError(f"TIGER on the HIP path: {name} is not supported")
        kwargs.pop("split", None), kwargs.pop("use_cache", None), kwargs.pop("return_dict", None), kwargs.pop("cache_position", None)
        if kwargs:
            raise TypeError(f"TIGER.forward: unexpected arguments {sorted(kwargs)}")
        if labels is not None and decoder_input_ids is None:
            decoder_input_ids = self._shift_right(labels.to(input_ids.device))
        if decoder_input_ids is None:
            raise ValueError("You have to specify either decoder_input_ids or labels")
        train = labels is not None and torch.is_grad_enabled()
        shared = _SharedGrad(gathers=2) if train and self.shared.weight.requires_grad else None
        # (the encoder's gather is the other user of the table's gradient buffer: it gets the same hand-over object)
        self._check(input_ids, MAX_LONG_ENCODER_LEN, "encoder")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if packed:
            keep, pack = None, self._pack(input_ids, attention_mask, lengths)
        else:
            keep, pack = (attention_mask.to(input_ids.device) != 0).to(torch.uint8).contiguous(), None
        enc = self._stack(self.encoder, input_ids, keep, shared=shared, pack=pack)
        out = self.decode(decoder_input_ids.to(input_ids.device), enc, keep, shared, pack)
        loss = None
        if labels is not None:
            flat = labels.to(input_ids.device).long().flatten()
            rows = (flat != -100).nonzero()[:, 0].contiguous()
            if rows.numel() == 0:
                loss = out.sum() * 0.0 + float("nan")                           # CrossEntropyLoss over no rows
            else:
                loss = CatalogCEFn.apply(out * (1.0 / self.temperature), rows, self.shared.weight, flat[rows].contiguous(), shared)
        if want_logits is None:
            want_logits = not train
        return loss, (self.logits(out) if want_logits else None)


# ---- decoding ----------------------------------------------------------------------------------------------------------------------
class _DecoderEval:
    """The decoder without autograd for beam search: the concatenated weights once per search, the cross-attention keys / values
    once per USER and layer; a beam row reads its user's copy through the attention kernel's row map."""

    def __init__(self, model: "TIGER", enc: torch.Tensor, keep):
        """enc [B, Se, D] with keep uint8 [B, Se], or the packed encoder output [T, D] with its PackedRows"""
        c = model.config
        self.pack = keep if isinstance(keep, PackedRows) else None
        if self.pack is not None:
            self.model, self.keep, self.users, self.Se = model, None, self.pack.off.n, self.pack.S
        else:
            self.model, self.keep, self.users, self.Se = model, keep, enc.shape[0], enc.shape[1]
        ef = enc.reshape(-1, c.d_model).contiguous()
        self.layers = []
        with ops.f32_matmul("f32"):
            for l, blk in enumerate(model.decoder.block):
                a, e = blk.layer[0], blk.layer[1]
                cat = lambda *ws: torch.cat([w.weight.detach() for w in ws], 0).contiguous()
                self.layers.append(dict(
                    ln0=a.layer_norm.weight.detach(), wqkv=cat(a.SelfAttention.q, a.SelfAttention.k, a.SelfAttention.v),
                    wo=a.SelfAttention.o.weight.detach(), ln1=e.layer_norm.weight.detach(), cq=e.EncDecAttention.q.weight.detach(),
                    kv=_linear(ef, cat(e.EncDecAttention.k, e.EncDecAttention.v)), co=e.EncDecAttention.o.weight.detach(),
                    **model._eval_ffn_weights(model.decoder, l)))

    @ops.scoped_f32_matmul(lambda *a: "f32")
    def last_rows(self, ids: torch.Tensor, kv_rows: torch.Tensor) -> torch.Tensor:
        """the decoder output at the last position of ids [N, S], scaled for the tied head: [N, D]; kv_rows int32 [N]: the user"""
        m, c = self.model, self.model.config
        N, S = ids.shape
        h, d, eps, dev = c.num_heads, c.d_kv, c.layer_norm_epsilon, ids.device
        I = h * d
        x = torch.empty(N * S, c.d_model, **_f32(dev))
        ops.embedding_fwd(ids.contiguous(), m.shared.weight.detach(), x)
        table = m.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        rel = _BiasStack(table, m._bucket(S, False, dev), S, len(self.layers)).rel
        lse = torch.empty(N, h, S, **_f32(dev))
        xpack = (self.pack.dense_offsets(N, S, dev), self.pack.off) if self.pack is not None else None
        route = m._route(m.decoder, ids)
        for L in self.layers:
            qkv = _linear(_rms(x, L["ln0"], eps), L["wqkv"])
            c0 = torch.empty(N * S, I, **_f32(dev))
            _attn_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, N, S, S, h, d, True, 0.0, 0, c0, lse)
            x = add_dropout(x, _linear(c0, L["wo"]), 0.0, 0)
            q1 = _linear(_rms(x, L["ln1"], eps), L["cq"])
            c1 = torch.empty(N * S, I, **_f32(dev))
            _attn_fwd(q1, L["kv"][:, :I], L["kv"][:, I:], None, self.keep, N, S, self.Se, h, d, False, 0.0, 0, c1, lse,
                      kv_rows=kv_rows, kv_batch=self.users, pack=xpack)
            x = add_dropout(x, _linear(c1, L["co"]), 0.0, 0)
            x = m._eval_ffn(x, L, route)
        last = x.view(N, S, -1)[:, -1, :].contiguous()
        return _rms(last, m.decoder.final_layer_norm.weight.detach(), eps) * (c.d_model ** -0.5)

    @ops.scoped_f32_matmul(lambda *a: "f32")
    def all_rows(self, ids: torch.Tensor, per_user: int) -> torch.Tensor:
        """the decoder output at EVERY position of ids [N, S], scaled for the tied head: [N, S, D].  The rows are user-major, N =
        users x per_user: user b owns rows b per_user .. (score_items' candidates).  The cross attention of a user's per_user x S
        query rows shares one staged copy of its K / V (gamer_t5_attn_candidates); encoders beyond ops.T5_MAX_S run on the
        key-streaming kernels through the row map, as last_rows does."""
        m, c = self.model, self.model.config
        N, S = ids.shape
        if N != self.users * per_user:
            raise ValueError(f"all_rows: {N} rows are not {self.users} users x {per_user}")
        h, d, eps, dev = c.num_heads, c.d_kv, c.layer_norm_epsilon, ids.device
        I = h * d
        x = torch.empty(N * S, c.d_model, **_f32(dev))
        ops.embedding_fwd(ids.contiguous(), m.shared.weight.detach(), x)
        table = m.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        rel = _BiasStack(table, m._bucket(S, False, dev), S, len(self.layers)).rel
        lse = torch.empty(N, h, S, **_f32(dev))
        long = self.Se > ops.T5_MAX_S
        if long:
            kv_rows = (torch.arange(N, device=dev, dtype=torch.int32) // per_user).contiguous()
            xpack = (self.pack.dense_offsets(N, S, dev), self.pack.off) if self.pack is not None else None
        route = m._route(m.decoder, ids)
        for L in self.layers:
            qkv = _linear(_rms(x, L["ln0"], eps), L["wqkv"])
            c0 = torch.empty(N * S, I, **_f32(dev))
            _attn_fwd(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], rel, None, N, S, S, h, d, True, 0.0, 0, c0, lse)
            x = add_dropout(x, _linear(c0, L["wo"]), 0.0, 0)
            q1 = _linear(_rms(x, L["ln1"], eps), L["cq"])
            c1 = torch.empty(N * S, I, **_f32(dev))
            if long:
                _attn_fwd(q1, L["kv"][:, :I], L["kv"][:, I:], None, self.keep, N, S, self.Se, h, d, False, 0.0, 0, c1, lse,
                          kv_rows=kv_rows, kv_batch=self.users, pack=xpack)
            else:
                ops.t5_attn_candidates(q1, L["kv"][:, :I], L["kv"][:, I:], self.keep, self.users, per_user * S, self.Se, h, d, c1,
                                       k_off=self.pack.off if self.pack is not None else None)
            x = add_dropout(x, _linear(c1, L["co"]), 0.0, 0)
            x = m._eval_ffn(x, L, route)
        return (_rms(x, m.decoder.final_layer_norm.weight.detach(), eps) * (c.d_model ** -0.5)).view(N, S, -1)


@torch.no_grad()
def beam_search(model: TIGER, input_ids, attention_mask, trie, num_beams: int, max_new_tokens: int, decoder_prefix=None, packed=False,
                lengths=None):
    """Trie-constrained beam search as ``generate(..., num_beams=k, num_return_sequences=k, prefix_allowed_tokens_fn=...,
    early_stopping=True)`` runs it for ref:SeqRec/tasks/test_decoder.py and test_SMB_decoder.py.  ``trie``: a decode.ItemTrie over
    the full decoder sequences ([decoder_start] + ...), every one of them ``len(prefix) + max_new_tokens`` tokens long (so all
    hypotheses end at the same step, with </s> when the trie holds it).  ``decoder_prefix``: int64 [P] or [B, P], default
    [decoder_start_token_id].  Returns (sequences [B num_beams, P + max_new_tokens], sequences_scores [B num_beams]), the beams of
    user b at rows b num_beams .., best first; score = sum of log-probabilities / max_new_tokens (length_penalty 1 over the
    generated tokens).  The encoder and the cross-attention keys / values run once per user; a beam row reads its user's copy
    (row -> user map of gamer_t5_attn_fwd).  The decoder re-runs its at most 8 tokens every step: no self-attention cache."""
    dev = input_ids.device
    c = model.config
    B = input_ids.shape[0]
    nb, K = num_beams, 2 * num_beams
    N = B * nb
    V = model.shared.weight.shape[0]
    if decoder_prefix is None:
        decoder_prefix = torch.full((B, 1), c.decoder_start_token_id, dtype=torch.int64)
    prefix = torch.as_tensor(decoder_prefix, dtype=torch.int64).to(dev)
    if prefix.dim() == 1:
        prefix = prefix[None, :].expand(B, -1)
    prefix = prefix.contiguous()
    P = prefix.shape[1]
    if P < 1 or P + max_new_tokens - 1 > MAX_DECODER_LEN:
        raise NotImplementedError(f"tiger.beam_search: 1 <= prefix and prefix + new tokens <= {MAX_DECODER_LEN + 1}")
    was_training = model.training
    model.eval()
    try:
        enc, keep = model.encode(input_ids, attention_mask, packed, lengths)     # (packed: keep is the batch's PackedRows)
        dec = _DecoderEval(model, enc, keep)
        seqs = prefix[:, None, :].expand(B, nb, P).contiguous()
        run_scores = torch.zeros(B, nb, device=dev)
        run_scores[:, 1:] = -1e9                                                  # only beam 0 is live at the first step (HF)
        node = torch.zeros(N, dtype=torch.int32, device=dev)
        nxt = torch.empty_like(node)
        for t in range(P):
            ops.trie_advance(node, prefix[:, t].repeat_interleave(nb).contiguous(), trie.child_start, trie.child_tok, trie.child_node, nxt)
            node, nxt = nxt.clone(), nxt
        scores = torch.empty(N, V, device=dev)
        users = torch.arange(B, device=dev, dtype=torch.int32)
        beam_user = users.repeat_interleave(nb).contiguous()
        E = model.shared.weight.detach()
        final = None
        for step in range(max_new_tokens):
            cur = P + step
            if step == 0:                                                         # every beam of a user holds the same prefix
                last, rows = dec.last_rows(prefix, users), beam_user
            else:
                last, rows = dec.last_rows(seqs.reshape(N, cur), beam_user), torch.arange(N, device=dev, dtype=torch.int32)
            logits2d = torch.empty(last.shape[0], V, **_f32(dev))
            with ops.f32_matmul("f32"):
                ops.linear_fwd(last, last.shape[1], E, E.shape[1], logits2d, V, last.shape[0], V, E.shape[1])
            ops.trie_logprobs(logits2d, rows, run_scores.reshape(N).contiguous(), node, trie.child_start, trie.child_tok, V, scores)
            top_s, top_i = torch.topk(scores.view(B, nb * V), K)
            beam_i, tok = top_i // V, top_i % V
            cand = torch.cat([torch.gather(seqs, 1, beam_i[:, :, None].expand(B, K, cur)), tok[:, :, None]], 2)
            if step == max_new_tokens - 1:
                final = (cand[:, :nb].reshape(N, cur + 1), (top_s[:, :nb] / max_new_tokens).reshape(N))
                break
            seqs = cand[:, :nb].contiguous()
            run_scores = top_s[:, :nb].contiguous()
            parent = (beam_i[:, :nb] + torch.arange(B, device=dev)[:, None] * nb).reshape(N)
            ops.trie_advance(node[parent].contiguous(), tok[:, :nb].reshape(N).contiguous(), trie.child_start, trie.child_tok,
                             trie.child_node, nxt)
            node, nxt = nxt.clone(), nxt
        return final
    finally:
        model.train(was_training)


_LOGIT_FLOATS = 1 << 28            # score_items forms at most this many logits at a time (1 GiB of fp32)


@torch.no_grad()
def score_items(model: TIGER, input_ids, attention_mask, items, decoder_prefix=None, packed=False, lengths=None,
                max_rows: int = 65536) -> torch.Tensor:
    """Log-likelihood of GIVEN items after every user's history: scores [B, C] fp32,
    scores[b, c] = (1 / T) * sum_t log_softmax(logits_t)[items[.., c, t]] over the whole vocabulary, on the logits ``beam_search``
    forms (the decoder output scaled by d_model ** -0.5 against the tied table, no temperature) - what ``beam_search`` returns as
    ``sequences_scores`` for the same tokens.  ``items``: int64 [C, T] - one list for every user - or [B, C, T], a list per user;
    the T tokens are those ``beam_search`` generates (``max_new_tokens`` of them, </s> included where the trie carries it).
    ``decoder_prefix``, ``packed`` and ``lengths`` as in ``beam_search``.
    The encoder and the cross-attention K | V of every decoder layer run ONCE per user; the candidates go through the decoder
    teacher-forced ([prefix | item tokens but the last], P + T - 1 <= MAX_DECODER_LEN positions) in balanced chunks of at most
    ``max_rows // B`` per user, the last one padded by repeating the last candidate.  One decoder pass per chunk gives every scored
    position (_DecoderEval.all_rows: cross attention on gamer_t5_attn_candidates, the key-streaming kernels beyond 128 encoder
    tokens).  Token 0 depends on the prefix alone and is scored from one row per user; the log-probabilities come from
    gamer_token_logprob (per-row LSE + pick, no [N, V] log-softmax)."""
    items = torch.as_tensor(items)
    if items.dim() not in (2, 3) or items.dtype != torch.int64:
        raise ValueError(f"score_items: items must be int64 [C, T] or [B, C, T], got {items.dtype} {tuple(items.shape)}")
    if input_ids.dim() != 2:
        raise ValueError(f"score_items: input_ids [B, S] (got {tuple(input_ids.shape)})")
    B = input_ids.shape[0]
    if items.dim() == 3 and items.shape[0] != B:
        raise ValueError(f"score_items: items [B, C, T] has {items.shape[0]} lists for {B} users")
    C, T = items.shape[-2:]
    if C < 1 or T < 1:
        raise ValueError(f"score_items: empty item list {tuple(items.shape)}")
    if max_rows < B:
        raise ValueError(f"score_items: max_rows = {max_rows} < {B} users (one candidate per user is the smallest chunk)")
    dev = input_ids.device
    c = model.config
    if decoder_prefix is None:
        decoder_prefix = torch.full((B, 1), c.decoder_start_token_id, dtype=torch.int64)
    prefix = torch.as_tensor(decoder_prefix, dtype=torch.int64)
    if prefix.dim() == 1:
        prefix = prefix[None, :].expand(B, -1)
    if prefix.dim() != 2 or prefix.shape[0] != B:
        raise ValueError(f"score_items: decoder_prefix [P] or [{B}, P] (got {tuple(prefix.shape)})")
    P = prefix.shape[1]
    S = P + T - 1
    if P < 1 or S > MAX_DECODER_LEN:
        raise NotImplementedError(f"tiger.score_items: 1 <= prefix and prefix + item tokens <= {MAX_DECODER_LEN + 1}")
    was_training = model.training
    model.eval()
    try:
        enc, keep = model.encode(input_ids, attention_mask, packed, lengths)     # (packed: keep is the batch's PackedRows)
        dec = _DecoderEval(model, enc, keep)
        prefix = prefix.to(dev).contiguous()
        it = items.to(dev)
        if it.dim() == 2:
            it = it[None].expand(B, C, T)
        E = model.shared.weight.detach()
        V, D = E.shape
        n_chunks = -(-C // max(1, max_rows // B))
        chunk = -(-C // n_chunks)                                  # (balanced: the last chunk is padded by < n_chunks candidates)
        N = B * chunk
        user = (torch.arange(N, device=dev, dtype=torch.int32) // chunk).contiguous()
        first = torch.arange(B, device=dev) * chunk
        out = torch.empty(B, n_chunks * chunk, **_f32(dev))
        acc = torch.empty(N, **_f32(dev))
        step = max(B, min(N, _LOGIT_FLOATS // V))
        logits = torch.empty(step, V, **_f32(dev))

        def head(rows):
            with ops.f32_matmul("f32"):
                ops.linear_fwd(rows, D, E, D, logits, V, rows.shape[0], V, D)

        for ci in range(n_chunks):
            c0 = ci * chunk
            cols = torch.arange(c0, c0 + chunk, device=dev).clamp_(max=C - 1)      # (the last chunk repeats the last candidate)
            tok = it.index_select(1, cols).reshape(N, T)
            ids = torch.cat([prefix[:, None, :].expand(B, chunk, P).reshape(N, P), tok[:, :T - 1]], 1).contiguous()
            x = dec.all_rows(ids, chunk)                                            # [N, S, D]
            tok = tok.t().contiguous()                                              # [T, N]
            # token 0: position P - 1 sees the prefix alone, the same row for every candidate of a user
            head(x[first, P - 1, :].contiguous())
            ops.token_logprob(logits, user, tok[0], V, acc)
            for t in range(1, T):
                xt = x[:, P - 1 + t, :]
                for n0 in range(0, N, step):
                    n1 = min(N, n0 + step)
                    head(xt[n0:n1].contiguous())
                    ops.token_logprob(logits, None, tok[t, n0:n1], V, acc[n0:n1], accumulate=True)
            out[:, c0:c0 + chunk] = acc.view(B, chunk)
        return out[:, :C] / T
    finally:
        model.train(was_training)
