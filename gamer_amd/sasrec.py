"""SASRec, the first discriminative baseline of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface and parameter names as the reference (ref:SeqRec/models/discriminative/SASRec/model.py,
ref:SeqRec/modules/model_base/seq_model.py): ``item_embedding`` [n_items + 1, H], ``position_embedding`` [max_his_len, H],
``trm_encoder.layer.{l}.*`` (``gamer_amd.modules``), ``LayerNorm``.  A reference ``best_model.pth`` state dict loads here and
one saved here loads into the reference class.

Every step runs as HIP kernels, with no PyTorch fallback:
  input block   dropout(LayerNorm(item_emb[ids] + pos_emb[s]))   gamer_seq_embed_ln_fwd; backward: gamer_residual_dropout_bwd,
                gamer_layernorm_bwd, gamer_embedding_bwd_large (any table size, padding row skipped), gamer_position_bwd
  encoder       gamer_amd.modules.TransformerEncoder
  head          nn.CrossEntropyLoss()(h @ E^T, target) on the last valid position of each row: gamer_catalog_ce_fwd / _bwd,
                which never write the [B, n_items + 1] scores
  ranking       full_sort_topk: gamer_catalog_topk (scores never materialised); full_sort_predict builds the full score matrix
                as the reference does (small catalogues, tests)

Reference behaviour kept on purpose:
  * ``self.apply(_init_weights)`` draws the whole item table from normal(0, 0.02), row 0 included, so the padding row is not
    zero.  The input gather gives row 0 no gradient (padding_idx), the head does: it takes part in the softmax and the ranking.
  * The attention mask is causal plus key padding (``get_attention_mask``, additive finfo.min) on right-padded rows.
  * Every layer's FeedForward returns dense_2(act(dense_1(x))) with no residual (see gamer_amd.modules).
  * Dropout uses the project's counter-based hash masks, not torch's generator: the same seed gives the same bits, but the
    masks differ from the reference's.  Parity with the reference is checked with dropout off.
"""
from __future__ import annotations

import dataclasses
import json
import os

import torch
from torch import nn

from . import modules, ops


@dataclasses.dataclass
class SASRecConfig:
    """The keys and defaults of the reference's SASRecConfig (config/dis-models/SASRec/config.json)."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 128
    inner_size: int = 256
    dropout_prob: float = 0.5
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    loss_type: str = "CE"

    @classmethod
    def from_dict(cls, d: dict) -> "SASRecConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        unknown = set(d) - names
        if unknown:
            raise ValueError(f"SASRecConfig: unknown keys {sorted(unknown)}")
        return cls(**d)

    @classmethod
    def from_pretrained(cls, path: str) -> "SASRecConfig":
        f = os.path.join(path, "config.json")
        if not os.path.exists(f):
            raise ValueError(f"Can't find a configuration file at {f}.")
        with open(f, encoding="utf-8") as fh:
            return cls.from_dict(json.load(fh))

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)


class _Seeds:
    value = 0x5A5E


def _next_seed() -> int:
    _Seeds.value += 1
    return _Seeds.value


class _SharedGrad:
    """The item table's gradient buffer of one calculate_loss call: the head's backward (which runs first) writes its dE into
    it and returns no gradient for the table; the input block's backward accumulates the gather's rows into the same buffer
    and returns it - one [V, H] tensor instead of two plus autograd's sum."""

    def __init__(self):
        self.dE = None


class _InputBlockFn(torch.autograd.Function):
    """dropout(LayerNorm(E[ids] + P[s])) for ids [B, S]; gradients of E (padding row 0 skipped), P, the LayerNorm."""

    @staticmethod
    def forward(ctx, ids, E, P, w, b, eps, p, seed, shared=None):
        B, S = ids.shape
        H = E.shape[1]
        f32 = dict(dtype=torch.float32, device=E.device)
        v, y = torch.empty(B * S, H, **f32), torch.empty(B, S, H, **f32)
        mean, rstd = torch.empty(B * S, **f32), torch.empty(B * S, **f32)
        ops.seq_embed_ln_fwd(ids, E, P, w, b, eps, p, seed, v, y, mean, rstd)
        ctx.meta = (p, seed, E.shape, P.shape)
        ctx.shared = shared
        ctx.save_for_backward(ids, v, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, v, w, mean, rstd = ctx.saved_tensors
        p, seed, e_shape, p_shape = ctx.meta
        B, S = ids.shape
        H = v.shape[1]
        f32 = dict(dtype=torch.float32, device=v.device)
        g = dy.reshape(B * S, H).contiguous().float()
        if p > 0:
            gm = torch.empty_like(g)
            ops.residual_dropout_bwd(g, p, seed, gm)
            g = gm
        dv = torch.empty(B * S, H, **f32)
        pw, pb = torch.empty(modules._N_PARTIAL, H, **f32), torch.empty(modules._N_PARTIAL, H, **f32)
        ops.layernorm_bwd(v, w, mean, rstd, g, dv, pw, pb)
        dw, db = torch.empty(H, **f32), torch.empty(H, **f32)
        ops.colsum_reduce(pw, dw)
        ops.colsum_reduce(pb, db)
        dE = ctx.shared.dE if ctx.shared is not None and ctx.shared.dE is not None else torch.zeros(e_shape, **f32)
        if ctx.shared is not None:
            ctx.shared.dE = None
        ops.embedding_bwd_large(ids, dv, 0, dE)
        dP = torch.zeros(p_shape, **f32)
        ops.position_bwd(dv.view(B, S, H), dP[:S])
        return None, dE, dP, dw, db, None, None, None, None


class _CatalogCEFn(torch.autograd.Function):
    """mean over rows r of CE(out[rows[r]] @ E^T, target[r]): the [R, V] scores exist only as register tiles.  With ``bias`` (any
    shape holding V values; BERT4Rec's head) the scores are out @ E[:V]^T + bias and the bias gets its gradient."""

    @staticmethod
    def forward(ctx, out, rows, E, target, shared=None, bias=None, V=None):
        H = out.shape[-1]
        x = out.reshape(-1, H)
        R = rows.numel()
        f32 = dict(dtype=torch.float32, device=out.device)
        lse, loss = torch.empty(R, **f32), torch.empty((), **f32)
        bad = torch.zeros(1, dtype=torch.int32, device=out.device)
        if bias is None and V is None:
            ops.catalog_ce_fwd(x, rows, E, target, lse, loss, bad)
        else:
            ops.catalog_ce_bias_fwd(x, rows, E, None if bias is None else bias.detach().reshape(-1), target, lse, loss, bad, V)
        n_bad = int(bad.item())
        if n_bad:
            raise IndexError(f"SASRec.calculate_loss: {n_bad} target(s) outside [0, {E.shape[0] if V is None else V})")
        ctx.save_for_backward(x, rows, E, target, lse, bias)
        ctx.out_shape = out.shape
        ctx.shared = shared
        ctx.V = V
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, rows, E, target, lse, bias = ctx.saved_tensors
        dx = torch.zeros(ctx.out_shape, dtype=torch.float32, device=x.device)
        dE = torch.zeros_like(E)
        dbias = None
        if bias is None and ctx.V is None:
            ops.catalog_ce_bwd(x, rows, E, target, lse, dloss.float().contiguous(), 1.0 / rows.numel(), dE=dE, dh=dx)
        else:
            dbias = torch.empty_like(bias) if bias is not None and ctx.needs_input_grad[5] else None
            ops.catalog_ce_bias_bwd(x, rows, E, None if bias is None else bias.detach().reshape(-1), target, lse,
                                    dloss.float().contiguous(), 1.0 / rows.numel(), dE=dE, dh=dx,
                                    dbias=None if dbias is None else dbias.view(-1), V=ctx.V)
        if ctx.shared is not None:
            ctx.shared.dE = dE                   # the input block's backward adds the gather's rows and returns it
            return dx, None, None, None, None, dbias, None
        return dx, None, dE, None, None, dbias, None


class SASRec(nn.Module):
    def __init__(self, config: SASRecConfig, n_items: int, max_his_len: int, **kwargs):
        super().__init__()
        if config.loss_type == "BPR":
            raise NotImplementedError("SASRec: loss_type 'BPR' (negative-sampling tasks) is not supported on the HIP path")
        if config.loss_type != "CE":
            raise NotImplementedError("Make sure 'loss_type' in ['BPR', 'CE']!")
        if config.hidden_size % 4 or config.hidden_size > 256:
            raise NotImplementedError("SASRec on the HIP path: hidden_size % 4 == 0 and hidden_size <= 256")
        self.config = config
        self.n_items = n_items
        self.n_layers, self.n_heads = config.n_layers, config.n_heads
        self.hidden_size, self.inner_size = config.hidden_size, config.inner_size
        self.dropout_prob, self.hidden_act = config.dropout_prob, config.hidden_act
        self.layer_norm_eps, self.initializer_range = config.layer_norm_eps, config.initializer_range
        self.max_seq_length = max_his_len
        self.loss_type = config.loss_type
        self.item_embedding = nn.Embedding(n_items + 1, self.hidden_size, padding_idx=0)
        self.position_embedding = nn.Embedding(max_his_len, self.hidden_size)
        layer = modules.TransformerEncoderLayer(d_model=self.hidden_size, nhead=self.n_heads, dim_feedforward=self.inner_size,
                                                dropout=self.dropout_prob, activation=self.hidden_act,
                                                layer_norm_eps=self.layer_norm_eps)
        self.trm_encoder = modules.TransformerEncoder(encoder_layer=layer, num_layers=self.n_layers)
        self.LayerNorm = nn.LayerNorm(self.hidden_size, eps=self.layer_norm_eps)
        self.dropout = nn.Dropout(self.dropout_prob)
        self.apply(self._init_weights)

    def _init_weights(self, module: nn.Module):
        # as the reference: every Linear / Embedding weight from normal(0, initializer_range), the item table's row 0 included
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    def get_attention_mask(self, item_seq: torch.Tensor) -> torch.Tensor:
        """causal + key padding, additive finfo.min (SeqModel.get_attention_mask, bidirectional=False)"""
        keep = (item_seq != 0)[:, None, None, :].expand(-1, -1, item_seq.size(1), -1)
        keep = torch.tril(keep).float()
        return (1.0 - keep) * torch.finfo(torch.float32).min

    def _encode(self, item_seq: torch.Tensor, shared=None) -> torch.Tensor:
        if not item_seq.is_cuda:
            raise RuntimeError("gamer_amd.sasrec runs on the HIP device only (no CPU fallback)")
        if item_seq.size(1) > self.max_seq_length:
            raise ValueError(f"sequence length {item_seq.size(1)} > max_his_len {self.max_seq_length}")
        p = self.dropout_prob if self.training else 0.0
        x = _InputBlockFn.apply(item_seq.long().contiguous(), self.item_embedding.weight, self.position_embedding.weight,
                                self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps, p, _next_seed(), shared)
        return self.trm_encoder(x, self.get_attention_mask(item_seq))

    @staticmethod
    def _last_rows(item_seq, item_seq_len):
        B, S = item_seq.shape
        n = item_seq_len.to(item_seq.device).long()
        if n.shape != (B,) or int(n.min()) < 1 or int(n.max()) > S:
            raise IndexError(f"seq_len must hold {B} values in [1, {S}]")          # (the reference's gather raises too)
        return torch.arange(B, device=item_seq.device) * S + (n - 1)

    def forward(self, item_seq: torch.Tensor, item_seq_len: torch.Tensor) -> torch.Tensor:
        rows = self._last_rows(item_seq, item_seq_len)
        out = self._encode(item_seq)
        return out.reshape(-1, out.shape[-1])[rows]          # gather_indexes, [B, H]

    def calculate_loss(self, interaction: dict) -> torch.Tensor:
        item_seq = interaction["inputs"]
        rows = self._last_rows(item_seq, interaction["seq_len"])
        shared = _SharedGrad() if torch.is_grad_enabled() and self.item_embedding.weight.requires_grad else None
        out = self._encode(item_seq, shared)
        target = interaction["target"].to(item_seq.device).long().contiguous()
        return _CatalogCEFn.apply(out, rows, self.item_embedding.weight, target, shared)

    def full_sort_predict(self, interaction: dict) -> torch.Tensor:
        """[B, n_items + 1] scores as the reference builds them (-inf outside item_range); small catalogues and tests."""
        item_seq = interaction["inputs"]
        seq_output = self.forward(item_seq, interaction["seq_len"])
        emb = self.item_embedding.weight
        start, end = interaction["item_range"] if "item_range" in interaction else (0, emb.shape[0])
        B, H = seq_output.shape
        n = int(end) - int(start)
        part = torch.empty(B, n, dtype=torch.float32, device=item_seq.device)
        with ops.f32_matmul("f32"):
            ops.linear_fwd(seq_output.contiguous(), H, emb[start:end].detach(), H, part, n, B, n, H)
        scores = torch.full((B, self.n_items + 1), float("-inf"), device=item_seq.device)
        scores[:, start:end] = part
        return scores

    @torch.no_grad()
    def full_sort_topk(self, interaction: dict, k: int):
        """(indices [B, k], scores [B, k]) of the k best items (within item_range when given), as a stable argsort of the
        reference's full_sort_predict reads them; the scores are never materialised (gamer_catalog_topk)."""
        item_seq = interaction["inputs"]
        rows = self._last_rows(item_seq, interaction["seq_len"])
        out = self._encode(item_seq)
        start, end = interaction["item_range"] if "item_range" in interaction else (0, self.n_items + 1)
        return ops.catalog_topk(out, self.item_embedding.weight.detach(), k, int(start), int(end), row_idx=rows)
