"""GRU4Rec, the default backbone of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface and parameter names as the reference (ref:SeqRec/models/discriminative/GRU4Rec/model.py,
ref:SeqRec/modules/model_base/seq_model.py): ``item_embedding`` [n_items + 1, E], ``gru_layers`` (an ``nn.GRU(bias=False,
batch_first=True)`` used as the parameter container only: ``weight_ih_l{k}`` [3H, E or H], ``weight_hh_l{k}`` [3H, H]),
``dense`` [E, H] + [E].  A reference ``best_model.pth`` state dict loads here and one saved here loads into the reference class.

Every step runs as HIP kernels, with no PyTorch fallback (nn.GRU's forward is never called):
  input block   emb_dropout(E[ids])   gamer_embedding_fwd + gamer_residual_dropout_fwd; backward: gamer_residual_dropout_bwd,
                gamer_embedding_bwd_large (padding row skipped) into the head's item-table gradient
  GRU layer     gi = x W_ih^T (fp32 GEMM over B L rows), then gamer_gru_fwd: all L steps in one launch; backward: gamer_gru_bwd
                (one launch), dW_ih = dgi^T x, dW_hh = dgh_next^T h, dx = dgi W_ih (fp32 GEMMs)
  dense         on the gathered rows (position seq_len - 1) only: the only rows the output reads (rec_common.GatherLinearFn)
  head          rec_common's catalogue-wide CE (gamer_catalog_ce_fwd / _bwd) and top K (gamer_catalog_topk), one shared [V, E]
                item-table gradient

Reference behaviour kept on purpose:
  * ``GRU4RecConfig`` ignores unknown keys as the reference's pydantic model does: the shipped config.json spells
    ``num_layers`` / ``dropout_prob``, so the effective values are the class defaults n_layers = 1 and dropout = 0.3.
  * ``apply(_init_weights)`` draws the whole item table with xavier_normal_, row 0 included (the padding row is not zero), and
    applies xavier_uniform_ to weight_hh_l0 and weight_ih_l0 only: layers above 0 and ``dense`` keep PyTorch's default init.
  * Dropout uses the project's counter-based hash masks, not torch's generator: the same seed gives the same bits, but the
    masks differ from the reference's.  Parity with the reference is checked with dropout off.
"""
from __future__ import annotations

import dataclasses

import torch
from torch import nn
from torch.nn.init import xavier_normal_, xavier_uniform_

from . import ops
from .rec_common import CatalogCEFn, ConfigBase, EmbedDropoutFn, GatherLinearFn, SeqRecMixin, _next_seed


@dataclasses.dataclass
class GRU4RecConfig(ConfigBase):
    """The fields and defaults of the reference's GRU4RecConfig (ref:SeqRec/models/discriminative/GRU4Rec/config.py).  The
    reference's pydantic model drops unknown keys without a word; from_dict says which ones are dropped."""
    embedding_size: int = 64
    hidden_size: int = 128
    n_layers: int = 1
    dropout: float = 0.3
    loss_type: str = "CE"
    _unknown_keys = "warn"


class _GRULayerFn(torch.autograd.Function):
    """One nn.GRU(bias=False) layer over x [B, L, In] from h_{-1} = 0: h [B, L, H] (gamer_gru_fwd / gamer_gru_bwd)."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, w_ih, w_hh, lens, train):
        B, L, In = x.shape
        H = w_hh.shape[1]
        f32 = dict(dtype=torch.float32, device=x.device)
        x = x.contiguous()
        gi = torch.empty(B, L, 3 * H, **f32)
        ops.linear_fwd(x.view(B * L, In), In, w_ih, In, gi.view(B * L, 3 * H), 3 * H, B * L, 3 * H, In)
        h = torch.empty(B, L, H, **f32)
        gates = torch.empty(ops.gru_gates_floats(B, L, H), **f32) if train else None
        ops.gru_fwd(gi, w_hh, h, gates, lens)
        if train:
            ctx.save_for_backward(x, w_ih, w_hh, h, gates, lens)
        return h

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dh):
        x, w_ih, w_hh, h, gates, lens = ctx.saved_tensors
        B, L, In = x.shape
        H = w_hh.shape[1]
        f32 = dict(dtype=torch.float32, device=x.device)
        dgi, dgh = torch.empty(B, L, 3 * H, **f32), torch.empty(B, L, 3 * H, **f32)
        ops.gru_bwd(dh.contiguous().float(), h, gates, w_hh, dgi, dgh, lens)
        T = B * L
        dgi2, dgh2 = dgi.view(T, 3 * H), dgh.view(T, 3 * H)
        dw_ih, dw_hh = torch.zeros_like(w_ih), torch.zeros_like(w_hh)
        ops.linear_wgrad(dgi2, 3 * H, x.view(T, In), In, dw_ih, In, T, 3 * H, In)
        ops.linear_wgrad(dgh2, 3 * H, h.view(T, H), H, dw_hh, H, T, 3 * H, H)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(B, L, In, **f32)
            ops.linear_dgrad(dgi2, 3 * H, w_ih, In, dx.view(T, In), In, T, 3 * H, In)
        return dx, dw_ih, dw_hh, None, None


class GRU4Rec(SeqRecMixin, nn.Module):
    def __init__(self, config: GRU4RecConfig, n_items: int, **kwargs):
        super().__init__()
        if config.loss_type == "BPR":
            raise NotImplementedError("GRU4Rec: loss_type 'BPR' (negative-sampling tasks) is not supported on the HIP path")
        if config.loss_type != "CE":
            raise NotImplementedError("Make sure 'loss_type' in ['BPR', 'CE']!")
        E, H = config.embedding_size, config.hidden_size
        if E % 4 or not 4 <= E <= 256 or H % 16 or not 16 <= H <= 256 or config.n_layers < 1:
            raise NotImplementedError("GRU4Rec on the HIP path: embedding_size % 4 == 0 in [4, 256], hidden_size % 16 == 0 in "
                                      "[16, 256], n_layers >= 1")
        self.config = config
        self.n_items = n_items
        self.max_his_len = kwargs.get("max_his_len")            # (no position table: any sequence length runs)
        self.embedding_size, self.hidden_size = E, H
        self.num_layers = config.n_layers
        self.dropout_prob = config.dropout
        self.loss_type = config.loss_type
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        self.item_embedding = nn.Embedding(n_items + 1, E, padding_idx=0)
        self.emb_dropout = nn.Dropout(self.dropout_prob)
        self.gru_layers = nn.GRU(input_size=E, hidden_size=H, num_layers=self.num_layers, bias=False, batch_first=True)
        self.dense = nn.Linear(H, E)
        self.apply(self._init_weights)

    def _init_weights(self, module: nn.Module):
        # as the reference: the whole item table (row 0 included) from xavier_normal_, layer 0 of the GRU xavier_uniform_
        if isinstance(module, nn.Embedding):
            xavier_normal_(module.weight)
        elif isinstance(module, nn.GRU):
            xavier_uniform_(module.weight_hh_l0)
            xavier_uniform_(module.weight_ih_l0)

    def _encode(self, item_seq: torch.Tensor, rows: torch.Tensor, lens: torch.Tensor, shared=None) -> torch.Tensor:
        """dense(GRU(emb_dropout(E[ids])))[rows]: [R, E]"""
        self._require_device(item_seq)
        p = self.dropout_prob if self.training else 0.0
        x = EmbedDropoutFn.apply(item_seq.long().contiguous(), self.item_embedding.weight, p, _next_seed(), shared)
        for k in range(self.num_layers):
            w_ih, w_hh = getattr(self.gru_layers, f"weight_ih_l{k}"), getattr(self.gru_layers, f"weight_hh_l{k}")
            train = torch.is_grad_enabled() and (x.requires_grad or w_ih.requires_grad or w_hh.requires_grad)
            x = _GRULayerFn.apply(x, w_ih, w_hh, lens, train)      # (train: keep the gates for the backward)
        return GatherLinearFn.apply(x, rows, self.dense.weight, self.dense.bias, ops.ACTIVATIONS["none"])

    def _rows_and_lens(self, item_seq, item_seq_len):
        rows = self._last_rows(item_seq, item_seq_len)
        return rows, item_seq_len.to(item_seq.device).long().contiguous()

    def forward(self, item_seq: torch.Tensor, item_seq_len: torch.Tensor) -> torch.Tensor:
        rows, lens = self._rows_and_lens(item_seq, item_seq_len)
        return self._encode(item_seq, rows, lens)                    # gather_indexes(dense(h), seq_len - 1), [B, E]

    def calculate_loss(self, interaction: dict) -> torch.Tensor:
        item_seq = interaction["inputs"]
        rows, lens = self._rows_and_lens(item_seq, interaction["seq_len"])
        shared = self._shared_grad()
        out = self._encode(item_seq, rows, lens, shared)
        target = interaction["target"].to(item_seq.device).long().contiguous()
        all_rows = torch.arange(out.shape[0], device=out.device)
        return CatalogCEFn.apply(out, all_rows, self.item_embedding.weight, target, shared)

    @torch.no_grad()
    def full_sort_topk(self, interaction: dict, k: int):
        """(indices [B, k], scores [B, k]) of the k best items (within item_range when given), as a stable argsort of the
        reference's full_sort_predict reads them; the scores are never materialised (gamer_catalog_topk)."""
        out = self.forward(interaction["inputs"], interaction["seq_len"])
        start, end = interaction["item_range"] if "item_range" in interaction else (0, self.n_items + 1)
        return ops.catalog_topk(out, self.item_embedding.weight.detach(), k, int(start), int(end))
