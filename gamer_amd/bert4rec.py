"""BERT4Rec, the third classic baseline of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface, parameter and state-dict names as the reference (ref:SeqRec/models/discriminative/BERT4Rec/model.py,
ref:SeqRec/modules/layers/transformer.py DotProductPredictionHead): ``output_bias`` [n_items + 1] (never used by forward, so it
gets no gradient; saved and loaded), ``item_embedding`` [n_items + 2, H] (row 0 pads, row n_items + 1 is ``<MASK>``),
``position_embedding``, ``LayerNorm``, ``trm_encoder.layer.{l}.*``, ``output_ffn``, ``output_ln``, ``head.out.0``, ``head.bias``
[1, n_items + 1] and ``head.token_embeddings``, the item table again (two state-dict keys, one parameter).  A reference
``best_model.pth`` loads here and one saved here loads into the reference class.

Every step runs as HIP kernels, with no PyTorch fallback:
  masking       reconstruct_train_data: gamer_cloze_mask (masked sequence, labels, and the row-major list of the M masked
                positions with their targets, which the head consumes)
  input block   rec_common.InputBlockFn (SASRec's too): gamer_seq_embed_ln_fwd and its backward, the item table's gradient buffer shared with the head
  encoder       gamer_amd.modules.TransformerEncoder with the bidirectional (key padding only) additive mask
  output chain  head.out(output_ln(gelu(output_ffn(x)))) then ReLU, on the M gathered rows only (the reference applies
                output_ffn to all B L rows and gathers afterwards: the same values and gradients): fp32 GEMMs,
                gamer_bias_act_fwd / _bwd, gamer_layernorm_fwd / _bwd
  head          nn.CrossEntropyLoss()(y @ E[:n_items + 1]^T + head.bias, target): gamer_catalog_ce_bias_fwd / _bwd, which never
                write the [M, n_items + 1] scores; ranking: gamer_catalog_topk_bias (rec_common.ClozeMixin, shared with MBSTR)

Reference behaviour kept on purpose:
  * ``apply(_init_weights)`` reaches the item table through ``item_embedding`` and through ``head.token_embeddings`` (nn.Module.apply
    does not deduplicate), so the table is drawn twice and the second draw stays; rows 0 and ``<MASK>`` are drawn like the rest.
  * A fine-tuning row (``ft_ratio``) gets position ``min(seq_len, max_seq_length - 1)`` masked.  For a row shorter than the batch
    width that is a padding slot: the row gets a mask token appended and label 0 there, so it adds no term to the loss; only rows
    of full length get their last item masked with a label.
  * That index is applied to a tensor of the batch's width, so a batch whose longest row is shorter than ``max_seq_length`` raises
    IndexError (here on the host, before any launch).
  * No masked position in a batch (M = 0): the loss is NaN and every parameter the loss depends on gets an all-zero gradient.
  * ``full_sort_predict`` ignores ``item_range``.
  * Masks (cloze and dropout) come from the project's counter-based hash, not torch's generator: the same seed gives the same
    bits, but the masks differ from the reference's.  Parity with the reference is checked with injected masks and dropout off.
"""
from __future__ import annotations

import dataclasses

import torch
from torch import nn

from . import modules, ops
from .rec_common import (ClozeMixin, DotProductPredictionHead, DropUnknownConfig, InputBlockFn, _next_seed, layernorm_bwd,
                         linear_act_bwd, linear_act_fwd)


@dataclasses.dataclass(init=False)
class BERT4RecConfig(DropUnknownConfig):
    """The fields and defaults of the reference's BERT4RecConfig (ref:SeqRec/models/discriminative/BERT4Rec/config.py); unknown keys
    are dropped, as the reference's pydantic model does (the point GRU4RecConfig makes)."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 64
    inner_size: int = 256
    dropout_prob: float = 0.2
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    mask_ratio: float = 0.2
    ft_ratio: float = 0.5
    loss_type: str = "CE"


class _OutputChainFn(torch.autograd.Function):
    """relu(head.out.0(output_ln(gelu(output_ffn(x[rows]))))) for the rows of x's [B L, H] view: [M, H]; dx is zero elsewhere."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, rows, w1, b1, lnw, lnb, eps, w2, b2):
        H = x.shape[-1]
        f32 = dict(dtype=torch.float32, device=x.device)
        xg = x.reshape(-1, H)[rows].contiguous()
        M = xg.shape[0]
        pre1, a1 = linear_act_fwd(xg, w1, b1, ops.ACTIVATIONS["gelu"])
        y1 = torch.empty(M, H, **f32)
        mean, rstd = torch.empty(M, **f32), torch.empty(M, **f32)
        ops.layernorm_fwd(a1, None, lnw, lnb, eps, None, y1, mean, rstd)
        pre2, out = linear_act_fwd(y1, w2, b2, ops.ACTIVATIONS["relu"])
        ctx.save_for_backward(xg, rows, w1, pre1, a1, lnw, mean, rstd, y1, w2, pre2)
        ctx.x_shape = x.shape
        return out

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        xg, rows, w1, pre1, a1, lnw, mean, rstd, y1, w2, pre2 = ctx.saved_tensors
        dy1, dw2, db2 = linear_act_bwd(dout.contiguous().float().clone(), pre2, y1, w2, ops.ACTIVATIONS["relu"])
        da1, dlnw, dlnb = layernorm_bwd(a1, lnw, mean, rstd, dy1)
        dxg, dw1, db1 = linear_act_bwd(da1, pre1, xg, w1, ops.ACTIVATIONS["gelu"])
        dx = torch.zeros(ctx.x_shape, dtype=torch.float32, device=xg.device)
        dx.view(-1, xg.shape[1])[rows] = dxg                        # (rows are distinct positions)
        return dx, None, dw1, db1, dlnw, dlnb, None, dw2, db2


class BERT4Rec(ClozeMixin, nn.Module):
    def __init__(self, config: BERT4RecConfig, n_items: int, max_his_len: int, **kwargs):
        super().__init__()
        if config.loss_type != "CE":
            raise NotImplementedError("BERT4Rec: only loss_type 'CE' is supported (as the reference: 'Only support CE loss now')")
        if config.hidden_size % 4 or config.hidden_size > 256:
            raise NotImplementedError("BERT4Rec on the HIP path: hidden_size % 4 == 0 and hidden_size <= 256")
        self.config = config
        self.n_items = n_items
        self.n_layers, self.n_heads = config.n_layers, config.n_heads
        self.hidden_size, self.inner_size = config.hidden_size, config.inner_size
        self.dropout_prob, self.hidden_act = config.dropout_prob, config.hidden_act
        self.layer_norm_eps, self.initializer_range = config.layer_norm_eps, config.initializer_range
        self.ft_ratio, self.mask_ratio = config.ft_ratio, config.mask_ratio
        self.max_seq_length = max_his_len
        self.mask_token = n_items + 1
        self.loss_type = config.loss_type
        # (created in the reference's order, so a seeded construction draws the same initial weights)
        H = self.hidden_size
        self.item_embedding = nn.Embedding(n_items + 2, H, padding_idx=0)          # 0: <PAD>, n_items + 1: <MASK>
        self.position_embedding = nn.Embedding(max_his_len, H)
        self.dropout = nn.Dropout(self.dropout_prob)
        self.LayerNorm = nn.LayerNorm(H, eps=self.layer_norm_eps)
        layer = modules.TransformerEncoderLayer(d_model=H, nhead=self.n_heads, dim_feedforward=self.inner_size,
                                                dropout=self.dropout_prob, activation=self.hidden_act,
                                                layer_norm_eps=self.layer_norm_eps)
        self.trm_encoder = modules.TransformerEncoder(layer, self.n_layers)
        self.output_ffn = nn.Linear(H, H)
        self.output_gelu = nn.GELU()
        self.output_ln = nn.LayerNorm(H, eps=self.layer_norm_eps)
        self.output_bias = nn.Parameter(torch.zeros(n_items + 1))
        self.head = DotProductPredictionHead(d_model=H, n_items=n_items, token_embeddings=self.item_embedding)
        self.apply(self._init_weights)

    def _init_weights(self, module: nn.Module):
        # as the reference: Linear / Embedding weights from normal(0, initializer_range) (the shared table is visited twice),
        # Linear biases zero, LayerNorms untouched
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    # ---- masking ---------------------------------------------------------------------------------------------------------------
    def _cloze(self, item_seq: torch.Tensor, seq_len: torch.Tensor, seed=None, want_words=False):
        self._require_device(item_seq)
        B, L = item_seq.shape
        n = seq_len.to(item_seq.device).long().contiguous()
        lo, hi = torch.stack([seq_len.min(), seq_len.max()]).tolist() if seq_len.shape == (B,) else (0, 0)     # (one host read)
        if lo < 1 or hi > L:
            raise IndexError(f"seq_len must hold {B} values in [1, {L}]")
        p = min(hi, self.max_seq_length - 1)
        if p >= L:
            # the reference indexes a [B, L] tensor with min(seq_len, max_seq_length - 1) for every row
            raise IndexError(f"index {p} (min(seq_len, max_seq_length - 1)) is out of bounds for dimension 1 with size {L}: a batch "
                             f"of width {L} < max_seq_length {self.max_seq_length} holds a row with seq_len {L}")
        seed = _next_seed() if seed is None else int(seed)
        return ops.cloze_mask(item_seq.long().contiguous(), n, self.mask_ratio, self.ft_ratio, self.mask_token, self.max_seq_length,
                              seed, want_words)

    def reconstruct_train_data(self, item_seq: torch.Tensor, seq_len: torch.Tensor, seed=None):
        """(masked_item_seq, labels) of the cloze task; ``seed`` fixes the masks (default: the module's running counter)."""
        masked, labels = self._cloze(item_seq, seq_len, seed)[:2]
        return masked, labels

    # ---- encoder ---------------------------------------------------------------------------------------------------------------
    def get_attention_mask(self, item_seq: torch.Tensor) -> torch.Tensor:
        """key padding only, additive finfo.min, [B, 1, 1, L] (SeqModel.get_attention_mask, bidirectional=True, before its expand)"""
        keep = (item_seq != 0)[:, None, None, :].float()
        return (1.0 - keep) * torch.finfo(torch.float32).min

    def _encode(self, item_seq: torch.Tensor, shared=None) -> torch.Tensor:
        self._require_device(item_seq)
        if item_seq.size(1) > self.max_seq_length:
            raise ValueError(f"sequence length {item_seq.size(1)} > max_his_len {self.max_seq_length}")
        p = self.dropout_prob if self.training else 0.0
        x = InputBlockFn.apply(item_seq.long().contiguous(), self.item_embedding.weight, self.position_embedding.weight,
                               self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps, p, _next_seed(), shared)
        return self.trm_encoder(x, self.get_attention_mask(item_seq))

    def _head_input(self, item_seq: torch.Tensor, rows: torch.Tensor, shared=None) -> torch.Tensor:
        """the head's ReLU output on the rows (flat positions) given: [M, H]"""
        x = self._encode(item_seq, shared)
        lin = self.head.out[0]
        return _OutputChainFn.apply(x, rows, self.output_ffn.weight, self.output_ffn.bias, self.output_ln.weight,
                                    self.output_ln.bias, self.layer_norm_eps, lin.weight, lin.bias)

    # ---- the cloze task (ClozeMixin: _loss, calculate_loss, full_sort_predict, full_sort_topk) -----------------------------------
    def forward(self, item_seq: torch.Tensor, labels: torch.Tensor, candidates=None):
        """(valid_logits [M, n_items + 1], valid_labels [M]) of the positions with labels != 0, the scores materialised (tests and
        small catalogues; no gradient flows through the scores: training goes through calculate_loss)."""
        self._refuse_candidates(candidates)
        return self._scores_at_labels(item_seq, labels)

    def _extra(self, item_seq, interaction):
        self._require_device(item_seq)
        return ()

    def _draw_cloze(self, interaction: dict):
        masked, _, rows, targets, count = self._cloze(interaction["inputs"], interaction["seq_len"])
        M = int(count.item())                              # (the step's host read: the number of masked positions)
        return masked, (), rows[:M], targets[:M]

    @staticmethod
    def _in_graph(name: str) -> bool:
        return name != "output_bias" and "feed_forward.LayerNorm" not in name
