"""SASRec, the first discriminative baseline of ``train_SMB_rec``, on the HIP path.

Same nn.Module surface and parameter names as the reference (ref:SeqRec/models/discriminative/SASRec/model.py,
ref:SeqRec/modules/model_base/seq_model.py): ``item_embedding`` [n_items + 1, H], ``position_embedding`` [max_his_len, H],
``trm_encoder.layer.{l}.*`` (``gamer_amd.modules``), ``LayerNorm``.  A reference ``best_model.pth`` state dict loads here and
one saved here loads into the reference class.

Every step runs as HIP kernels, with no PyTorch fallback (the input block, the head and the ranking are the pieces of
``gamer_amd.rec_common`` that the other baselines use too):
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

import torch
from torch import nn

from . import modules, ops
from .rec_common import CatalogCEFn, ConfigBase, InputBlockFn, SeqRecMixin, _next_seed


@dataclasses.dataclass
class SASRecConfig(ConfigBase):
    """The keys and defaults of the reference's SASRecConfig (config/dis-models/SASRec/config.json); an unknown key raises."""
    n_layers: int = 2
    n_heads: int = 2
    hidden_size: int = 128
    inner_size: int = 256
    dropout_prob: float = 0.5
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-12
    initializer_range: float = 0.02
    loss_type: str = "CE"


class SASRec(SeqRecMixin, nn.Module):
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
        self._require_device(item_seq)
        if item_seq.size(1) > self.max_seq_length:
            raise ValueError(f"sequence length {item_seq.size(1)} > max_his_len {self.max_seq_length}")
        p = self.dropout_prob if self.training else 0.0
        x = InputBlockFn.apply(item_seq.long().contiguous(), self.item_embedding.weight, self.position_embedding.weight,
                               self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps, p, _next_seed(), shared)
        return self.trm_encoder(x, self.get_attention_mask(item_seq))

    def forward(self, item_seq: torch.Tensor, item_seq_len: torch.Tensor) -> torch.Tensor:
        rows = self._last_rows(item_seq, item_seq_len)
        out = self._encode(item_seq)
        return out.reshape(-1, out.shape[-1])[rows]          # gather_indexes, [B, H]

    def calculate_loss(self, interaction: dict) -> torch.Tensor:
        item_seq = interaction["inputs"]
        rows = self._last_rows(item_seq, interaction["seq_len"])
        shared = self._shared_grad()
        out = self._encode(item_seq, shared)
        target = interaction["target"].to(item_seq.device).long().contiguous()
        return CatalogCEFn.apply(out, rows, self.item_embedding.weight, target, shared)

    @torch.no_grad()
    def full_sort_topk(self, interaction: dict, k: int):
        """(indices [B, k], scores [B, k]) of the k best items (within item_range when given), as a stable argsort of the
        reference's full_sort_predict reads them; the scores are never materialised (gamer_catalog_topk)."""
        item_seq = interaction["inputs"]
        rows = self._last_rows(item_seq, interaction["seq_len"])
        out = self._encode(item_seq)
        start, end = interaction["item_range"] if "item_range" in interaction else (0, self.n_items + 1)
        return ops.catalog_topk(out, self.item_embedding.weight.detach(), k, int(start), int(end), row_idx=rows)
