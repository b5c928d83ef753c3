"""What the discriminative baselines of ``train_SMB_rec`` (SASRec, GRU4Rec, BERT4Rec, MBSTR) share on the HIP path.

Only pieces that at least two models use live here; a model's own layers and heads stay in its module.
  seeds          ``_Seeds`` / ``_next_seed``: the running counter the cloze masks and the input dropout draw from
  ``_SharedGrad``  one item-table gradient buffer per calculate_loss call, written by the head and by the input gather
  functions      ``InputBlockFn`` (dropout(LayerNorm(E[ids] + P[s]))), ``EmbedDropoutFn`` (dropout(E[ids])), ``GatherLinearFn``
                 (act(x[rows] W^T + b)), ``_GatherRowsFn`` (x[rows], rows may repeat), ``CatalogCEFn`` (catalogue-wide cross
                 entropy, the scores never written)
  helpers        ``colsum``, ``linear_act_bwd``, ``layernorm_bwd``: re-exported from layer_blocks, where the layers' blocks live
  ``ConfigBase``   from_dict / from_pretrained / to_dict of the config dataclasses, with the model's rule for unknown keys
  mixins         ``SeqRecMixin`` (all four models) and ``ClozeMixin`` (the cloze models): methods only, no ``__init__`` and no
                 submodules, so every model still creates its parameters in the reference's order
  ``DotProductPredictionHead``  the parameter holder of BERT4Rec's head, which MBSTR uses with ``behavior_head=False``
"""
from __future__ import annotations

import dataclasses
import json
import os
import warnings

import torch
from torch import nn

from . import ops
from .layer_blocks import (_dropout_bwd, colsum, dropout_fwd, layernorm_bwd, linear_act_bwd,  # noqa: F401  (re-exported)
                           linear_act_fwd)


class ConfigBase:
    """from_dict / from_pretrained / to_dict of a config dataclass.  ``_unknown_keys`` says what from_dict does with a key that is
    no field: "raise" (ValueError), "warn" (dropped, with a UserWarning that names it) or "drop" (dropped without a word, as the
    reference's pydantic models do)."""
    _unknown_keys = "raise"

    @classmethod
    def from_dict(cls, d: dict):
        names = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(d) - names)
        if unknown and cls._unknown_keys == "raise":
            raise ValueError(f"{cls.__name__}: unknown keys {unknown}")
        if unknown and cls._unknown_keys == "warn":
            warnings.warn(f"{cls.__name__}: ignoring unknown keys {unknown} (as the reference does)", stacklevel=2)
        return cls(**{k: v for k, v in d.items() if k in names})

    @classmethod
    def from_pretrained(cls, path: str):
        f = os.path.join(path, "config.json")
        if not os.path.exists(f):
            raise ValueError(f"Can't find a configuration file at {f}.")
        with open(f, encoding="utf-8") as fh:
            return cls.from_dict(json.load(fh))

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)


class DropUnknownConfig(ConfigBase):
    """A ``@dataclasses.dataclass(init=False)`` config whose constructor drops unknown keys too."""
    _unknown_keys = "drop"

    def __init__(self, **kwargs):
        for f in dataclasses.fields(self):
            setattr(self, f.name, kwargs.get(f.name, f.default))


class _Seeds:
    value = 0x5A5E


def _next_seed() -> int:
    _Seeds.value += 1
    return _Seeds.value


class _SharedGrad:
    """The item table's gradient buffer of one calculate_loss call: the head's backward (which runs first) writes its dE into
    it and returns no gradient for the table; the input block's backward accumulates the gather's rows into the same buffer
    and returns it - one [V, H] tensor instead of two plus autograd's sum.  ``gathers`` > 1 (TIGER: the encoder's and the
    decoder's inputs): every gather but the last hands the buffer on through ``give`` and returns no gradient itself."""

    def __init__(self, gathers: int = 1):
        self.dE = None
        self.gathers = gathers

    @staticmethod
    def take(shared, shape, device):
        """the head's dE when there is one (handed over once), else zeros"""
        if shared is None or shared.dE is None:
            return torch.zeros(shape, dtype=torch.float32, device=device)
        dE, shared.dE = shared.dE, None
        return dE

    @staticmethod
    def give(shared, dE):
        """after a gather added its rows to ``dE``: None when another gather is still to come (the buffer waits for it), else dE"""
        if shared is None:
            return dE
        shared.gathers -= 1
        if shared.gathers > 0:
            shared.dE = dE
            return None
        return dE


# ---- autograd functions --------------------------------------------------------------------------------------------------------
class InputBlockFn(torch.autograd.Function):
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
        dv, dw, db = layernorm_bwd(v, w, mean, rstd, _dropout_bwd(dy, H, p, seed))
        dE = _SharedGrad.take(ctx.shared, e_shape, v.device)
        ops.embedding_bwd_large(ids, dv, 0, dE)
        dP = torch.zeros(p_shape, dtype=torch.float32, device=v.device)
        ops.position_bwd(dv.view(B, S, H), dP[:S])
        return None, dE, dP, dw, db, None, None, None, None


class EmbedDropoutFn(torch.autograd.Function):
    """dropout(E[ids]) for ids [B, L]; the gradient of E (row ``pad_id`` skipped; -1: no padding row) into the shared table
    gradient, which is returned by the last of its gathers."""

    @staticmethod
    def forward(ctx, ids, E, p, seed, shared=None, pad_id=0):
        B, L = ids.shape
        D = E.shape[1]
        x = torch.empty(B * L, D, dtype=torch.float32, device=E.device)
        ops.embedding_fwd(ids, E, x)
        x = dropout_fwd(x, p, seed)
        ctx.meta = (p, seed, E.shape, pad_id)
        ctx.shared = shared
        ctx.save_for_backward(ids)
        return x.view(B, L, D)

    @staticmethod
    def backward(ctx, dx):
        ids, = ctx.saved_tensors
        p, seed, e_shape, pad_id = ctx.meta
        g = _dropout_bwd(dx, e_shape[1], p, seed)
        dE = _SharedGrad.take(ctx.shared, e_shape, g.device)
        ops.embedding_bwd_large(ids, g, pad_id, dE)
        return None, _SharedGrad.give(ctx.shared, dE), None, None, None, None


class GatherLinearFn(torch.autograd.Function):
    """act(x[rows] w^T + b) for the rows of x's [B L, H] view, ``act`` a code of ops.ACTIVATIONS: [R, N]; dx is zero outside the
    gathered rows, which must be distinct."""

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def forward(ctx, x, rows, w, b, act):
        xg = x.reshape(-1, x.shape[-1])[rows].contiguous()
        pre, out = linear_act_fwd(xg, w, b, act)
        ctx.save_for_backward(xg, rows, w, None if act == 0 else pre)
        ctx.x_shape, ctx.act = x.shape, act
        return out

    @staticmethod
    @ops.scoped_f32_matmul(lambda *a: "f32")
    def backward(ctx, dout):
        xg, rows, w, pre = ctx.saved_tensors
        dxg, dw, db = linear_act_bwd(dout.contiguous().float().clone(), pre, xg, w, ctx.act)
        dx = torch.zeros(ctx.x_shape, dtype=torch.float32, device=xg.device)
        dx.view(-1, xg.shape[1])[rows] = dxg
        return dx, None, dw, db, None


class _GatherRowsFn(torch.autograd.Function):
    """x.view(-1, H)[rows] for rows that may repeat (MBHT: the padded slots of masked_index all point at position 0); the backward
    adds the repeats in slot order (gamer_embedding_bwd_large: no float atomics)."""

    @staticmethod
    def forward(ctx, x, rows):
        H = x.shape[-1]
        xf = x.reshape(-1, H).contiguous().float()
        y = torch.empty(rows.numel(), H, dtype=torch.float32, device=x.device)
        ops.embedding_fwd(rows, xf, y)
        ctx.save_for_backward(rows)
        ctx.x_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, = ctx.saved_tensors
        H = ctx.x_shape[-1]
        dx = torch.zeros(ctx.x_shape, dtype=torch.float32, device=dy.device)
        ops.embedding_bwd_large(rows, dy.contiguous().float(), -1, dx.view(-1, H))
        return dx, None


class CatalogCEFn(torch.autograd.Function):
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
            raise IndexError(f"calculate_loss: {n_bad} target(s) outside [0, {E.shape[0] if V is None else V})")
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


# ---- parameter holder ----------------------------------------------------------------------------------------------------------
class DotProductPredictionHead(nn.Module):
    """Parameter holder with the reference's names: ``out.0`` (Linear + ReLU), ``bias`` [1, n_items + 1] and the shared table."""

    def __init__(self, d_model: int, n_items: int, token_embeddings: nn.Embedding):
        super().__init__()
        self.token_embeddings = token_embeddings
        self.vocab_size = n_items + 1
        self.out = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU())
        self.bias = nn.Parameter(torch.zeros(1, self.vocab_size))


# ---- mixins (methods only) -----------------------------------------------------------------------------------------------------
class SeqRecMixin:
    """What every baseline does around its encoder.  The model has ``item_embedding`` and ``n_items``."""

    def _require_device(self, t: torch.Tensor):
        if not t.is_cuda:
            raise RuntimeError(f"{type(self).__module__} runs on the HIP device only (no CPU fallback)")

    @staticmethod
    def _last_rows(item_seq, item_seq_len):
        """the flat position of item seq_len - 1 of every row"""
        B, S = item_seq.shape
        n = item_seq_len.to(item_seq.device).long()
        if n.shape != (B,) or int(n.min()) < 1 or int(n.max()) > S:
            raise IndexError(f"seq_len must hold {B} values in [1, {S}]")          # (the reference's gather raises too)
        return torch.arange(B, device=item_seq.device) * S + (n - 1)

    def _shared_grad(self):
        return _SharedGrad() if torch.is_grad_enabled() and self.item_embedding.weight.requires_grad else None

    def _item_scores(self, y: torch.Tensor, V: int, bias=None, start: int = 0, table=None) -> torch.Tensor:
        """y @ E[start:V]^T (+ bias), materialised: [R, V - start]; E = ``table`` (default: the item table)"""
        R, H = y.shape
        n = V - start
        out = torch.empty(R, n, dtype=torch.float32, device=y.device)
        E = self.item_embedding.weight if table is None else table
        with ops.f32_matmul("f32"):
            ops.linear_fwd(y.contiguous(), H, E[start:V].detach(), H, out, n, R, n, H)
        return out if bias is None else out + bias.detach()

    def full_sort_predict(self, interaction: dict) -> torch.Tensor:
        """[B, n_items + 1] scores as the reference builds them (-inf outside item_range); small catalogues and tests."""
        item_seq = interaction["inputs"]
        seq_output = self.forward(item_seq, interaction["seq_len"])
        start, end = interaction["item_range"] if "item_range" in interaction else (0, self.n_items + 1)
        scores = torch.full((seq_output.shape[0], self.n_items + 1), float("-inf"), device=item_seq.device)
        scores[:, start:end] = self._item_scores(seq_output, int(end), start=int(start))
        return scores


class ClozeMixin(SeqRecMixin):
    """The cloze task of BERT4Rec and MBSTR: scores and loss on the masked positions, ranking at position seq_len - 1 of an input
    that already ends with the mask token.  ``extra`` is the tuple of per-token inputs a model has besides the items (MBSTR: the
    types; BERT4Rec: none); it is passed through to the model untouched.  The model provides
      _head_input(item_seq, *extra, rows, shared=None)   the head's hidden state on the flat positions ``rows``: [M, H]
      _extra(item_seq, interaction)                      the device check of item_seq, and ``extra`` from the interaction
      _draw_cloze(interaction)                           (masked, extra, rows, targets) of a fresh masking: ONE host read
      _in_graph(name)                                    whether the loss reaches the parameter of that name
    and ``head``, whose ``bias`` (when it has one) is added to the scores.  A model whose head scores against something else than
    the item table itself (PBAT: a table derived from two) overrides ``_head_table``."""

    @property
    def _head_bias(self):
        return getattr(self.head, "bias", None)

    def _head_table(self, shared=None):
        """(table [>= V, H'], bias or None, V, shared): what the head's hidden state is scored against - rows [0, V) of the table
        plus the bias - and the gradient buffer the cross entropy hands its table gradient to (None: it returns it to autograd)."""
        return self.item_embedding.weight, self._head_bias, self.n_items + 1, shared

    def _cloze_scores(self, y: torch.Tensor) -> torch.Tensor:
        """the materialised scores [R, V] of head inputs y"""
        E, bias, V, _ = self._head_table()
        return self._item_scores(y, V, bias, table=E)

    def _refuse_candidates(self, candidates):
        if candidates is not None:
            raise NotImplementedError(f"{type(self).__name__}.forward: candidates (the negative-sampling tasks) are not supported "
                                      "on the HIP path")

    def _scores_at_labels(self, item_seq, labels, extra=()):
        """what forward returns: (valid_logits [M, n_items + 1], valid_labels [M]) of the positions with labels != 0, the scores
        materialised (tests and small catalogues; no gradient flows through the scores: training goes through calculate_loss)"""
        flat = labels.to(item_seq.device).flatten()
        rows = (flat != 0).nonzero()[:, 0]
        if rows.numel() == 0:
            return torch.empty(0, self.n_items + 1, device=item_seq.device), flat[rows]
        with torch.no_grad():
            return self._cloze_scores(self._head_input(item_seq, *extra, rows)), flat[rows]

    def _loss(self, masked, *rest) -> torch.Tensor:
        *extra, rows, targets = rest
        if rows.numel() == 0:
            # what nn.CrossEntropyLoss gives for no rows: NaN, with an all-zero gradient for every parameter of the graph
            return sum((p * 0.0).sum() for n, p in self.named_parameters() if self._in_graph(n)) + float("nan")
        shared = self._shared_grad()
        y = self._head_input(masked, *extra, rows, shared)
        all_rows = torch.arange(y.shape[0], device=y.device)
        E, bias, V, shared = self._head_table(shared)
        return CatalogCEFn.apply(y, all_rows, E, targets, shared, bias, V)

    def calculate_loss(self, interaction: dict, masked_labels=None) -> torch.Tensor:
        """The cloze loss of one batch.  ``masked_labels`` = (masked_item_seq, labels) injects the masking (parity tests); by
        default gamer_cloze_mask draws it.  One host read per step (the number of masked positions M, and what the model checks
        with it).  M = 0: NaN, and backward() leaves every parameter gradient exactly zero, as the reference."""
        if masked_labels is None:
            masked, extra, rows, targets = self._draw_cloze(interaction)
        else:
            masked, labels = masked_labels
            extra = self._extra(masked, interaction)
            flat = labels.to(masked.device).long().flatten()
            rows = (flat != 0).nonzero()[:, 0]
            targets = flat[rows]
        self.last_masked_count = int(rows.numel())
        return self._loss(masked.long().contiguous(), *extra, rows.contiguous(), targets.contiguous())

    def _last_hidden(self, interaction: dict) -> torch.Tensor:
        item_seq = interaction["inputs"]
        extra = self._extra(item_seq, interaction)
        rows = self._last_rows(item_seq, interaction["seq_len"])
        return self._head_input(item_seq, *extra, rows)

    @torch.no_grad()
    def full_sort_predict(self, interaction: dict) -> torch.Tensor:
        """[B, n_items + 1] scores (the head's bias added) from position seq_len - 1 of the input as given: the evaluation data
        already ends with the mask token.  ``item_range`` is ignored, as in the reference.  Small catalogues and tests."""
        return self._cloze_scores(self._last_hidden(interaction))

    @torch.no_grad()
    def full_sort_topk(self, interaction: dict, k: int):
        """(indices [B, k], scores [B, k]) of the k best of items [0, n_items + 1), as a stable argsort of full_sort_predict reads
        them (lower index on ties); the scores are never materialised (gamer_catalog_topk / _topk_bias); <MASK> is never scored."""
        y = self._last_hidden(interaction)
        E, bias, V, _ = self._head_table()
        E = E.detach()
        if bias is None:
            return ops.catalog_topk(y, E, k, 0, V)
        return ops.catalog_topk_bias(y, E, bias.detach().reshape(-1), k, 0, V, V=V)
