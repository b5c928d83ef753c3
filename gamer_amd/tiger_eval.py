"""Ranking GIVEN items with the T5 backbones: what ``--eval_mode exact | sampled`` of train_tiger, train_tiger_smb, train_tiger_mb and
train_pbatransformer share.

Beam search only tells whether a target is among the ``num_beams`` survivors.  ``tiger.score_items`` gives every item its exact
log-likelihood, so a target can be ranked in the whole catalogue ("exact") or among the user's targets + N sampled negatives
("sampled", the protocol of the reference's discriminative baselines: ``SMBDisNegSampleEvalDataset``, ``sample_sort_predict``,
ref:SeqRec/trainers/SMBRec.py:102-107) - the modes of ``evaluate.evaluate_behavior`` for the Qwen3 family, with the same helpers:
negatives from ``evaluate.sample_candidates`` (a seeded ``torch.Generator``; the catalogue minus the user's history items and
targets; its ValueError when too few remain), ranks and metric sums from ``evaluate.target_ranks`` / ``rank_metrics`` (any k, equal
scores rank by candidate index, lower first).  A catalogue here is an int64 [n_items, K] array of distinct token rows; the items a
command scores may carry more tokens (</s>) or fewer (a behaviour token that the decoder prefix holds) than the rows it indexes.
"""
from __future__ import annotations

import torch

from . import evaluate

MODES = evaluate.MODES


def add_eval_flags(ap):
    ap.add_argument("--eval_mode", choices=MODES, default=None,
                    help="how the test ranks a target: beam (the default when unset: among the num_beams survivors), exact (among all "
                         "items of the test catalogue, by tiger.score_items) or sampled (among the targets + --eval_num_neg negatives)")
    ap.add_argument("--eval_num_neg", type=int, default=1000, help="negatives per user of --eval_mode sampled")


def ranked(a) -> bool:
    """whether the command's test ranks given items (exact / sampled) instead of running the beam search"""
    return getattr(a, "eval_mode", None) in ("exact", "sampled")


def distinct_rows(rows) -> torch.Tensor:
    """int64 [n, K]: the distinct rows in their first-seen order"""
    seen = dict.fromkeys(tuple(int(t) for t in r) for r in rows)
    return torch.tensor(list(seen), dtype=torch.int64)


def rows_to_items(index, rows, strict=False):
    """the catalogue rows of token tuples.  A history tuple that is no item of the catalogue (another behaviour's, a cut row) is
    dropped; ``strict`` (targets): it raises KeyError, as evaluate's exact mode does - a target outside the catalogue cannot be ranked"""
    out = []
    for r in rows:
        key = tuple(int(t) for t in r)
        if key in index:
            out.append(index[key])
        elif strict:
            raise KeyError(f"target {key} is not an item of the test catalogue")
    return out


def build_candidates(mode, n_items, targets_idx, history_idx, num_neg, generator):
    """(cand, is_target).  "exact": cand = None, every user is scored on the whole catalogue, is_target bool [B, n_items].
    "sampled": cand int64 [B, max targets + num_neg] catalogue rows from evaluate.sample_candidates - a user's distinct targets
    first, then its negatives, -1 = padding - and is_target marks the leading target columns."""
    B = len(targets_idx)
    if mode == "exact":
        is_target = torch.zeros(B, n_items, dtype=torch.bool)
        for b, ts in enumerate(targets_idx):
            is_target[b, [int(t) for t in ts]] = True
        return None, is_target
    if mode != "sampled":
        raise ValueError(f"mode {mode!r}: 'exact' or 'sampled' rank given items")
    cand = evaluate.sample_candidates(n_items, targets_idx, history_idx, num_neg, generator)
    is_target = torch.zeros(cand.shape, dtype=torch.bool)
    for b, ts in enumerate(targets_idx):
        is_target[b, :len({int(t) for t in ts})] = True
    return cand, is_target


def rank_batch(score_fn, items, mode, targets_idx, history_idx, targets, metric_list, num_neg, generator, top=0):
    """One test batch.  ``items`` int64 [n_items, T]: what is scored for every catalogue row; ``score_fn(items [C, T] or [B, C, T])``
    -> scores [B, C] (tiger.score_items on the batch).  ``targets``: per user the target items, as metrics.get_metrics_results
    counts them.  Returns (metric SUMS over the users, ranks int64 [B] of every user's best target, per user the catalogue rows
    of its ``top`` best candidates, best first)."""
    cand, is_target = build_candidates(mode, items.shape[0], targets_idx, history_idx, num_neg, generator)
    scores = score_fn(items if cand is None else items[cand.clamp(min=0)]).detach().float().cpu()
    if cand is not None:
        scores = scores.masked_fill(cand < 0, float("-inf"))                # (users with fewer targets: the padding ranks last)
    sums = evaluate.rank_metrics(scores, is_target, targets, metric_list)
    best = []
    if top > 0:
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :top]
        rows = order if cand is None else cand.gather(1, order)
        best = [[int(i) for i in r if i >= 0] for r in rows.tolist()]
    return sums, evaluate.target_ranks(scores, is_target), best


def tag_results(res, a):
    """the mode and its number of negatives as extra keys of a result row (or of every row of a list); a beam evaluation that was
    not asked for by name keeps the file it always wrote"""
    if getattr(a, "eval_mode", None) is None:
        return res
    for row in (res if isinstance(res, list) else [res]):
        row["eval_mode"] = a.eval_mode
        if a.eval_mode == "sampled":
            row["num_neg"] = a.eval_num_neg
    return res


def history_rows(samples, n, token_count, skip):
    """the history of sample n of a flat sample set (ptr / n_history / tokens) as item rows of ``token_count`` tokens without their
    first ``skip`` (the behaviour token)"""
    a, h = int(samples.ptr[n]), int(samples.n_history[n])
    return samples.tokens[a:a + h].reshape(-1, token_count)[:, skip:]
