"""Evaluation loop of one target behaviour: beam search + ranking metrics.

Mirror of ``TestSMBDecoder.test_single_behavior`` (ref:SeqRec/tasks/test_SMB_decoder.py:90-285) for the
Qwen3Multi backbones, the plain Qwen3 baseline and the Qwen3Moe family (which ignore ``actions``; ``beam_search`` picks the decode
session of the engine's variant - Qwen3MoeAction's users may have different target behaviours in one batch): every batch is a dict with left-padded
``input_ids`` / ``attention_mask`` / ``actions`` that already end with the target behaviour token (test_SMB_decoder.py:112-118) and ``targets``: per sample the
list of held-out items (token tuples of the 4 semantic IDs).  Under ``torch.distributed`` every rank evaluates its
own batches and the metric sums are all-reduced (the reference gathers Python objects; the sums are the same).

``mode`` chooses how a target is ranked.  "beam" (the default, the reference's protocol for the decoders): among the
``num_beams`` survivors of the constrained beam search.  "exact": among ALL items of the behaviour's catalogue, by the exact
log-likelihood ``decode.score_items`` gives every item - no pruning, any k, the target's true rank.  "sampled": among the
user's targets + ``num_neg`` negatives drawn from the catalogue minus the user's items - the protocol of the reference's
discriminative baselines (``SMBDisNegSampleEvalDataset``, ``sample_sort_predict``, ref:SeqRec/trainers/SMBRec.py:102-107),
drawn here by a seeded ``torch.Generator`` (not a bit-exact restatement of its ``random.sample``).  Candidates of equal score
rank by their index, lower first.
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence

import torch

from . import metrics as gm
from .decode import ItemTrie, beam_search, score_items

MODES = ("beam", "exact", "sampled")


def ranked_hits(scores: torch.Tensor, is_target: torch.Tensor, k: int = None):
    """scores [B, C], is_target [B, C] bool -> per user the 0/1 hit list of its candidates, best first (the first ``k`` when
    given): the ``topk`` lists ``metrics.get_metrics_results`` takes.  Equal scores rank by candidate index, lower first."""
    order = torch.sort(scores.detach().float().cpu(), dim=1, descending=True, stable=True).indices
    hits = is_target.cpu().gather(1, order)
    return hits[:, :k].to(torch.int64).tolist() if k is not None else hits.to(torch.int64).tolist()


def target_ranks(scores: torch.Tensor, is_target: torch.Tensor) -> torch.Tensor:
    """0-based rank of every user's best-ranked target among its candidates (C when a user has none), by ``ranked_hits``' order."""
    order = torch.sort(scores.detach().float().cpu(), dim=1, descending=True, stable=True).indices
    hits = is_target.cpu().gather(1, order)
    C = hits.shape[1]
    pos = torch.where(hits, torch.arange(C)[None, :].expand_as(hits), torch.full_like(order, C))
    return pos.min(1).values


def rank_metrics(scores: torch.Tensor, is_target: torch.Tensor, targets, metric_list: Sequence[str]) -> Dict[str, float]:
    """Metric SUMS over the users (as ``metrics.get_metrics_results``) of a score matrix over given candidates, for any k."""
    kmax = max(int(m.split("@")[1]) for m in metric_list)
    return gm.get_metrics_results(ranked_hits(scores, is_target, kmax), metric_list, targets)


def catalogue_index(catalogue: torch.Tensor) -> Dict[tuple, int]:
    """token tuple -> row of ``catalogue`` [n_items, T] (the first row of a duplicated item)."""
    index = {}
    for i, row in enumerate(catalogue.tolist()):
        index.setdefault(tuple(row), i)
    return index


def history_items(input_ids: torch.Tensor, index: Dict[tuple, int], item_len: int):
    """Per prompt the catalogue rows of the items it holds: every window of ``item_len`` tokens that is an item (the code
    levels have disjoint token ranges, so a window matches only at an item's own position)."""
    out = []
    for row in input_ids.tolist():
        out.append({index[w] for j in range(len(row) - item_len + 1) if (w := tuple(row[j:j + item_len])) in index})
    return out


def sample_candidates(n_items: int, targets_idx, exclude_idx, num_neg: int, generator: torch.Generator) -> torch.Tensor:
    """[B, max targets + num_neg] int64 catalogue rows, -1 = padding: a user's distinct targets first, then ``num_neg`` distinct
    negatives drawn uniformly from the catalogue minus the user's targets and ``exclude_idx`` (its history).  The draw depends
    on the generator's state alone: the same seed gives the same candidates."""
    B = len(targets_idx)
    tg = [list(dict.fromkeys(int(t) for t in ts)) for ts in targets_idx]
    width = max(len(t) for t in tg) + num_neg
    out = torch.full((B, width), -1, dtype=torch.int64)
    for b in range(B):
        free = torch.ones(n_items, dtype=torch.bool)
        banned = list(set(tg[b]) | {int(i) for i in exclude_idx[b]})
        if banned:
            free[torch.tensor(banned)] = False
        pool = free.nonzero().flatten()
        if len(pool) < num_neg:
            raise ValueError(f"user {b}: {len(pool)} items are left for {num_neg} negatives")
        neg = pool[torch.randperm(len(pool), generator=generator)[:num_neg]]
        out[b, :len(tg[b])] = torch.tensor(tg[b], dtype=torch.int64)
        out[b, len(tg[b]):len(tg[b]) + num_neg] = neg
    return out


def _score_batch(engine, batch, items, max_rows):
    return score_items(engine, batch["input_ids"], batch["attention_mask"], batch["actions"], items,
                       session_ids=batch.get("session_ids"), extended_session_ids=batch.get("extended_session_ids"),
                       max_rows=max_rows)


def _exact_batch(engine, batch, catalogue, index, metric_list, max_rows):
    scores = _score_batch(engine, batch, catalogue, max_rows)
    is_target = torch.zeros(scores.shape, dtype=torch.bool)
    for b, ts in enumerate(batch["targets"]):
        for t in ts:
            is_target[b, index[tuple(int(x) for x in t)]] = True
    return rank_metrics(scores, is_target, batch["targets"], metric_list)


def _sampled_batch(engine, batch, catalogue, index, metric_list, num_neg, generator, max_rows):
    item_len = catalogue.shape[1]
    tg = [[index[tuple(int(x) for x in t)] for t in ts] for ts in batch["targets"]]
    cand = sample_candidates(catalogue.shape[0], tg, history_items(batch["input_ids"], index, item_len), num_neg, generator)
    pad = cand < 0
    scores = _score_batch(engine, batch, catalogue[cand.clamp(min=0)], max_rows).cpu()
    scores = scores.masked_fill(pad, float("-inf"))           # (users with fewer targets: the padding ranks last)
    is_target = torch.zeros(cand.shape, dtype=torch.bool)
    for b, ts in enumerate(tg):
        is_target[b, :len(set(ts))] = True
    return rank_metrics(scores, is_target, batch["targets"], metric_list)


@torch.no_grad()
def evaluate_behavior(engine, batches: Iterable[Dict], trie: ItemTrie, num_beams: int = 20,
                      metric_list: Sequence[str] = ("hit@1", "hit@5", "hit@10", "ndcg@5", "ndcg@10"),
                      item_len: int = 4, mode: str = "beam", catalogue: torch.Tensor = None, num_neg: int = 1000,
                      seed: int = 42, max_rows: int = 65536) -> Dict[str, float]:
    """``mode`` "exact" / "sampled" (see the module docstring) need ``catalogue`` [n_items, item_len] int64, the token tuples of
    the behaviour's items without the behaviour token; ``num_neg`` and ``seed`` are the sampled protocol's."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {MODES}")
    sums = {m: 0.0 for m in metric_list}
    total = 0
    if mode != "beam":
        if catalogue is None:
            raise ValueError(f"mode={mode!r} ranks given items: pass catalogue [n_items, item_len]")
        catalogue = torch.as_tensor(catalogue).to(torch.int64).cpu()
        index = catalogue_index(catalogue)
        generator = torch.Generator().manual_seed(seed)
    for batch in batches:
        if mode == "exact":
            res = _exact_batch(engine, batch, catalogue, index, metric_list, max_rows)
        elif mode == "sampled":
            res = _sampled_batch(engine, batch, catalogue, index, metric_list, num_neg, generator, max_rows)
        else:
            seqs, scores = beam_search(engine, batch["input_ids"], batch["attention_mask"], batch["actions"], trie,
                                       num_beams, item_len, session_ids=batch.get("session_ids"),
                                       extended_session_ids=batch.get("extended_session_ids"))
            pred = seqs[:, -item_len:].cpu().tolist()
            topk = gm.get_topk_results(pred, scores.cpu().tolist(), batch["targets"], num_beams)
            res = gm.get_metrics_results(topk, metric_list, batch["targets"])
        for m in metric_list:
            sums[m] += res[m]
        total += len(batch["targets"])
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        vec = torch.tensor([sums[m] for m in metric_list] + [float(total)], dtype=torch.float64,
                           device=engine.device if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(vec)
        for i, m in enumerate(metric_list):
            sums[m] = float(vec[i])
        total = int(vec[-1])
    out = {m: sums[m] / max(total, 1) for m in metric_list}
    out["samples"] = total
    return out


@torch.no_grad()
def evaluate_dataset(engine, data, max_his_len: int, behaviors: Sequence[str] = None, num_beams: int = 20,
                     batch_size: int = 64, metric_list: Sequence[str] = ("hit@1", "hit@5", "hit@10", "ndcg@5", "ndcg@10"),
                     rank: int = 0, world: int = 1, mode: str = "beam", num_neg: int = 1000, seed: int = 42,
                     max_rows: int = 65536) -> Dict[str, Dict[str, float]]:
    """``TestSMBDecoder.test`` over a dataset directory (test_SMB_decoder.py:408-440, 455-540): for every behaviour
    the test users that hold it in their last session, prompts from ``gamer_amd.data.Collator.test`` (history + the
    behaviour token), beams constrained to that behaviour's item trie.  ``data`` is a ``gamer_amd.data.SMBData``."""
    from . import data as gdata
    samples = data.test_samples(max_his_len)
    coll = gdata.Collator(data)
    out = {}
    for beh in (behaviors if behaviors is not None else data.behaviors):
        sub = samples.filter_by_behavior(beh)
        trie = ItemTrie(data.candidate_tokens(beh).tolist(), device=engine.device,
                        pad_token_id=engine.cfg.pad_token_id)

        def gen():
            for idx in gdata.batches(len(sub), batch_size, rank=rank, world=world):
                inputs, targets = coll.test(sub, idx, behavior=beh)
                yield {"input_ids": inputs["input_ids"], "attention_mask": inputs["attention_mask"],
                       "actions": inputs["actions"], "session_ids": inputs["session_ids"],
                       "extended_session_ids": inputs["extended_session_ids"],
                       "targets": [t.tolist() for t in targets]}
        catalogue = None if mode == "beam" else data.candidate_tokens(beh)[:, 1:]          # (without the behaviour token)
        out[beh] = evaluate_behavior(engine, gen(), trie, num_beams, metric_list, item_len=data.sole_item_len, mode=mode,
                                     catalogue=catalogue, num_neg=num_neg, seed=seed + rank, max_rows=max_rows)
    return out
