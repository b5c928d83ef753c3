"""--eval_mode / --eval_num_neg of the four T5 commands and the candidate lists, target flags and ranks that gamer_amd.tiger_eval
builds for them, on a toy catalogue with a stub scorer (no GPU)."""
import math

import pytest
import torch

from gamer_amd import evaluate, tiger_eval


def _parsers():
    from gamer_amd import train_pbatransformer, train_tiger, train_tiger_mb, train_tiger_smb
    return [(train_tiger, []), (train_tiger_smb, ["--tasks", "smb_explicit"]), (train_tiger_mb, ["--tasks", "mb_explicit"]),
            (train_pbatransformer, [])]


@pytest.mark.parametrize("n", range(4))
def test_the_four_commands_take_the_flags(n):
    mod, base = _parsers()[n]
    a = mod.parse_args(base)
    assert a.eval_mode is None and a.eval_num_neg == 1000 and not tiger_eval.ranked(a)
    for mode in ("beam", "exact", "sampled"):
        a = mod.parse_args(base + ["--eval_mode", mode, "--eval_num_neg", "7"])
        assert a.eval_mode == mode and a.eval_num_neg == 7 and tiger_eval.ranked(a) == (mode != "beam")
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--eval_mode", "greedy"])


# a toy catalogue of 12 items of 2 tokens; item i = (10 + i // 4, 20 + i)
CAT = torch.tensor([[10 + i // 4, 20 + i] for i in range(12)], dtype=torch.int64)
TARGETS = [[3], [5, 7], [0]]
HISTORY = [{1, 2}, {4}, set()]


def _stub(record):
    """score = -(second token), so item 0 ranks first; records what it was asked to score"""
    def score(items):
        record.append(items.clone())
        it = items if items.dim() == 3 else items[None].expand(3, -1, -1)
        return -it[..., 1].float()
    return score


def test_exact_ranks_the_whole_catalogue():
    seen = []
    tg_rows = [[CAT[t].tolist() for t in ts] for ts in TARGETS]
    sums, ranks, best = tiger_eval.rank_batch(_stub(seen), CAT, "exact", TARGETS, HISTORY, tg_rows, ["hit@1", "hit@4", "hit@12", "ndcg@8"],
                                              5, torch.Generator().manual_seed(0), top=3)
    assert len(seen) == 1 and torch.equal(seen[0], CAT)                       # one list for every user: the catalogue itself
    cand, is_target = tiger_eval.build_candidates("exact", 12, TARGETS, HISTORY, 5, torch.Generator())
    assert cand is None and is_target.shape == (3, 12)
    assert is_target.nonzero().tolist() == [[0, 3], [1, 5], [1, 7], [2, 0]]
    # the stub ranks item i at rank i: user 0's target at rank 3, user 1's at 5 and 7, user 2's at 0
    assert ranks.tolist() == [3, 5, 0]
    assert sums["hit@1"] == 1.0 and sums["hit@4"] == 2.0 and sums["hit@12"] == 3.0
    ndcg = (1 / math.log2(3 + 2)) / 1.0 + (1 / math.log2(5 + 2) + 1 / math.log2(7 + 2)) / (1 + 1 / math.log2(3)) + 1.0
    assert abs(sums["ndcg@8"] - ndcg) < 1e-12
    assert best == [[0, 1, 2]] * 3


def test_sampled_lists_targets_first_negatives_outside_history_and_targets():
    g = torch.Generator().manual_seed(11)
    cand, is_target = tiger_eval.build_candidates("sampled", 12, TARGETS, HISTORY, 5, g)
    assert cand.shape == (3, 2 + 5) and is_target.shape == cand.shape
    for b, (ts, h) in enumerate(zip(TARGETS, HISTORY)):
        row = cand[b].tolist()
        assert row[:len(ts)] == ts and is_target[b].tolist() == [True] * len(ts) + [False] * (7 - len(ts))
        neg = row[len(ts):len(ts) + 5]
        assert len(set(neg)) == 5 and not set(neg) & (set(ts) | h) and all(0 <= i < 12 for i in neg)
        assert row[len(ts) + 5:] == [-1] * (2 - len(ts))                      # users with fewer targets: padding
    again, _ = tiger_eval.build_candidates("sampled", 12, TARGETS, HISTORY, 5, torch.Generator().manual_seed(11))
    other, _ = tiger_eval.build_candidates("sampled", 12, TARGETS, HISTORY, 5, torch.Generator().manual_seed(12))
    assert torch.equal(cand, again) and not torch.equal(cand, other)
    with pytest.raises(ValueError, match="negatives"):
        tiger_eval.build_candidates("sampled", 12, TARGETS, HISTORY, 10, torch.Generator().manual_seed(0))      # user 0: 9 items left
    with pytest.raises(ValueError, match="mode"):
        tiger_eval.build_candidates("beam", 12, TARGETS, HISTORY, 5, g)


def test_sampled_scores_per_user_lists_and_padding_ranks_last():
    seen = []
    tg_rows = [[CAT[t].tolist() for t in ts] for ts in TARGETS]
    sums, ranks, best = tiger_eval.rank_batch(_stub(seen), CAT, "sampled", TARGETS, HISTORY, tg_rows, ["hit@1", "hit@7"], 5,
                                              torch.Generator().manual_seed(11), top=7)
    cand, _ = tiger_eval.build_candidates("sampled", 12, TARGETS, HISTORY, 5, torch.Generator().manual_seed(11))
    assert len(seen) == 1 and torch.equal(seen[0], CAT[cand.clamp(min=0)])    # [B, C, T]: a list per user
    for b in range(3):
        real = [i for i in cand[b].tolist() if i >= 0]
        assert best[b] == sorted(real)                                        # the stub's order; the padding is dropped from the top
        assert int(ranks[b]) == sorted(real).index(min(TARGETS[b]))
    assert sums["hit@7"] == 3.0 and sums["hit@1"] == float(sum(int(r) == 0 for r in ranks))


def test_ranks_and_metrics_from_fixed_scores_with_ties():
    scores = torch.tensor([[0.5, 0.9, 0.9, 0.1], [0.2, 0.2, 0.2, 0.2], [0.0, 1.0, 2.0, 3.0]])
    is_target = torch.tensor([[False, False, True, False], [False, True, False, True], [True, False, False, False]])
    # ties go to the lower candidate index: user 0's target (index 2) ranks behind index 1; user 1's targets at ranks 1 and 3
    assert evaluate.target_ranks(scores, is_target).tolist() == [1, 1, 3]
    targets = [[[1]], [[1], [2]], [[3]]]
    res = evaluate.rank_metrics(scores, is_target, targets, ["hit@1", "hit@2", "hit@4", "ndcg@2", "ndcg@4"])
    assert res["hit@1"] == 0.0 and res["hit@2"] == 2.0 and res["hit@4"] == 3.0
    ideal2 = 1 + 1 / math.log2(3)
    assert abs(res["ndcg@2"] - (1 / math.log2(3) + (1 / math.log2(3)) / ideal2 + 0.0)) < 1e-12
    assert abs(res["ndcg@4"] - (1 / math.log2(3) + (1 / math.log2(3) + 1 / math.log2(5)) / ideal2 + 1 / math.log2(5))) < 1e-12


def test_helpers_map_token_rows_to_catalogue_rows_and_tag_results():
    import argparse
    rows = [[1, 2], [3, 4], [1, 2], [5, 6]]
    cat = tiger_eval.distinct_rows(rows)
    assert cat.tolist() == [[1, 2], [3, 4], [5, 6]]
    index = {tuple(r): i for i, r in enumerate(cat.tolist())}
    assert tiger_eval.rows_to_items(index, [[5, 6], [9, 9], [1, 2]]) == [2, 0]          # a history row outside the catalogue: dropped
    with pytest.raises(KeyError, match="9, 9"):
        tiger_eval.rows_to_items(index, [[5, 6], [9, 9]], strict=True)                  # a target outside it cannot be ranked
    a = argparse.Namespace(eval_mode=None, eval_num_neg=1000)
    assert tiger_eval.tag_results({"hit@1": 0.5}, a) == {"hit@1": 0.5}
    a.eval_mode = "sampled"
    assert tiger_eval.tag_results([{"hit@1": 0.5}, {"hit@1": 0.1}], a) == [{"hit@1": 0.5, "eval_mode": "sampled", "num_neg": 1000},
                                                                            {"hit@1": 0.1, "eval_mode": "sampled", "num_neg": 1000}]
    a.eval_mode = "exact"
    assert tiger_eval.tag_results({"hit@1": 0.5}, a) == {"hit@1": 0.5, "eval_mode": "exact"}
