"""Evaluation modes of gamer_amd.evaluate (host logic, no GPU): ranking a target among given candidates from a [B, C] score
matrix ("exact" / "sampled"), the tie order, the negative sampler, and that ``mode="beam"`` is the unchanged beam path."""
import math

import pytest
import torch

from gamer_amd import evaluate as ev, metrics as gm


def test_ranks_and_metrics_from_a_score_matrix():
    scores = torch.tensor([[0.1, 0.9, 0.5, 0.3],          # target (column 2) is second
                           [0.4, 0.2, 0.3, 0.1],          # target (column 0) is first
                           [0.1, 0.2, 0.3, 0.4]])         # targets (columns 0 and 3) are last and first
    is_target = torch.tensor([[0, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 1]], dtype=torch.bool)
    targets = [[[2]], [[0]], [[0], [3]]]
    assert ev.ranked_hits(scores, is_target) == [[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 1]]
    assert ev.ranked_hits(scores, is_target, 2) == [[0, 1], [1, 0], [1, 0]]
    assert ev.target_ranks(scores, is_target).tolist() == [1, 0, 0]
    res = ev.rank_metrics(scores, is_target, targets, ["hit@1", "hit@2", "recall@4", "ndcg@4", "ndcg@30"])
    assert res["hit@1"] == 2.0 and res["hit@2"] == 3.0 and res["recall@4"] == 3.0
    ideal2 = 1.0 + 1.0 / math.log2(3)
    want = 1.0 / math.log2(3) + 1.0 + (1.0 + 1.0 / math.log2(5)) / ideal2
    assert abs(res["ndcg@4"] - want) < 1e-12 and abs(res["ndcg@30"] - want) < 1e-12      # any k, also past the candidates
    # the same numbers through metrics.py's own entry for predicted items
    topk = gm.get_topk_results([[2]] * 0 + [[c] for c in (1, 2, 3, 0)] + [[c] for c in (0, 2, 1, 3)] + [[c] for c in (3, 2, 1, 0)],
                               [4, 3, 2, 1] * 3, targets, 4)
    assert gm.get_metrics_results(topk, ["ndcg@4"], targets)["ndcg@4"] == pytest.approx(res["ndcg@4"], abs=1e-12)


def test_ties_rank_by_the_lower_candidate_index():
    scores = torch.tensor([[0.5, 0.5, 0.5, 0.7, 0.5]])
    assert ev.ranked_hits(scores, torch.tensor([[0, 0, 1, 0, 0]], dtype=torch.bool)) == [[0, 0, 0, 1, 0]]
    assert ev.target_ranks(scores, torch.tensor([[0, 0, 1, 0, 0]], dtype=torch.bool)).tolist() == [3]
    assert ev.target_ranks(scores, torch.tensor([[1, 0, 0, 0, 0]], dtype=torch.bool)).tolist() == [1]
    assert ev.target_ranks(scores, torch.tensor([[0, 0, 0, 0, 1]], dtype=torch.bool)).tolist() == [4]
    assert ev.target_ranks(scores, torch.zeros(1, 5, dtype=torch.bool)).tolist() == [5]
    # -inf padding ranks behind everything
    pad = torch.tensor([[float("-inf"), 0.0, float("-inf")]])
    assert ev.ranked_hits(pad, torch.tensor([[0, 1, 0]], dtype=torch.bool)) == [[1, 0, 0]]


def test_sampler_excludes_history_and_targets_and_is_reproducible():
    n_items, num_neg = 60, 20
    targets = [[5, 5, 7], [9], [11, 12]]                  # user 0 holds a duplicated target
    history = [{1, 2, 3, 5}, set(range(20, 50)), set()]
    cand = ev.sample_candidates(n_items, targets, history, num_neg, torch.Generator().manual_seed(7))
    assert cand.shape == (3, 2 + num_neg)
    assert cand[0, :2].tolist() == [5, 7] and cand[1, :1].tolist() == [9] and cand[2, :2].tolist() == [11, 12]
    for b, (tg, his) in enumerate(zip(targets, history)):
        n_t = len(set(tg))
        neg = cand[b, n_t:n_t + num_neg].tolist()
        assert len(set(neg)) == num_neg and all(0 <= i < n_items for i in neg)
        assert not set(neg) & (set(tg) | his)
        assert cand[b, n_t + num_neg:].tolist() == [-1] * (2 - n_t)
    again = ev.sample_candidates(n_items, targets, history, num_neg, torch.Generator().manual_seed(7))
    other = ev.sample_candidates(n_items, targets, history, num_neg, torch.Generator().manual_seed(8))
    assert torch.equal(cand, again) and not torch.equal(cand, other)
    with pytest.raises(ValueError, match="negatives"):
        ev.sample_candidates(n_items, [[9]], [set(range(20, 50))], 40, torch.Generator().manual_seed(0))


def test_history_items_are_read_from_the_prompt():
    catalogue = torch.tensor([[10, 20, 30], [11, 21, 31], [12, 22, 32], [10, 21, 32]])
    index = ev.catalogue_index(catalogue)
    ids = torch.tensor([[0, 0, 5, 10, 20, 30, 6, 12, 22, 32, 5],
                        [5, 10, 21, 32, 5, 10, 21, 32, 5, 11, 20]])
    assert ev.history_items(ids, index, 3) == [{0, 2}, {3}]


class _Engine:
    device = "cpu"


def _batch():
    return dict(input_ids=torch.tensor([[5, 10, 20, 30, 5], [5, 12, 22, 32, 5]]), attention_mask=torch.ones(2, 5, dtype=torch.int64),
                actions=torch.zeros(2, 5, dtype=torch.int64), targets=[[[11, 21, 31]], [[10, 21, 32]]])


def test_beam_mode_is_the_old_path(monkeypatch):
    seen = {}

    def fake_beam(engine, ids, am, act, trie, num_beams, item_len, **kw):
        seen["beam"] = seen.get("beam", 0) + 1
        seqs = torch.tensor([[5, 11, 21, 31], [5, 10, 20, 30], [5, 12, 22, 32], [5, 10, 21, 32]])
        return seqs, torch.tensor([-1.0, -2.0, -1.0, -2.0])

    def no_scoring(*a, **k):
        raise AssertionError("mode='beam' must not score items")
    monkeypatch.setattr(ev, "beam_search", fake_beam)
    monkeypatch.setattr(ev, "score_items", no_scoring)
    default = ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1", "hit@2"], item_len=3)
    named = ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1", "hit@2"], item_len=3, mode="beam")
    assert seen["beam"] == 2 and default == named == {"hit@1": 0.5, "hit@2": 1.0, "samples": 2}
    with pytest.raises(ValueError, match="mode"):
        ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1"], item_len=3, mode="full")
    with pytest.raises(ValueError, match="catalogue"):
        ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1"], item_len=3, mode="exact")


def test_exact_and_sampled_modes_rank_through_score_items(monkeypatch):
    catalogue = torch.tensor([[10, 20, 30], [11, 21, 31], [12, 22, 32], [10, 21, 32], [13, 23, 33], [14, 24, 34]])
    calls = []

    def fake_scores(engine, ids, am, act, items, session_ids=None, extended_session_ids=None, max_rows=65536):
        calls.append(tuple(items.shape))
        it = items if items.dim() == 3 else items[None].expand(ids.shape[0], *items.shape)
        return -(it[:, :, 0].float() - 11.0).abs()           # the closer the first code is to 11, the better

    def no_beams(*a, **k):
        raise AssertionError("no beam search in the scoring modes")
    monkeypatch.setattr(ev, "score_items", fake_scores)
    monkeypatch.setattr(ev, "beam_search", no_beams)
    res = ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1", "hit@3", "hit@4"], item_len=3, mode="exact",
                               catalogue=catalogue)
    # user 0: target row 1 scores best; user 1: target row 3 ties with rows 0 and 2 behind row 1 -> fourth, by its index
    assert res == {"hit@1": 0.5, "hit@3": 0.5, "hit@4": 1.0, "samples": 2} and calls == [(6, 3)]
    calls.clear()
    a = ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1", "hit@3"], item_len=3, mode="sampled", catalogue=catalogue,
                             num_neg=3, seed=1)
    b = ev.evaluate_behavior(_Engine(), [_batch()], None, 2, ["hit@1", "hit@3"], item_len=3, mode="sampled", catalogue=catalogue,
                             num_neg=3, seed=1)
    assert a == b and calls == [(2, 4, 3), (2, 4, 3)] and a["hit@1"] >= 0.5 and a["samples"] == 2


def test_train_cli_flags():
    from gamer_amd import train
    args = train.parse_args([])
    assert args.eval_mode is None and args.eval_num_neg == 1000
    args = train.parse_args(["--eval_mode", "sampled", "--eval_num_neg", "50"])
    assert args.eval_mode == "sampled" and args.eval_num_neg == 50
    with pytest.raises(SystemExit):
        train.parse_args(["--eval_mode", "full"])
