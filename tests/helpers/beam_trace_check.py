"""Check a trie-constrained beam search step by step against an independent scorer, within a stated noise bound.

``beam_search(..., return_trace=True)`` returns, per step, what it kept per user: ``(parent [B, nb], token [B, nb],
running_score [B, nb])``, best first.  Two implementations of one low-precision arithmetic do not keep the same beams when
candidates lie closer than their noise, so "the same beams as a reference" is not a property a bf16 search can be held to.
What it CAN be held to, given a scorer whose log-probabilities are within ``eps`` of the search's own:

  * every kept (parent, token) extends a kept prefix by one of its trie children, and no pair is kept twice;
  * |kept running score - (the parent's running score in the trace + the rescored log-prob)| <= eps;
  * the pruning is justified: min(kept, rescored) >= max(dropped candidates, rescored) - 2 eps;
  * as many candidates are kept as there are (up to the beam count), the kept scores are sorted, only beam 0 is a parent at
    step 0, and the final score is the last running score / number of new tokens.

Beam slots the search fills when a user has fewer candidates than beams carry a running score of about -1e9 (only beam 0 is
live at the first step) or -inf; they are "dead" here: never a parent of a candidate, never a kept candidate.

``scorer(step, prefixes)``: ``prefixes`` int64 [B, n, step] (n = 1 at step 0, else the beam count: the prefixes kept by the
previous step, dead slots included) -> log-probabilities of the next token [B, n, V].
``eps``: a float, or a callable evaluated after each scorer call (a bound that depends on the scorer's own logits).
"""
import torch

DEAD = -1e8          # running scores below this belong to dead slots


def check_trace(trace, final_scores, trie, first_tokens, scorer, eps):
    """trace: list of (parent, token, running_score) CPU tensors [B, nb]; final_scores [B * nb]; trie: ``.get(prefix)`` -> the
    allowed next tokens after ``prefix`` (which starts with the user's ``first_tokens[b]``, the prompt's last token).
    Raises AssertionError naming the step, user and property; returns statistics of the run."""
    steps = len(trace)
    B, nb = trace[0][0].shape
    prefixes = torch.zeros(B, 1, 0, dtype=torch.int64)
    prev_score = torch.zeros(B, 1, dtype=torch.float64)
    stats = dict(pruned_steps=0, max_score_err=0.0, min_margin=float("inf"), max_candidates=0, eps=0.0)
    for s, (parent, token, score) in enumerate(trace):
        parent, token, score = parent.cpu().to(torch.int64), token.cpu().to(torch.int64), score.cpu().to(torch.float64)
        logp = scorer(s, prefixes).cpu().to(torch.float64)
        e = float(eps() if callable(eps) else eps)
        stats["eps"] = max(stats["eps"], e)
        assert logp.shape[:2] == prefixes.shape[:2], f"step {s}: the scorer returned {tuple(logp.shape)}"
        for b in range(B):
            where = f"step {s}, user {b}"
            live_prev = [i for i in range(prefixes.shape[1]) if float(prev_score[b, i]) > DEAD]
            if s == 0:
                assert live_prev == [0]
            cand = {}                                    # (parent slot, token) -> rescored running score
            for i in live_prev:
                for t in trie.get([int(first_tokens[b])] + prefixes[b, i].tolist()):
                    cand[(i, int(t))] = float(prev_score[b, i]) + float(logp[b, i, int(t)])
            stats["max_candidates"] = max(stats["max_candidates"], len(cand))
            sc = score[b]
            assert bool((sc[:-1] >= sc[1:]).all()), f"{where}: kept scores are not sorted: {sc.tolist()}"
            live = [j for j in range(nb) if float(sc[j]) > DEAD]
            assert live == list(range(len(live))), f"{where}: a dead slot ranks above a live one"
            assert len(live) == min(nb, len(cand)), f"{where}: {len(live)} live beams kept of {len(cand)} candidates, {nb} beams"
            kept = {}
            for j in live:
                pt = (int(parent[b, j]), int(token[b, j]))
                if s == 0:
                    assert pt[0] == 0, f"{where}: beam {j} continues beam {pt[0]}, only beam 0 is live at the first step"
                assert pt in cand, f"{where}: kept beam {j} = (parent {pt[0]}, token {pt[1]}) is not a trie child of a kept prefix"
                assert pt not in kept, f"{where}: (parent {pt[0]}, token {pt[1]}) is kept twice"
                kept[pt] = cand[pt]
                err = abs(float(sc[j]) - cand[pt])
                stats["max_score_err"] = max(stats["max_score_err"], err)
                assert err <= e, f"{where}: beam {j} running score {float(sc[j])} vs rescored {cand[pt]}: {err} > eps {e}"
            dropped = [v for pt, v in cand.items() if pt not in kept]
            if dropped:
                stats["pruned_steps"] += 1
                margin = min(kept.values()) - max(dropped)
                stats["min_margin"] = min(stats["min_margin"], margin)
                assert margin >= -2 * e, (f"{where}: a dropped candidate rescored {max(dropped)} beats a kept one rescored "
                                          f"{min(kept.values())} by more than 2 eps = {2 * e}")
        # the prefixes this step kept, in slot order (dead slots included: they are what the next scorer call is indexed by)
        n_prev = prefixes.shape[1]
        par = parent.clamp(0, n_prev - 1)
        prefixes = torch.cat([torch.gather(prefixes, 1, par[:, :, None].expand(B, nb, s)), token[:, :, None]], 2)
        prev_score = score
    final = final_scores.cpu().to(torch.float32).view(B, nb)
    last = trace[-1][2].cpu().to(torch.float32)
    assert torch.equal(final, last / steps), "the final scores are not the last running scores / number of new tokens"
    stats["prefixes"] = prefixes                          # [B, nb, steps]: the generated tokens of every returned beam
    return stats
