"""decode.score_items: exact log-likelihoods of given items on the cached decode path, against the cache-free scoring forward of
``prompt + item`` (the only way to get these numbers without it) and against ``beam_search``.

Fixtures: the decode fixtures of every model family (tests/golden/decode_*_small.npz; 48-item catalogue, G = 2, so 48 rows per
user are 96 query rows of a (sample, kv head) - past gamer_attn_decode's 64).  B = 3 users; Qwen3Multi's are users 1-3 of
behaviour 1: two whose target row has no lower-level prompt key (the uniform average over all keys), one that has, one of them
left-padded by 25 of 31 tokens.  The bar, 2e-5 absolute, is the one tests/test_decode.py holds the cached search to against the
re-run.  Measured maxima are printed.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

from gamer_amd import decode, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-5
USERS = [1, 2, 3]


def _fx(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta_json"]))


def _case(kind, matmul=None, dtype="f32"):
    """(engine, session class, prompts dict, items [C, T]) of a model family on its decode fixture."""
    from gamer_amd.engine import Engine
    kw = {} if matmul is None else dict(matmul=matmul)
    if kind in ("multi", "session"):
        from gamer_amd.config import Qwen3MultiConfig
        from oracle import qwen3multi_oracle as orc
        z, meta = _fx("decode_small" if kind == "multi" else "decode_session_small")
        ocfg = orc.OracleConfig.from_dict(meta["config"])
        sd = orc.init_state_dict(ocfg, seed=meta["weight_seed"])
        for k, v in sd.items():
            if v.dim() == 2:
                sd[k] = v * meta["weight_scale"]
        sd["model.embed_tokens.weight"][synthetic.PAD_ID] = 0
        eng = Engine(Qwen3MultiConfig(**meta["config"]), temperature=0.7, dtype=dtype,
                     **(dict(variant="session") if kind == "session" else {}), **kw)
        cls, tag, keys = decode.DecodeSession, "b1", ("input_ids", "attention_mask", "actions")
        if kind == "session":
            keys += ("session_ids", "extended_session_ids")
    elif kind == "qwen3":
        import qwen3_weights
        from gamer_amd.config import Qwen3Config
        z, meta = _fx("decode_qwen3_small")
        sd = qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"], scale=meta["weight_scale"])
        eng = Engine(Qwen3Config(**meta["config"]), temperature=0.7, variant="qwen3", **kw)
        cls, tag, keys = decode.Qwen3DecodeSession, "b1", ("input_ids", "attention_mask")
    elif kind == "qwen3moe":
        import qwen3moe_weights as mw
        from gamer_amd.config import Qwen3MoeConfig
        z, meta = _fx("decode_moe_small")
        sd = mw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
        eng = Engine(Qwen3MoeConfig(**meta["config"]), temperature=0.7, variant="qwen3moe", **kw)
        cls, tag, keys = decode.Qwen3MoeDecodeSession, "b1", ("input_ids", "attention_mask")
    elif kind == "qwen3moe_action":
        import qwen3moe_action_weights as aw
        from gamer_amd.config import Qwen3MoeActionConfig
        z, meta = _fx("decode_moe_action_small")
        sd = aw.init_state_dict(meta["config"], meta["weight_seed"], meta["weight_scale"])
        eng = Engine(Qwen3MoeActionConfig(**meta["config"]), temperature=0.7, variant="qwen3moe_action", **kw)
        cls, tag, keys = decode.Qwen3MoeActionDecodeSession, "m0", ("input_ids", "attention_mask")
    else:
        raise KeyError(kind)
    eng.load_state_dict(sd)
    meta["state_dict"] = sd
    p = {k: torch.from_numpy(z[f"{tag}_{k}"])[USERS] for k in keys}
    items = synthetic.item_tokens(torch.from_numpy(z["catalogue"]), 1, meta["codebook"])[:, 1:].contiguous()
    assert items.shape[0] >= 33 and items.shape[0] * (eng.cfg.num_attention_heads // eng.cfg.num_key_value_heads) > 64
    assert int((p["attention_mask"] == 0).sum(1).max()) >= 15            # a heavily left-padded user
    return eng, cls, p, items, meta


def _score(eng, p, items, **kw):
    return decode.score_items(eng, p["input_ids"], p["attention_mask"], p.get("actions"), items,
                              session_ids=p.get("session_ids"), extended_session_ids=p.get("extended_session_ids"), **kw)


def _rerun_scores(eng, cls, p, items):
    """The cache-free scoring forward of prompt + item for every (user, item): log-softmax at the T positions, mean (fp64).
    The generated tokens take the behaviour level and session id of the target behaviour token and the next extended ids, as in
    ``beam_search(use_cache=False)``."""
    dev = eng.device
    ids, am = p["input_ids"].to(dev), p["attention_mask"].to(dev)
    B, L0 = ids.shape
    it = items.to(dev)
    if it.dim() == 2:
        it = it[None].expand(B, *it.shape)
    C, T = it.shape[1:]
    N, S, V = B * C, L0 + T - 1, eng.cfg.vocab_size
    flat = torch.cat([ids[:, None, :].expand(B, C, L0), it[:, :, :T - 1]], 2).reshape(N, S).contiguous()
    am_ = torch.cat([am, am.new_ones(B, T - 1)], 1).repeat_interleave(C, 0)
    act = None
    if "actions" in p:
        a0 = p["actions"].to(dev)
        act = torch.cat([a0, a0[:, -1:].expand(B, T - 1)], 1).repeat_interleave(C, 0)
    sess = {}
    if "session_ids" in p:
        sid0, ext0 = p["session_ids"].to(dev), p["extended_session_ids"].to(dev)
        ext = torch.cat([ext0, ext0[:, -1:] + torch.arange(1, T, device=dev)[None, :]], 1)
        sess = dict(session_ids=torch.cat([sid0, sid0[:, -1:].expand(B, T - 1)], 1).repeat_interleave(C, 0),
                    extended_session_ids=ext.repeat_interleave(C, 0))
    cls._eval_forward(eng, flat, am_, act, sess, L0)
    lg = eng.ws.logits[:N * S].view(N, S, -1)[:, L0 - 1:, :V].double()
    lp = torch.log_softmax(lg, -1).gather(2, it.reshape(N, T, 1)).squeeze(2)
    return lp.mean(1).view(B, C).cpu()


@pytest.mark.parametrize("kind,matmul", [("multi", "split3"), ("multi", "f32"), ("session", None), ("qwen3", None),
                                         ("qwen3moe", None), ("qwen3moe_action", None)])
def test_scores_match_the_cache_free_forward(kind, matmul):
    eng, cls, p, items, _ = _case(kind, matmul)
    if kind == "multi":
        lv = p["actions"][:, -1:]
        empty = ~(((p["actions"][:, :-1] < lv) & (p["attention_mask"][:, :-1] == 1)).any(1))
        assert empty.any() and not empty.all()               # uniform target rows and an ordinary one
    if kind == "qwen3moe_action":
        assert len(set(p["input_ids"][:, -1].tolist())) > 1  # target behaviours differ: a step's rows sit in several experts
    if kind in ("qwen3", "qwen3moe"):
        assert len(set((p["attention_mask"] == 0).sum(1).tolist())) > 1      # per-row RoPE offsets
    got = _score(eng, p, items).cpu().double()
    ref = _rerun_scores(eng, cls, p, items)
    err = float((got - ref).abs().max())
    print(f"score_items vs cache-free forward, {kind} {matmul or eng.matmul}: max abs err {err:.3e}")
    assert got.shape == (len(USERS), items.shape[0]) and err < BAR, err
    # a list per user (here: every user's catalogue in another order) gives the same numbers as the shared list
    per_user = torch.stack([items.roll(b, 0) for b in range(len(USERS))])
    got_b = _score(eng, p, per_user).cpu().double()
    back = torch.stack([got_b[b].roll(-b, 0) for b in range(len(USERS))])
    assert float((back - got).abs().max()) < BAR
    assert torch.equal(_score(eng, p, items[None].expand(len(USERS), *items.shape).contiguous()).cpu().double(), got)


def test_scores_match_beam_search_and_bound_it():
    eng, cls, p, items, meta = _case("multi")
    B, beams, T = len(USERS), meta["beams"], items.shape[1]
    trie = decode.ItemTrie(torch.cat([p["input_ids"][:1, -1:].expand(items.shape[0], 1), items], 1).tolist())
    seq, sc = decode.beam_search(eng, p["input_ids"], p["attention_mask"], p["actions"], trie, beams, T, reorder_cross_cache=True)
    found = seq[:, -T:].view(B, beams, T)
    got = _score(eng, p, found)
    err = float((got - sc.view(B, beams)).abs().max())
    print(f"score_items vs beam_search scores: max abs err {err:.3e}")
    assert err < BAR, err
    exact = _score(eng, p, items)
    assert bool((exact.max(1).values >= sc.view(B, beams)[:, 0] - BAR).all())


def test_chunks_share_one_prompt_pass(monkeypatch):
    eng, cls, p, items, _ = _case("multi")
    one = _score(eng, p, items)
    calls = []
    orig = eng.forward

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(eng, "forward", counted)
    B, C = len(USERS), items.shape[0]
    three = _score(eng, p, items, max_rows=B * (-(-C // 3)))
    assert len(calls) == 1
    st = next(iter(eng._score_static.values()))
    assert st.gen[next(iter(st.gen))][0].shape[0] == B * (-(-C // 3))        # caches sized by the chunk, not by C
    err = float((three - one).abs().max())
    print(f"score_items three chunks vs one: max abs diff {err:.3e}")
    assert err < BAR, err
    ragged = _score(eng, p, items[:-5], max_rows=B * 16)                      # 43 candidates in chunks of 15: a padded last chunk
    assert float((ragged - one[:, :-5]).abs().max()) < BAR


def test_beam_search_buffers_are_not_disturbed():
    eng, cls, p, items, meta = _case("multi")
    beams, T = meta["beams"], items.shape[1]
    trie = decode.ItemTrie(torch.cat([p["input_ids"][:1, -1:].expand(items.shape[0], 1), items], 1).tolist())
    run = lambda: decode.beam_search(eng, p["input_ids"], p["attention_mask"], p["actions"], trie, beams, T)
    seq0, sc0 = run()
    keys = list(eng._decode_static)
    _score(eng, p, items)
    _score(eng, p, items[:beams])                            # ... also at the beam search's own rows-per-user count
    assert list(eng._decode_static) == keys
    seq1, sc1 = run()
    assert torch.equal(seq0, seq1) and torch.equal(sc0, sc1)


def test_bf16_engine_is_refused_by_name():
    eng, cls, p, items, _ = _case("multi", dtype="bf16")
    with pytest.raises(NotImplementedError, match="score_items"):
        _score(eng, p, items)


def test_module_method():
    from gamer_amd.config import Qwen3MultiConfig
    from gamer_amd.modeling import Qwen3MultiWithTemperature
    eng, cls, p, items, meta = _case("multi")
    model = Qwen3MultiWithTemperature(Qwen3MultiConfig(**meta["config"]))
    model.set_hyper(0.7)
    model.load_state_dict(meta["state_dict"])
    got = model.score_items(input_ids=p["input_ids"], attention_mask=p["attention_mask"], actions=p["actions"], items=items)
    assert float((got.cpu() - _score(eng, p, items).cpu()).abs().max()) < BAR


def test_evaluation_modes_rank_with_exact_scores():
    """evaluate_behavior(mode="exact" / "sampled") on the engine: a user's target ranks where its exact score puts it."""
    from gamer_amd.evaluate import evaluate_behavior, target_ranks
    eng, cls, p, items, meta = _case("multi")
    scores = _score(eng, p, items).cpu()
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    targets = [[items[order[0, 0]].tolist()], [items[order[1, 2]].tolist()], [items[order[2, 9]].tolist()]]      # ranks 0, 2, 9
    batch = dict(p, targets=targets)
    res = evaluate_behavior(eng, [batch], None, metric_list=["hit@1", "hit@3", "hit@10", "ndcg@10"], item_len=items.shape[1],
                            mode="exact", catalogue=items)
    assert res["samples"] == 3 and res["hit@1"] == pytest.approx(1 / 3) and res["hit@3"] == pytest.approx(2 / 3) and res["hit@10"] == 1.0
    assert res["ndcg@10"] == pytest.approx((1.0 + 1.0 / np.log2(4) + 1.0 / np.log2(11)) / 3, abs=1e-9)
    # sampled: 10 negatives outside the prompt's items; user 0's target is the best of the whole catalogue, so of any sample
    res = evaluate_behavior(eng, [batch], None, metric_list=["hit@1", "hit@11"], item_len=items.shape[1], mode="sampled",
                            catalogue=items, num_neg=10, seed=3)
    assert res["hit@11"] == 1.0 and res["hit@1"] >= 1 / 3 - 1e-12
    is_target = torch.zeros_like(scores, dtype=torch.bool)
    for b, r in enumerate((0, 2, 9)):
        is_target[b, order[b, r]] = True
    assert target_ranks(scores, is_target).tolist() == [0, 2, 9]
