"""tiger.score_items / pbatransformer.score_items on the GPU: the exact log-likelihood of given items against HF's ``generate`` (the
reference beams and scores of tests/golden/tiger_small.npz), against the fixture's teacher-forced logits, against the model's own
``forward`` and ``beam_search``, across chunking, packed rows and the long-encoder fallback, with PBATransformer's routed FFNs, and
the train command's --eval_mode.

Bars.  Fixture numbers: relative error < 1e-3, the bar test_beam_search_finds_generates_beams holds beam_search to on the same scores.
The model's own forward / beam_search / another chunking: |difference| < 2e-5 on mean log-probabilities of O(1..10), the bar of
tests/test_score_items_gpu.py for the same comparisons (fp32 sums in another order)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_pbatransformer_gpu as tp  # noqa: E402  (the model builders and fixtures of the two backbones' own tests)
import test_tiger_gpu as tt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = tt.DEV
BAR = 2e-5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


@pytest.fixture(scope="module")
def fx():
    z = np.load(tt.FX)
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def pfx():
    z = np.load(tp.FX)
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def model(fx):
    return tt._model(fx, "a")[0]


def _batch(fx, n=3):
    z, _ = fx
    return torch.from_numpy(z["a/input_ids"][:n]).to(DEV), torch.from_numpy(z["a/attention_mask"][:n]).to(DEV)


def _forward_scores(m, ids, am, items, prefix):
    """mean over the T positions of log_softmax(forward logits)[item token]: items [B, C, T], prefix [B, P] -> [B, C] (fp64 sums)"""
    B, C, T = items.shape
    P = prefix.shape[1]
    dec_in = torch.cat([prefix[:, None, :].expand(B, C, P), items[:, :, :T - 1]], 2).reshape(B * C, P + T - 1)
    m.eval()
    with torch.no_grad():
        _, logits = m(ids.repeat_interleave(C, 0), am.repeat_interleave(C, 0), decoder_input_ids=dec_in.to(DEV))
    lp = torch.log_softmax(logits[:, P - 1:, :].double(), -1).gather(2, items.reshape(B * C, T, 1).to(DEV))[..., 0]
    return lp.mean(1).view(B, C)


def _items(B, C, T, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (B, C, T), generator=g, dtype=torch.int64)


# ---- against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [4, 20])
@pytest.mark.parametrize("tag", ["plain", "prefix"])
def test_reference_beams_get_generates_scores(fx, model, tag, nb):
    from gamer_amd import tiger
    z, _ = fx
    ids, am = _batch(fx)
    prefix = torch.from_numpy(z[f"a/prefix_{tag}"])
    P = prefix.shape[1]
    beams = torch.from_numpy(z[f"a/beams_{tag}_{nb}"])
    assert torch.equal(beams[:, :P].view(3, nb, P), prefix[:, None, :].expand(3, nb, P))
    items = beams[:, P:].reshape(3, nb, -1).contiguous()
    got = tiger.score_items(model, ids, am, items, decoder_prefix=None if tag == "plain" else prefix)
    err = tt._rel(got.reshape(-1), torch.from_numpy(z[f"a/scores_{tag}_{nb}"]))
    print(f"score_items vs generate's sequences_scores ({tag}, {nb} beams): rel {err:.3e}")
    assert got.shape == (3, nb) and got.dtype == torch.float32 and err < 1e-3


def test_teacher_forced_fixture_logits(fx, model):
    """a/logits are the reference's un-tempered lm_head outputs (test_forward_without_labels_gives_the_logits compares the model's
    un-tempered logits with them; the temperature 0.7 only enters its loss), which is what score_items is defined on.  Labels past
    </s> are -100; the reference's decoder input holds the pad token there, so the item is the label row with pad in their place:
    the same decoder input, every one of the T positions compared."""
    from gamer_amd import tiger
    z, _ = fx
    ids, am = _batch(fx, 5)
    tokens = torch.from_numpy(z["a/labels"]).clamp(min=0)
    want = torch.log_softmax(torch.from_numpy(z["a/logits"]).double(), -1).gather(2, tokens[:, :, None])[..., 0].mean(1)
    got = tiger.score_items(model, ids, am, tokens[:, None, :].contiguous())
    err = tt._rel(got[:, 0], want)
    print(f"score_items vs the fixture's teacher-forced logits: rel {err:.3e}")
    assert err < 1e-3


# ---- against the model's own forward and beam search --------------------------------------------------------------------------------
def test_forward_and_beam_search_agree(fx, model):
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    z, _ = fx
    ids, am = _batch(fx)
    items = _items(3, 7, 5, 2, 120, 3)
    start = torch.zeros(3, 1, dtype=torch.int64)
    got = tiger.score_items(model, ids, am, items)
    d_fwd = float((got.double() - _forward_scores(model, ids, am, items, start)).abs().max())
    trie = ItemTrie(z["a/trie_plain"].tolist(), device=DEV, pad_token_id=0)
    seqs, sc = tiger.beam_search(model, ids, am, trie, 4, 5)
    d_beam = float((tiger.score_items(model, ids, am, seqs[:, 1:].reshape(3, 4, 5).contiguous()) - sc.view(3, 4)).abs().max())
    # per-user prefixes (the behaviour token of the SMB / MB tasks)
    prefix = torch.from_numpy(z["a/prefix_prefix"])
    it4 = _items(3, 7, 4, 2, 120, 4)
    d_pre = float((tiger.score_items(model, ids, am, it4, decoder_prefix=prefix).double()
                   - _forward_scores(model, ids, am, it4, prefix)).abs().max())
    print(f"score_items: |d| vs forward {d_fwd:.3e}, vs beam_search's sequences_scores {d_beam:.3e}, with a [B, 2] prefix vs forward {d_pre:.3e}")
    assert d_fwd < BAR and d_beam < BAR and d_pre < BAR


def test_chunks_and_shared_lists(fx, model):
    from gamer_amd import tiger
    ids, am = _batch(fx)
    items = _items(3, 7, 5, 2, 120, 5)
    one = tiger.score_items(model, ids, am, items)
    three = tiger.score_items(model, ids, am, items, max_rows=9)             # 3 per user: chunks of 3, 3, 1 + 2 repeats
    shared = tiger.score_items(model, ids, am, items[0])
    expanded = tiger.score_items(model, ids, am, items[0][None].expand(3, -1, -1).contiguous())
    d_chunk, d_list = float((one - three).abs().max()), float((shared - expanded).abs().max())
    print(f"score_items: three chunks vs one {d_chunk:.3e}, [C, T] vs [B, C, T] {d_list:.3e}")
    assert one.shape == three.shape == (3, 7) and d_chunk < BAR and d_list < BAR
    assert float((shared[0] - one[0]).abs().max()) < BAR


def test_packed_rows_and_the_long_encoder(fx, model):
    from gamer_amd import tiger
    ids, am = _batch(fx, 5)
    assert len(set(am.sum(1).tolist())) > 1                                   # rows of different lengths
    items = _items(5, 7, 5, 2, 120, 6)
    dense = tiger.score_items(model, ids, am, items)
    packed = tiger.score_items(model, ids, am, items, packed=True)
    packed_l = tiger.score_items(model, ids, am, items, packed=True, lengths=am.sum(1).cpu())
    d_pack = float((dense - packed).abs().max())
    g = torch.Generator().manual_seed(7)
    lids = torch.randint(2, 120, (3, 200), generator=g)
    lam = torch.ones(3, 200, dtype=torch.int64)
    lam[1, 150:], lam[2, 129:] = 0, 0
    lids = (lids * lam).to(DEV)
    lam = lam.to(DEV)
    lit = _items(3, 7, 5, 2, 120, 8)
    start = torch.zeros(3, 1, dtype=torch.int64)
    want = _forward_scores(model, lids, lam, lit, start)
    d_long = float((tiger.score_items(model, lids, lam, lit).double() - want).abs().max())
    d_long_p = float((tiger.score_items(model, lids, lam, lit, packed=True).double() - want).abs().max())
    print(f"score_items: packed vs dense {d_pack:.3e}; 200 encoder tokens vs forward {d_long:.3e} (packed {d_long_p:.3e})")
    assert d_pack < BAR and torch.equal(packed, packed_l) and d_long < BAR and d_long_p < BAR


# ---- PBATransformer -----------------------------------------------------------------------------------------------------------------
def test_pbatransformer_routes_every_candidate_by_its_own_tokens(pfx):
    from gamer_amd import pbatransformer
    z, meta = pfx
    m, _ = tp._model(pfx, "a")
    ids, am = torch.from_numpy(z["a/input_ids"]).to(DEV), torch.from_numpy(z["a/attention_mask"]).to(DEV)
    b0, b1 = meta["behaviour_tokens"]
    prefix = torch.tensor([[0, b0], [0, b1], [0, b0]], dtype=torch.int64)     # users of mixed target behaviours
    items = torch.cat([_items(3, 7, 3, 20, 64, 9), torch.ones(3, 7, 1, dtype=torch.int64)], 2)      # 3 item tokens + </s>
    got = pbatransformer.score_items(m, ids, am, items, decoder_prefix=prefix)
    d = float((got.double() - _forward_scores(m, ids, am, items, prefix)).abs().max())
    print(f"pbatransformer.score_items vs forward {d:.3e}")
    assert d < BAR
    with pytest.raises(ValueError, match="behavior_maps"):
        pbatransformer.score_items(m, ids, am, items, decoder_prefix=torch.tensor([[0, 40]] * 3))
    m.check_inputs()                                                          # the counter was cleared by the raise
    with pytest.raises(NotImplementedError, match="packed"):
        pbatransformer.score_items(m, ids, am, items, decoder_prefix=prefix, packed=True)


# ---- side effects and refusals ----------------------------------------------------------------------------------------------------------
def test_no_side_effects_and_bad_arguments(fx, model):
    from gamer_amd import tiger
    from gamer_amd.decode import ItemTrie
    z, _ = fx
    ids, am = _batch(fx)
    trie = ItemTrie(z["a/trie_plain"].tolist(), device=DEV, pad_token_id=0)
    before = tiger.beam_search(model, ids, am, trie, 4, 5)
    items = _items(3, 7, 5, 2, 120, 10)
    model.train()
    try:
        tiger.score_items(model, ids, am, items)
        assert model.training
        after = tiger.beam_search(model, ids, am, trie, 4, 5)
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and model.training
        with pytest.raises(RuntimeError, match="HIP device only"):
            tiger.score_items(model, ids.cpu(), am.cpu(), items)
        assert model.training                                                 # restored after an exception
    finally:
        model.eval()
    bad = [(dict(items=items.to(torch.int32)), ValueError), (dict(items=items[0, 0]), ValueError),
           (dict(items=items[:, :0]), ValueError), (dict(items=items[:2]), ValueError), (dict(items=items, max_rows=2), ValueError),
           (dict(items=_items(3, 2, 9, 2, 120, 1)), NotImplementedError),
           (dict(items=_items(3, 2, 8, 2, 120, 1), decoder_prefix=torch.tensor([0, 5])), NotImplementedError),
           (dict(items=items, decoder_prefix=torch.zeros(2, 1, dtype=torch.int64)), ValueError)]
    for kw, exc in bad:
        with pytest.raises(exc):
            tiger.score_items(model, ids, am, **kw)
    assert tiger.score_items(model, ids, am, _items(3, 2, 8, 2, 120, 1)).shape == (3, 2)      # P + T - 1 = MAX_DECODER_LEN runs


# ---- the train command --------------------------------------------------------------------------------------------------------------
def test_train_tiger_eval_modes_end_to_end(tmp_path):
    from gamer_amd import synthetic, train_tiger
    root = tmp_path / "data"
    synthetic.write_seqrec_dataset(str(root), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=32, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128)))
    res_file = tmp_path / "res.json"
    common = ["--base_model", str(base), "--data_path", str(root), "--dataset", "Toy", "--max_his_len", "10", "--output_dir",
              str(tmp_path / "ckpt"), "--per_device_batch_size", "64", "--test_batch_size", "16", "--num_beams", "10", "--metrics",
              "hit@1,hit@10,ndcg@10,hit@60", "--results_file", str(res_file)]
    train_tiger.main(common + ["--epochs", "1", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    beam = json.loads(res_file.read_text())
    assert "eval_mode" not in beam                                            # no flag: the file it always wrote
    exact = train_tiger.main(common + ["--only_test", "--eval_mode", "exact"])
    assert json.loads(res_file.read_text()) == exact and exact["eval_mode"] == "exact" and "num_neg" not in exact
    assert all(np.isfinite(exact[k]) and 0.0 <= exact[k] <= 1.0 for k in ("hit@1", "hit@10", "ndcg@10"))
    assert exact["hit@60"] == 1.0                                             # k = the catalogue: every target is found
    sampled = train_tiger.main(common + ["--only_test", "--eval_mode", "sampled", "--eval_num_neg", "5"])
    assert sampled["eval_mode"] == "sampled" and sampled["num_neg"] == 5 and json.loads(res_file.read_text()) == sampled
    assert all(np.isfinite(sampled[k]) for k in ("hit@1", "hit@10", "ndcg@10")) and sampled["hit@10"] == 1.0      # 6 candidates
    assert train_tiger.main(common + ["--only_test", "--eval_mode", "sampled", "--eval_num_neg", "5"]) == sampled   # seeded draw


def test_the_logits_are_formed_in_pieces_with_a_partial_last_one(fx, model, monkeypatch):
    """score_items forms at most tiger._LOGIT_FLOATS logits at a time; here 5 rows of the 21 per position: pieces of 5, 5, 5, 5, 1"""
    from gamer_amd import tiger
    ids, am = _batch(fx)
    items = _items(3, 7, 5, 2, 120, 12)
    one = tiger.score_items(model, ids, am, items)
    monkeypatch.setattr(tiger, "_LOGIT_FLOATS", 5 * model.shared.weight.shape[0])
    pieces = tiger.score_items(model, ids, am, items)
    d = float((one - pieces).abs().max())
    print(f"score_items: logits in pieces of 5 rows vs one piece {d:.3e}")
    assert d < BAR


def _ranked_runs(main, common, res_file, k_all):
    """--only_test under exact and sampled on a trained checkpoint: the rows carry the mode, exact finds every target at k = the
    catalogue, the sampled draw is seeded"""
    exact = main(common + ["--only_test", "--eval_mode", "exact"])
    assert json.loads(res_file.read_text()) == exact and len(exact) >= 1
    for row in exact:
        assert row["eval_mode"] == "exact" and "num_neg" not in row and row[f"hit@{k_all}"] == 1.0
        assert all(np.isfinite(row[m]) and 0.0 <= row[m] <= 1.0 for m in ("hit@1", "ndcg@5"))
    sampled = main(common + ["--only_test", "--eval_mode", "sampled", "--eval_num_neg", "5"])
    for row in sampled:
        assert row["eval_mode"] == "sampled" and row["num_neg"] == 5 and row[f"hit@{k_all}"] == 1.0 and np.isfinite(row["ndcg@5"])
    assert main(common + ["--only_test", "--eval_mode", "sampled", "--eval_num_neg", "5"]) == sampled
    return exact, sampled


def _base(tmp_path, **extra):
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128, **extra)))
    return base


def _common(tmp_path, base, task, res_file):
    return ["--base_model", str(base), "--data_path", str(tmp_path / "data"), "--dataset", "Toy", "--tasks", task, "--max_his_len", "8",
            "--output_dir", str(tmp_path / "ckpt"), "--per_device_batch_size", "32", "--gradient_accumulation_steps", "1",
            "--test_batch_size", "16", "--num_beams", "10", "--metrics", "hit@1,ndcg@5,hit@60", "--results_file", str(res_file)]


def test_train_tiger_smb_eval_modes_end_to_end(tmp_path):
    from gamer_amd import synthetic, train_tiger_smb
    synthetic.write_smb_dataset(str(tmp_path / "data"), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    res_file = tmp_path / "res.json"
    common = _common(tmp_path, _base(tmp_path), "smb_explicit", res_file)
    beam = train_tiger_smb.main(common + ["--epochs", "1", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    assert all("eval_mode" not in r for r in beam)
    exact, sampled = _ranked_runs(train_tiger_smb.main, common, res_file, 60)
    assert [r["eval_type"] for r in exact] == [r["eval_type"] for r in beam]         # the layout of the beam file
    assert all(0.0 <= r["Avg. Duplicate Ratio"] <= 1.0 for r in exact[:-1] + sampled[:-1])


def test_train_tiger_mb_eval_modes_end_to_end(tmp_path):
    from gamer_amd import synthetic, train_tiger_mb
    synthetic.write_mb_dataset(str(tmp_path / "data"), "Toy", n_users=40, n_items=60, codebook=8, seed=0)
    res_file = tmp_path / "res.json"
    common = _common(tmp_path, _base(tmp_path), "mb_explicit", res_file)
    beam = train_tiger_mb.main(common + ["--epochs", "1", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    exact, _ = _ranked_runs(train_tiger_mb.main, common, res_file, 60)
    assert [r["eval_type"] for r in exact] == [r["eval_type"] for r in beam] == ["Target Behavior"]


def test_train_pbatransformer_eval_modes_end_to_end(tmp_path):
    from gamer_amd import synthetic, train_pbatransformer
    synthetic.write_smb_dataset(str(tmp_path / "data"), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    base = _base(tmp_path, behavior_injection=True, behavior_embedding_dim=16, sparse_layers_encoder=[], sparse_layers_decoder=[0, 1],
                 behavior_injection_encoder=[0], behavior_injection_decoder=[0], model_type="switch_transformers")
    res_file = tmp_path / "res.json"
    common = _common(tmp_path, base, "smb_explicit", res_file)
    train_pbatransformer.main(common + ["--epochs", "1", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    _ranked_runs(train_pbatransformer.main, common, res_file, 60)
