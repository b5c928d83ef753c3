"""TIGER on the SMB / MB multi-behaviour data on the GPU, against the real reference class at the real T5 vocabulary (32,100 + the
new tokens; tests/golden/tiger_smb.npz, tools/make_golden_tiger_smb.py): the model on batches that gamer_amd/t5_mb_data.py collates from
the regenerated datasets (one on the resident attention family, one on the key-streaming family, one MB batch), beam search per
behaviour against HF's ``generate``, and the two commands end to end.

Bars: those of tests/test_tiger_gpu.py / tests/test_tiger_long_gpu.py.  Model: per batch, twice the worst error of an fp32 torch
restatement of the whole model (tests/helpers/t5_attention_ref.py) against the fixture, never above 1e-3; relative error = largest
absolute difference over the largest reference magnitude of the tensor.  Beams: equal sequences, scores within 1e-3."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import t5_attention_ref as ref  # noqa: E402
import tiger_weights as tw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_smb.npz")
DEV = ref.DEV


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def datasets(fx, tmp_path_factory):
    """the fixture's two datasets, written again from their seeds -> (T5SMBData smb_explicit, T5MBData mb_explicit)"""
    from gamer_amd import synthetic, t5_mb_data
    _, meta = fx
    root = str(tmp_path_factory.mktemp("data"))
    synthetic.write_smb_dataset(root, meta["smb"]["name"], **meta["smb"]["kw"])
    synthetic.write_mb_dataset(root, meta["mb"]["name"], **meta["mb"]["kw"])
    return (t5_mb_data.T5SMBData(root, meta["smb"]["name"], "smb_explicit"), t5_mb_data.T5MBData(root, meta["mb"]["name"], "mb_explicit"))


@pytest.fixture(scope="module")
def models(fx):
    z, meta = fx
    return {name: ref.load_model(z, meta, name) for name in ("s", "m")}


def _collate(fx, datasets, tag):
    from gamer_amd import t5_mb_data
    z, meta = fx
    smb, mb = datasets
    data, index = (mb, meta["mb_index"]) if tag == "m/mb" else (smb, meta[tag.split("/")[1] + "_index"])
    assert data.vocab_size == meta["configs"][tag[0]]["vocab_size"] > 32100
    b = t5_mb_data.EncDecCollator(1024, data.token_count)(data.samples("train", meta["max_his_len"]), index)
    for k in ("input_ids", "attention_mask", "labels"):                   # the real collator's batch, bit for bit
        assert np.array_equal(b[k].numpy(), z[f"{tag}/{k}"]), (tag, k)
    return b["input_ids"], b["attention_mask"], b["labels"]


@pytest.mark.parametrize("tag", ["s/short", "s/long", "m/mb"])
def test_model_loss_logits_and_every_gradient_match_the_reference(fx, datasets, models, tag):
    """s/short: histories of 0, 1, 7 and 25 items, every row <= 128 tokens (the resident attention family); s/long: 0, 1, 26 and 30
    items = 1, 6, 131 and 151 tokens (the key-streaming family); m/mb: one mb_explicit batch.  The vocabulary is the real one, so
    the catalogue cross-entropy and the shared table's gradient run at V of about 32k."""
    from gamer_amd import tiger
    z, meta = fx
    name = tag[0]
    m, sd = models[name]
    ids, am, labels = _collate(fx, datasets, tag)
    lens = am.sum(1).tolist()
    if tag == "s/short":
        assert lens == [5 * n + 1 for n in meta["short_hist"]] and ids.shape[1] <= tiger.MAX_ENCODER_LEN
    elif tag == "s/long":
        assert lens == [5 * n + 1 for n in meta["long_hist"]] and ids.shape[1] == 5 * meta["max_his_len"] + 1 > tiger.MAX_ENCODER_LEN
        assert 131 in lens
    m.train()                                                       # (dropout_rate 0: the training path, CatalogCEFn and all)
    for p in m.parameters():
        p.grad = None
    loss, logits = m(ids.to(DEV), am.to(DEV), labels=labels.to(DEV), want_logits=True)
    loss.backward()
    r_loss, r_logits, r_grads = ref.restated_model(sd, meta["configs"][name], ids, am, labels, meta["temperature"])
    params = dict(m.named_parameters())
    assert set(params) == set(meta[name]["param_keys"]) and meta[name]["no_grad"] == []
    cols = torch.from_numpy(z[f"{tag}/logit_cols"]).to(DEV)
    on = (labels != -100).to(DEV)
    want_logits, want_sumsq = z[f"{tag}/logits"], float(z[f"{tag}/logits_sumsq"])
    kernel, torch32 = {}, {}
    for out, lg in ((kernel, logits), (torch32, r_logits)):
        rows = lg[on]
        assert rows.shape[1] == meta["configs"][name]["vocab_size"]
        out["logits"] = ref.rel_err(rows[:, cols], want_logits)
        out["sumsq/logits"] = 0.5 * abs(float((rows.double() ** 2).sum()) - want_sumsq) / want_sumsq
    ref_loss = float(z[f"{tag}/loss"])
    kernel["loss"], torch32["loss"] = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(float(r_loss) - ref_loss) / abs(ref_loss)
    for k, p in params.items():
        want_rows = torch.from_numpy(z[f"{tag}/grad/{k}"])
        rows = torch.from_numpy(z[f"{tag}/table_rows"]) if k == "shared.weight" else tw.sample_rows(p.shape)
        assert p.grad is not None and want_rows.shape[0] == rows.numel(), k
        kernel[k], torch32[k] = ref.rel_err(p.grad[rows.to(DEV)], want_rows), ref.rel_err(r_grads[k][rows.to(DEV)], want_rows)
        # the rows the fixture does not hold: the whole tensor's sum of squares, whose relative error is twice the values'
        want = float(z[f"{tag}/grad_checksum/{k}"][1])
        kernel["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: p.grad.cpu()})[0][1]) - want) / want
        torch32["sumsq/" + k] = 0.5 * abs(float(tw.checksums({k: r_grads[k].cpu()})[0][1]) - want) / want
    bar = min(2.0 * max(torch32.values()), 1e-3)
    worst = max(kernel, key=kernel.get)
    print(f"{tag}: kernel worst {kernel[worst]:.3e} ({worst}), logits {kernel['logits']:.3e}, loss {kernel['loss']:.3e}, table "
          f"{kernel['shared.weight']:.3e}; fp32 torch worst {max(torch32.values()):.3e}, logits {torch32['logits']:.3e}; bar {bar:.3e}")
    for k, e in kernel.items():
        assert e <= bar, (k, e, bar)


@pytest.mark.parametrize("nb", [4, 20])
def test_beam_search_per_behaviour_finds_generates_beams(fx, datasets, models, nb):
    """test_SMB_decoder.py's call: prefix [0, <behavior>], the behaviour's trie ([0] + <behavior> + item + </s>), max_new_tokens =
    sole_item_len, three users of different history length per behaviour"""
    from gamer_amd import t5_mb_data, tiger
    from gamer_amd.decode import ItemTrie
    z, meta = fx
    smb, _ = datasets
    m, _ = models["s"]
    base = smb.samples("test", meta["max_his_len"])
    coll = t5_mb_data.EncDecCollator(1024, smb.token_count)
    assert meta["s"]["smallest_gap"] > meta["gap"] and len(meta["beam_behaviors"]) == 2
    for b in meta["beam_behaviors"]:
        rec = meta["s"]["beams"][b]
        inputs, _ = coll.test(base.filter_by_behavior(b), rec["users"])
        assert inputs["attention_mask"].sum(1).tolist() == rec["enc_lens"] and len(set(rec["enc_lens"])) == 3
        seqs_all = smb.trie_sequences(b, 0)
        assert len(seqs_all) >= 20
        trie = ItemTrie(seqs_all, device=DEV, pad_token_id=0)
        prefix = torch.tensor([0, smb.behavior_token_ids[b]])
        seqs, scores = tiger.beam_search(m, inputs["input_ids"].to(DEV), inputs["attention_mask"].to(DEV), trie, nb, smb.sole_item_len,
                                         decoder_prefix=prefix)
        assert torch.equal(seqs.cpu(), torch.from_numpy(z[f"s/beams/{b}/{nb}"]).long()), (b, nb)
        err = ref.rel_err(scores, torch.from_numpy(z[f"s/scores/{b}/{nb}"]))
        print(f"behaviour {b}, {nb} beams: score error {err:.3e}")
        assert err < 1e-3


def test_mb_target_behaviour_search_finds_generates_beams(fx, datasets, models):
    """test_MB_decoder.py's target-behaviour call: prefix [0, <behavior_target>], the trie ends every item with </s>; generate is
    asked for 10 new tokens and stops at </s> after the item"""
    from gamer_amd import t5_mb_data, tiger
    from gamer_amd.decode import ItemTrie
    z, meta = fx
    _, mb = datasets
    m, _ = models["m"]
    rec = meta["m"]
    assert mb.target_behavior == rec["target_behavior"] and rec["smallest_gap"] > meta["gap"]
    inputs, _ = t5_mb_data.EncDecCollator(512).test(mb.test_samples(meta["max_his_len"], mb.target_behavior), rec["users"])
    assert inputs["attention_mask"].sum(1).tolist() == rec["enc_lens"]
    trie = ItemTrie(mb.trie_sequences(mb.target_behavior, 0), device=DEV, pad_token_id=0)
    prefix = torch.tensor(mb.decoder_prefix(0))
    seqs, scores = tiger.beam_search(m, inputs["input_ids"].to(DEV), inputs["attention_mask"].to(DEV), trie, 4, mb.token_count + 2 - len(prefix),
                                     decoder_prefix=prefix)
    want = torch.from_numpy(z["m/beams/4"]).long()
    assert bool((want[:, -1] == 1).all()) and torch.equal(seqs.cpu(), want)
    assert ref.rel_err(scores, torch.from_numpy(z["m/scores/4"])) < 1e-3


# ---- the commands end to end -----------------------------------------------------------------------------------------------------------
def _base_model(tmp_path):
    base = tmp_path / "base"
    base.mkdir()
    (base / "config.json").write_text(json.dumps(dict(d_model=64, d_kv=64, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=2,
                                                      dropout_rate=0.1, vocab_size=32128)))
    return base


def _epoch_losses(log, tag):
    rows = [l for l in log.splitlines() if l.startswith(f"[{tag}] epoch ")]
    return [float(l.split(" loss ")[1].split()[0]) for l in rows], [float(l.split(" eval_loss ")[1].split()[0]) for l in rows]


def _check_checkpoint(fx, path, vocab):
    """the keys and shapes of the real class resized to the same vocabulary"""
    _, meta = fx
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == meta["s"]["keys"]
    for k, shape in zip(meta["s"]["keys"], meta["s"]["shapes"]):
        assert list(sd[k].shape) == ([vocab] + shape[1:] if k in tw.TIED else shape), k


@pytest.mark.parametrize("task,accum", [("smb_explicit", "2"), ("smb_explicit_decoder_2", "1")])
def test_train_tiger_smb_end_to_end(fx, tmp_path, capsys, task, accum):
    """smb_explicit with the reference's default of two micro-batches per update; the augmented task's fewer samples step per batch"""
    from gamer_amd import synthetic, t5_mb_data, train_tiger_smb
    root = tmp_path / "data"
    synthetic.write_smb_dataset(str(root), "Toy", n_users=40, n_items=60, codebook=8, seed=1)
    out = tmp_path / "ckpt"
    metrics = "hit@1,hit@5,recall@5,ndcg@5"
    common = ["--base_model", str(_base_model(tmp_path)), "--data_path", str(root), "--dataset", "Toy", "--tasks", task, "--max_his_len", "8",
              "--output_dir", str(out), "--per_device_batch_size", "16", "--gradient_accumulation_steps", accum, "--test_batch_size", "16",
              "--num_beams", "10", "--metrics", metrics, "--results_file", str(tmp_path / "res.json")]
    res = train_tiger_smb.main(common + ["--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    train, _ = _epoch_losses(capsys.readouterr().out, "train_tiger_smb")
    assert len(train) == 2 and all(np.isfinite(train)) and train[1] < train[0], train
    data = t5_mb_data.T5SMBData(str(root), "Toy", task)
    _check_checkpoint(fx, out / "best_model.pth", data.vocab_size)
    assert [r["eval_type"] for r in res] == [f"Behavior {b}" for b in data.behaviors] + ["Merged Behavior"]
    rows, merged = res[:-1], res[-1]
    counts = [r["collision_info"]["total"] for r in rows]
    for m in metrics.split(","):
        assert all(0.0 <= r[m] <= 1.0 for r in rows)
        assert merged[m] == pytest.approx(sum(r[m] * n for r, n in zip(rows, counts)) / sum(counts), rel=1e-12, abs=1e-15)
    assert all(0.0 <= r["Avg. Duplicate Ratio"] <= 1.0 for r in rows) and "Avg. Duplicate Ratio" not in merged
    assert json.load(open(tmp_path / "res.json")) == res
    again = train_tiger_smb.main(common + ["--only_test"])
    assert again == res
    one = train_tiger_smb.main(common + ["--only_test", "--behaviors", data.behaviors[-1]])
    assert len(one) == 2 and {k: v for k, v in one[0].items()} == rows[-1]


def test_train_tiger_mb_end_to_end(fx, tmp_path, capsys):
    from gamer_amd import synthetic, t5_mb_data, train_tiger_mb
    root = tmp_path / "data"
    synthetic.write_mb_dataset(str(root), "Toy", n_users=40, n_items=60, codebook=8, seed=0)    # (six users end on the target behaviour)
    out = tmp_path / "ckpt"
    common = ["--base_model", str(_base_model(tmp_path)), "--data_path", str(root), "--dataset", "Toy", "--tasks", "mb_explicit", "--max_his_len",
              "8", "--output_dir", str(out), "--per_device_batch_size", "32", "--test_batch_size", "16", "--num_beams", "10",
              "--metrics", "hit@1,hit@5,ndcg@5", "--results_file", str(tmp_path / "res.json")]
    res = train_tiger_mb.main(common + ["--epochs", "2", "--learning_rate", "3e-3", "--warmup_ratio", "0.0"])
    train, _ = _epoch_losses(capsys.readouterr().out, "train_tiger_mb")
    assert len(train) == 2 and all(np.isfinite(train)) and train[1] < train[0], train
    data = t5_mb_data.T5MBData(str(root), "Toy", "mb_explicit")
    _check_checkpoint(fx, out / "best_model.pth", data.vocab_size)
    assert len(res) == 1 and res[0]["eval_type"] == "Target Behavior" and res[0]["collision_info"]["total"] > 0
    assert all(0.0 <= res[0][m] <= 1.0 for m in ("hit@1", "hit@5", "ndcg@5")) and res[0]["hit@1"] <= res[0]["hit@5"]
    assert json.load(open(tmp_path / "res.json")) == res
    assert train_tiger_mb.main(common + ["--only_test"]) == res
