"""The SMB data layer of TIGER (gamer_amd/t5_mb_data.py, gamer_amd/train_tiger_smb.py) without a GPU, bit for bit against the real
``SMBExplicitDataset`` / ``SMBExplicitDatasetForDecoder`` + ``T5Tokenizer(legacy=True)`` + ``EncoderDecoderCollator`` /
``EncoderDecoderTestCollator`` (tests/golden/tiger_smb_data.npz, tools/make_golden_tiger_smb.py): the vocabulary, the sample counts, a
seeded shuffle of training batches (empty histories, the augmented task's seeded copies), validation batches cut by a small
``model_max_length``, the test collator, the per-behaviour tries, the refusals, the 512-token rule, the parsers' defaults, and the
duplicate-ratio / merged-row arithmetic on beams that the real ``generate`` returned."""
import json
import os

import numpy as np
import pytest
import torch

from gamer_amd import data as smb_data, synthetic, t5_mb_data, tiger, train_tiger_smb
from gamer_amd.decode import ItemTrie
from gamer_amd.metrics import get_metrics_results, get_topk_results

FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_smb_data.npz")
GPU_FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_smb.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def root(fx, tmp_path_factory):
    _, meta = fx
    d = tmp_path_factory.mktemp("smb")
    synthetic.write_smb_dataset(str(d), meta["name"], **meta["kw"])
    return str(d)


def _padded(t, width, fill):
    a = t.numpy()
    return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=fill)


def _compare_batches(z, meta, task, split, samples, coll, order):
    B, W, fill = meta["batch"], meta["width"], meta["fill"]
    want = {k: z[f"{task}::{split}_{k}"] for k in ("input_ids", "attention_mask", "labels")}
    assert len(samples) == want["input_ids"].shape[0]                                          # the sample count
    for b0 in range(0, len(order), B):
        out = coll(samples, order[b0:b0 + B])
        assert out["split"] == split
        for k, w in (("input_ids", W), ("attention_mask", W), ("labels", 8)):
            assert out[k].dtype == torch.int64
            assert np.array_equal(_padded(out[k], w, fill), want[k][b0:b0 + B]), (task, split, b0, k)
    return want


@pytest.mark.parametrize("task", ["smb_explicit", "smb_explicit_decoder", "smb_explicit_decoder_2"])
def test_vocabulary_counts_and_collated_batches_equal_the_reference(fx, root, task):
    z, meta = fx
    d = t5_mb_data.T5SMBData(root, meta["name"], task)
    assert d.vocab_size == int(z[f"{task}::vocab_size"]) and d.new_tokens == z[f"{task}::vocab_tokens"].tolist()
    assert [d.tokens[t] for t in d.new_tokens] == z[f"{task}::vocab_ids"].tolist()
    assert z[f"{task}::vocab_ids"].tolist() == list(range(32100, d.vocab_size))
    assert d.tokens.pad_id == 0 and d.tokens["</s>"] == 1
    train = d.samples("train", meta["max_his_len"])
    order = np.random.RandomState(meta["order_seed"]).permutation(len(train))
    want = _compare_batches(z, meta, task, "train", train, t5_mb_data.EncDecCollator(1024, d.token_count), order)
    assert [train.behavior[n] for n in order] == z[f"{task}::train_behavior"].tolist()
    if task == "smb_explicit":
        # a user's first session has an empty history: the one-token row [</s>]; some batch holds one next to longer rows
        first = want["input_ids"][:, 0] == 1
        assert first.any() and not first.all()
        B = meta["batch"]
        assert any(first[b:b + B].any() and not first[b:b + B].all() for b in range(0, len(first), B))
    if task == "smb_explicit_decoder_2":
        assert len(train) > len(t5_mb_data.T5SMBData(root, meta["name"], "smb_explicit_decoder").samples("train", meta["max_his_len"]))
    # the validation set each task is paired with, cut by a small model_max_length
    valid = d.samples("valid", meta["max_his_len"])
    want = _compare_batches(z, meta, task, "valid", valid, t5_mb_data.EncDecCollator(meta["cut"], d.token_count), np.arange(len(valid)))
    assert ((want["input_ids"] != meta["fill"]).sum(1).max()) == meta["cut"]
    cut_rows = want["input_ids"][:, meta["cut"] - 1] == 1
    assert cut_rows.any()


def test_collation_does_not_depend_on_the_batch_and_rejects_test_samples(fx, root):
    _, meta = fx
    d = t5_mb_data.T5SMBData(root, meta["name"], "smb_explicit")
    train = d.samples("train", meta["max_his_len"])
    coll = t5_mb_data.EncDecCollator(1024, d.token_count)
    whole = coll(train, range(len(train)))
    for n in (0, 5, len(train) - 1):
        one = coll(train, [n])
        L, T = one["input_ids"].shape[1], one["labels"].shape[1]
        assert torch.equal(whole["input_ids"][n, :L], one["input_ids"][0]) and int(whole["input_ids"][n, L:].abs().sum()) == 0
        assert torch.equal(whole["labels"][n, :T], one["labels"][0])
        assert int(one["input_ids"][0, -1]) == 1 and int(one["labels"][0, -1]) == 1
    assert whole["behavior"] == train.behavior
    with pytest.raises(ValueError, match="test"):
        coll(d.samples("test", meta["max_his_len"]), [0])
    with pytest.raises(ValueError):
        t5_mb_data.EncDecCollator(0)


def test_test_collator_inputs_targets_and_history_items(fx, root):
    z, meta = fx
    d = t5_mb_data.T5SMBData(root, meta["name"], "smb_explicit")
    base = d.samples("test", meta["max_his_len"])
    coll = t5_mb_data.EncDecCollator(1024, d.token_count)
    assert set(meta["tests"]["smb_explicit"]) == set(d.behaviors)
    for b, want in meta["tests"]["smb_explicit"].items():
        sub = base.filter_by_behavior(b)
        inputs, targets = coll.test(sub, range(len(sub)))
        assert np.array_equal(inputs["input_ids"].numpy(), z[f"smb_explicit::test::{b}::input_ids"])
        assert np.array_equal(inputs["attention_mask"].numpy(), z[f"smb_explicit::test::{b}::attention_mask"])
        assert inputs["behavior"] == want["behavior"]
        bt = d.behavior_token_ids[b]
        assert [[[bt] + row for row in tg.tolist()] for tg in targets] == want["targets"]
        assert [h.tolist() for h in inputs["inters_item_list"]] == want["history_items"]
    with pytest.raises(ValueError, match="token_count"):
        t5_mb_data.EncDecCollator(1024).test(base, [0])


def test_tries_allow_the_reference_tries_tokens(fx, root):
    _, meta = fx
    d = t5_mb_data.T5SMBData(root, meta["name"], "smb_explicit")
    for b, want in meta["tests"]["smb_explicit"].items():
        seqs = d.trie_sequences(b, 0)
        assert len(seqs) == want["n_candidates"] and all(s[0] == 0 and s[1] == d.behavior_token_ids[b] and s[-1] == 1 for s in seqs)
        trie = ItemTrie(seqs, device="cpu", pad_token_id=0)
        assert len(want["trie"]) == 3
        for probe in want["trie"]:
            s = probe["sequence"]
            assert s in seqs
            for p in range(1, len(s) + 1):
                assert sorted(trie.get(s[:p])) == probe["allowed"][p - 1], (b, s, p)
            assert probe["allowed"][-1] == [] and probe["allowed"][-2] == [1]


def test_a_new_token_that_is_a_t5_piece_is_refused(root, fx, tmp_path):
    _, meta = fx
    vocab = t5_mb_data.t5_base_vocab()
    assert len(vocab) == 32100 and vocab["<pad>"] == 0 and vocab["</s>"] == 1 and vocab["<unk>"] == 2
    assert vocab["<extra_id_0>"] == 32099 and vocab["<extra_id_99>"] == 32000 and sorted(vocab.values()) == list(range(32100))
    d = synthetic.write_smb_dataset(str(tmp_path), "Clash", n_users=6, n_items=8)
    path = os.path.join(d, "Clash.index.json")
    index = json.load(open(path))
    index["0"][0] = "<extra_id_7>"
    json.dump(index, open(path, "w"))
    with pytest.raises(ValueError, match="extra_id_7"):
        t5_mb_data.T5SMBData(str(tmp_path), "Clash", "smb_explicit")
    # the pieces of a tokenizer.json next to config.json are found as well
    base = tmp_path / "base"
    base.mkdir()
    pieces = [["<pad>", 0.0], ["</s>", 0.0], ["<unk>", 0.0]] + [[f"p{i}", -1.0] for i in range(3, 32000)]
    pieces[10][0] = "<a_3>"
    pieces += [[f"<extra_id_{k}>", 0.0] for k in range(99, -1, -1)]
    (base / "tokenizer.json").write_text(json.dumps(dict(model=dict(vocab=pieces), added_tokens=[dict(id=0, content="<pad>")])))
    with pytest.raises(ValueError, match="a_3"):
        t5_mb_data.T5SMBData(root, meta["name"], "smb_explicit", base_model=str(base))
    (base / "tokenizer.json").write_text(json.dumps(dict(model=dict(vocab=pieces[:-1]))))
    with pytest.raises(ValueError, match="32100"):
        t5_mb_data.t5_base_vocab(str(base))


def test_the_default_token_table_is_unchanged():
    t = smb_data.TokenTable(["<b_1>", "<a_1>"])
    assert t.pad_id == 4 and t["<b_1>"] == 14 and t["<a_1>"] == 15 and len(t) == 16
    t5 = smb_data.TokenTable(["<a_1>"], {"<pad>": 0, "</s>": 1}, pad_token="<pad>")
    assert t5.pad_id == 0 and t5["<a_1>"] == 2
    with pytest.raises(KeyError):
        smb_data.TokenTable(["<a_1>"], {"<pad>": 0})


@pytest.mark.parametrize("task", ["smb", "smb_explicit_back", "smb_augment_3"])
def test_refused_training_tasks_are_named(root, fx, task):
    _, meta = fx
    with pytest.raises(NotImplementedError, match=task):
        t5_mb_data.T5SMBData(root, meta["name"], task)
    with pytest.raises(NotImplementedError, match=task):
        train_tiger_smb.parse_args(["--tasks", task])


@pytest.mark.parametrize("task", ["smb", "smb_explicit_back", "smb_augment_0.5", "smb_explicit_valid", "smb_valid_augment_0.5", "smb_drop_gt"])
def test_refused_test_tasks_are_named(task):
    with pytest.raises(NotImplementedError, match=task):
        train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--test_task", task])


def test_the_512_token_rule_at_its_boundary():
    assert tiger.MAX_LONG_ENCODER_LEN == 512
    a = train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--max_his_len", "100"])               # 100 x 5 + 1 = 501
    assert a.max_his_len == 100 and a.model_max_length == 1024
    # the rule is max_his_len x tokens per item + 1 > 512: at 5 tokens per item 102 items give 511 tokens, the last length that
    # fits, and 103 give 516; at 6 tokens per item (a five-token index) 102 items give 613
    assert train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--max_his_len", "102"]).max_his_len == 102
    for argv, kw, largest in ((["--max_his_len", "103"], {}, 102), (["--max_his_len", "102"], dict(token_count=6), 85),
                              (["--max_his_len", "0"], {}, 102), (["--max_his_len", "103", "--model_max_length", "513"], {}, 102)):
        with pytest.raises(NotImplementedError) as e:
            train_tiger_smb.parse_args(["--tasks", "smb_explicit"] + argv, **kw)
        assert "512" in str(e.value) and "MAX_LONG_ENCODER_LEN" in str(e.value) and f"is {largest}" in str(e.value), str(e.value)
    # a --model_max_length within the limit cuts every row to it, as the reference's tokenizer does
    assert train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--max_his_len", "200", "--model_max_length", "512"]).max_his_len == 200
    assert t5_mb_data.max_row_tokens(100, 5) == 501 and t5_mb_data.largest_max_his_len(512, 5) == 102


def test_parser_defaults_are_the_reference_parsers(fx):
    _, meta = fx
    a = vars(train_tiger_smb.parse_args(["--tasks", "smb_explicit"]))
    ref = meta["defaults"]["train_SMB_decoder"]
    assert ref["model_max_length"] == 1024 and ref["gradient_accumulation_steps"] == 2
    for k, v in ref.items():
        if k != "tasks":
            assert a[k] == v, (k, a[k], v)
    with pytest.raises(NotImplementedError, match="seqrec"):
        train_tiger_smb.parse_args([])                                              # (the reference's default task is train_decoder's)
    ref = meta["defaults"]["test_SMB_decoder"]
    for k in ("results_file", "test_batch_size", "num_beams", "metrics", "behaviors"):
        assert a[k] == ref[k], (k, a[k], ref[k])
    assert a["test_task"] == "smb_explicit" and a["only_test"] is False
    for flag in (["--fp16"], ["--bf16"], ["--deepspeed", "ds.json"], ["--resume_from_checkpoint", "x"]):
        with pytest.raises(NotImplementedError, match=flag[0][2:]):
            train_tiger_smb.parse_args(["--tasks", "smb_explicit"] + flag)
    with pytest.raises(NotImplementedError):
        train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--backbone", "PBATransformer"])
    with pytest.raises(NotImplementedError, match="save_and_eval_strategy"):
        train_tiger_smb.parse_args(["--tasks", "smb_explicit", "--save_and_eval_strategy", "steps"])


def test_duplicate_ratio_and_merged_row_on_recorded_beams(fx):
    """the beams of the real class's ``generate`` (20 per user, three users per behaviour), scored by the reference's ranking functions
    and its duplicate-ratio / merged-row arithmetic when the fixture was made"""
    z, meta = fx
    rec = meta["recorded"]
    metrics = rec["metrics"]
    rows, counts = [], []
    for b, want in rec["beams"].items():
        seqs, scores = z[f"recorded::{b}::beams"], z[f"recorded::{b}::scores"]
        assert seqs.shape == (60, 6)
        pred = seqs[:, 2:].tolist()
        targets = want["targets"]
        topk = get_topk_results(pred, scores.tolist(), targets, 20)
        row = {m: v / 3 for m, v in get_metrics_results(topk, metrics, targets).items()}
        row["Avg. Duplicate Ratio"] = float(np.mean([train_tiger_smb.duplicate_ratio(pred[i * 20:(i + 1) * 20], want["history_items"][i])
                                                     for i in range(3)]))
        for k, v in want["row"].items():
            assert row[k] == pytest.approx(v, rel=1e-12, abs=1e-15), (b, k)
        rows.append(row), counts.append(3)
    merged = train_tiger_smb.merge_rows(rows, counts, metrics)
    assert merged.pop("eval_type") == "Merged Behavior"
    for k, v in rec["merged"].items():
        assert merged[k] == pytest.approx(v, rel=1e-12, abs=1e-15), k
    assert train_tiger_smb.merge_rows([{"hit@1": 1.0}, {"hit@1": 0.0}], [1, 3], ["hit@1"])["hit@1"] == 0.25
    assert train_tiger_smb.duplicate_ratio([[1, 2], [1, 2], [3, 4]], [[3, 4], [5, 6]]) == 0.5
    assert train_tiger_smb.duplicate_ratio([], [[1, 2]]) == 0
