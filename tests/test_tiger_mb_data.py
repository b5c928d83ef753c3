"""The MB data layer of TIGER (gamer_amd/t5_mb_data.py, gamer_amd/train_tiger_mb.py) without a GPU, bit for bit against the real
``MBDataset`` / ``MBExplicitDataset`` / ``MBExplicitDatasetForDecoder`` + ``T5Tokenizer(legacy=True)`` + ``EncoderDecoderCollator`` /
``EncoderDecoderTestCollator`` (tests/golden/tiger_mb_data.npz, tools/make_golden_tiger_smb.py): for each of the five tasks (and an
augmented one) the vocabulary, the sample counts, a seeded shuffle of training batches and validation batches cut by a small
``model_max_length``; the test sets, the target behaviour's trie and decoder prefix, the refusals and the parser's defaults."""
import json
import os

import numpy as np
import pytest
import torch

from gamer_amd import mb_data, synthetic, t5_mb_data, train_tiger_mb
from gamer_amd.decode import ItemTrie

FX = os.path.join(os.path.dirname(__file__), "golden", "tiger_mb_data.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FX)
    return z, json.loads(str(z["meta_json"]))


@pytest.fixture(scope="module")
def root(fx, tmp_path_factory):
    _, meta = fx
    d = tmp_path_factory.mktemp("mb")
    synthetic.write_mb_dataset(str(d), meta["name"], **meta["kw"])
    return str(d)


def _padded(t, width, fill):
    a = t.numpy()
    return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=fill)


def _compare_batches(z, meta, task, split, samples, coll, order):
    B, W, fill = meta["batch"], meta["width"], meta["fill"]
    want = {k: z[f"{task}::{split}_{k}"] for k in ("input_ids", "attention_mask", "labels")}
    assert len(samples) == want["input_ids"].shape[0]
    for b0 in range(0, len(order), B):
        out = coll(samples, order[b0:b0 + B])
        for k, w in (("input_ids", W), ("attention_mask", W), ("labels", 8)):
            assert out[k].dtype == torch.int64
            assert np.array_equal(_padded(out[k], w, fill), want[k][b0:b0 + B]), (task, split, b0, k)
    return want


def test_the_fixture_covers_every_task(fx):
    _, meta = fx
    assert {t for t in meta["tasks"] if not t.startswith("mb_explicit_decoder_")} == set(mb_data.TASKS)
    assert "mb_explicit_decoder_3" in meta["tasks"]


@pytest.mark.parametrize("task", ["mb", "mb_explicit", "mb_explicit_filter", "mb_explicit_decoder", "mb_explicit_decoder_3", "mb_explicit_back"])
def test_vocabulary_counts_and_collated_batches_equal_the_reference(fx, root, task):
    z, meta = fx
    d = t5_mb_data.T5MBData(root, meta["name"], task)
    assert d.vocab_size == int(z[f"{task}::vocab_size"]) and d.new_tokens == z[f"{task}::vocab_tokens"].tolist()
    assert [d.tokens[t] for t in d.new_tokens] == z[f"{task}::vocab_ids"].tolist() == list(range(32100, d.vocab_size))
    assert d.tokens.pad_id == 0
    assert (len(d.behavior_token_ids) == 0) == (task == "mb")
    train = d.samples("train", meta["max_his_len"])
    order = np.random.RandomState(meta["order_seed"]).permutation(len(train))
    _compare_batches(z, meta, task, "train", train, t5_mb_data.EncDecCollator(512), order)
    assert [train.behavior[n] for n in order] == z[f"{task}::train_behavior"].tolist()
    valid = d.samples("valid", meta["max_his_len"])
    want = _compare_batches(z, meta, task, "valid", valid, t5_mb_data.EncDecCollator(meta["cut"]), np.arange(len(valid)))
    assert ((want["input_ids"] != meta["fill"]).sum(1).max()) == meta["cut"] and (want["input_ids"][:, meta["cut"] - 1] == 1).any()


@pytest.mark.parametrize("task", ["mb", "mb_explicit", "mb_explicit_filter"])
def test_test_sets_tries_and_prefix(fx, root, task):
    z, meta = fx
    d = t5_mb_data.T5MBData(root, meta["name"], task)
    coll = t5_mb_data.EncDecCollator(512)
    full = d.samples("test", meta["max_his_len"])
    inputs, _ = coll.test(full, range(len(full)))
    assert np.array_equal(inputs["input_ids"].numpy(), z[f"{task}::test::all::input_ids"])
    (b, want), = meta["tests"][task].items()
    assert b == d.target_behavior
    sub = d.test_samples(meta["max_his_len"], b)
    inputs, targets = coll.test(sub, range(len(sub)))
    assert np.array_equal(inputs["input_ids"].numpy(), z[f"{task}::test::{b}::input_ids"])
    assert np.array_equal(inputs["attention_mask"].numpy(), z[f"{task}::test::{b}::attention_mask"])
    assert inputs["behavior"] == want["behavior"] and set(want["behavior"]) == {b}
    assert [t.tolist() for t in targets] == [[t] for t in want["targets"]]
    seqs = d.trie_sequences(b, 0)
    assert len(seqs) == want["n_candidates"]
    trie = ItemTrie(seqs, device="cpu", pad_token_id=0)
    for probe in want["trie"]:
        s = probe["sequence"]
        assert s in seqs and len(s) == 1 + d.token_count + 1
        for p in range(1, len(s) + 1):
            assert sorted(trie.get(s[:p])) == probe["allowed"][p - 1], (task, s, p)
    prefix = d.decoder_prefix(0)
    assert prefix == ([0] if task == "mb" else [0, d.behavior_token_ids[b]])
    assert all(s[:len(prefix)] == prefix for s in seqs)
    info = d.collision_info(sub)
    assert info["total"] == len(sub) and 0 <= info["collision_samples"] <= len(sub)


def test_refusals(fx, root):
    _, meta = fx
    with pytest.raises(NotImplementedError, match="mb_explicit_back"):
        t5_mb_data.T5MBData(root, meta["name"], "mb_explicit_back").samples("test", 6)
    with pytest.raises(NotImplementedError, match="mb_other"):
        t5_mb_data.T5MBData(root, meta["name"], "mb_other")
    with pytest.raises(NotImplementedError, match="mb_explicit_back"):
        train_tiger_mb.parse_args(["--tasks", "mb_explicit_back", "--only_test"])
    assert train_tiger_mb.parse_args(["--tasks", "mb_explicit_back"]).test_task is None
    with pytest.raises(NotImplementedError, match="mb_explicit_back"):
        train_tiger_mb.parse_args(["--tasks", "mb_explicit", "--test_task", "mb_explicit_back"])
    with pytest.raises(ValueError, match="vocabulary"):
        train_tiger_mb.parse_args(["--tasks", "mb", "--test_task", "mb_explicit"])
    with pytest.raises(NotImplementedError, match="filter"):
        train_tiger_mb.parse_args(["--tasks", "mb", "--filter"])
    with pytest.raises(NotImplementedError, match="seqrec"):
        train_tiger_mb.parse_args([])
    for flag in (["--fp16"], ["--bf16"], ["--deepspeed", "ds.json"], ["--resume_from_checkpoint", "x"]):
        with pytest.raises(NotImplementedError, match=flag[0][2:]):
            train_tiger_mb.parse_args(["--tasks", "mb"] + flag)
    # the 512-token rule: the default --model_max_length, 512, cuts every row; a larger one does not
    assert train_tiger_mb.parse_args(["--tasks", "mb_explicit", "--max_his_len", "200"]).model_max_length == 512
    assert train_tiger_mb.parse_args(["--tasks", "mb_explicit", "--max_his_len", "102", "--model_max_length", "1024"]).max_his_len == 102
    assert train_tiger_mb.parse_args(["--tasks", "mb", "--max_his_len", "127", "--model_max_length", "1024"]).max_his_len == 127
    for argv, largest in ((["--tasks", "mb_explicit", "--max_his_len", "103"], 102), (["--tasks", "mb", "--max_his_len", "128"], 127)):
        with pytest.raises(NotImplementedError) as e:
            train_tiger_mb.parse_args(argv + ["--model_max_length", "1024"])
        assert "512" in str(e.value) and f"is {largest}" in str(e.value)


def test_parser_defaults_are_the_reference_parsers(fx):
    _, meta = fx
    a = vars(train_tiger_mb.parse_args(["--tasks", "mb_explicit"]))
    ref = meta["defaults"]["train_MB_decoder"]
    assert ref["model_max_length"] == 512
    for k, v in ref.items():
        if k != "tasks":
            assert a[k] == v, (k, a[k], v)
    ref = meta["defaults"]["test_MB_decoder"]
    for k in ("results_file", "test_batch_size", "num_beams", "metrics", "filter"):
        assert a[k] == ref[k], (k, a[k], ref[k])
    assert a["test_task"] == "mb_explicit" and a["only_test"] is False
    assert train_tiger_mb.parse_args(["--tasks", "mb"]).test_task == "mb"
    assert train_tiger_mb.parse_args(["--tasks", "mb_explicit_decoder_3"]).test_task == "mb_explicit_filter"
    assert train_tiger_mb.parse_args(["--tasks", "mb_explicit_filter"]).test_task == "mb_explicit_filter"
