"""The MB data layer (gamer_amd/mb_data.py) against the real reference: ``load_MB_datasets`` for every MB task, the extended
Qwen2Tokenizer and ``DecoderOnlyCollator`` with train_MB_decoder.py's ``only_train_response`` (tests/golden/mb_data_small.npz
from tools/make_golden_mb_data.py, on the seeded ``synthetic.write_mb_dataset`` directory).  Tensors bit for bit, training
and validation sets; the Qwen3Moe config of each task, and its refusal of ``mb_explicit_back``.  No GPU."""
import json
import os

import numpy as np
import pytest

from gamer_amd import synthetic
from gamer_amd.mb_data import MBCollator, MBData, qwen3moe_config

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    z = np.load(os.path.join(GOLDEN, "mb_data_small.npz"))
    meta = json.loads(str(z["meta_json"]))
    root = tmp_path_factory.mktemp("mb")
    synthetic.write_mb_dataset(str(root), meta["name"])
    return z, meta, str(root)


@pytest.mark.parametrize("task", ["mb", "mb_explicit", "mb_explicit_filter", "mb_explicit_decoder", "mb_explicit_decoder_3",
                                  "mb_explicit_back"])
def test_loader_and_collator_equal_the_reference(fixture, task):
    z, meta, root = fixture
    data = MBData(root, meta["name"], task)
    assert data.new_tokens == [str(t) for t in z[f"{task}::vocab_tokens"]]
    assert [data.tokens[t] for t in data.new_tokens] == z[f"{task}::vocab_ids"].tolist()
    assert len(data.tokens) == int(z[f"{task}::vocab_size"])
    coll = MBCollator(data)
    for split, samples in (("train", data.train_samples(meta["max_his_len"])),
                           ("valid", data.valid_samples(meta["max_his_len"]))):
        assert samples.behavior == [str(b) for b in z[f"{task}::{split}_behavior"]], split
        ids, am, lab = z[f"{task}::{split}_input_ids"], z[f"{task}::{split}_attention_mask"], z[f"{task}::{split}_labels"]
        assert len(samples) == ids.shape[0]
        for b0 in range(0, len(samples), meta["batch"]):
            out = coll.train(samples, range(b0, min(b0 + meta["batch"], len(samples))))
            L = out["input_ids"].shape[1]
            rows = slice(b0, b0 + out["input_ids"].shape[0])
            assert (ids[rows, L:] == meta["fill"]).all() and L <= meta["width"]
            np.testing.assert_array_equal(out["input_ids"].numpy(), ids[rows, :L], err_msg=f"{split} {b0}")
            np.testing.assert_array_equal(out["attention_mask"].numpy(), am[rows, :L], err_msg=f"{split} {b0}")
            np.testing.assert_array_equal(out["labels"].numpy(), lab[rows, :L], err_msg=f"{split} {b0}")


def test_qwen3moe_config_of_each_task_and_the_back_refusal(fixture):
    z, meta, root = fixture
    plain = qwen3moe_config(MBData(root, meta["name"], "mb"), 20)
    assert (plain.use_behavior_token, plain.num_behavior, plain.behavior_maps, plain.behavior_injection_decoder) == \
        (False, 0, {}, [])
    assert (plain.num_positions, plain.num_experts, plain.n_positions) == (4, 5, 21)
    plain.validate()
    data = MBData(root, meta["name"], "mb_explicit_decoder_3")
    exp = qwen3moe_config(data, 20)
    assert exp.use_behavior_token and exp.num_positions == 5 and exp.num_experts == 6
    assert exp.behavior_maps == {str(data.behavior_token_ids[b]): i for i, b in enumerate(data.behaviors)}
    assert exp.vocab_size == len(data.tokens)
    exp.validate()
    with pytest.raises(ValueError, match="mb_explicit_back"):
        qwen3moe_config(MBData(root, meta["name"], "mb_explicit_back"), 20)
    with pytest.raises(NotImplementedError):
        MBData(root, meta["name"], "smb_explicit")
