"""The data tasks of BERT4Rec against the REAL reference classes (tests/golden/smb_dis_target.npz,
tools/make_golden_smb_dis_target.py): SMBDisUserLevelDataset (training split of smb_dis_decoder / smb_dis_diff_decoder, with
its seeded random crop of long users) and SMBDisTargetDataset (their validation split; the test split of smb_dis_target /
smb_dis_target_diff) + TraditionalCollator / TraditionalTestCollator tensors bit for bit, every behaviour filter."""
import json
import os
import random

import numpy as np
import pytest

from gamer_amd import smb_dis_target_data as tdata, synthetic

FX = os.path.join(os.path.dirname(__file__), "golden", "smb_dis_target.npz")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    meta = json.loads(str(np.load(FX)["meta_json"]))
    root = str(tmp_path_factory.mktemp("smbt"))
    synthetic.write_smb_dataset(root, "syn", **meta["data"])
    return root, meta


def _load(root, L, diff, mode):
    if mode == "test":
        task = "smb_dis_target_diff" if diff else "smb_dis_target"
        return task, tdata.load_test(root, "syn", L, task)
    task = "smb_dis_diff_decoder" if diff else "smb_dis_decoder"
    trains, valid = tdata.load_train_valid(root, "syn", L, task)
    assert len(trains) == 1
    return task, trains[0] if mode == "train" else valid


@pytest.mark.parametrize("diff", [False, True])
@pytest.mark.parametrize("mode", ["train", "valid", "test"])
def test_tensors_match_reference(data_dir, diff, mode):
    root, meta = data_dir
    z = np.load(FX)
    before = sorted(os.listdir(os.path.join(root, "syn")))
    random.seed(123)                                       # whatever the stream held: the training pass seeds it itself
    task, ds = _load(root, meta["max_his_len"], diff, mode)
    assert ds.num_items == int(z[f"{task}/num_items"])
    for vname in ["all"] + ds.behaviors:
        v = ds if vname == "all" else ds.filter_by_behavior(vname)
        key = f"{task}/{mode}/{vname}"
        assert len(v) == int(z[key + "/n"]), key
        if len(v) == 0 or (mode != "train" and vname == "all"):
            continue
        if mode == "train":
            batch, targets = tdata.collate(v.samples), None
        else:
            batch, targets = tdata.collate(v.samples, test=True)
        ref_keys = {k[len(key) + 1:] for k in z.files if k.startswith(key + "/")} - {"n", "targets_flat", "targets_len"}
        assert set(batch) == ref_keys, key
        for k, t in batch.items():
            got = np.asarray(t) if k == "item_range" else t.numpy()
            assert got.dtype == z[f"{key}/{k}"].dtype and np.array_equal(got, z[f"{key}/{k}"]), (key, k)
        if targets is not None:
            assert np.array_equal([x for t in targets for x in t], z[key + "/targets_flat"]), key
            assert np.array_equal([len(t) for t in targets], z[key + "/targets_len"]), key
    assert sorted(os.listdir(os.path.join(root, "syn"))) == before          # no pickle caches written


def test_fixture_exercises_the_random_crop():
    assert json.loads(str(np.load(FX)["meta_json"]))["cropped_users"] > 0


def test_evaluation_rows_end_with_the_mask_token(data_dir):
    root, meta = data_dir
    L = meta["max_his_len"]
    t = tdata.load_test(root, "syn", L, "smb_dis_target")
    assert all(s["inters"][-1] == t.num_items + 1 and len(s["inters"]) <= L and s["inter_behaviors"][-1] == -1 for s in t.samples)
    f = t.filter_by_behavior("cart")
    assert all(s["inter_behaviors"][-1] == t.behaviors.index("cart") for s in f.samples)
    assert all(s["inter_behaviors"][-1] == -1 for s in t.samples)            # the unfiltered rows are not modified
    d = tdata.load_test(root, "syn", L, "smb_dis_target_diff").filter_by_behavior("buy")
    assert all(s["item_range"] == (2 * d.num + 1, 3 * d.num + 1) and s["inters"][-1] == 3 * d.num + 1 for s in d.samples)


@pytest.mark.parametrize("task", ["smb_dis", "smb_dis_target", "smb_dis_sample_decoder"])
def test_other_training_tasks_refused(data_dir, task):
    root, meta = data_dir
    with pytest.raises(NotImplementedError, match="smb_dis_decoder, smb_dis_diff_decoder"):
        tdata.load_train_valid(root, "syn", meta["max_his_len"], task)


@pytest.mark.parametrize("task", ["smb_dis", "smb_dis_decoder", "smb_dis_sample_target"])
def test_other_test_tasks_refused(data_dir, task):
    root, meta = data_dir
    with pytest.raises(NotImplementedError, match="smb_dis_target, smb_dis_target_diff"):
        tdata.load_test(root, "syn", meta["max_his_len"], task)
