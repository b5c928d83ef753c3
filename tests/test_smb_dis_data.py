"""The SMBDis data layer and the discriminative metrics against the REAL reference classes (tests/golden/smb_dis_small.npz,
tools/make_golden_smb_dis.py): SMBDisDataset + TraditionalCollator / TraditionalTestCollator tensors bit for bit for smb_dis
and smb_dis_diff, every split and behaviour filter; SMBRec.Trainer.evaluate's metric loop on fixed scores."""
import json
import os

import numpy as np
import pytest

from gamer_amd import smb_dis_data, synthetic
from gamer_amd.metrics import topk_rank_metrics

FX = os.path.join(os.path.dirname(__file__), "golden", "smb_dis_small.npz")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    meta = json.loads(str(np.load(FX)["meta_json"]))
    root = str(tmp_path_factory.mktemp("smb"))
    synthetic.write_smb_dataset(root, "syn", **meta["data"])
    return root, meta


@pytest.mark.parametrize("task", ["smb_dis", "smb_dis_diff"])
@pytest.mark.parametrize("mode", ["train", "valid", "test"])
def test_tensors_match_reference(data_dir, task, mode):
    root, meta = data_dir
    z = np.load(FX)
    ds = smb_dis_data.SMBDisData(root, "syn", meta["max_his_len"], mode, diff=task.endswith("diff"))
    assert ds.num_items == int(z[f"{task}/num_items"])
    before = sorted(os.listdir(os.path.join(root, "syn")))
    for vname in ["all"] + ds.behaviors:
        v = ds if vname == "all" else ds.filter_by_behavior(vname)
        key = f"{task}/{mode}/{vname}"
        assert len(v) == int(z[key + "/n"]), key
        if len(v) == 0 or (mode != "train" and vname == "all"):
            continue
        if mode == "train":
            batch, targets = smb_dis_data.collate(v.samples), None
        else:
            batch, targets = smb_dis_data.collate(v.samples, test=True)
        ref_keys = {k[len(key) + 1:] for k in z.files if k.startswith(key + "/")} - {"n", "targets_flat", "targets_len"}
        assert set(batch) == ref_keys, key
        for k, t in batch.items():
            got = np.asarray(t) if k == "item_range" else t.numpy()
            assert got.dtype == z[f"{key}/{k}"].dtype and np.array_equal(got, z[f"{key}/{k}"]), (key, k)
        if targets is not None:
            assert np.array_equal([x for t in targets for x in t], z[key + "/targets_flat"]), key
            assert np.array_equal([len(t) for t in targets], z[key + "/targets_len"]), key
    assert sorted(os.listdir(os.path.join(root, "syn"))) == before          # no pickle caches written


def test_item_range_only_on_the_diff_test_split(data_dir):
    root, meta = data_dir
    for mode in ("train", "valid"):
        d = smb_dis_data.SMBDisData(root, "syn", meta["max_his_len"], mode, diff=True).filter_by_behavior("buy")
        assert all("item_range" not in s for s in d.samples)
    t = smb_dis_data.SMBDisData(root, "syn", meta["max_his_len"], "test", diff=True).filter_by_behavior("cart")
    assert all(s["item_range"] == (1 * t.num + 1, 2 * t.num + 1) for s in t.samples)


@pytest.mark.parametrize("task", ["smb_dis_sample", "smb_dis_neg", "smb_dis_target", "smb_dis_decoder", "smb_dis_diff_neg"])
def test_other_tasks_refused(data_dir, task):
    root, meta = data_dir
    with pytest.raises(NotImplementedError, match="smb_dis, smb_dis_diff"):
        smb_dis_data.load_train_valid(root, "syn", meta["max_his_len"], task)
    with pytest.raises(NotImplementedError, match="smb_dis, smb_dis_diff"):
        smb_dis_data.load_test(root, "syn", meta["max_his_len"], task)


def test_metrics_match_reference_loop():
    z = np.load(FX)
    meta = json.loads(str(z["meta_json"]))
    scores = z["metric/scores"]
    lens = z["metric/targets_len"]
    flat = z["metric/targets_flat"].tolist()
    targets, o = [], 0
    for n in lens:
        targets.append(flat[o:o + n])
        o += n
    ranks = np.argsort(-scores, axis=1)                     # the reference loop's ranking
    K = max(int(m.split("@")[1]) for m in meta["metrics"])
    vals = topk_rank_metrics(ranks[:, :K], targets, meta["metrics"])
    got = [np.mean(vals[m]) for m in meta["metrics"]]
    assert np.array_equal(np.asarray(got, dtype=np.float64), z["metric/values"])
