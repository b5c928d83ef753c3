"""``add_uid=True`` on the data classes and loaders against the REAL reference classes (tests/golden/smb_dis_uid.npz,
tools/make_golden_smb_dis_uid.py): the samples and collated tensors of smb_dis_decoder (train, valid), smb_dis_target (test), their
``diff`` forms and smb_dis, bit for bit with ``"uid"`` = int(user key) + 1; the default emits no ``"uid"``."""
import json
import os
import random

import numpy as np
import pytest

from gamer_amd import smb_dis_data as sdata, smb_dis_target_data as tdata, synthetic

FX = os.path.join(os.path.dirname(__file__), "golden", "smb_dis_uid.npz")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    meta = json.loads(str(np.load(FX)["meta_json"]))
    root = str(tmp_path_factory.mktemp("smbu"))
    synthetic.write_smb_dataset(root, "syn", **meta["data"])
    return root, meta


def _load(root, L, family, diff, mode, **kw):
    if family == "smb_dis":
        task, mod = ("smb_dis_diff" if diff else "smb_dis"), sdata
        test_task = task
    else:
        task, mod = ("smb_dis_diff_decoder" if diff else "smb_dis_decoder"), tdata
        test_task = "smb_dis_target_diff" if diff else "smb_dis_target"
    if mode == "test":
        return test_task, mod.load_test(root, "syn", L, test_task, **kw)
    trains, valid = mod.load_train_valid(root, "syn", L, task, **kw)
    return task, trains[0] if mode == "train" else valid


@pytest.mark.parametrize("family", ["decoder", "smb_dis"])
@pytest.mark.parametrize("diff", [False, True])
@pytest.mark.parametrize("mode", ["train", "valid", "test"])
def test_tensors_match_reference(data_dir, family, diff, mode):
    root, meta = data_dir
    z = np.load(FX)
    random.seed(321)
    task, ds = _load(root, meta["max_his_len"], family, diff, mode, add_uid=True)
    assert all(s["uid"] >= 1 for s in ds.samples)
    seen = 0
    for vname in ["all"] + ds.behaviors:
        v = ds if vname == "all" else ds.filter_by_behavior(vname)
        key = f"{task}/{mode}/{vname}"
        assert len(v) == int(z[key + "/n"]), key
        if len(v) == 0 or (mode != "train" and vname == "all"):
            continue
        batch, targets = (sdata.collate(v.samples), None) if mode == "train" else sdata.collate(v.samples, test=True)
        ref_keys = {k[len(key) + 1:] for k in z.files if k.startswith(key + "/")} - {"n", "targets_flat", "targets_len"}
        assert set(batch) == ref_keys and "uid" in batch, key
        for k, t in batch.items():
            got = np.asarray(t) if k == "item_range" else t.numpy()
            assert got.dtype == z[f"{key}/{k}"].dtype and np.array_equal(got, z[f"{key}/{k}"]), (key, k)
        if targets is not None:
            assert np.array_equal([x for t in targets for x in t], z[key + "/targets_flat"]), key
            assert np.array_equal([len(t) for t in targets], z[key + "/targets_len"]), key
        seen += 1
    assert seen > 0


def test_uid_is_the_user_key_plus_one(data_dir):
    root, meta = data_dir
    ds = tdata.load_test(root, "syn", meta["max_his_len"], "smb_dis_target", add_uid=True)
    assert [s["uid"] for s in ds.samples] == [int(u) + 1 for u in ds.inters]
    assert max(s["uid"] for s in ds.samples) <= ds.num_users


@pytest.mark.parametrize("family", ["decoder", "smb_dis"])
@pytest.mark.parametrize("mode", ["train", "valid", "test"])
def test_default_has_no_uid(data_dir, family, mode):
    root, meta = data_dir
    _, ds = _load(root, meta["max_his_len"], family, False, mode)
    assert all("uid" not in s for s in ds.samples)
    v = ds if mode == "train" else ds.filter_by_behavior(ds.target_behavior)
    batch = sdata.collate(v.samples) if mode == "train" else sdata.collate(v.samples, test=True)[0]
    assert "uid" not in batch
    random.seed(321)
    _, du = _load(root, meta["max_his_len"], family, False, mode, add_uid=True)
    assert [{k: x for k, x in s.items() if k != "uid"} for s in du.samples] == ds.samples
