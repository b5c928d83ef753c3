#!/usr/bin/env python3
"""Golden fixture of the data tasks with ``add_uid=True`` (what PBAT trains and tests on), from the REAL reference classes.

  * ``SMBDisUserLevelDataset`` (ref:SeqRec/datasets/SMB_dis_dataset.py): the training split of smb_dis_decoder / smb_dis_diff_decoder;
  * ``SMBDisTargetDataset``: their validation split and the test split of smb_dis_target / smb_dis_target_diff;
  * ``SMBDisDataset``: the three splits of smb_dis / smb_dis_diff;
every one built with ``add_uid=True``, unfiltered and filtered by every behaviour, collated by ``TraditionalCollator`` /
``TraditionalTestCollator`` (which emit ``"uid"`` = int(user key) + 1), over the directory
``synthetic.write_smb_dataset(tmp, "syn", **DATA)`` writes.  Keys: ``{task}/{mode}/{view}/...`` as in
tests/golden/smb_dis_target.npz.  It checks that every collated batch carries ``uid`` and that more than one user occurs.

Usage:  python tools/make_golden_smb_dis_uid.py      (needs the reference checkout; CPU only)
"""
import importlib.machinery
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smb_dis_uid.npz")
DATA = dict(n_users=40, n_items=50, seed=7, min_sessions=2, max_sessions=8)
MAX_LEN = 6


def _pkg(name):
    if name not in sys.modules:
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(_ref_loader.REF_ROOT, *name.split("."))]
        pkg.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        pkg.__spec__.submodule_search_locations = pkg.__path__
        sys.modules[name] = pkg


def task_name(family, diff, mode):
    if family == "smb_dis":
        return "smb_dis_diff" if diff else "smb_dis"
    if mode == "test":
        return "smb_dis_target_diff" if diff else "smb_dis_target"
    return "smb_dis_diff_decoder" if diff else "smb_dis_decoder"


def main():
    _ref_loader._install_shims()
    for n in ("SeqRec", "SeqRec.datasets"):
        _pkg(n)
    from SeqRec.datasets.SMB_dis_dataset import SMBDisDataset, SMBDisTargetDataset, SMBDisUserLevelDataset
    from SeqRec.datasets.collator_traditional import TraditionalCollator, TraditionalTestCollator
    fx, users, batches = {}, set(), 0
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_smb_dataset(tmp, "syn", **DATA)
        for family in ("decoder", "smb_dis"):
            for diff in (False, True):
                for mode in ("train", "valid", "test"):
                    if family == "smb_dis":
                        cls = SMBDisDataset
                    else:
                        cls = SMBDisUserLevelDataset if mode == "train" else SMBDisTargetDataset
                    ds = cls(dataset="syn", data_path=tmp, max_his_len=MAX_LEN, mode=mode, diff=diff, add_uid=True)
                    task = task_name(family, diff, mode)
                    views = [("all", ds)] + [(b, ds.filter_by_behavior(b)) for b in ds.behaviors]
                    for vname, v in views:
                        key = f"{task}/{mode}/{vname}"
                        fx[key + "/n"] = np.asarray(len(v))
                        if len(v) == 0 or (mode != "train" and vname == "all"):
                            continue             # (unfiltered valid / test rows hold behaviour lists: the collator refuses them)
                        items = [v[i] for i in range(len(v))]
                        if mode == "train":
                            batch, targets = TraditionalCollator()(items), None
                        else:
                            batch, targets = TraditionalTestCollator()(items)
                        assert "uid" in batch, key
                        users.update(batch["uid"].tolist())
                        batches += 1
                        for k, t in batch.items():
                            fx[f"{key}/{k}"] = np.asarray(t) if k == "item_range" else t.numpy()
                        if targets is not None:
                            fx[key + "/targets_flat"] = np.asarray([x for tg in targets for x in tg], dtype=np.int64)
                            fx[key + "/targets_len"] = np.asarray([len(tg) for tg in targets], dtype=np.int64)
    assert len(users) > 1 and min(users) >= 1
    fx["meta_json"] = np.asarray(json.dumps(dict(data=DATA, max_his_len=MAX_LEN, users=len(users), batches=batches)))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), {batches} batches, {len(users)} users")


if __name__ == "__main__":
    main()
