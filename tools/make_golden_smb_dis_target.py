#!/usr/bin/env python3
"""Golden fixture of the data tasks BERT4Rec runs on, from the REAL reference classes.

  * ``SMBDisUserLevelDataset`` (ref:SeqRec/datasets/SMB_dis_dataset.py), the training split of smb_dis_decoder and
    smb_dis_diff_decoder, unfiltered and filtered by every behaviour, collated by ``TraditionalCollator``;
  * ``SMBDisTargetDataset``, the validation split of those tasks and the test split of smb_dis_target / smb_dis_target_diff,
    filtered by every behaviour, collated by ``TraditionalTestCollator``;
over the directory ``synthetic.write_smb_dataset(tmp, "syn", **DATA)`` writes (long users included, so that the seeded random
crop of the user-level split is exercised), in the layout of tests/golden/smb_dis_small.npz.  Keys: ``{task}/{mode}/{view}/...``
with task smb_dis_decoder / smb_dis_diff_decoder for train and valid, smb_dis_target / smb_dis_target_diff for test.

Usage:  python tools/make_golden_smb_dis_target.py      (needs the reference checkout; CPU only)
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

OUT = os.path.join(ROOT, "tests", "golden", "smb_dis_target.npz")
DATA = dict(n_users=60, n_items=50, seed=5, min_sessions=2, max_sessions=9)
MAX_LEN = 6


def _pkg(name):
    if name not in sys.modules:
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(_ref_loader.REF_ROOT, *name.split("."))]
        pkg.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        pkg.__spec__.submodule_search_locations = pkg.__path__
        sys.modules[name] = pkg


def main():
    _ref_loader._install_shims()
    for n in ("SeqRec", "SeqRec.datasets"):
        _pkg(n)
    from SeqRec.datasets.SMB_dis_dataset import SMBDisTargetDataset, SMBDisUserLevelDataset
    from SeqRec.datasets.collator_traditional import TraditionalCollator, TraditionalTestCollator
    fx = {}
    cropped = 0
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_smb_dataset(tmp, "syn", **DATA)
        for diff in (False, True):
            for mode in ("train", "valid", "test"):
                if mode == "train":
                    ds = SMBDisUserLevelDataset(dataset="syn", data_path=tmp, max_his_len=MAX_LEN, mode=mode, diff=diff)
                    if not diff:
                        full = {u: ds.inters[u][:ds.valid_pos[u]] for u in ds.inters if ds.valid_pos[u] > 0}
                        tails = [[i + 1 for i in v[-MAX_LEN:]] for v in full.values()]
                        cropped = sum(d["inters"] != t for d, t in zip(ds.inter_data, tails))
                else:
                    ds = SMBDisTargetDataset(dataset="syn", data_path=tmp, max_his_len=MAX_LEN, mode=mode, diff=diff)
                if mode == "test":
                    task = "smb_dis_target_diff" if diff else "smb_dis_target"
                else:
                    task = "smb_dis_diff_decoder" if diff else "smb_dis_decoder"
                fx[f"{task}/num_items"] = np.asarray(ds.num_items)
                views = [("all", ds)] + [(b, ds.filter_by_behavior(b)) for b in ds.behaviors]
                for vname, v in views:
                    key = f"{task}/{mode}/{vname}"
                    fx[key + "/n"] = np.asarray(len(v))
                    if len(v) == 0 or (mode != "train" and vname == "all"):
                        continue                 # (unfiltered valid / test rows hold behaviour lists: the collator refuses them)
                    items = [v[i] for i in range(len(v))]
                    if mode == "train":
                        batch = TraditionalCollator()(items)
                        targets = None
                    else:
                        batch, targets = TraditionalTestCollator()(items)
                    for k, t in batch.items():
                        fx[f"{key}/{k}"] = np.asarray(t) if k == "item_range" else t.numpy()
                    if targets is not None:
                        fx[key + "/targets_flat"] = np.asarray([x for tg in targets for x in tg], dtype=np.int64)
                        fx[key + "/targets_len"] = np.asarray([len(tg) for tg in targets], dtype=np.int64)
    fx["meta_json"] = np.asarray(json.dumps(dict(data=DATA, max_his_len=MAX_LEN, cropped_users=int(cropped))))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), {cropped} users cropped at random")


if __name__ == "__main__":
    main()
