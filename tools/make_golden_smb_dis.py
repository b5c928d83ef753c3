#!/usr/bin/env python3
"""Golden fixture of the SMBDis data layer and the discriminative metrics, from the REAL reference classes.

  * ``SMBDisDataset`` (ref:SeqRec/datasets/SMB_dis_dataset.py) for smb_dis and smb_dis_diff, every split, unfiltered and
    filtered by every behaviour, collated by ``TraditionalCollator`` (train) / ``TraditionalTestCollator`` (valid, test),
    over the directory ``synthetic.write_smb_dataset(tmp, "syn", seed=3)`` writes;
  * ``SMBRec.Trainer.evaluate``'s metric loop (ref:SeqRec/trainers/SMBRec.py) on fixed scores and target lists, through a
    stand-in model whose full_sort_predict returns those scores (wandb stubbed).

Usage:  python tools/make_golden_smb_dis.py      (needs the reference checkout; CPU only)
"""
import importlib.machinery
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smb_dis_small.npz")
DATA = dict(n_users=30, n_items=50, seed=3, min_sessions=2, max_sessions=6)
MAX_LEN = 6
METRICS = ["hit@1", "hit@5", "hit@10", "recall@1", "recall@5", "recall@10", "ndcg@5", "ndcg@10"]


def _pkg(name):
    if name not in sys.modules:
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(_ref_loader.REF_ROOT, *name.split("."))]
        pkg.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        pkg.__spec__.submodule_search_locations = pkg.__path__
        sys.modules[name] = pkg


def main():
    _ref_loader._install_shims()
    for n in ("SeqRec", "SeqRec.datasets", "SeqRec.trainers"):
        _pkg(n)
    if "wandb" not in sys.modules:
        w = types.ModuleType("wandb")
        w.log = lambda *a, **k: None
        sys.modules["wandb"] = w
    from SeqRec.datasets.SMB_dis_dataset import SMBDisDataset
    from SeqRec.datasets.collator_traditional import TraditionalCollator, TraditionalTestCollator
    from SeqRec.trainers.SMBRec import Trainer
    fx = {}
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_smb_dataset(tmp, "syn", **DATA)
        for diff in (False, True):
            task = "smb_dis_diff" if diff else "smb_dis"
            for mode in ("train", "valid", "test"):
                ds = SMBDisDataset(dataset="syn", data_path=tmp, max_his_len=MAX_LEN, mode=mode, diff=diff)
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
    # the metric loop on fixed scores (ties included: integer-valued scores)
    g = torch.Generator().manual_seed(11)
    N, V = 40, 30
    scores = torch.randint(0, 12, (N, V), generator=g).float()
    targets = [torch.randint(0, V, (int(torch.randint(1, 5, (1,), generator=g)),), generator=g).tolist() for _ in range(N)]

    class _Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def full_sort_predict(self, batch):
            return scores[batch["rows"]]
    loader = [({"rows": torch.arange(i, min(i + 16, N))}, targets[i:i + 16]) for i in range(0, N, 16)]
    tr = Trainer(_Model(), [], loader, "adamw", 1e-3, 0.0, 1, 0, tmp, 1, METRICS)
    tr.global_step = 0
    res = tr.evaluate()
    fx["metric/scores"] = scores.numpy()
    fx["metric/targets_flat"] = np.asarray([x for t in targets for x in t], dtype=np.int64)
    fx["metric/targets_len"] = np.asarray([len(t) for t in targets], dtype=np.int64)
    fx["metric/values"] = np.asarray([res[m] for m in METRICS], dtype=np.float64)
    fx["meta_json"] = np.asarray(json.dumps(dict(data=DATA, max_his_len=MAX_LEN, metrics=METRICS)))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
