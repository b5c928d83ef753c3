"""The session-wise multi-behaviour data of the discriminative baselines (``train_SMB_rec``).

Restates ``SMBDisDataset`` (ref:SeqRec/datasets/SMB_dis_dataset.py:14-385) for the tasks ``smb_dis`` and ``smb_dis_diff``,
their validation sets and test tasks (ref:SeqRec/datasets/loading_SMB_dis.py), and the tensors of ``TraditionalCollator`` /
``TraditionalTestCollator`` (ref:SeqRec/datasets/collator_traditional.py).  Only the fields those collators read are kept:
the history items and behaviours, the target item(s) and behaviour, and the test split's ``item_range`` under ``diff``.
The reference's pickle caches in the dataset directory are neither read nor written.

Items are ``item + 1`` (0 pads); with ``diff`` an item seen under behaviour b is ``b * num + item + 1`` and the table has
``len(behaviors) * num`` rows besides the padding row.  Samples (SMB_dis_dataset.py:193-294):
  train  every position i >= 1 before the validation session, history = the items before i's session
  valid  the validation session's items as targets, history = everything before it
  test   the last session's items as targets, history = everything before it
"""
from __future__ import annotations

import copy
import json
import os
from typing import List, Tuple

import numpy as np
import torch

SUPPORTED_TASKS = ("smb_dis", "smb_dis_diff")


def _check_task(task: str) -> bool:
    t = task.lower()
    if t not in SUPPORTED_TASKS:
        raise NotImplementedError(f"task {task!r}: the HIP path supports {', '.join(SUPPORTED_TASKS)} "
                                  f"(negative-sampling, target, sample and decoder tasks are not restated)")
    return t == "smb_dis_diff"


class SMBDisData:
    """One split (``mode`` in train / valid / test) of ``SMBDisDataset(diff=...)``; ``samples`` is a list of dicts with
    ``inters``, ``inter_behaviors``, ``item`` (an int for train, a list for valid / test), ``behavior`` and optionally
    ``item_range``; with ``add_uid`` (the reference's ``--add_uid``, for PBAT) also ``uid`` = int(user key) + 1 (0 pads)."""

    def __init__(self, data_path: str, dataset: str, max_his_len: int, mode: str, diff: bool = False, add_uid: bool = False):
        if mode not in ("train", "valid", "test"):
            raise NotImplementedError(mode)
        self.dataset, self.max_his_len, self.mode, self.diff, self.add_uid = dataset, max_his_len, mode, diff, add_uid
        d = os.path.join(data_path, dataset)

        def load(suffix):
            with open(os.path.join(d, dataset + suffix)) as f:
                return json.load(f)
        self.inters = load(".SMB.inter.json")
        self.history_behaviors = load(".SMB.behavior.json")
        session = load(".SMB.session.json")
        self.behavior_level = load(".behavior_level.json")
        self.num = max(item for items in self.inters.values() for item in items) + 1
        self.num_users = max(int(u) for u in self.inters) + 1
        top = max(self.behavior_level.values())
        tops = [b for b, lv in self.behavior_level.items() if lv == top]
        if len(tops) != 1:
            raise ValueError(f"Expected exactly one target behavior with max level, but found {len(tops)}: {tops}")
        self.target_behavior = tops[0]
        self.behaviors = list(self.behavior_level)
        self.target_behavior_index = self.behaviors.index(self.target_behavior)
        # session positions (SMB_dis_dataset.py:80-96)
        self.session, self.train_pos, self.valid_pos, self.test_pos = {}, {}, {}, {}
        for uid, sids in session.items():
            s = np.asarray(sids) - np.min(sids)
            self.session[uid] = s
            uniq = np.unique(s)
            self.test_pos[uid] = int(np.where(s == uniq[-1])[0].min())
            self.valid_pos[uid] = int(np.where(s == uniq[-2])[0].min()) if len(uniq) >= 2 else -1
            if len(uniq) >= 3:
                self.train_pos[uid] = {int(sid): int(np.where(s == sid)[0].min()) for sid in uniq[:-2]}
        self.samples = {"train": self._train, "valid": self._valid, "test": self._test}[mode]()

    @property
    def num_items(self) -> int:
        return len(self.behaviors) * self.num if self.diff else self.num

    def item_id(self, item: int, behavior: str) -> int:
        return (self.behaviors.index(behavior) * self.num if self.diff else 0) + item + 1

    def _hist(self, items, behaviors):
        if self.max_his_len > 0:
            items, behaviors = items[-self.max_his_len:], behaviors[-self.max_his_len:]
        return [self.item_id(i, b) for i, b in zip(items, behaviors)], [self.behaviors.index(b) for b in behaviors]

    def _train(self):
        out = []
        for uid in self.inters:
            vp = self.valid_pos[uid]
            if vp <= 0:
                continue
            items, behs = self.inters[uid][:vp], self.history_behaviors[uid][:vp]
            for i in range(1, len(items)):
                pos = self.train_pos[uid][int(self.session[uid][i])]
                inters, ib = self._hist(items[:pos], behs[:pos])
                if not inters:
                    continue
                out.append(self._with_uid(dict(item=self.item_id(items[i], behs[i]), inters=inters, inter_behaviors=ib,
                                               behavior=self.behaviors.index(behs[i])), uid))
        return out

    def _with_uid(self, sample: dict, uid) -> dict:
        if self.add_uid:
            sample["uid"] = int(uid) + 1
        return sample

    def _session_sample(self, uid, start, end):
        items, behs = self.inters[uid][:end], self.history_behaviors[uid][:end]
        tgt = [self.item_id(items[i], behs[i]) for i in range(start, len(items))]
        tb = [self.behaviors.index(behs[i]) for i in range(start, len(items))]
        if not tgt:
            raise ValueError(f"Session for user {uid} is empty after position {start}.")
        inters, ib = self._hist(items[:start], behs[:start])
        return self._with_uid(dict(item=tgt, inters=inters, inter_behaviors=ib, behavior=tb), uid)

    def _valid(self):
        return [self._session_sample(uid, self.valid_pos[uid], self.test_pos[uid]) for uid in self.inters]

    def _test(self):
        return [self._session_sample(uid, self.test_pos[uid], len(self.inters[uid])) for uid in self.inters]

    def filter_by_behavior(self, behavior: str) -> "SMBDisData":
        """SMBDisDataset.filter_by_behavior: valid / test keep the rows whose session has the behaviour, with that behaviour's
        items as targets (``list(set(...))``, as the reference); under ``diff`` the test split gets the behaviour's item_range."""
        bi = self.behaviors.index(behavior)
        if self.samples and isinstance(self.samples[0]["behavior"], list):
            kept = []
            for s in self.samples:
                if bi not in s["behavior"]:
                    continue
                items = list(set(it for it, b in zip(s["item"], s["behavior"]) if b == bi))
                kept.append(dict(s, item=items, behavior=bi))
        else:
            kept = [s for s in self.samples if s["behavior"] == bi]
        out = copy.copy(self)
        out.samples = kept
        out.target_behavior = behavior
        if self.diff and self.mode == "test":
            rng = (bi * self.num + 1, (bi + 1) * self.num + 1)
            out.samples = [dict(s, item_range=rng) for s in kept]
        return out

    def __len__(self) -> int:
        return len(self.samples)


def load_train_valid(data_path: str, dataset: str, max_his_len: int, tasks: str,
                     add_uid: bool = False) -> Tuple[List[SMBDisData], SMBDisData]:
    """load_SMBDis_datasets for smb_dis / smb_dis_diff: the training splits of every task and the validation split of the
    last task's kind (unfiltered; the trainer filters it by the target behaviour)."""
    trains, diff = [], False
    for t in tasks.split(","):
        diff = _check_task(t)
        trains.append(SMBDisData(data_path, dataset, max_his_len, "train", diff, add_uid))
    return trains, SMBDisData(data_path, dataset, max_his_len, "valid", diff, add_uid)


def load_test(data_path: str, dataset: str, max_his_len: int, test_task: str, add_uid: bool = False) -> SMBDisData:
    return SMBDisData(data_path, dataset, max_his_len, "test", _check_task(test_task), add_uid)


def collate(samples: list, test: bool = False):
    """TraditionalCollator (test=False) / TraditionalTestCollator (test=True: (batch, target lists), no ``target`` key)."""
    seq_len = [len(s["inters"]) for s in samples]
    L = max(seq_len)
    batch = {
        "inputs": torch.tensor([s["inters"] + [0] * (L - len(s["inters"])) for s in samples], dtype=torch.long),
        "behaviors": torch.tensor([[b + 1 for b in s["inter_behaviors"]] + [0] * (L - len(s["inters"])) for s in samples],
                                  dtype=torch.long),
        "seq_len": torch.tensor(seq_len, dtype=torch.long),
    }
    if not test:
        batch["target"] = torch.tensor([s["item"] for s in samples], dtype=torch.long)
    batch["behavior"] = torch.tensor([s["behavior"] + 1 for s in samples], dtype=torch.long)
    if "item_range" in samples[0]:
        batch["item_range"] = samples[0]["item_range"]
    if "uid" in samples[0]:
        batch["uid"] = torch.tensor([s["uid"] for s in samples], dtype=torch.long)
    if test:
        return batch, [s["item"] for s in samples]
    return batch
