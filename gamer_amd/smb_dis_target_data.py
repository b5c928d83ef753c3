"""The data tasks BERT4Rec is trained and tested on (``train_SMB_rec`` with ``smb_dis_decoder`` / ``smb_dis_target``).

Restates, on top of ``smb_dis_data.SMBDisData``:
  ``SMBDisUserLevelDataset`` (ref:SeqRec/datasets/SMB_dis_dataset.py:538-571), the training split of the tasks
      ``smb_dis_decoder`` and ``smb_dis_diff_decoder``: one sample per user, the whole history before the validation session
      (the last ``max_his_len`` items of it).  A user with more than ``max_his_len`` items is cropped to a random window of
      ``max_his_len`` items with probability 0.2; the reference seeds ``random``, numpy and torch with 42 before the pass
      (``set_seed(42)``) and so does this, drawing from Python's ``random`` stream in the same order.
  ``SMBDisTargetDataset`` (SMB_dis_dataset.py:424-486), the validation split of those tasks (``load_SMBDis_datasets``: ``*_decoder``
      tasks validate on it) and the test tasks ``smb_dis_target`` / ``smb_dis_target_diff``: the history cut to
      ``max_his_len - 1`` items plus the mask token ``num_items + 1``; the behaviour of that last slot is -1 until
      ``filter_by_behavior`` sets it to the behaviour evaluated.
Collation is ``smb_dis_data.collate``.  The reference's pickle caches are neither read nor written.
"""
from __future__ import annotations

import random
from typing import List, Tuple

import numpy as np
import torch

from .smb_dis_data import SMBDisData, collate  # noqa: F401  (collate: the loaders' companion, re-exported)

TRAIN_TASKS = ("smb_dis_decoder", "smb_dis_diff_decoder")
TEST_TASKS = ("smb_dis_target", "smb_dis_target_diff")


def _diff(task: str, allowed) -> bool:
    t = task.lower()
    if t not in allowed:
        raise NotImplementedError(f"task {task!r}: smb_dis_target_data supports {', '.join(allowed)} here")
    return "diff" in t


class SMBDisUserLevelData(SMBDisData):
    """``SMBDisUserLevelDataset``: the training split only (its valid / test splits are SMBDisData's)."""

    def _train(self):
        random.seed(42)                                     # set_seed(42), as the reference's pass begins
        np.random.seed(42)
        torch.manual_seed(42)
        out = []
        for uid in self.inters:
            vp = self.valid_pos[uid]
            if vp <= 0:
                continue
            items, behs = self.inters[uid][:vp], self.history_behaviors[uid][:vp]
            if len(items) > self.max_his_len and random.random() > 0.8:
                begin = random.randint(0, len(items) - self.max_his_len - 1)
                items, behs = items[begin:begin + self.max_his_len], behs[begin:begin + self.max_his_len]
            inters, ib = self._hist(items, behs)
            out.append(self._with_uid(dict(item=self.item_id(items[-1], behs[-1]), inters=inters, inter_behaviors=ib,
                                           behavior=self.behaviors.index(behs[-1])), uid))
        return out


class SMBDisTargetData(SMBDisData):
    """``SMBDisTargetDataset``'s valid / test splits: history of at most max_his_len - 1 items, then the mask token."""

    def __init__(self, data_path: str, dataset: str, max_his_len: int, mode: str, diff: bool = False, add_uid: bool = False):
        if mode not in ("valid", "test"):
            raise NotImplementedError(f"SMBDisTargetData: mode {mode!r} (the target tasks' training split is not restated)")
        super().__init__(data_path, dataset, max_his_len, mode, diff, add_uid)

    def _session_sample(self, uid, start, end):
        s = super()._session_sample(uid, start, end)
        n = self.max_his_len - 1
        inters, ib = s["inters"], s["inter_behaviors"]
        if n > 0:                                           # (_get_inters(max_his_len=n): no cut for n <= 0)
            inters, ib = inters[-n:], ib[-n:]
        elif self.max_his_len > 0:
            # the base sample was already cut to max_his_len; n <= 0 asks for the whole history
            items, behs = self.inters[uid][:start], self.history_behaviors[uid][:start]
            inters = [self.item_id(i, b) for i, b in zip(items, behs)]
            ib = [self.behaviors.index(b) for b in behs]
        return dict(s, inters=inters + [self.num_items + 1], inter_behaviors=ib + [-1])

    def filter_by_behavior(self, behavior: str) -> "SMBDisTargetData":
        out = super().filter_by_behavior(behavior)
        bi = self.behaviors.index(behavior)
        out.samples = [dict(s, inter_behaviors=s["inter_behaviors"][:-1] + [bi]) for s in out.samples]
        return out


def load_train_valid(data_path: str, dataset: str, max_his_len: int, tasks: str,
                     add_uid: bool = False) -> Tuple[List[SMBDisData], SMBDisData]:
    """load_SMBDis_datasets for smb_dis_decoder / smb_dis_diff_decoder: the user-level training splits of every task and the
    target validation split of the last task's kind (unfiltered; the trainer filters it by the target behaviour)."""
    trains, diff = [], False
    for t in tasks.split(","):
        diff = _diff(t, TRAIN_TASKS)
        trains.append(SMBDisUserLevelData(data_path, dataset, max_his_len, "train", diff, add_uid))
    return trains, SMBDisTargetData(data_path, dataset, max_his_len, "valid", diff, add_uid)


def load_test(data_path: str, dataset: str, max_his_len: int, test_task: str, add_uid: bool = False) -> SMBDisData:
    return SMBDisTargetData(data_path, dataset, max_his_len, "test", _diff(test_task, TEST_TASKS), add_uid)
