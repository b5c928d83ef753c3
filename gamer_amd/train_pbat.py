"""``python -m gamer_amd.train_pbat``: train and test PBAT on session-wise multi-behaviour data (``train_SMB_rec`` with
``--backbone PBAT --add_uid``).

The arguments, the loop, the printed lines and the files (``best_model.pth``, ``result-{test_task}.json``) are
``gamer_amd.train_rec``'s (``train_rec.run``); the data is BERT4Rec's and MBSTR's: the user-level task ``smb_dis_decoder`` (or
``smb_dis_diff_decoder``) for training, ``smb_dis_target`` (``smb_dis_target_diff``) for validation and test
(``gamer_amd.smb_dis_target_data``), here with ``add_uid`` on: every sample carries ``uid`` = user key + 1 and the collator emits
``"uid"``, which PBAT's user embeddings read.  ``--base_model`` defaults to ``./config/dis-models/PBAT``.  The model gets
``n_behaviors`` from the dataset's behaviour list and ``n_users`` from its user keys.
"""
from __future__ import annotations

import functools
import sys

from . import smb_dis_target_data, train_rec
from .pbat import PBAT, PBATConfig

BACKBONES = {"PBAT": (PBAT, PBATConfig)}


def parse_args(argv=None):
    return train_rec.parse_args(argv, prog="python -m gamer_amd.train_pbat", backbone="PBAT", backbones=BACKBONES,
                                tasks="smb_dis_decoder", test_task="smb_dis_target")


def main(argv=None):
    a = parse_args(argv)
    return train_rec.run(a, *BACKBONES[a.backbone], functools.partial(smb_dis_target_data.load_train_valid, add_uid=True),
                         functools.partial(smb_dis_target_data.load_test, add_uid=True), smb_dis_target_data.collate,
                         tag="train_pbat", pass_n_users=True)


if __name__ == "__main__":
    main(sys.argv[1:])
