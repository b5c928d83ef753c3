"""``python -m gamer_amd.train_mbstr``: train and test MBSTR on session-wise multi-behaviour data (``train_SMB_rec`` with
``--backbone MBSTR``).

The arguments, the loop, the printed lines and the files (``best_model.pth``, ``result-{test_task}.json``) are
``gamer_amd.train_rec``'s (``train_rec.run``); the data is BERT4Rec's: MBSTR trains on the user-level task ``smb_dis_decoder``
(or ``smb_dis_diff_decoder``) and validates / tests on ``smb_dis_target`` (``smb_dis_target_diff``), whose rows end with the mask
token carrying the target's behaviour (``gamer_amd.smb_dis_target_data``); the collator's ``"behaviors"`` are the token types.
``--base_model`` defaults to ``./config/dis-models/MBSTR``.  The model gets ``n_behaviors`` from the dataset's behaviour list.
"""
from __future__ import annotations

import sys

from . import smb_dis_target_data, train_rec
from .mbstr import MBSTR, MBSTRConfig

BACKBONES = {"MBSTR": (MBSTR, MBSTRConfig)}


def parse_args(argv=None):
    return train_rec.parse_args(argv, prog="python -m gamer_amd.train_mbstr", backbone="MBSTR", backbones=BACKBONES,
                                tasks="smb_dis_decoder", test_task="smb_dis_target")


def main(argv=None):
    a = parse_args(argv)
    return train_rec.run(a, *BACKBONES[a.backbone], smb_dis_target_data.load_train_valid, smb_dis_target_data.load_test,
                         smb_dis_target_data.collate, tag="train_mbstr")


if __name__ == "__main__":
    main(sys.argv[1:])
