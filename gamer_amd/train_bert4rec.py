"""``python -m gamer_amd.train_bert4rec``: train and test BERT4Rec on session-wise multi-behaviour data (``train_SMB_rec`` with
``--backbone BERT4Rec``).

The arguments, the loop, the printed lines and the files (``best_model.pth``, ``result-{test_task}.json``) are
``gamer_amd.train_rec``'s (``train_rec.run``); what differs is the data: BERT4Rec trains on the user-level task
``smb_dis_decoder`` (or ``smb_dis_diff_decoder``) and validates / tests on ``smb_dis_target`` (``smb_dis_target_diff``), whose
rows end with the mask token (``gamer_amd.smb_dis_target_data``).  ``--base_model`` defaults to
``./config/dis-models/BERT4Rec``.

As in the reference, a training batch whose longest row is shorter than ``--max_his_len`` raises IndexError in the cloze masking
(``gamer_amd.bert4rec``): the batches of real data hold a user of at least ``max_his_len`` interactions.
"""
from __future__ import annotations

import sys

from . import smb_dis_target_data, train_rec
from .bert4rec import BERT4Rec, BERT4RecConfig

BACKBONES = {"BERT4Rec": (BERT4Rec, BERT4RecConfig)}


def parse_args(argv=None):
    return train_rec.parse_args(argv, prog="python -m gamer_amd.train_bert4rec", backbone="BERT4Rec", backbones=BACKBONES,
                                tasks="smb_dis_decoder", test_task="smb_dis_target")


def main(argv=None):
    a = parse_args(argv)
    return train_rec.run(a, *BACKBONES[a.backbone], smb_dis_target_data.load_train_valid, smb_dis_target_data.load_test,
                         smb_dis_target_data.collate, tag="train_bert4rec")


if __name__ == "__main__":
    main(sys.argv[1:])
