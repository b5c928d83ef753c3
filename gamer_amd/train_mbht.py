"""``python -m gamer_amd.train_mbht``: train and test MBHT on session-wise multi-behaviour data (``train_SMB_rec`` with
``--backbone MBHT``).

The arguments, the loop, the printed lines and the files (``best_model.pth``, ``result-{test_task}.json``) are
``gamer_amd.train_rec``'s (``train_rec.run``), on the same data as SASRec and GRU4Rec (tasks ``smb_dis`` / ``smb_dis_diff``,
``gamer_amd.smb_dis_data``).  As the reference does for this backbone alone, the model trains on the target behaviour's rows only,
only the target behaviour is tested (the "Merged Behavior" entry then equals it), and the model gets ``target_behavior_id =
target_behavior_index + 1``.  ``--base_model`` defaults to ``./config/dis-models/MBHT``; ``max_his_len + 1`` must be divisible by
the config's ``scales[1]`` and ``scales[2]`` (39 for the shipped [5, 4, 20]).
"""
from __future__ import annotations

import sys

from . import smb_dis_data, train_rec
from .mbht import MBHT, MBHTConfig

BACKBONES = {"MBHT": (MBHT, MBHTConfig)}


def parse_args(argv=None):
    return train_rec.parse_args(argv, prog="python -m gamer_amd.train_mbht", backbone="MBHT", backbones=BACKBONES, tasks="smb_dis",
                                test_task="smb_dis")


def main(argv=None):
    a = parse_args(argv)
    return train_rec.run(a, *BACKBONES[a.backbone], smb_dis_data.load_train_valid, smb_dis_data.load_test, smb_dis_data.collate,
                         tag="train_mbht", train_target_only=True, test_target_only=True, pass_target_behavior_id=True)


if __name__ == "__main__":
    main(sys.argv[1:])
