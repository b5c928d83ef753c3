"""The one seeded weight recipe of the SASRec fixture (tests/golden/sasrec_small.npz).

The fixture generator (tools/make_golden_sasrec.py, which loads the weights into the reference's ``SASRec``) and the tests
(which load them into ``gamer_amd.sasrec.SASRec``) both build the weights here; the fixture pins them with per-tensor fp64
checksums.  Matrices and tables from normal(0, std) (std larger than the reference's 0.02 so that the scores spread), the item
table's row 0 included as in the reference; LayerNorm weights near 1, biases small.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import numpy as np
import torch


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int, std: float = 0.1) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if k.endswith("LayerNorm.weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias"):
            t = 0.02 * t
        else:
            t = std * t
        sd[k] = t.float()
    return sd


def checksums(sd) -> np.ndarray:
    """per tensor: (sum, sum of squares, sum of index-weighted values) in fp64"""
    out = []
    for t in sd.values():
        x = t.detach().double().reshape(-1)
        w = torch.arange(x.numel(), dtype=torch.float64) % 97
        out.append([float(x.sum()), float((x * x).sum()), float((x * w).sum())])
    return np.asarray(out, dtype=np.float64)
