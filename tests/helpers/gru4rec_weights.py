"""The one seeded weight recipe of the GRU4Rec fixture (tests/golden/gru4rec_small.npz).

The fixture generator (tools/make_golden_gru4rec.py, which loads the weights into the reference's ``GRU4Rec``) and the tests
(which load them into ``gamer_amd.gru4rec.GRU4Rec``) both build the weights here; the fixture pins them with per-tensor fp64
checksums.  The item table (row 0 included, as in the reference) from normal(0, 0.3) so that the scores spread; GRU and dense
matrices from normal(0, 1 / sqrt(fan_in)) so that the gates are neither saturated nor linear; biases small.  CPU only, no
gamer_amd import."""
from collections import OrderedDict

import numpy as np
import torch


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if k == "item_embedding.weight":
            t = 0.3 * t
        elif k.endswith(".bias"):
            t = 0.02 * t
        else:
            t = t / np.sqrt(shp[1])
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
