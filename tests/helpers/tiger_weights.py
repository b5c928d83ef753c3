"""The one seeded weight recipe of the TIGER fixture (tests/golden/tiger_small.npz).

The fixture generator (tools/make_golden_tiger.py, which loads the weights into the reference's ``TIGER``) and the tests (which
load them into ``gamer_amd.tiger.TIGER``) both build the weights here; the fixture pins them with per-tensor fp64 checksums.
The four tied keys hold one tensor.  Layer-norm weights near 1; Linear weights normal(0, fan_in ** -0.5), the query projections
at half of that: T5 does not scale its scores, so they come out with a spread of about 4 - large enough that the softmax is far
from uniform, as in a trained model.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import numpy as np
import torch

TIED = ("shared.weight", "encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight")


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    table = None
    for k, shp in shapes.items():
        if k in TIED:
            if table is None:
                table = torch.randn(*shp, generator=g, dtype=torch.float64).float()
            sd[k] = table
            continue
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith("relative_attention_bias.weight"):
            t = 0.5 * t
        elif k.endswith(".q.weight"):
            t = 0.5 * shp[1] ** -0.5 * t
        else:
            t = shp[1] ** -0.5 * t
        sd[k] = t.float()
    return sd


def sample_rows(shape, budget: int = 2048) -> torch.Tensor:
    """the rows of a gradient that the fixture stores: all of them up to ``budget`` values, else every step-th row"""
    n = int(np.prod(shape))
    step = 1 if n <= budget or len(shape) < 2 else -(-n // budget)
    return torch.arange(0, shape[0], step)


def checksums(sd) -> np.ndarray:
    """per tensor: (sum, sum of squares, sum of index-weighted values) in fp64"""
    out = []
    for t in sd.values():
        x = t.detach().double().reshape(-1)
        w = torch.arange(x.numel(), dtype=torch.float64) % 97
        out.append([float(x.sum()), float((x * x).sum()), float((x * w).sum())])
    return np.asarray(out, dtype=np.float64)
