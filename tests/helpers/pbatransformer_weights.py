"""The one seeded weight recipe of the PBATransformer fixture (tests/golden/pbatransformer_small.npz).

The fixture generator (tools/make_golden_pbatransformer.py, which loads the weights into the reference's
``PBATransformerForConditionalGeneration``) and the tests (which load them into ``gamer_amd.pbatransformer``) both build the weights
here; the fixture pins them with per-tensor fp64 checksums.  The recipe is tiger_weights' (the four tied keys hold one tensor,
layer-norm weights near 1, Linear weights normal(0, fan_in ** -0.5), the query projections at half of that); the behaviour
embeddings are normal(0, 1), so that the injected columns of ``wi`` move the activations as much as the hidden columns do and
every expert's weights are drawn on their own.  CPU only, no gamer_amd import."""
from collections import OrderedDict

import torch

import tiger_weights
from tiger_weights import TIED, checksums  # noqa: F401  (one recipe for the checksums)

BUDGET = 768                                                        # (three configs with a dozen experts each: the file stays below 1 MiB)


def sample_rows(shape) -> torch.Tensor:
    """the rows of a gradient that the fixture stores: tiger_weights.sample_rows with a budget of 768 values per tensor"""
    return tiger_weights.sample_rows(shape, BUDGET)


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
        elif k.endswith("behavior_embedding.weight"):
            pass
        elif k.endswith(".q.weight"):
            t = 0.5 * shp[1] ** -0.5 * t
        else:
            t = shp[1] ** -0.5 * t
        sd[k] = t.float()
    return sd
