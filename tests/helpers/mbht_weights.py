"""The one seeded weight recipe of the MBHT fixture (tests/golden/mbht_small.npz).

The fixture generator (tools/make_golden_mbht.py, which loads the weights into the reference's ``MBHT``) and the tests (which load
them into ``gamer_amd.mbht.MBHT``) both build the weights here; the fixture pins them with per-tensor fp64 checksums.  The item
table gets a common positive offset, so that the gated item vectors of the hypergraph branch point into one orthant and no cosine
similarity is negative (none is clamped to 0.01); ``metric_w1`` / ``metric_w2`` are drawn around 1 for the same reason.  The
sequence-axis projections (``E``, ``F``, ``out_fc``) mix a whole row, so they are drawn larger than the matrices.  CPU only, no
gamer_amd import."""
from collections import OrderedDict

import torch

from sasrec_weights import checksums  # noqa: F401  (same checksum recipe)

OFFSET = 0.5


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int, std: float = 0.15) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if k == "item_embedding.weight":
            t = OFFSET + 0.3 * t
        elif k in ("metric_w1", "metric_w2"):
            t = 1.0 + 0.3 * t
        elif k.endswith("LayerNorm.weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias") or k == "gating_bias":
            t = 0.05 * t
        elif k.endswith((".E.weight", ".F.weight", ".out_fc.weight")):
            t = 0.3 * t
        elif k in ("attn", "attn_weights"):
            t = 0.4 * t
        else:
            t = std * t
        sd[k] = t.float()
    return sd
