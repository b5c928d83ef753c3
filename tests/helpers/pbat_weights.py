"""The one seeded weight recipe of the PBAT fixture (tests/golden/pbat_small.npz).

The fixture generator (tools/make_golden_pbat.py, which loads the weights into the reference's ``PBAT``) and the tests (which load
them into ``gamer_amd.pbat.PBAT``) both build the weights here; the fixture pins them with per-tensor fp64 checksums.  The scales
are chosen for the fixture: the generator prints every compared gradient tensor's largest magnitude against the median tensor's
and none may fall below 1e-3 of it.  ``head.token_embeddings_{m, c}.weight`` are the item tables again (one tensor under two
state-dict keys each).  CPU only, no gamer_amd import."""
from collections import OrderedDict

import torch

from sasrec_weights import checksums  # noqa: F401  (same checksum recipe)

ALIASES = {"head.token_embeddings_m.weight": "item_embedding_m.embedding.weight",
           "head.token_embeddings_c.weight": "item_embedding_c.embedding.weight"}
# (the relation Gaussians are the user x behaviour distances times the relation embeddings: with LayerNorm weights near 1 the
# distances reach tens, the relation covariances underflow and the attention saturates - every score gradient vanishes)
SCALES = (
    ("type_relation_embedding_m.LayerNorm.weight", 0.1), ("type_relation_embedding_c.LayerNorm.weight", 0.1),
    ("type_relation_embedding_m.LayerNorm.bias", 0.02), ("type_relation_embedding_c.LayerNorm.bias", 0.02),
    ("Wub.weight", 0.05),
    ("embedding.weight", 0.5),
    ("position_embedding_m.weight", 0.5), ("position_embedding_c.weight", 0.5),
    (".Wq1.weight", 0.3), (".Wq2.weight", 0.3), (".Wk1.weight", 0.3), (".Wk2.weight", 0.3),
)


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int, std: float = 0.15) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        if k in ALIASES:
            sd[k] = sd[ALIASES[k]]
            continue
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        scale = next((s for suffix, s in SCALES if k.endswith(suffix)), None)
        if scale is not None:
            t = scale * t
        elif k.endswith("LayerNorm.weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias"):
            t = 0.05 * t
        else:
            t = std * t
        sd[k] = t.float()
    return sd
