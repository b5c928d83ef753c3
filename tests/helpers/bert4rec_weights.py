"""The one seeded weight recipe of the BERT4Rec fixture (tests/golden/bert4rec_small.npz).

The fixture generator (tools/make_golden_bert4rec.py, which loads the weights into the reference's ``BERT4Rec``) and the tests
(which load them into ``gamer_amd.bert4rec.BERT4Rec``) both build the weights here; the fixture pins them with per-tensor fp64
checksums.  As tests/helpers/sasrec_weights.py, except that ``head.bias`` is of order 1 (a zero bias would leave the head's bias
path untested) and ``head.token_embeddings.weight`` is the item table again (one tensor under two state-dict keys).  CPU only,
no gamer_amd import."""
from collections import OrderedDict

import torch

from sasrec_weights import checksums  # noqa: F401  (same checksum recipe)


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int, std: float = 0.1) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        if k == "head.token_embeddings.weight":
            sd[k] = sd["item_embedding.weight"]
            continue
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        if k == "head.bias":
            t = 0.7 * t
        elif k.endswith("LayerNorm.weight") or k == "output_ln.weight":
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias") or k == "output_bias":
            t = 0.02 * t
        else:
            t = std * t
        sd[k] = t.float()
    return sd
