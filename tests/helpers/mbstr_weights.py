"""The one seeded weight recipe of the MBSTR fixture (tests/golden/mbstr_small.npz).

The fixture generator (tools/make_golden_mbstr.py, which loads the weights into the reference's ``MBSTR``) and the tests (which
load them into ``gamer_amd.mbstr.MBSTR``) both build the weights here; the fixture pins them with per-tensor fp64 checksums.
With the reference's own initialisation the gradients span seven orders of magnitude (W1 2e-7, item_embedding 4), so the scales
below are chosen for the fixture: the generator prints every compared gradient tensor's largest magnitude against the median
tensor's and none may fall below 1e-3 of it.  ``head.token_embeddings.weight`` is the item table again (one tensor under two
state-dict keys).  CPU only, no gamer_amd import."""
from collections import OrderedDict

import torch

from sasrec_weights import checksums  # noqa: F401  (same checksum recipe)

SCALES = (
    ("item_embedding.weight", 0.5),
    (".W1", 0.5), (".W2", 0.5), (".alpha1", 1.0), (".alpha2", 1.0),
    (".query", 0.25), (".key", 0.25), (".value", 0.25),
    ("relative_attention_bias.weight", 0.5),
    ("head.w_gates", 0.3),
    ("head.bias", 0.7),
)


def init_state_dict(shapes: "OrderedDict[str, tuple]", seed: int, std: float = 0.15) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for k, shp in shapes.items():
        if k == "head.token_embeddings.weight":
            sd[k] = sd["item_embedding.weight"]
            continue
        t = torch.randn(*shp, generator=g, dtype=torch.float64)
        scale = next((s for suffix, s in SCALES if k.endswith(suffix)), None)
        if scale is not None:
            t = scale * t
        elif k.endswith("LayerNorm.weight") or k == "head.ln.weight":
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias"):
            t = 0.05 * t
        else:
            t = std * t
        sd[k] = t.float()
    return sd
