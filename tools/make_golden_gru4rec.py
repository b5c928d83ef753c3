#!/usr/bin/env python3
"""Golden fixture of GRU4Rec, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.GRU4Rec.model.GRU4Rec`` (ref:SeqRec/models/discriminative/GRU4Rec/model.py) in two
configurations - the shipped one (E 64, H 128, 1 layer) and a two-layer one (E 32, H 64) - with more than 8191 items, loads the
seeded weights of ``tests/helpers/gru4rec_weights.py`` (pinned by fp64 checksums), and records with dropout off (``eval()``
for the forward pass, ``train()`` with dropout p = 0 for the loss), per configuration under the prefix "a/" or "b/":
  * forward output [B, E] and calculate_loss on right-padded rows of lengths 1 to L;
  * every parameter's gradient; the item table's only as checksums plus sampled rows (row 0 always among them), the GRU
    matrices' as checksums plus every 4th row;
  * full_sort_predict scores on sampled columns and the stable argsort's first 10 columns, without and with an item_range;
  * the reference's state-dict keys and shapes.
It also records the configuration the reference's GRU4RecConfig loads from the shipped config.json.

Usage:  python tools/make_golden_gru4rec.py      (needs the reference checkout; CPU only)
"""
import importlib.machinery
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import _ref_loader  # noqa: E402
import gru4rec_weights as gw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gru4rec_small.npz")
CONFIGS = {"a": dict(embedding_size=64, hidden_size=128, n_layers=1, dropout=0.0, loss_type="CE"),
           "b": dict(embedding_size=32, hidden_size=64, n_layers=2, dropout=0.0, loss_type="CE")}
N_ITEMS, L, SEED = 9000, 12, 5
LENS = [12, 1, 5, 3, 12, 2, 7]
ITEM_RANGE = (3001, 6001)


def reference_gru4rec():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.GRU4Rec.config import GRU4RecConfig
    from SeqRec.models.discriminative.GRU4Rec.model import GRU4Rec
    return GRU4Rec, GRU4RecConfig


def record(GRU4Rec, GRU4RecConfig, cfg, wseed, fx, tag):
    torch.manual_seed(0)
    model = GRU4Rec(GRU4RecConfig(**cfg), N_ITEMS, max_his_len=L)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    sd = gw.init_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(SEED + wseed)
    B = len(LENS)
    inputs = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(LENS):
        inputs[b, :n] = torch.randint(1, N_ITEMS + 1, (n,), generator=g)
    seq_len = torch.tensor(LENS, dtype=torch.long)
    target = torch.randint(1, N_ITEMS + 1, (B,), generator=g)
    target[0] = 0                                                  # the padding row as a target: the head reaches it
    inter = dict(inputs=inputs, seq_len=seq_len, target=target)
    model.eval()
    with torch.no_grad():
        out = model(inputs, seq_len)
        scores = model.full_sort_predict(dict(inter))
        scores_r = model.full_sort_predict(dict(inter, item_range=ITEM_RANGE))
    model.train()
    model.zero_grad()
    loss = model.calculate_loss(dict(inter))
    loss.backward()
    rows = sorted(set([0, 1, 2, N_ITEMS]) | set(inputs.flatten().tolist()) | set(target.tolist()))
    cols = sorted(set(torch.randint(0, N_ITEMS + 1, (64,), generator=g).tolist()) | {0, 1, N_ITEMS} | set(target.tolist()))
    p = tag + "/"
    fx.update({p + "inputs": inputs.numpy(), p + "seq_len": seq_len.numpy(), p + "target": target.numpy(), p + "out": out.numpy(),
               p + "loss": np.asarray(float(loss.detach())), p + "weight_checksums": gw.checksums(sd), p + "rows": np.asarray(rows),
               p + "cols": np.asarray(cols), p + "scores_cols": scores[:, cols].numpy(), p + "scores_r_cols": scores_r[:, cols].numpy(),
               p + "top10": torch.argsort(-scores, dim=1, stable=True)[:, :10].numpy(),
               p + "top10_r": torch.argsort(-scores_r, dim=1, stable=True)[:, :10].numpy()})
    for k, prm in model.named_parameters():
        gr = prm.grad.detach()
        if k == "item_embedding.weight":
            fx[p + "grad_item_rows"] = gr[rows].numpy()
            fx[p + "grad_item_checksum"] = gw.checksums({k: gr})[0]
        elif k.startswith("gru_layers."):
            fx[p + "grad4/" + k] = gr[::4].numpy()                 # (every 4th row, keeps the file small) + checksums
            fx[p + "grad_checksum/" + k] = gw.checksums({k: gr})[0]
        else:
            fx[p + "grad/" + k] = gr.numpy()
    print(f"{tag}: loss {float(loss.detach()):.6f}")
    return dict(config=cfg, weight_seed=wseed, keys=list(shapes), shapes=[list(s) for s in shapes.values()])


def main():
    GRU4Rec, GRU4RecConfig = reference_gru4rec()
    fx = {}
    meta = dict(n_items=N_ITEMS, max_his_len=L, item_range=list(ITEM_RANGE), configs={})
    for i, (tag, cfg) in enumerate(CONFIGS.items()):
        meta["configs"][tag] = record(GRU4Rec, GRU4RecConfig, cfg, 11 + i, fx, tag)
    shipped = os.path.join(_ref_loader.REF_ROOT, "config", "dis-models", "GRU4Rec")
    meta["shipped_json"] = json.load(open(os.path.join(shipped, "config.json")))
    meta["shipped_effective"] = GRU4RecConfig.from_pretrained(shipped).model_dump()
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
