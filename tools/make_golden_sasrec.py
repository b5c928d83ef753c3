#!/usr/bin/env python3
"""Golden fixture of SASRec, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.SASRec.model.SASRec`` (ref:SeqRec/models/discriminative/SASRec/model.py) at a small
config (hidden 64, 2 heads, 2 layers) with more than 8191 items, loads the seeded weights of
``tests/helpers/sasrec_weights.py`` (pinned by fp64 checksums), and records with dropout off (``eval()`` for the forward
pass, ``train()`` with every dropout p = 0 for the loss):
  * forward output [B, H] and calculate_loss on right-padded rows that include length 1;
  * every parameter's gradient; the item table's only as checksums plus sampled rows (row 0 always among them);
  * full_sort_predict scores on sampled columns and the stable argsort's first 10 columns, without and with an item_range
    (the smb_dis_diff test layout);
  * the reference's state-dict keys and shapes.

Usage:  python tools/make_golden_sasrec.py      (needs the reference checkout; CPU only)
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
import sasrec_weights as sw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sasrec_small.npz")
CFG = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=128, dropout_prob=0.0, hidden_act="gelu", layer_norm_eps=1e-12,
           initializer_range=0.02, loss_type="CE")
N_ITEMS, MAX_LEN, B, SEED, WSEED = 9000, 8, 6, 5, 7
LENS = [8, 1, 5, 3, 8, 2]
ITEM_RANGE = (3001, 6001)


def reference_sasrec():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.SASRec.config import SASRecConfig
    from SeqRec.models.discriminative.SASRec.model import SASRec
    return SASRec, SASRecConfig


def main():
    SASRec, SASRecConfig = reference_sasrec()
    torch.manual_seed(0)
    model = SASRec(SASRecConfig(**CFG), N_ITEMS, MAX_LEN)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    sd = sw.init_state_dict(shapes, WSEED)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(SEED)
    inputs = torch.zeros(B, MAX_LEN, dtype=torch.long)
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
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}   # (FeedForward.LayerNorm: none)
    rows = sorted(set([0, 1, 2, N_ITEMS]) | set(inputs.flatten().tolist()) | set(target.tolist()))
    cols = sorted(set(torch.randint(0, N_ITEMS + 1, (64,), generator=g).tolist()) | {0, 1, N_ITEMS} | set(target.tolist()))
    fx = {"inputs": inputs.numpy(), "seq_len": seq_len.numpy(), "target": target.numpy(), "out": out.numpy(),
          "loss": np.asarray(float(loss)), "weight_checksums": sw.checksums(sd), "rows": np.asarray(rows), "cols": np.asarray(cols),
          "scores_cols": scores[:, cols].numpy(), "scores_r_cols": scores_r[:, cols].numpy(),
          "top10": torch.argsort(-scores, dim=1, stable=True)[:, :10].numpy(),
          "top10_r": torch.argsort(-scores_r, dim=1, stable=True)[:, :10].numpy()}
    for k, gr in grads.items():
        if k == "item_embedding.weight":
            fx["grad_item_rows"] = gr[rows].numpy()
            fx["grad_item_checksum"] = sw.checksums({k: gr})[0]
        else:
            fx["grad/" + k] = gr.numpy()
    meta = dict(config=CFG, n_items=N_ITEMS, max_his_len=MAX_LEN, weight_seed=WSEED, item_range=list(ITEM_RANGE),
                keys=list(shapes), shapes=[list(s) for s in shapes.values()])
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), loss {float(loss):.6f}")


if __name__ == "__main__":
    main()
