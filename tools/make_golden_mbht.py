#!/usr/bin/env python3
"""Golden fixture of MBHT, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.MBHT.model.MBHT`` (ref:SeqRec/models/discriminative/MBHT/model.py) at 60 items, 3 behaviours,
hidden 32, 2 heads, inner 64, hyper_len 4, with ``dropout_prob = 0`` and ``hgnn_layer.dropout = 0.0`` set on the instance, in train
mode on a batch of 6 rows, in two configurations:
  a/   max_his_len 15, scales [3, 4, 8], enable_hg on,  enable_ms on
  b/   max_his_len 7,  scales [2, 2, 4], enable_hg off, enable_ms on
It loads the seeded weights of ``tests/helpers/mbht_weights.py`` (pinned by fp64 checksums) and records
  * the four outputs of the real ``reconstruct_train_data`` under ``random.seed``;
  * ``forward``'s output, the loss, every parameter's gradient and the names of the parameters left without one;
  * ``full_sort_predict`` scores and the stable argsort's first 10 for an evaluation batch;
  * the state-dict keys and shapes of the two configurations and of ``enable_ms=False``, and the seeded initialisation's checksums
    (``gating_bias``, uninitialised memory in the reference, is left out of them).
The batch holds a row with n = 1, a row with n < hyper_len, a full row and a repeated item; the mask seed is searched until two
adjacent masked positions and a masked position 0 occur.  For every row of every similarity matrix the generator meets (training and
evaluation batch) it asserts that no similarity is negative and that the k-th selected value exceeds the best unselected value of
an item that is not among the selected ones by more than 1e-4, so that fp32 cannot flip a selection; it draws another weight seed
otherwise.  No row is left out of any comparison.

Usage:  python tools/make_golden_mbht.py      (needs the reference checkout; CPU only)
"""
import importlib.machinery
import json
import os
import random
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import _ref_loader  # noqa: E402
import mbht_weights as mw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mbht_small.npz")
BASE = dict(n_layers=2, n_heads=2, hidden_size=32, inner_size=64, dropout_prob=0.0, hidden_act="gelu", layer_norm_eps=1e-12,
            initializer_range=0.02, mask_ratio=0.4, loss_type="CE", hyper_len=4)
CASES = OrderedDict([
    ("a/", dict(cfg=dict(BASE, scales=[3, 4, 8], enable_hg=True, enable_ms=True), max_his_len=15, lens=[1, 3, 15, 9, 12, 6])),
    ("b/", dict(cfg=dict(BASE, scales=[2, 2, 4], enable_hg=False, enable_ms=True), max_his_len=7, lens=[1, 3, 7, 5, 6, 2])),
])
PLAIN = dict(BASE, scales=[2, 2, 4], enable_hg=True, enable_ms=False)            # (state-dict keys and seeded init only)
N_ITEMS, NB, TARGET_BEHAVIOR_ID, SEED, INIT_SEED, MARGIN = 60, 3, 3, 5, 3, 1e-4


def reference_mbht():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.MBHT.config import MBHTConfig
    from SeqRec.models.discriminative.MBHT.model import MBHT
    return MBHT, MBHTConfig


def batch(lens, max_his_len):
    g = torch.Generator().manual_seed(SEED)
    B, W = len(lens), max(lens)
    inputs, behaviors = torch.zeros(B, W, dtype=torch.long), torch.zeros(B, W, dtype=torch.long)
    for b, n in enumerate(lens):
        inputs[b, :n] = torch.randperm(N_ITEMS, generator=g)[:n] + 1
        behaviors[b, :n] = torch.randint(1, NB + 1, (n,), generator=g)
    inputs[3, 4] = inputs[3, 1]                                                  # a repeated item ...
    inputs[4, 5] = inputs[4, 0]
    inputs[4, 2] = inputs[4, 0]                                                  # ... and one that occurs three times
    target = torch.randint(1, N_ITEMS + 1, (B,), generator=g)
    target[4] = inputs[4, 3]                                                     # the target repeats a history item
    behavior = torch.full((B,), TARGET_BEHAVIOR_ID, dtype=torch.long)
    # evaluation rows: histories of other lengths (a full one among them)
    ev_lens = [max(1, min(max_his_len, n + d)) for n, d in zip(lens, (0, 1, 0, -2, 1, 3))]
    ev, evb = torch.zeros(B, max_his_len, dtype=torch.long), torch.zeros(B, max_his_len, dtype=torch.long)
    for b, n in enumerate(ev_lens):
        ev[b, :n] = torch.randint(1, N_ITEMS + 1, (n,), generator=g)
        evb[b, :n] = torch.randint(1, NB + 1, (n,), generator=g)
    return inputs, behaviors, target, behavior, ev, evb


def selection_margin(model, item_seq):
    """(smallest margin, smallest similarity) over every live row of the similarity matrices of item_seq [B, L]"""
    with torch.no_grad():
        e = model.item_embedding(item_seq)
        x = e * torch.sigmoid(e.matmul(model.gating_weight) + model.gating_bias)
        xm = torch.stack((model.metric_w1 * x, model.metric_w2 * x)).mean(0)
        z = F.normalize(xm)                                                       # (dim 1 of [B, l, H], as the reference calls it)
        sim = z @ z.transpose(1, 2)
    worst, low = float("inf"), float("inf")
    for b in range(item_seq.shape[0]):
        n = int(torch.count_nonzero(item_seq[b]))
        s, seq = sim[b, :n, :n], item_seq[b, :n]
        low = min(low, float(s.min()))
        k = min(model.hglen, n)
        for i in range(n):
            vals, idx = torch.sort(s[i], descending=True, stable=True)
            chosen = set(seq[idx[:k]].tolist())
            rest = [float(v) for v, j in zip(vals[k:], idx[k:]) if int(seq[j]) not in chosen]
            if rest:
                worst = min(worst, float(vals[k - 1]) - max(rest))
    return worst, low


def shapes_of(model):
    return OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())


def record(MBHT, MBHTConfig, prefix, case, fx):
    cfg, max_his_len, lens = case["cfg"], case["max_his_len"], case["lens"]
    torch.manual_seed(0)
    model = MBHT(MBHTConfig(**cfg), N_ITEMS, max_his_len, TARGET_BEHAVIOR_ID, NB)
    model.hgnn_layer.dropout = 0.0
    shapes = shapes_of(model)
    inputs, behaviors, target, behavior, ev, evb = batch(lens, max_his_len)
    model.train()
    wseed = 7
    while True:
        sd = mw.init_state_dict(shapes, wseed)
        model.load_state_dict(sd)
        mask_seed = 11
        while True:
            random.seed(mask_seed)
            masked, pos_items, masked_index, types = model.reconstruct_train_data(inputs, behaviors, target, behavior)
            m = masked == model.mask_token
            if bool((m[:, :-1] & m[:, 1:]).any()) and bool(m[:, 0].any()) and bool((m[:, 0] & (m.sum(1) > 1)).any()):
                break
            mask_seed += 1
        ev_items, _ = model.reconstruct_test_data(ev, torch.count_nonzero(ev, 1), evb)
        margins = [selection_margin(model, masked), selection_margin(model, ev_items)]
        margin, low = min(x[0] for x in margins), min(x[1] for x in margins)
        if not cfg["enable_hg"] or (margin > MARGIN and low > 0):
            break
        wseed += 1
    mask_nums = torch.count_nonzero(pos_items, dim=1)
    model.zero_grad()
    out = model.forward(masked, types, mask_positions_nums=(masked_index, mask_nums))
    random.seed(mask_seed)
    loss = model.calculate_loss(dict(inputs=inputs, behaviors=behaviors, target=target, behavior=behavior))
    loss.backward()
    named = dict(model.named_parameters())
    grads = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    no_grad = [k for k, p in named.items() if p.grad is None]
    model.eval()
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inputs=ev, behaviors=evb))
    model.train()
    P = prefix
    fx.update({P + "inputs": inputs.numpy(), P + "behaviors": behaviors.numpy(), P + "target": target.numpy(),
               P + "behavior": behavior.numpy(), P + "masked": masked.numpy(), P + "pos_items": pos_items.numpy(),
               P + "masked_index": masked_index.numpy(), P + "types": types.numpy(), P + "out": out.detach().numpy(),
               P + "loss": np.asarray(float(loss)), P + "weight_checksums": mw.checksums(sd), P + "eval_inputs": ev.numpy(),
               P + "eval_behaviors": evb.numpy(), P + "scores": scores.numpy(),
               P + "top10": torch.argsort(-scores, dim=1, stable=True)[:, :10].numpy()})
    for k, gr in grads.items():
        fx[P + "grad/" + k] = gr.numpy()
    n_hist = [int(x) for x in torch.count_nonzero(inputs, 1)]
    m = masked == model.mask_token
    mags = {k: float(g_.abs().max()) for k, g_ in grads.items()}
    print(f"[{prefix}] gradient magnitudes (largest |g| per tensor):")
    for k, v in sorted(mags.items(), key=lambda kv: kv[1]):
        print(f"    {v:.3e}  {k}")
    cond = dict(row_with_n_1=1 in n_hist, row_below_hyper_len=any(1 < n < cfg["hyper_len"] for n in n_hist),
                full_row=max_his_len in n_hist, repeated_item=any(len(set(r[r != 0].tolist())) < int((r != 0).sum()) for r in inputs),
                adjacent_masks=bool((m[:, :-1] & m[:, 1:]).any()), masked_position_0=bool(m[:, 0].any()),
                counted_positions=int((masked_index > 0).sum()), no_zero_gradient=min(mags.values()) > 0)
    print(f"[{prefix}] conditions: {json.dumps(cond)}; selection margin {margin:.3e}, smallest similarity {low:.3e}")
    assert all(cond.values()), cond
    return dict(config=cfg, n_items=N_ITEMS, max_his_len=max_his_len, n_behaviors=NB, target_behavior_id=TARGET_BEHAVIOR_ID,
                weight_seed=wseed, mask_seed=mask_seed, keys=list(shapes), shapes=[list(s) for s in shapes.values()],
                parameter_names=list(named), no_grad=no_grad, conditions=cond, loss=float(loss),
                selection_margin=margin, smallest_similarity=low)


def main():
    MBHT, MBHTConfig = reference_mbht()
    fx, meta = {}, {}
    init = {}
    for name, cfg, mhl in (("a/", CASES["a/"]["cfg"], 15), ("b/", CASES["b/"]["cfg"], 7), ("plain/", PLAIN, 7)):
        torch.manual_seed(INIT_SEED)
        model = MBHT(MBHTConfig(**cfg), N_ITEMS, mhl, TARGET_BEHAVIOR_ID, NB)
        sd = OrderedDict((k, v) for k, v in model.state_dict().items() if k != "gating_bias")
        fx[name + "init_checksums"] = mw.checksums(sd)
        shapes = shapes_of(model)
        init[name] = dict(config=cfg, max_his_len=mhl, keys=list(shapes), shapes=[list(s) for s in shapes.values()])
    defaults = MBHTConfig().model_dump() if hasattr(MBHTConfig(), "model_dump") else MBHTConfig().dict()
    unknown_ok = MBHTConfig(foo=1, **CASES["a/"]["cfg"])
    for prefix, case in CASES.items():
        meta[prefix] = record(MBHT, MBHTConfig, prefix, case, fx)
    meta.update(init_seed=INIT_SEED, init=init, config_defaults=defaults, unknown_key_dropped=not hasattr(unknown_ok, "foo"))
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), loss {meta['a/']['loss']:.6f} / {meta['b/']['loss']:.6f}")


if __name__ == "__main__":
    main()
