#!/usr/bin/env python3
"""Golden fixture of MBSTR, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.MBSTR.model.MBSTR`` (ref:SeqRec/models/discriminative/MBSTR/model.py) at a small config
(hidden 32, 2 heads, 2 layers, 4 behaviours) with more than 8191 items, loads the seeded weights of
``tests/helpers/mbstr_weights.py`` (pinned by fp64 checksums), and records with dropout off:
  * ``(masked_item_seq, labels)`` of the real ``reconstruct_train_data`` under a torch seed;
  * ``forward``'s logits on sampled columns, its labels, the loss of ``loss_fct`` on them;
  * every parameter's gradient; the item table's only as checksums plus sampled rows; the parameters left without ``.grad`` (the
    experts' LayerNorms) and those whose gradient is exactly zero (pair index 0's bias table, index 0 of query / key / value);
  * ``full_sort_predict`` on evaluation rows (ending with the mask token) on sampled columns and the stable argsort's first 10;
  * the state-dict keys and shapes, the aliasing of the two table keys, the seeded initialisation's checksums;
  * the M = 0 behaviour, the errors of ``behavior_moe=False`` / ``n_behaviors=1`` and of a type out of range;
  * the relative-position buckets of every k - q at L = 1, 50, 128 for (num_buckets, max_distance) = (32, 40) and (16, 20);
  * a second config with ``behavior_position_bias=False, behavior_head=False`` (keys ``b/...``).
It checks, and writes into ``meta_json``: every type 1 .. b occurs; every pair index 1 .. b b occurs among the non-padding
(query, key) pairs of some row; rows of length 1 and of full length occur; M >= 2 b; no compared gradient tensor's largest
magnitude is below 1e-3 of the median tensor's (the table is printed).

Usage:  python tools/make_golden_mbstr.py      (needs the reference checkout; CPU only)
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
import mbstr_weights as mw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mbstr_small.npz")
CFG = dict(n_layers=2, n_heads=2, hidden_size=32, inner_size=64, dropout_prob=0.0, hidden_act="relu", layer_norm_eps=1e-12,
           initializer_range=0.02, mask_ratio=0.3, loss_type="CE", num_buckets=32, max_distance=40, behavior_head=True,
           behavior_attention=True, behavior_moe=True, behavior_position_bias=True, n_shared_experts=3, n_specific_experts=1)
CFG_B = dict(CFG, behavior_position_bias=False, behavior_head=False, hidden_act="gelu")
N_ITEMS, N_ITEMS_B, MAX_LEN, NB, SEED, WSEED, MASK_SEED, INIT_SEED = 9000, 300, 8, 4, 5, 7, 11, 3
LENS = [8, 1, 5, 3, 8, 2, 8, 8, 6, 8]
B = len(LENS)
INIT_N_ITEMS, INIT_MAX_LEN = 500, 12
BUCKET_CASES = [(1, 32, 40), (50, 32, 40), (128, 32, 40), (1, 16, 20), (50, 16, 20), (128, 16, 20)]


def reference_mbstr():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.MBSTR.config import MBSTRConfig
    from SeqRec.models.discriminative.MBSTR.model import MBSTR
    from SeqRec.modules.layers.mbs_transformer import RelativePositionBias
    return MBSTR, MBSTRConfig, RelativePositionBias


def batch(n_items):
    g = torch.Generator().manual_seed(SEED)
    inputs = torch.zeros(B, MAX_LEN, dtype=torch.long)
    behaviors = torch.zeros(B, MAX_LEN, dtype=torch.long)
    for b, n in enumerate(LENS):
        inputs[b, :n] = torch.randint(1, n_items + 1, (n,), generator=g)
        behaviors[b, :n] = torch.randint(1, NB + 1, (n,), generator=g)
    behaviors[0] = torch.tensor([1, 2, 3, 4, 4, 3, 2, 1])          # every pair index in one row
    # evaluation rows: the history cut to MAX_LEN - 1 items plus the mask token (which carries the target's behaviour)
    ev, evb, ev_len = torch.zeros_like(inputs), torch.zeros_like(behaviors), []
    for b, n in enumerate(LENS):
        n = min(n, MAX_LEN - 1)
        ev[b, :n], evb[b, :n] = inputs[b, :n], behaviors[b, :n]
        ev[b, n], evb[b, n] = n_items + 1, 1 + b % NB
        ev_len.append(n + 1)
    return inputs, behaviors, ev, evb, torch.tensor(ev_len, dtype=torch.long)


def record(MBSTR, MBSTRConfig, cfg, n_items, prefix, fx):
    torch.manual_seed(0)
    model = MBSTR(MBSTRConfig(**cfg), n_items, MAX_LEN, NB)
    state = model.state_dict()
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in state.items())
    alias = state["item_embedding.weight"].data_ptr() == state["head.token_embeddings.weight"].data_ptr()
    sd = mw.init_state_dict(shapes, WSEED)
    model.load_state_dict(sd)
    inputs, behaviors, ev, evb, ev_len = batch(n_items)
    model.train()
    mask_seed = MASK_SEED
    while True:
        torch.manual_seed(mask_seed)
        masked, labels = model.reconstruct_train_data(inputs)
        if int((labels != 0).sum()) >= 2 * NB and bool((labels[1] != 0).any()):      # (the row of one item is masked too)
            break
        mask_seed += 1
    logits, valid_labels = model.forward(masked, behaviors, labels)
    model.zero_grad()
    loss = model.loss_fct(logits, valid_labels)
    loss.backward()
    named = dict(model.named_parameters())
    grads = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    no_grad = [k for k, p in named.items() if p.grad is None]
    zero_grad = [k for k, g_ in grads.items() if not bool(g_.any())]
    zero_index0 = [k for k, g_ in grads.items() if k.rsplit(".", 1)[-1] in ("query", "key", "value") and not bool(g_[0].any())]
    model.eval()
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inputs=ev, behaviors=evb, seq_len=ev_len))
    # M = 0
    model.train()
    model.mask_ratio = 0.0
    model.zero_grad()
    m0 = model.calculate_loss(dict(inputs=inputs, behaviors=behaviors))
    m0.backward()
    m0_zero = all(bool((p.grad == 0).all()) for k, p in model.named_parameters() if p.grad is not None)
    m0_none = [k for k, p in model.named_parameters() if p.grad is None]
    try:
        model.forward(masked, behaviors + (behaviors == NB) * 1, labels)
        type_error = ""
    except Exception as e:                                              # noqa: BLE001
        type_error = f"{type(e).__name__}: {e}"

    g = torch.Generator().manual_seed(SEED + 1)
    rows = sorted(set([0, 1, 2, n_items, n_items + 1]) | set(inputs.flatten().tolist()) | set(valid_labels.tolist()))
    cols = sorted(set(torch.randint(0, n_items + 1, (64,), generator=g).tolist()) | {0, 1, n_items} | set(valid_labels.tolist()))
    P = prefix
    fx.update({P + "inputs": inputs.numpy(), P + "behaviors": behaviors.numpy(), P + "masked": masked.numpy(),
               P + "labels": labels.numpy(), P + "valid_labels": valid_labels.numpy(),
               P + "logits_cols": logits.detach()[:, cols].numpy(), P + "loss": np.asarray(float(loss)),
               P + "weight_checksums": mw.checksums(sd), P + "rows": np.asarray(rows), P + "cols": np.asarray(cols),
               P + "eval_inputs": ev.numpy(), P + "eval_behaviors": evb.numpy(), P + "eval_seq_len": ev_len.numpy(),
               P + "scores_cols": scores[:, cols].numpy(), P + "top10": torch.argsort(-scores, dim=1, stable=True)[:, :10].numpy()})
    for k, gr in grads.items():
        if k == "item_embedding.weight":
            fx[P + "grad_item_rows"] = gr[rows].numpy()
            fx[P + "grad_item_checksum"] = mw.checksums({k: gr})[0]
        else:
            fx[P + "grad/" + k] = gr.numpy()
    # the conditions on the fixture
    types_seen = sorted(set(behaviors[behaviors != 0].tolist()))
    pairs = set()
    for b in range(B):
        t = behaviors[b][behaviors[b] != 0]
        pairs |= set(((t[:, None] - 1) * NB + t[None, :]).flatten().tolist())
    mags = {k: float(g_.abs().max()) for k, g_ in grads.items() if k not in zero_grad}
    med = float(np.median(list(mags.values())))
    print(f"[{prefix or 'a/'}] gradient magnitudes (largest |g| per compared tensor; median {med:.3e}):")
    for k, v in sorted(mags.items(), key=lambda kv: kv[1]):
        print(f"    {v:.3e}  {v / med:9.2e} x median  {k}")
    cond = dict(every_type_occurs=types_seen == list(range(1, NB + 1)),
                every_pair_index_occurs=pairs == set(range(1, NB * NB + 1)),
                rows_of_length_1_and_full=1 in LENS and MAX_LEN in LENS,
                M_at_least_2b=int(valid_labels.numel()) >= 2 * NB,
                smallest_gradient_over_median=min(mags.values()) / med,
                gradient_scales_ok=min(mags.values()) >= 1e-3 * med)
    print(f"[{prefix or 'a/'}] conditions: {json.dumps(cond)}")
    assert all(v for k, v in cond.items() if k != "smallest_gradient_over_median"), cond
    return dict(config=cfg, n_items=n_items, max_his_len=MAX_LEN, n_behaviors=NB, weight_seed=WSEED, mask_seed=mask_seed,
                keys=list(shapes), shapes=[list(s) for s in shapes.values()], table_keys_alias=bool(alias),
                parameter_names=list(named), no_grad=no_grad, zero_grad=zero_grad, zero_index0=zero_index0,
                m0_loss_is_nan=bool(torch.isnan(m0)), m0_grads_all_zero=bool(m0_zero), m0_no_grad=m0_none, type_error=type_error,
                M=int(valid_labels.numel()), conditions=cond, loss=float(loss))


def main():
    MBSTR, MBSTRConfig, RelativePositionBias = reference_mbstr()
    fx = {}
    torch.manual_seed(INIT_SEED)
    init = MBSTR(MBSTRConfig(), INIT_N_ITEMS, INIT_MAX_LEN, NB)
    fx["init_checksums"] = mw.checksums(init.state_dict())
    init_keys, init_params = len(init.state_dict()), sum(p.numel() for p in init.parameters())
    unknown_ok = MBSTRConfig(foo=1, **CFG)
    errors = {}
    for name, kw, nb in (("behavior_moe_false", dict(behavior_moe=False), NB), ("n_behaviors_1", {}, 1)):
        try:
            m = MBSTR(MBSTRConfig(**dict(CFG, **kw)), 50, MAX_LEN, nb)
            m(torch.ones(2, MAX_LEN, dtype=torch.long), torch.ones(2, MAX_LEN, dtype=torch.long), torch.ones(2, MAX_LEN, dtype=torch.long))
            errors[name] = ""
        except Exception as e:                                          # noqa: BLE001
            errors[name] = f"{type(e).__name__}: {e}"
    for L, nbk, md in BUCKET_CASES:
        rp = torch.arange(L)[None, :] - torch.arange(L)[:, None]
        bk = RelativePositionBias._relative_position_bucket(rp, num_buckets=nbk, max_distance=md)
        by_offset = torch.stack([bk[max(0, -r), max(0, -r) + r] for r in range(-(L - 1), L)])
        assert all(bool((torch.diagonal(bk, r) == by_offset[r + L - 1]).all()) for r in range(-(L - 1), L))      # a function of k - q
        fx[f"buckets/{L}_{nbk}_{md}"] = by_offset.numpy().astype(np.int32)
    meta = record(MBSTR, MBSTRConfig, CFG, N_ITEMS, "", fx)
    meta_b = record(MBSTR, MBSTRConfig, CFG_B, N_ITEMS_B, "b/", fx)
    meta.update(init_seed=INIT_SEED, init_n_items=INIT_N_ITEMS, init_max_his_len=INIT_MAX_LEN, init_keys=init_keys,
                init_parameters=init_params, unknown_key_dropped=not hasattr(unknown_ok, "foo"), reference_errors=errors,
                bucket_cases=BUCKET_CASES, second=meta_b)
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), loss {meta['loss']:.6f} / {meta_b['loss']:.6f}, M {meta['M']} / {meta_b['M']}")
    print(json.dumps({k: v for k, v in meta.items() if k not in ("keys", "shapes", "parameter_names", "second")}))


if __name__ == "__main__":
    main()
