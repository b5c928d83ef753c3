#!/usr/bin/env python3
"""Golden fixture of PBAT, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.PBAT.model.PBAT`` (ref:SeqRec/models/discriminative/PBAT/model.py) at two small configs -
(a) hidden 32, 2 heads, 2 layers, 4 behaviours, ``hidden_act="elu"``, more than 8191 items; (b, keys ``b/...``) 4 heads,
2 behaviours, ``"gelu"``, 300 items (the reference cannot run with ONE head: the ``.squeeze()`` of its distance drops the head
axis and the context's ``view`` raises; the error text is recorded as ``h1_error``) - with 12 users, B = 10, L = 8 and dropout 0, loads the seeded weights of
``tests/helpers/pbat_weights.py`` (pinned by fp64 checksums), and records:
  * ``(masked_item_seq, labels)`` of the real ``reconstruct_train_data`` under a torch seed;
  * ``forward``'s logits on sampled columns, its labels, the loss of ``loss_fct`` on them;
  * every parameter's gradient; the two item tables' only as checksums plus sampled rows; the parameters left without ``.grad``
    (the experts' LayerNorms);
  * ``full_sort_predict`` on evaluation rows (ending with the mask token) on sampled columns and ``argsort(-scores)``'s first 10;
  * the state-dict keys and shapes, the aliasing of the table keys, the seeded initialisation's checksums;
  * the B = 1 ``IndexError``, the M = 1 loss (1-D logits) and the M = 0 behaviour.
It checks, and writes into ``meta_json``: every type occurs; every (query type, key type) pair occurs among the non-padding
positions of some row; rows of length 1 and of full length occur; no compared gradient tensor's largest magnitude is below 1e-3 of
the median tensor's (the table is printed).

Usage:  python tools/make_golden_pbat.py      (needs the reference checkout; CPU only)
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
import pbat_weights as pw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pbat_small.npz")
CFG = dict(n_layers=2, n_heads=2, hidden_size=32, inner_size=64, dropout_prob=0.0, hidden_act="elu", layer_norm_eps=1e-12,
           initializer_range=0.02, mask_ratio=0.3, loss_type="CE")
CFG_B = dict(CFG, n_heads=4, hidden_act="gelu")
N_ITEMS, N_ITEMS_B, N_USERS, MAX_LEN, NB, NB_B, SEED, WSEED, MASK_SEED, INIT_SEED = 9000, 300, 12, 8, 4, 2, 5, 7, 11, 3
LENS = [8, 1, 5, 3, 8, 2, 8, 8, 6, 8]
B = len(LENS)
INIT_N_ITEMS, INIT_N_USERS, INIT_MAX_LEN, INIT_NB = 500, 20, 12, 3
TABLES = ("item_embedding_m.embedding.weight", "item_embedding_c.embedding.weight")


def reference_pbat():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.PBAT.config import PBATConfig
    from SeqRec.models.discriminative.PBAT.model import PBAT
    return PBAT, PBATConfig


def batch(n_items, nb):
    g = torch.Generator().manual_seed(SEED)
    inputs = torch.zeros(B, MAX_LEN, dtype=torch.long)
    behaviors = torch.zeros(B, MAX_LEN, dtype=torch.long)
    for b, n in enumerate(LENS):
        inputs[b, :n] = torch.randint(1, n_items + 1, (n,), generator=g)
        behaviors[b, :n] = torch.randint(1, nb + 1, (n,), generator=g)
    behaviors[0] = torch.tensor([1 + i % nb for i in range(MAX_LEN)])           # every pair of types in one row
    uid = torch.tensor([1 + (3 * b) % N_USERS for b in range(B)], dtype=torch.long)
    # evaluation rows: the history cut to MAX_LEN - 1 items plus the mask token (which carries the target's behaviour)
    ev, evb, ev_len = torch.zeros_like(inputs), torch.zeros_like(behaviors), []
    for b, n in enumerate(LENS):
        n = min(n, MAX_LEN - 1)
        ev[b, :n], evb[b, :n] = inputs[b, :n], behaviors[b, :n]
        ev[b, n], evb[b, n] = n_items + 1, 1 + b % nb
        ev_len.append(n + 1)
    return inputs, behaviors, uid, ev, evb, torch.tensor(ev_len, dtype=torch.long)


def record(PBAT, PBATConfig, cfg, n_items, nb, prefix, fx):
    torch.manual_seed(0)
    model = PBAT(PBATConfig(**cfg), n_items, N_USERS, MAX_LEN, nb)
    state = model.state_dict()
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in state.items())
    alias = all(state[k].data_ptr() == state[v].data_ptr() for k, v in pw.ALIASES.items())
    sd = pw.init_state_dict(shapes, WSEED)
    model.load_state_dict(sd)
    inputs, behaviors, uid, ev, evb, ev_len = batch(n_items, nb)
    model.train()
    mask_seed = MASK_SEED
    while True:
        torch.manual_seed(mask_seed)
        masked, labels = model.reconstruct_train_data(inputs)
        if int((labels != 0).sum()) >= 2 * nb and bool((labels[1] != 0).any()):      # (the row of one item is masked too)
            break
        mask_seed += 1
    logits, valid_labels = model.forward(masked, behaviors, uid, labels)
    model.zero_grad()
    loss = model.loss_fct(logits, valid_labels)
    loss.backward()
    named = dict(model.named_parameters())
    grads = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    no_grad = [k for k, p in named.items() if p.grad is None]
    zero_grad = [k for k, g_ in grads.items() if not bool(g_.any())]
    model.eval()
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inputs=ev, behaviors=evb, uid=uid, seq_len=ev_len))
    # B = 1
    try:
        model.full_sort_predict(dict(inputs=ev[:1], behaviors=evb[:1], uid=uid[:1], seq_len=ev_len[:1]))
        b1_error = ""
    except Exception as e:                                              # noqa: BLE001
        b1_error = f"{type(e).__name__}: {e}"
    # M = 1: one label in the batch; the head returns 1-D logits
    model.train()
    one = torch.zeros_like(labels)
    one[0, 2] = inputs[0, 2]
    masked1 = inputs.clone()
    masked1[0, 2] = n_items + 1
    l1, vl1 = model.forward(masked1, behaviors, uid, one)
    m1_loss = float(model.loss_fct(l1, vl1))
    # M = 0
    model.mask_ratio = 0.0
    model.zero_grad()
    try:
        m0 = model.calculate_loss(dict(inputs=inputs, behaviors=behaviors, uid=uid))
        m0.backward()
        m0_nan = bool(torch.isnan(m0))
        m0_zero = all(bool((p.grad == 0).all()) for k, p in model.named_parameters() if p.grad is not None)
        m0_none = [k for k, p in model.named_parameters() if p.grad is None]
        m0_error = ""
    except Exception as e:                                              # noqa: BLE001
        m0_nan, m0_zero, m0_none, m0_error = False, False, [], f"{type(e).__name__}: {e}"
    try:
        model.forward(masked, behaviors + (behaviors == nb) * 1, uid, labels)
        type_error = ""
    except Exception as e:                                              # noqa: BLE001
        type_error = f"{type(e).__name__}: {e}"

    g = torch.Generator().manual_seed(SEED + 1)
    rows = sorted(set([0, 1, 2, n_items, n_items + 1]) | set(inputs.flatten().tolist()) | set(valid_labels.tolist()))
    cols = sorted(set(torch.randint(0, n_items + 1, (64,), generator=g).tolist()) | {0, 1, n_items} | set(valid_labels.tolist()))
    P = prefix
    fx.update({P + "inputs": inputs.numpy(), P + "behaviors": behaviors.numpy(), P + "uid": uid.numpy(), P + "masked": masked.numpy(),
               P + "labels": labels.numpy(), P + "valid_labels": valid_labels.numpy(),
               P + "logits_cols": logits.detach()[:, cols].numpy(), P + "loss": np.asarray(float(loss)),
               P + "weight_checksums": pw.checksums(sd), P + "rows": np.asarray(rows), P + "cols": np.asarray(cols),
               P + "eval_inputs": ev.numpy(), P + "eval_behaviors": evb.numpy(), P + "eval_seq_len": ev_len.numpy(),
               P + "scores_cols": scores[:, cols].numpy(), P + "top10": torch.argsort(-scores, dim=1)[:, :10].numpy(),
               P + "top10_scores": torch.sort(scores, dim=1, descending=True)[0][:, :11].numpy(),
               P + "m1_masked": masked1.numpy(), P + "m1_labels": one.numpy(), P + "m1_loss": np.asarray(m1_loss)})
    for k, gr in grads.items():
        if k in TABLES:
            fx[P + "grad_rows/" + k] = gr[rows].numpy()
            fx[P + "grad_checksum/" + k] = pw.checksums({k: gr})[0]
        else:
            fx[P + "grad/" + k] = gr.numpy()
    types_seen = sorted(set(behaviors[behaviors != 0].tolist()))
    pairs = set()
    for b in range(B):
        t = behaviors[b][behaviors[b] != 0]
        pairs |= set((t[:, None] * (nb + 1) + t[None, :]).flatten().tolist())
    want_pairs = {i * (nb + 1) + j for i in range(1, nb + 1) for j in range(1, nb + 1)}
    mags = {k: float(g_.abs().max()) for k, g_ in grads.items() if k not in zero_grad}
    med = float(np.median(list(mags.values())))
    print(f"[{prefix or 'a/'}] gradient magnitudes (largest |g| per compared tensor; median {med:.3e}):")
    for k, v in sorted(mags.items(), key=lambda kv: kv[1]):
        print(f"    {v:.3e}  {v / med:9.2e} x median  {k}")
    cond = dict(every_type_occurs=types_seen == list(range(1, nb + 1)),
                every_type_pair_occurs=pairs == want_pairs,
                rows_of_length_1_and_full=1 in LENS and MAX_LEN in LENS,
                M_at_least_2b=int(valid_labels.numel()) >= 2 * nb,
                smallest_gradient_over_median=min(mags.values()) / med,
                gradient_scales_ok=min(mags.values()) >= 1e-3 * med)
    print(f"[{prefix or 'a/'}] conditions: {json.dumps(cond)}")
    assert all(v for k, v in cond.items() if k != "smallest_gradient_over_median"), cond
    return dict(config=cfg, n_items=n_items, n_users=N_USERS, max_his_len=MAX_LEN, n_behaviors=nb, weight_seed=WSEED,
                mask_seed=mask_seed, keys=list(shapes), shapes=[list(s) for s in shapes.values()], table_keys_alias=bool(alias),
                parameter_names=list(named), no_grad=no_grad, zero_grad=zero_grad, b1_error=b1_error,
                m0_loss_is_nan=m0_nan, m0_grads_all_zero=bool(m0_zero), m0_no_grad=m0_none, m0_error=m0_error, type_error=type_error,
                M=int(valid_labels.numel()), m1_logits_dim=int(l1.dim()), conditions=cond, loss=float(loss))


def main():
    PBAT, PBATConfig = reference_pbat()
    fx = {}
    torch.manual_seed(INIT_SEED)
    init = PBAT(PBATConfig(), INIT_N_ITEMS, INIT_N_USERS, INIT_MAX_LEN, INIT_NB)
    fx["init_checksums"] = pw.checksums(init.state_dict())
    init_keys, init_params = len(init.state_dict()), sum(p.numel() for p in init.parameters())
    unknown_ok = PBATConfig(foo=1, **CFG)
    try:
        one_head = PBAT(PBATConfig(**dict(CFG, n_heads=1)), 50, N_USERS, MAX_LEN, NB_B)
        t = torch.ones(2, MAX_LEN, dtype=torch.long)
        one_head(t, t, torch.ones(2, dtype=torch.long), t)
        h1_error = ""
    except Exception as e:                                              # noqa: BLE001
        h1_error = f"{type(e).__name__}: {e}"
    meta = record(PBAT, PBATConfig, CFG, N_ITEMS, NB, "", fx)
    meta_b = record(PBAT, PBATConfig, CFG_B, N_ITEMS_B, NB_B, "b/", fx)
    meta.update(init_seed=INIT_SEED, init_n_items=INIT_N_ITEMS, init_n_users=INIT_N_USERS, init_max_his_len=INIT_MAX_LEN,
                init_n_behaviors=INIT_NB, init_keys=init_keys, init_state_keys=list(init.state_dict()), init_parameters=init_params,
                unknown_key_dropped=not hasattr(unknown_ok, "foo"), h1_error=h1_error, config_defaults=PBATConfig().model_dump(), second=meta_b)
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), loss {meta['loss']:.6f} / {meta_b['loss']:.6f}, M {meta['M']} / {meta_b['M']}")
    print(json.dumps({k: v for k, v in meta.items() if k not in ("keys", "shapes", "parameter_names", "second", "init_state_keys")}))


if __name__ == "__main__":
    main()
