#!/usr/bin/env python3
"""Golden fixture of BERT4Rec, generated from the REAL reference class.

Builds ``SeqRec.models.discriminative.BERT4Rec.model.BERT4Rec`` (ref:SeqRec/models/discriminative/BERT4Rec/model.py) at a small
config (hidden 64, 2 heads, 2 layers) with more than 8191 items, loads the seeded weights of
``tests/helpers/bert4rec_weights.py`` (pinned by fp64 checksums; ``head.bias`` non-zero), and records with dropout off:
  * ``(masked_item_seq, labels)`` of the real ``reconstruct_train_data`` under a torch seed, chosen as the first seed from
    MASK_SEED on whose draw holds a fine-tuning row of full length (last item masked, with a label), a fine-tuning row shorter
    than the batch (mask token appended, no label) and a cloze row with a label; the rows include lengths 1 and MAX_LEN;
  * ``forward``'s logits on sampled columns, its labels, the loss of ``loss_fct`` on them;
  * every parameter's gradient; the item table's only as checksums plus sampled rows (row 0, the labels' rows and <MASK> among
    them); ``output_bias`` gets none;
  * ``full_sort_predict`` on evaluation rows (ending with the mask token) on sampled columns and the stable argsort's first 10,
    without and with an ``item_range`` (which BERT4Rec ignores);
  * the state-dict keys and shapes, the aliasing of the two table keys, the seeded initialisation's checksums;
  * the IndexError of a batch narrower than ``max_seq_length`` and the M = 0 behaviour (NaN loss, all-zero gradients).

Usage:  python tools/make_golden_bert4rec.py      (needs the reference checkout; CPU only)
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
import bert4rec_weights as bw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bert4rec_small.npz")
CFG = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=128, dropout_prob=0.0, hidden_act="gelu", layer_norm_eps=1e-12,
           initializer_range=0.02, mask_ratio=0.3, ft_ratio=0.5, loss_type="CE")
N_ITEMS, MAX_LEN, SEED, WSEED, MASK_SEED, INIT_SEED = 9000, 8, 5, 7, 11, 3
LENS = [8, 1, 5, 3, 8, 2, 8, 8, 6, 8]
B = len(LENS)
INIT_N_ITEMS, INIT_MAX_LEN = 50, 8


def reference_bert4rec():
    _ref_loader._install_shims()
    ref = _ref_loader.REF_ROOT
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.discriminative"):
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from SeqRec.models.discriminative.BERT4Rec.config import BERT4RecConfig
    from SeqRec.models.discriminative.BERT4Rec.model import BERT4Rec
    return BERT4Rec, BERT4RecConfig


def main():
    BERT4Rec, BERT4RecConfig = reference_bert4rec()
    fx = {}
    # seeded initialisation
    torch.manual_seed(INIT_SEED)
    init = BERT4Rec(BERT4RecConfig(**CFG), INIT_N_ITEMS, INIT_MAX_LEN)
    fx["init_checksums"] = bw.checksums(init.state_dict())
    unknown_ok = BERT4RecConfig(foo=1, **CFG)
    # the model under test
    torch.manual_seed(0)
    model = BERT4Rec(BERT4RecConfig(**CFG), N_ITEMS, MAX_LEN)
    state = model.state_dict()
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in state.items())
    alias = state["item_embedding.weight"].data_ptr() == state["head.token_embeddings.weight"].data_ptr()
    sd = bw.init_state_dict(shapes, WSEED)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(SEED)
    inputs = torch.zeros(B, MAX_LEN, dtype=torch.long)
    for b, n in enumerate(LENS):
        inputs[b, :n] = torch.randint(1, N_ITEMS + 1, (n,), generator=g)
    seq_len = torch.tensor(LENS, dtype=torch.long)
    model.train()
    mask_seed = MASK_SEED
    while True:
        torch.manual_seed(mask_seed)
        masked, labels = model.reconstruct_train_data(inputs, seq_len)
        appended = (masked == N_ITEMS + 1) & (inputs == 0)
        ft_full = [b for b in range(B) if LENS[b] == MAX_LEN and (masked[b] == N_ITEMS + 1).sum() == 1 and labels[b, -1] != 0]
        cloze = [b for b in range(B) if not appended[b].any() and (labels[b] != 0).any() and b not in ft_full]
        if appended.any() and ft_full and cloze:
            break
        mask_seed += 1
    logits, valid_labels = model.forward(masked, labels)
    model.zero_grad()
    loss = model.loss_fct(logits, valid_labels)
    loss.backward()
    named = dict(model.named_parameters())
    grads = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    no_grad = [k for k, p in named.items() if p.grad is None]
    # evaluation rows: the history cut to MAX_LEN - 1 items plus the mask token
    ev = torch.zeros(B, MAX_LEN, dtype=torch.long)
    ev_len = []
    for b, n in enumerate(LENS):
        n = min(n, MAX_LEN - 1)
        ev[b, :n] = inputs[b, :n]
        ev[b, n] = N_ITEMS + 1
        ev_len.append(n + 1)
    ev_len = torch.tensor(ev_len, dtype=torch.long)
    model.eval()
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inputs=ev, seq_len=ev_len))
        scores_r = model.full_sort_predict(dict(inputs=ev, seq_len=ev_len, item_range=(3001, 6001)))
    # observations
    model.train()
    try:
        model.reconstruct_train_data(inputs[1:4, :5], seq_len[1:4])
        index_error = ""
    except IndexError as e:
        index_error = str(e)
    model.mask_ratio, model.ft_ratio = 0.0, 0.0
    model.zero_grad()
    m0 = model.calculate_loss(dict(inputs=inputs, seq_len=seq_len))
    m0.backward()
    m0_zero = all(bool((p.grad == 0).all()) for k, p in model.named_parameters() if p.grad is not None)
    m0_none = [k for k, p in model.named_parameters() if p.grad is None]

    rows = sorted(set([0, 1, 2, N_ITEMS, N_ITEMS + 1]) | set(inputs.flatten().tolist()) | set(valid_labels.tolist()))
    cols = sorted(set(torch.randint(0, N_ITEMS + 1, (64,), generator=g).tolist()) | {0, 1, N_ITEMS} | set(valid_labels.tolist()))
    fx.update({"inputs": inputs.numpy(), "seq_len": seq_len.numpy(), "masked": masked.numpy(), "labels": labels.numpy(),
               "valid_labels": valid_labels.numpy(), "logits_cols": logits.detach()[:, cols].numpy(),
               "loss": np.asarray(float(loss)), "weight_checksums": bw.checksums(sd), "rows": np.asarray(rows),
               "cols": np.asarray(cols), "eval_inputs": ev.numpy(), "eval_seq_len": ev_len.numpy(),
               "scores_cols": scores[:, cols].numpy(), "scores_equal_with_item_range": np.asarray(bool(torch.equal(scores, scores_r))),
               "top10": torch.argsort(-scores, dim=1, stable=True)[:, :10].numpy()})
    for k, gr in grads.items():
        if k == "item_embedding.weight":
            fx["grad_item_rows"] = gr[rows].numpy()
            fx["grad_item_checksum"] = bw.checksums({k: gr})[0]
        else:
            fx["grad/" + k] = gr.numpy()
    meta = dict(config=CFG, n_items=N_ITEMS, max_his_len=MAX_LEN, weight_seed=WSEED, mask_seed=mask_seed, init_seed=INIT_SEED,
                init_n_items=INIT_N_ITEMS, init_max_his_len=INIT_MAX_LEN, keys=list(shapes), shapes=[list(s) for s in shapes.values()],
                table_keys_alias=bool(alias), parameter_names=list(named), no_grad=no_grad, index_error=index_error,
                unknown_key_dropped=not hasattr(unknown_ok, "foo"), m0_loss_is_nan=bool(torch.isnan(m0)),
                m0_grads_all_zero=bool(m0_zero), m0_no_grad=m0_none, ft_full_rows=ft_full, cloze_rows=cloze,
                appended_rows=sorted(set(appended.nonzero()[:, 0].tolist())),
                head_bias_grad_nonzero=int((grads["head.bias"] != 0).sum()))
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), loss {float(loss):.6f}, M {valid_labels.numel()}, mask seed {mask_seed}")
    print(json.dumps({k: v for k, v in meta.items() if k not in ("keys", "shapes", "parameter_names")}))


if __name__ == "__main__":
    main()
