#!/usr/bin/env python3
"""Golden fixture of TIGER at encoder lengths above 128, generated from the REAL reference class as tools/make_golden_tiger.py does
(whose loader, weight seeding, item set and plain beam search are imported).  With dropout off and temperature 0.7 it records:
  * config C (d_model 64, 2 heads of 64, 2 + 2 layers, d_ff 128, vocab 120): four rows of encoder lengths 300, 129, 512 and 1,
    right-padded to 512, labels of 3 - 5 tokens; config D (6 heads of 32, d_ff 256, vocab 300): two rows of lengths 257 and 200;
  * logits, loss and every parameter gradient, large ones as evenly spaced rows plus fp64 checksums (tiger_weights.sample_rows);
  * config C's ``generate`` beams at 4 and 20 beams on the first three rows over the 40-item trie; the weight seed is redrawn
    until the 2 k best scores of every step differ by more than 1e-4 and the plain beam search finds HF's beams;
  * the bucket function's output for both directions at length 512.
Only data goes into the fixture.

Usage:  python tools/make_golden_tiger_long.py      (needs the reference checkout; CPU only)
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_tiger as base  # noqa: E402
from make_golden_tiger import tw  # noqa: E402

OUT = os.path.join(base.ROOT, "tests", "golden", "tiger_long.npz")
CONFIGS = {"c": base.CONFIGS["a"], "d": dict(base.CONFIGS["b"], d_kv=32)}
ENC_LENS = {"c": [300, 129, 512, 1], "d": [257, 200]}
LABEL_LENS = {"c": [5, 3, 4, 5], "d": [5, 4]}
BUCKET_LEN = 512


def build(TIGER, T5Config, name, wseed):
    model = TIGER(T5Config(**CONFIGS[name]))
    if not hasattr(model, "model_parallel"):
        model.model_parallel = False
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    sd = tw.init_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    model.set_hyper(base.TEMPERATURE)
    return model, shapes, sd


def batch(name, seed):
    g = torch.Generator().manual_seed(seed)
    V = CONFIGS[name]["vocab_size"]
    lens, llens = ENC_LENS[name], LABEL_LENS[name]
    ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
    labels = torch.full((len(lens), max(llens)), -100, dtype=torch.long)
    for r, (n, m) in enumerate(zip(lens, llens)):
        ids[r, :n - 1] = torch.randint(2, V, (n - 1,), generator=g)
        ids[r, n - 1] = 1                                            # every row ends with </s>
        labels[r, :m - 1] = torch.randint(2, V, (m - 1,), generator=g)
        labels[r, m - 1] = 1
    return ids, (ids != 0).long(), labels


def beams(model, Trie, prefix_allowed_tokens_fn, ids, am):
    seqs = [[0] + it + [1] for it in base.items()]
    fn = prefix_allowed_tokens_fn(Trie(seqs))
    prefix = torch.zeros(ids.shape[0], 1, dtype=torch.long)
    out, gap = {"trie_plain": np.asarray(seqs)}, float("inf")
    for nb in (4, 20):
        with torch.no_grad():
            o = model.generate(input_ids=ids, attention_mask=am, decoder_input_ids=prefix, max_new_tokens=10, prefix_allowed_tokens_fn=fn,
                               num_beams=nb, num_return_sequences=nb, output_scores=True, return_dict_in_generate=True,
                               early_stopping=True)
        s, sc, g_ = base.plain_beam_search(model, ids, am, prefix, fn, nb, base.ITEM_LEN + 1)
        if not torch.equal(s, o.sequences) or float((sc - o.sequences_scores).abs().max()) > 1e-5:
            raise RuntimeError(f"the plain beam search does not find generate's beams ({nb} beams)")
        gap = min(gap, g_)
        out[f"beams_plain_{nb}"] = o.sequences.numpy()
        out[f"scores_plain_{nb}"] = o.sequences_scores.numpy()
    return out, gap


def main():
    TIGER, T5Config, T5Attention, Trie, prefix_allowed_tokens_fn = base.reference_tiger()
    fx, meta = {}, dict(configs=CONFIGS, temperature=base.TEMPERATURE, item_len=base.ITEM_LEN, gap=base.GAP, enc_lens=ENC_LENS)
    for name in CONFIGS:
        wseed = 21 if name == "c" else 22
        while True:
            torch.manual_seed(0)
            model, shapes, sd = build(TIGER, T5Config, name, wseed)
            model.eval()
            ids, am, labels = batch(name, 5)
            if name != "c":
                break
            bm, gap = beams(model, Trie, prefix_allowed_tokens_fn, ids[:3], am[:3])
            if gap > base.GAP:
                break
            print(f"weight seed {wseed}: smallest gap {gap:.2e} <= {base.GAP}, redrawing")
            wseed += 100
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=am, labels=labels)
        out.loss.backward()
        fx.update({f"{name}/input_ids": ids.numpy().astype(np.int16), f"{name}/attention_mask": am.numpy().astype(np.int8),
                   f"{name}/labels": labels.numpy(), f"{name}/logits": out.logits.detach().numpy(), f"{name}/loss": np.asarray(float(out.loss)),
                   f"{name}/weight_checksums": tw.checksums(sd)})
        none = []
        for k, p in model.named_parameters():
            if p.grad is None:
                none.append(k)
            else:
                g = p.grad.detach()
                fx[f"{name}/grad/{k}"] = g[tw.sample_rows(g.shape)].numpy()
                fx[f"{name}/grad_checksum/{k}"] = tw.checksums({k: g})[0]
        meta[name] = dict(weight_seed=wseed, keys=list(shapes), shapes=[list(s) for s in shapes.values()], no_grad=none,
                          param_keys=[k for k, _ in model.named_parameters()])
        if name == "c":
            fx.update({f"c/{k}": v for k, v in bm.items()})
            meta["c"]["smallest_gap"] = gap
    S = BUCKET_LEN
    rp = torch.arange(S)[None, :] - torch.arange(S)[:, None]
    for bid in (True, False):
        full = T5Attention._relative_position_bucket(rp, bidirectional=bid, num_buckets=32, max_distance=128)
        fx[f"bucket/{'bi' if bid else 'uni'}/{S}"] = torch.cat([full[S - 1, :S - 1], full[0, :]]).numpy().astype(np.int32)
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
