#!/usr/bin/env python3
"""Golden fixture of TIGER, generated from the REAL reference class.

Builds ``SeqRec.models.generative.TIGER.model.TIGER`` (ref:SeqRec/models/generative/TIGER/model.py, HF's
T5ForConditionalGeneration with a temperature) at two small configs, loads the seeded weights of
``tests/helpers/tiger_weights.py`` (pinned by fp64 checksums) and records, with dropout off:
  * config A (d_model 64, 2 heads of 64, 2 + 2 layers, d_ff 128, vocab 120): 5 rows of ragged encoder length up to 23, labels
    of 3 - 5 tokens padded with -100, temperature 0.7; config B (6 heads, d_ff 256, vocab 300): 3 rows of encoder length 101, so
    that the offsets pass the exact buckets and the logarithmic ones;
  * HF's state-dict key list and shapes, logits, loss and every parameter gradient (both bias tables and the shared table); a
    gradient of more than 2048 values is stored as evenly spaced rows (tiger_weights.sample_rows) plus fp64 checksums of the whole
    tensor, which keeps the file below 1 MiB;
  * config A's ``generate`` beams (sequences and sequences_scores) at 4 and 20 beams, without a decoder prefix (the
    test_decoder.py call: the trie holds [start] + item + </s>) and with one (the test_SMB_decoder.py call: [start, behaviour] +
    item, max_new_tokens = 4), on rows of different padding over a trie of 40 items.  A plain restatement of the beam search on
    the same model checks that the 2 k best scores of every step differ by more than 1e-4 (no tie can decide a beam) and that it
    finds HF's beams; the weight seed is redrawn until that holds;
  * the bucket function's output for both directions at lengths 1, 8, 101, 128 and 300;
  * ``train_decoder``'s parser defaults.
Only data goes into the fixture.

Usage:  python tools/make_golden_tiger.py      (needs the reference checkout; CPU only)
"""
import argparse
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
import tiger_weights as tw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tiger_small.npz")
BASE = dict(d_kv=64, num_layers=2, num_decoder_layers=2, relative_attention_num_buckets=32, relative_attention_max_distance=128,
            dropout_rate=0.0, layer_norm_epsilon=1e-6, initializer_factor=1.0, feed_forward_proj="relu", tie_word_embeddings=True,
            pad_token_id=0, eos_token_id=1, decoder_start_token_id=0)
CONFIGS = {
    "a": dict(BASE, d_model=64, num_heads=2, d_ff=128, vocab_size=120),
    "b": dict(BASE, d_model=64, num_heads=6, d_ff=256, vocab_size=300),
}
TEMPERATURE = 0.7
ENC_LENS = {"a": [23, 9, 17, 1, 12], "b": [101, 101, 101]}
LABEL_LENS = {"a": [5, 3, 4, 5, 3], "b": [5, 4, 5]}
N_ITEMS, ITEM_LEN, BEHAVIOURS = 40, 4, (5, 6)
BUCKET_LENS = (1, 8, 101, 128, 300)
GAP = 1e-4


def _packages(*names):
    ref = _ref_loader.REF_ROOT
    for parent in names:
        if parent not in sys.modules:
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(ref, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg


def reference_tiger():
    _ref_loader._install_shims()
    _packages("SeqRec", "SeqRec.models", "SeqRec.models.generative", "SeqRec.models.generative.TIGER", "SeqRec.generation")
    from transformers import T5Config
    import transformers.models.t5.modeling_t5 as mt5
    from transformers.models.t5.modeling_t5 import T5Attention
    if not hasattr(mt5, "__HEAD_MASK_WARNING_MSG"):                    # (a name the reference imports, removed from transformers 5.x)
        setattr(mt5, "__HEAD_MASK_WARNING_MSG", "")
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn
    from SeqRec.models.generative.TIGER.model import TIGER
    return TIGER, T5Config, T5Attention, Trie, prefix_allowed_tokens_fn


def task_defaults():
    _packages("SeqRec.tasks", "SeqRec.datasets", "SeqRec.utils")
    from SeqRec.tasks.train_decoder import TrainDecoder
    parser = argparse.ArgumentParser()
    TrainDecoder.add_sub_parsers(parser.add_subparsers())
    return vars(parser.parse_args(["train_decoder"]))


def build(TIGER, T5Config, name, wseed):
    model = TIGER(T5Config(**CONFIGS[name]))
    if not hasattr(model, "model_parallel"):                           # (read by the reference's forward; gone from transformers 5.x)
        model.model_parallel = False
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    sd = tw.init_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    model.set_hyper(TEMPERATURE)
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


def items():
    """40 items of 4 tokens: 20 distinct first tokens (so that 20 beams are all live after the first step)"""
    g = torch.Generator().manual_seed(3)
    seen, out = set(), []
    while len(out) < N_ITEMS:
        it = [10 + len(out) % 20] + [30 + 22 * c + int(torch.randint(0, 22, (1,), generator=g)) for c in range(1, ITEM_LEN)]
        if tuple(it) not in seen:
            seen.add(tuple(it))
            out.append(it)
    return out


def plain_beam_search(model, ids, am, prefix, allowed, nb, steps):
    """the beam search of decode.beam_search on the reference model; returns (sequences, scores, smallest gap among the finite
    2 nb best of any step)"""
    B = ids.shape[0]
    seqs = prefix[:, None, :].expand(B, nb, prefix.shape[1]).clone()
    run = torch.zeros(B, nb)
    run[:, 1:] = -1e9
    gap = float("inf")
    for step in range(steps):
        cur = seqs.shape[2]
        flat = seqs.reshape(B * nb, cur)
        with torch.no_grad():
            lg = model(input_ids=ids.repeat_interleave(nb, 0), attention_mask=am.repeat_interleave(nb, 0),
                       decoder_input_ids=flat).logits[:, -1]
        lp = torch.log_softmax(lg, -1)
        mask = torch.full_like(lp, float("-inf"))
        for n in range(B * nb):
            mask[n, allowed(n // nb, flat[n])] = 0.0
        sc = (lp + mask + run.reshape(-1, 1)).view(B, -1)
        top_s, top_i = torch.topk(sc, 2 * nb)
        V = lp.shape[1]
        for b in range(B):
            live = top_s[b][top_s[b] > -1e8]
            if live.numel() > 1:
                gap = min(gap, float((live[:-1] - live[1:]).min()))
        beam_i, tok = top_i // V, top_i % V
        cand = torch.cat([torch.gather(seqs, 1, beam_i[:, :, None].expand(B, 2 * nb, cur)), tok[:, :, None]], 2)
        seqs, run = cand[:, :nb].contiguous(), top_s[:, :nb].contiguous()
    return seqs.reshape(B * nb, -1), (run / steps).reshape(-1), gap


def beams(model, Trie, prefix_allowed_tokens_fn, ids, am):
    its = items()
    out = {}
    gap = float("inf")
    B = ids.shape[0]
    beh = torch.tensor([BEHAVIOURS[r % 2] for r in range(B)])
    for tag, seqs, prefix, steps, hf_new in (
            ("plain", [[0] + it + [1] for it in its], torch.zeros(B, 1, dtype=torch.long), ITEM_LEN + 1, 10),
            ("prefix", [[0, bt] + it for bt in BEHAVIOURS for it in its], torch.stack([torch.zeros(B, dtype=torch.long), beh], 1),
             ITEM_LEN, ITEM_LEN)):
        fn = prefix_allowed_tokens_fn(Trie(seqs))
        out[f"trie_{tag}"] = np.asarray(seqs)
        out[f"prefix_{tag}"] = prefix.numpy()
        for nb in (4, 20):
            with torch.no_grad():
                o = model.generate(input_ids=ids, attention_mask=am, decoder_input_ids=prefix, max_new_tokens=hf_new,
                                   prefix_allowed_tokens_fn=fn, num_beams=nb, num_return_sequences=nb, output_scores=True,
                                   return_dict_in_generate=True, early_stopping=True)
            s, sc, g_ = plain_beam_search(model, ids, am, prefix, fn, nb, steps)
            if not torch.equal(s, o.sequences) or float((sc - o.sequences_scores).abs().max()) > 1e-5:
                raise RuntimeError(f"the plain beam search does not find generate's beams ({tag}, {nb} beams)")
            gap = min(gap, g_)
            out[f"beams_{tag}_{nb}"] = o.sequences.numpy()
            out[f"scores_{tag}_{nb}"] = o.sequences_scores.numpy()
    return out, gap


def main():
    TIGER, T5Config, T5Attention, Trie, prefix_allowed_tokens_fn = reference_tiger()
    fx, meta = {}, dict(configs=CONFIGS, temperature=TEMPERATURE, behaviours=list(BEHAVIOURS), item_len=ITEM_LEN, gap=GAP)
    for name in CONFIGS:
        wseed = 11 if name == "a" else 12
        while True:
            torch.manual_seed(0)
            model, shapes, sd = build(TIGER, T5Config, name, wseed)
            model.eval()
            ids, am, labels = batch(name, 5)
            if name != "a":
                break
            bm, gap = beams(model, Trie, prefix_allowed_tokens_fn, ids[:3], am[:3])
            if gap > GAP:
                break
            print(f"weight seed {wseed}: smallest gap {gap:.2e} <= {GAP}, redrawing")
            wseed += 100
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=am, labels=labels)
        out.loss.backward()
        fx.update({f"{name}/input_ids": ids.numpy(), f"{name}/attention_mask": am.numpy(), f"{name}/labels": labels.numpy(),
                   f"{name}/logits": out.logits.detach().numpy(), f"{name}/loss": np.asarray(float(out.loss)),
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
        if name == "a":
            fx.update({f"a/{k}": v for k, v in bm.items()})
            meta["a"]["smallest_gap"] = gap
    for S in BUCKET_LENS:
        rp = torch.arange(S)[None, :] - torch.arange(S)[:, None]
        for bid in (True, False):
            full = T5Attention._relative_position_bucket(rp, bidirectional=bid, num_buckets=32, max_distance=128)
            # the bucket depends on j - i only: row S - 1 holds the offsets -(S - 1) .. 0, row 0 the offsets 0 .. S - 1
            vec = torch.cat([full[S - 1, :S - 1], full[0, :]])
            fx[f"bucket/{'bi' if bid else 'uni'}/{S}"] = vec.numpy().astype(np.int32)
    cfg = T5Config.from_pretrained(os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "TIGER"))
    meta["shipped_config"] = {k: getattr(cfg, k) for k in ("d_model", "d_kv", "d_ff", "num_layers", "num_decoder_layers", "num_heads",
                                                           "relative_attention_num_buckets", "relative_attention_max_distance",
                                                           "dropout_rate", "layer_norm_epsilon", "initializer_factor", "feed_forward_proj",
                                                           "tie_word_embeddings", "vocab_size", "pad_token_id", "eos_token_id",
                                                           "decoder_start_token_id")}
    meta["train_decoder_defaults"] = {k: v for k, v in task_defaults().items() if isinstance(v, (int, float, str, bool, type(None)))}
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
