#!/usr/bin/env python3
"""Golden fixture of PBATransformer, generated from the REAL reference classes.

Builds ``SeqRec.models.generative.PBATransformer.PBATransformerForConditionalGeneration`` (ref:SeqRec/models/generative/
PBATransformer/model.py) at small configs (vocab 64, d_model 64, d_kv 64, 2 heads, d_ff 96, behaviour dim 16, num_positions 4,
2 behaviours, 2 + 2 layers, temperature 0.7, eval mode, dropout off), loads the seeded weights of
``tests/helpers/pbatransformer_weights.py`` (pinned by fp64 checksums) and records
  a     encoder sparse in layer 1, injection in layers 0 and 1; decoder sparse in both layers, injection in layer 0; 3 rows of
        3, 2 and 1 items (13 tokens, right-padded): loss, logits, the outputs of both routers, every parameter gradient (tensors
        of more than 768 values as evenly spaced rows plus fp64 checksums of the whole tensor, as tiger_small.npz), weight checksums
  b     the same with Moe_behavior_only=True (two experts; the reference routes the item tokens to position 2, which no expert
        owns: they get a zero feed-forward output, and so they do here)
  c     use_behavior_token=False: no injection, ids without behaviour tokens
  long  33 items, 133 tokens, 2 rows (the key-streaming attention under the routed FFN): loss and logits only
  gen   from a's weights: ``generate(num_beams=3, num_return_sequences=3, max_new_tokens=5, use_cache=False)`` for 2 users under
        a trie whose second token is always a mapped behaviour token; sequences and sequences_scores.  A plain restatement of the
        beam search on the same model finds the same beams and measures, at every step and user, the gap between the last kept
        and the first dropped candidate score relative to the score's magnitude; the weight seed is redrawn until the smallest
        gap exceeds 1e-3, so that the beam test is not decided by rounding.

The reference classes do not run as they are under transformers 5.x.  The reference is never edited; this tool, at run time,
  1. stubs ``loguru`` and bypasses the package ``__init__`` files (as make_golden_tiger does),
  2. sets ``PBATransformerForConditionalGeneration._tied_weights_keys`` to the mapping {"encoder.embed_tokens.weight":
     "shared.weight", "decoder.embed_tokens.weight": "shared.weight", "lm_head.weight": "shared.weight"},
  3. gives ``PBATransformerStack`` a ``get_head_mask`` that returns ``[None] * n``,
  4. calls the model with ``use_cache=False`` (the cached path needs EncoderDecoderCache.from_legacy_cache, which is gone),
  5. passes ``generate`` a ``prefix_allowed_tokens_fn`` from a trie whose second token is always a mapped behaviour token (free
     generation indexes ``behavior_embedding`` out of range).
  6. wraps the ``forward`` of the installed SwitchTransformersLayerSelfAttention / SwitchTransformersLayerCrossAttention so that they
     return what the reference's block unpacks, the layout of the transformers 4.51 it pins: (hidden, present key / values,
     position bias[, attention weights]).  The installed 5.x layers return (hidden, position bias, attention weights); unwrapped,
     the reference's stack reads the attention weights (None) as block 0's position bias and every later block runs without
     the relative bias - it runs, but it is not the model.  With the wrapper block 0's bias is shared by the stack, as under 4.51.
The shims are recorded in the fixture's ``meta_json``.  tests/helpers/pbatransformer_ref.py, an independent restatement of the
model, agrees with the recorded numbers to the rounding of the reference's fp32 arithmetic (tests/test_pbatransformer.py).  Only
data goes into the fixture.

Usage:  python tools/make_golden_pbatransformer.py      (needs the reference checkout; CPU only)
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import _ref_loader  # noqa: E402
import pbatransformer_weights as pw  # noqa: E402
from make_golden_tiger import _packages  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pbatransformer_small.npz")
P, BEH, NPOS = 4, (10, 11), 50
BASE = dict(vocab_size=64, d_model=64, d_kv=64, num_heads=2, d_ff=96, num_layers=2, num_decoder_layers=2,
            relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0, layer_norm_epsilon=1e-6,
            initializer_factor=1.0, feed_forward_proj="relu", dense_act_fn="relu", tie_word_embeddings=True, pad_token_id=0,
            eos_token_id=1, decoder_start_token_id=0, behavior_injection=True, behavior_embedding_dim=16, num_positions=P,
            num_behavior=len(BEH), n_positions=NPOS, sparse_layers_encoder=[1], sparse_layers_decoder=[0, 1],
            behavior_injection_encoder=[0, 1], behavior_injection_decoder=[0], Moe_behavior_only=False, shared_expert=False,
            use_behavior_token=True, behavior_maps={str(t): i for i, t in enumerate(BEH)}, use_user_token=False)
CONFIGS = {
    "a": dict(BASE),
    "b": dict(BASE, Moe_behavior_only=True),
    "c": dict(BASE, use_behavior_token=False, behavior_injection=False, behavior_injection_encoder=[], behavior_injection_decoder=[]),
}
CONFIGS["long"] = CONFIGS["a"]
ITEMS = {"a": [3, 2, 1], "b": [3, 2, 1], "c": [3, 2, 1], "long": [33, 33]}
TEMPERATURE = 0.7
GAP = 1e-3
NB, NEW = 3, 5
SHIMS = ["loguru stubbed, package __init__ files bypassed",
         "PBATransformerForConditionalGeneration._tied_weights_keys set to the {tied key: 'shared.weight'} mapping",
         "PBATransformerStack.get_head_mask returns [None] * n",
         "every call with use_cache=False",
         "generate under a prefix_allowed_tokens_fn whose second token is always a mapped behaviour token",
         "the installed Switch attention layers' forward wrapped to return transformers 4.51's (hidden, present, position bias[, weights])"]


def reference():
    _ref_loader._install_shims()
    _packages("SeqRec", "SeqRec.models", "SeqRec.models.generative", "SeqRec.models.generative.PBATransformer", "SeqRec.generation")
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn
    from SeqRec.models.generative.PBATransformer.configuration import PBATransformerConfig
    from SeqRec.models.generative.PBATransformer.model import PBATransformerForConditionalGeneration, PBATransformerStack
    tied = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight")
    PBATransformerForConditionalGeneration._tied_weights_keys = {k: "shared.weight" for k in tied}
    PBATransformerStack.get_head_mask = lambda self, head_mask, n, *a, **k: [None] * n
    import transformers.models.switch_transformers.modeling_switch_transformers as mst
    for cls in (mst.SwitchTransformersLayerSelfAttention, mst.SwitchTransformersLayerCrossAttention):
        if not getattr(cls, "_legacy_outputs", False):
            def forward(self, *a, _orig=cls.forward, output_attentions=False, **k):
                for legacy in ("layer_head_mask", "past_key_value", "use_cache", "query_length"):
                    k.pop(legacy, None)
                out, position_bias, weights = _orig(self, *a, **k)
                return (out, None, position_bias) + ((weights,) if output_attentions else ())
            cls.forward, cls._legacy_outputs = forward, True
    return PBATransformerForConditionalGeneration, PBATransformerConfig, Trie, prefix_allowed_tokens_fn


def build(Model, Config, name, wseed):
    model = Model(Config(**CONFIGS[name]))
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
    sd = pw.init_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    model.set_hyper(TEMPERATURE)
    return model.eval(), shapes, sd


def item(g, behaviour_token):
    sem = [int(torch.randint(20, 64, (1,), generator=g)) for _ in range(P - (behaviour_token is not None))]
    return ([behaviour_token] if behaviour_token is not None else []) + sem


def batch(name, seed):
    """ids [B, S] right-padded rows of items + </s>, their mask, labels [B, P + 1] = one item + </s>"""
    g = torch.Generator().manual_seed(seed)
    beh = CONFIGS[name]["use_behavior_token"]
    counts = ITEMS[name]
    S = max(counts) * P + 1
    ids = torch.zeros(len(counts), S, dtype=torch.long)
    labels = torch.zeros(len(counts), P + 1, dtype=torch.long)
    for r, n in enumerate(counts):
        row = []
        for i in range(n):
            row += item(g, BEH[(r + i) % 2] if beh else None)
        ids[r, :len(row) + 1] = torch.tensor(row + [1])
        labels[r] = torch.tensor(item(g, BEH[(r + 1) % 2] if beh else None) + [1])
    return ids, (ids != 0).long(), labels


def trie_sequences():
    """[start, behaviour, three semantic tokens, </s>]: 12 items under each behaviour, several sharing their first tokens"""
    g = torch.Generator().manual_seed(9)
    seen = []
    while len(seen) < 12:
        it = [20 + len(seen) % 4, 30 + int(torch.randint(0, 3, (1,), generator=g)), 40 + int(torch.randint(0, 20, (1,), generator=g))]
        if it not in seen:
            seen.append(it)
    return [[0, b] + it + [1] for b in BEH for it in seen]


def plain_beam_search(model, ids, am, allowed, nb, steps):
    """the beam search of gamer_amd.tiger.beam_search on the reference model (use_cache=False: every hypothesis is routed by its
    own tokens); returns (sequences, scores, smallest relative gap between the last kept and the first dropped candidate)"""
    B = ids.shape[0]
    seqs = torch.zeros(B, nb, 1, dtype=torch.long)
    run = torch.zeros(B, nb)
    run[:, 1:] = -1e9
    gap = float("inf")
    for step in range(steps):
        cur = seqs.shape[2]
        flat = seqs.reshape(B * nb, cur)
        with torch.no_grad():
            lg = model(input_ids=ids.repeat_interleave(nb, 0), attention_mask=am.repeat_interleave(nb, 0), decoder_input_ids=flat,
                       use_cache=False).logits[:, -1]
        lp = torch.log_softmax(lg, -1)
        mask = torch.full_like(lp, float("-inf"))
        for n in range(B * nb):
            mask[n, allowed(n // nb, flat[n])] = 0.0
        sc = (lp + mask + run.reshape(-1, 1)).view(B, -1)
        top_s, top_i = torch.topk(sc, 2 * nb)
        V = lp.shape[1]
        for b in range(B):
            kept, dropped = float(top_s[b, nb - 1]), float(top_s[b, nb])
            if kept > -1e8 and dropped > -1e8:
                gap = min(gap, (kept - dropped) / max(abs(kept), abs(dropped)))
            live = top_s[b, :nb][top_s[b, :nb] > -1e8]
            if live.numel() > 1:                                       # the order among the kept ones decides the rows' order
                gap = min(gap, float(((live[:-1] - live[1:]) / live[1:].abs()).min()))
        beam_i, tok = top_i // V, top_i % V
        cand = torch.cat([torch.gather(seqs, 1, beam_i[:, :, None].expand(B, 2 * nb, cur)), tok[:, :, None]], 2)
        seqs, run = cand[:, :nb].contiguous(), top_s[:, :nb].contiguous()
    return seqs.reshape(B * nb, -1), (run / steps).reshape(-1), gap


def beams(model, Trie, prefix_allowed_tokens_fn, ids, am):
    seqs = trie_sequences()
    fn = prefix_allowed_tokens_fn(Trie(seqs))
    with torch.no_grad():
        o = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=NEW, prefix_allowed_tokens_fn=fn, num_beams=NB,
                           num_return_sequences=NB, output_scores=True, return_dict_in_generate=True, early_stopping=True,
                           use_cache=False, do_sample=False)
    s, sc, gap = plain_beam_search(model, ids, am, fn, NB, NEW)
    if not torch.equal(s, o.sequences) or float((sc - o.sequences_scores).abs().max()) > 1e-5:
        raise RuntimeError("the plain beam search does not find generate's beams")
    return {"gen/trie": np.asarray(seqs), "gen/sequences": o.sequences.numpy(), "gen/sequences_scores": o.sequences_scores.numpy(),
            "gen/input_ids": ids.numpy(), "gen/attention_mask": am.numpy()}, gap


def main():
    Model, Config, Trie, prefix_allowed_tokens_fn = reference()
    fx, meta = {}, dict(configs=CONFIGS, temperature=TEMPERATURE, behaviour_tokens=list(BEH), num_positions=P, gap=GAP, shims=SHIMS,
                        num_beams=NB, max_new_tokens=NEW)
    seeds = {"a": 21, "b": 22, "c": 23}
    for name in ("a", "b", "c", "long"):
        wseed = seeds.get(name, None)
        if name == "long":
            wseed = meta["a"]["weight_seed"]
        while True:
            torch.manual_seed(0)
            model, shapes, sd = build(Model, Config, name, wseed)
            ids, am, labels = batch(name, 5)
            if name != "a":
                break
            bm, gap = beams(model, Trie, prefix_allowed_tokens_fn, ids[:2], am[:2])
            if gap > GAP:
                break
            print(f"weight seed {wseed}: smallest gap {gap:.2e} <= {GAP}, redrawing")
            wseed += 100
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=am, labels=labels, use_cache=False)
        fx.update({f"{name}/input_ids": ids.numpy(), f"{name}/attention_mask": am.numpy(), f"{name}/labels": labels.numpy(),
                   f"{name}/logits": out.logits.detach().numpy(), f"{name}/loss": np.asarray(float(out.loss.detach()))})
        if name == "long":
            meta["long"] = dict(weight_seed=wseed, config="a")
            continue
        out.loss.backward()
        dec_in = model._shift_right(labels)
        with torch.no_grad():
            ep, eb = model.encoder.router(ids.clone())
            dp, db = model.decoder.router(dec_in.clone(), cache_position=torch.arange(dec_in.shape[1]))
        fx.update({f"{name}/router/enc_pos": ep.numpy().astype(np.int32), f"{name}/router/enc_beh": eb.numpy().astype(np.int32),
                   f"{name}/router/dec_pos": dp.numpy().astype(np.int32), f"{name}/router/dec_beh": db.numpy().astype(np.int32),
                   f"{name}/decoder_input_ids": dec_in.numpy(), f"{name}/weight_checksums": pw.checksums(sd)})
        none = []
        for k, p in model.named_parameters():
            if p.grad is None:
                none.append(k)
            else:
                g = p.grad.detach()
                fx[f"{name}/grad/{k}"] = g[pw.sample_rows(g.shape)].numpy()
                fx[f"{name}/grad_checksum/{k}"] = pw.checksums({k: g})[0]
        meta[name] = dict(weight_seed=wseed, keys=list(shapes), shapes=[list(s) for s in shapes.values()], no_grad=none,
                          param_keys=[k for k, _ in model.named_parameters()], num_experts=int(model.config.num_experts))
        if name == "a":
            fx.update(bm)
            meta["a"]["smallest_gap"] = gap
    cfg = Config.from_pretrained(os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "PBATransformer"))
    meta["shipped_config"] = {k: getattr(cfg, k) for k in (
        "d_model", "d_kv", "d_ff", "num_layers", "num_decoder_layers", "num_heads", "relative_attention_num_buckets",
        "relative_attention_max_distance", "dropout_rate", "layer_norm_epsilon", "initializer_factor", "vocab_size", "pad_token_id",
        "eos_token_id", "decoder_start_token_id", "behavior_injection", "behavior_embedding_dim", "num_positions", "num_behavior",
        "sparse_layers_encoder", "sparse_layers_decoder", "behavior_injection_encoder", "behavior_injection_decoder",
        "Moe_behavior_only", "shared_expert", "use_behavior_token", "use_user_token", "num_experts", "dense_act_fn")}
    fx["meta_json"] = np.asarray(json.dumps(meta))
    np.savez_compressed(OUT, **fx)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
