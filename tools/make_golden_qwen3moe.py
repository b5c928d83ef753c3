#!/usr/bin/env python3
"""Golden fixtures of the Qwen3Moe model, generated from the REAL reference.

Runs the reference's ``Qwen3MoeWithTemperature`` (ref:SeqRec/models/generative/Qwen3Moe/model.py) under the installed
transformers 5.x, built from ``config/s2s-models/Qwen3Moe/config.json`` with the run-time fields train_MB_decoder.py:319-362
sets, at a small size.  Weights come from ``tests/helpers/qwen3moe_weights.py`` (pinned by fp64 checksums); the reference's
state-dict key list is stored and checked against the recipe's.  Every dropout p = 0, gradients under
``sdpa_kernel(SDPBackend.MATH)``.

Importing model.py needs shims beyond ``oracle/_ref_loader.py``'s: ``QWEN3_MOE_INPUTS_DOCSTRING``, ``KwargsForCausalLM`` and
``logger`` are gone from transformers 5.x's ``modeling_qwen3_moe``, and 5.x reads ``_tied_weights_keys`` as a
{target: source} dict where the reference lists the tied head.

Generation: transformers 5.x's ``Qwen3MoeAttention.forward`` takes the cache as ``past_key_values=``; the reference's decoder
layer passes ``past_key_value=``, which lands in ``**kwargs`` and is ignored - the cache is never filled, and a cached
``generate`` would attend over the new token alone.  The decode fixture is therefore generated with ``use_cache=False``
(every step re-runs the whole sequence: routing by column, ``cache_position = arange``, RoPE positions from the attention
mask), which is what the reference computes with a working cache.

  moe_small          shipped FFN (SwiGLU experts in every layer, injection layers [0, 1]), behaviour tokens
  moe_nobeh_small    use_behavior_token = False (task "mb": no behaviour tokens, no injection), a trailing eos
  moe_pba_small      PBATransformer experts, sparse layers [0, 2], behaviour tokens
  moe_small_bf16     "moe_small" with the forward under torch.autocast("cpu", bfloat16), backward outside it
  moe_router         the reference router's (position, behaviour) indices in every routing mode, training and prompt calls
  decode_moe_small   generate() with use_cache=False on left-padded prompts (whole items of padding)
  decode_moe_behonly_small  the same with Moe_behavior_only and sparse layers [0, 2] (semantic tokens skip the sparse FFN)

Usage:  python tools/make_golden_qwen3moe.py [case ...]     (needs the reference checkout; CPU only)
"""
import contextlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeConfig  # noqa: E402
import qwen3moe_weights as mw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SMALL = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
             intermediate_size=256, moe_intermediate_size=128, behavior_embedding_dim=64, behavior_injection_decoder=[0, 1])
CB, NB = 8, 3
CASES = {
    "moe_small": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), beh=True, B=3, n_items=9,
                      pad_rows={1: 4, 2: 1}, seed=41, wseed=11),
    "moe_nobeh_small": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), beh=False, B=3, n_items=9,
                            pad_rows={1: 4, 2: 1}, seed=42, wseed=12),
    "moe_pba_small": dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2]), beh=True, B=3, n_items=9,
                          pad_rows={1: 4, 2: 1}, seed=43, wseed=13),
    "moe_small_bf16": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), beh=True, B=3, n_items=9,
                           pad_rows={1: 4, 2: 1}, seed=41, wseed=11, amp=True),
}
N_POS = 12                                   # n_positions = max_his_len + 1 of the fixtures
N_CAT, BEAMS, B_DEC, MAX_HIS, WSEED_DEC, WSCALE = 48, 6, 4, 6, 23, 4.0


def load_reference_moe():
    """(Qwen3MoeWithTemperature, transformers' Qwen3MoeConfig) of the reference, with the transformers 5.x shims."""
    _ref_loader.load_reference_classes()          # (the shared shims and the package stubs)
    import transformers.models.qwen3_moe.modeling_qwen3_moe as mm
    from transformers.modeling_flash_attention_utils import FlashAttentionKwargs
    if not hasattr(mm, "KwargsForCausalLM"):
        mm.KwargsForCausalLM = FlashAttentionKwargs
    if not hasattr(mm, "QWEN3_MOE_INPUTS_DOCSTRING"):
        mm.QWEN3_MOE_INPUTS_DOCSTRING = ""
    if not hasattr(mm, "logger"):
        from transformers.utils import logging
        mm.logger = logging.get_logger("modeling_qwen3_moe")
    model_mod = importlib.import_module("SeqRec.models.generative.Qwen3Moe.model")
    # transformers 5.x reads the tied weights as {target: source}; the reference lists them (4.x form)
    model_mod.MyQwen3MoeForCausalLM._tied_weights_keys = {"lm_head.weight": "model.embed_tokens.weight"}
    from transformers import Qwen3MoeConfig as HFConfig
    return model_mod.Qwen3MoeWithTemperature, HFConfig


def hf_config(HFConfig, beh: bool, ffn: dict, P: int):
    """config.json of Qwen3Moe + the run-time fields of train_MB_decoder.py:319-362."""
    cfg = HFConfig.from_pretrained(os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "Qwen3Moe"))
    for k, v in {**SMALL, **ffn}.items():
        setattr(cfg, k, v)
    cfg.vocab_size = synthetic.vocab_size(CB, NB)
    if beh:
        cfg.num_behavior = NB
        cfg.behavior_maps = {int(k): int(v) for k, v in synthetic.behavior_maps(CB, NB).items()}
        cfg.use_behavior_token = True
    else:
        cfg.num_behavior = 0
        cfg.behavior_maps = {}
        cfg.use_behavior_token = False
        cfg.behavior_injection = False
        cfg.behavior_injection_encoder = []
        cfg.behavior_injection_decoder = []
    cfg.num_positions = P
    cfg.num_experts = 2 if cfg.Moe_behavior_only else P + 1
    cfg.n_positions = N_POS
    cfg.use_user_token = False
    cfg.dropout_rate = 0.0
    cfg.attention_dropout = 0.0
    return cfg


def our_config(cfg) -> dict:
    d = Qwen3MoeConfig.coerce(cfg).to_dict()
    d.pop("torch_dtype", None)
    return d


def build(beh: bool, ffn: dict, wseed: int, P: int, scale: float = 1.0):
    Model, HFConfig = load_reference_moe()
    cfg = hf_config(HFConfig, beh, ffn, P)
    d = our_config(cfg)
    sd = mw.init_state_dict(d, wseed, scale)
    model = Model(cfg)
    model.set_hyper(0.7)
    ref_keys = sorted(k for k in model.state_dict() if k != "lm_head.weight")
    assert ref_keys == sorted(sd), (set(ref_keys) ^ set(sd))
    for k, v in model.state_dict().items():
        if k != "lm_head.weight":
            assert tuple(v.shape) == tuple(sd[k].shape), k
    model.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True)
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr(), "head not tied"
    return model, cfg, d, sd, ref_keys


def strip_behaviour(batch, eos_rows=(0,)):
    """An MB batch without behaviour tokens: the synthetic SMB batch with every item's behaviour column removed (4 semantic
    tokens per item), and an eos appended to ``eos_rows`` (pad elsewhere) - the eos slot of the router's table."""
    S = batch["input_ids"].shape[1]
    keep = [c for c in range(S) if c % synthetic.TOKENS_PER_ITEM]
    out = {k: batch[k][:, keep].clone() for k in ("input_ids", "attention_mask", "labels")}
    B = out["input_ids"].shape[0]
    ids = torch.full((B, 1), synthetic.PAD_ID, dtype=torch.int64)
    am = torch.zeros(B, 1, dtype=torch.int64)
    lab = torch.full((B, 1), -100, dtype=torch.int64)
    for r in eos_rows:
        last = int(out["attention_mask"][r].sum())
        if last == out["input_ids"].shape[1]:
            ids[r, 0], am[r, 0], lab[r, 0] = synthetic.EOS_ID, 1, synthetic.EOS_ID
    out["input_ids"] = torch.cat([out["input_ids"], ids], 1)
    out["attention_mask"] = torch.cat([out["attention_mask"], am], 1)
    out["labels"] = torch.cat([out["labels"], lab], 1)
    return out


def case_batch(spec):
    batch = synthetic.make_batch(spec["B"], spec["n_items"], CB, NB, seed=spec["seed"], pad_rows=spec["pad_rows"])
    if not spec["beh"]:
        batch = strip_behaviour(batch)
    return {k: batch[k] for k in ("input_ids", "attention_mask", "labels")}


def run_case(name, spec):
    P = 5 if spec["beh"] else 4
    model, cfg, d, sd, ref_keys = build(spec["beh"], spec["ffn"], spec["wseed"], P)
    batch = case_batch(spec)
    fwd_in = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"])
    amp = bool(spec.get("amp"))
    autocast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if amp else contextlib.nullcontext
    model.eval()
    with torch.no_grad(), autocast():
        S = batch["input_ids"].shape[1]
        model.model.router.cached_input_id_sequence = None
        pos, beh = model.model.router(batch["input_ids"].clone(), cache_position=torch.arange(S))
        logits_raw = model(**fwd_in, use_cache=False).logits.float().clone()
        out_l = model(**fwd_in, labels=batch["labels"], use_cache=False)
        loss_mean, logits_scaled = float(out_l.loss), out_l.logits.float().clone()
        assert out_l.aux_loss == 0 and len(out_l.router_logits) == cfg.num_hidden_layers
    model.train()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    with sdpa_kernel(SDPBackend.MATH):
        with autocast():
            out_g = model(**fwd_in, labels=batch["labels"], use_cache=False)
        out_g.loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if k != "lm_head.weight"}
    gkeys = sorted(grads)
    keys, sums = mw.fp64_checksums(sd)
    res = dict(input_ids=batch["input_ids"].numpy(), attention_mask=batch["attention_mask"].numpy(),
               labels=batch["labels"].numpy(), router_position=pos.numpy().astype(np.int16),
               router_behavior=beh.numpy().astype(np.int16),
               loss_mean=np.float64(loss_mean), loss_train_mode=np.float64(float(out_g.loss)),
               logits_raw=logits_raw.numpy(), logits_scaled=logits_scaled.numpy(),
               state_dict_keys=np.array(ref_keys), weight_keys=np.array(keys), weight_checksums=sums,
               grad_keys=np.array(gkeys), grad_norms=np.array([float(grads[k].double().norm()) for k in gkeys]),
               global_grad_norm=np.float64(float(torch.sqrt(sum((grads[k].double() ** 2).sum() for k in gkeys)))))
    for k in gkeys:
        g = grads[k]
        if g.dim() == 1:
            res["grad::" + k] = g.numpy()
        else:
            res["gradsample::" + k] = g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].numpy()
    meta = dict(name=name, config=d, codebook=CB, temperature=0.7, weight_seed=spec["wseed"], batch_seed=spec["seed"],
                autocast="bfloat16" if amp else None, model="Qwen3MoeWithTemperature",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__,
                               sdpa_backend_for_grads="MATH"))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **res)
    print(f"[{name}] loss={loss_mean:.7f} gnorm={float(res['global_grad_norm']):.6f} -> {path} "
          f"({os.path.getsize(path) / 1e6:.3f} MB)")


def run_router():
    """The reference router (router.py) in every routing mode: (behaviour token, Moe_behavior_only) in {T, F}^2, on a training
    batch with pad and eos (cache_position = arange(S), as the model calls it) and on left-padded prompts."""
    _, HFConfig = load_reference_moe()
    from SeqRec.models.generative.Qwen3Moe.router import Qwen3MoeDecoderRouter
    res = {}
    modes = []
    for beh in (True, False):
        for behonly in (False, True):
            P = 5 if beh else 4
            tag = f"beh{int(beh)}_only{int(behonly)}"
            cfg = hf_config(HFConfig, beh, dict(Moe_behavior_only=behonly, sparse_layers_decoder=[0, 1, 2, 3]), P)
            router = Qwen3MoeDecoderRouter(cfg.n_positions, cfg)
            train = synthetic.make_batch(3, 9, CB, NB, seed=50, pad_rows={1: 4, 2: 1})
            if not beh:
                train = strip_behaviour(train)
            catalogue = synthetic.make_catalogue(N_CAT, CB, seed=3)
            prompt = synthetic.make_eval_batch(4, MAX_HIS, catalogue, 1, CB, NB, seed=61)
            if not beh:
                prompt = strip_behaviour(dict(prompt, labels=prompt["input_ids"].clone()), eos_rows=())
                prompt = {k: v[:, :-1] for k, v in prompt.items()}     # (no trailing behaviour token to drop: the pad column)
            for kind, b in (("train", train), ("prompt", prompt)):
                ids = b["input_ids"]
                router.cached_input_id_sequence = None
                pos, bi = router(ids.clone(), cache_position=torch.arange(ids.shape[1]))
                res[f"{tag}_{kind}_ids"] = ids.numpy()
                res[f"{tag}_{kind}_attention_mask"] = b["attention_mask"].numpy()
                res[f"{tag}_{kind}_position"] = pos.numpy().astype(np.int16)
                res[f"{tag}_{kind}_behavior"] = bi.numpy().astype(np.int16)
            modes.append(dict(tag=tag, use_behavior_token=beh, Moe_behavior_only=behonly, num_positions=P,
                              config=our_config(cfg)))
    res["meta_json"] = np.array(json.dumps(dict(modes=modes, n_positions=N_POS, codebook=CB)))
    path = os.path.join(OUT, "moe_router.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


DECODE = {"decode_moe_small": dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]),
          "decode_moe_behonly_small": dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 2], Moe_behavior_only=True)}


def run_decode(name):
    load_reference_moe()
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn_by_last_token
    model, cfg, d, sd, ref_keys = build(True, DECODE[name], WSEED_DEC, 5, WSCALE)
    model.eval()
    model.generation_config.pad_token_id = synthetic.PAD_ID
    catalogue = synthetic.make_catalogue(N_CAT, CB, seed=3)
    all_item_tokens = [synthetic.item_tokens(catalogue, b, CB).tolist() for b in range(NB)]
    last_token_set = set(t[-1] for beh in all_item_tokens for t in beh)
    last_token_set.add(synthetic.PAD_ID)
    keys, sums = mw.fp64_checksums(sd)
    res = dict(catalogue=catalogue.numpy(), state_dict_keys=np.array(ref_keys), weight_keys=np.array(keys),
               weight_checksums=sums)
    for tb in range(NB):
        batch = synthetic.make_eval_batch(B_DEC, MAX_HIS, catalogue, tb, CB, NB, seed=60 + tb)
        pads = (batch["attention_mask"] == 0).sum(1)
        assert bool((pads % 5 == 0).all()), "prompts are padded by whole items"
        fn = prefix_allowed_tokens_fn_by_last_token(Trie(all_item_tokens[tb]), last_token_set)
        with torch.no_grad():
            out = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], max_new_tokens=4,
                                 prefix_allowed_tokens_fn=fn, num_beams=BEAMS, num_return_sequences=BEAMS,
                                 output_scores=True, return_dict_in_generate=True, early_stopping=True, use_cache=False)
        scores = out.sequences_scores
        gaps = (scores.view(B_DEC, BEAMS)[:, :-1] - scores.view(B_DEC, BEAMS)[:, 1:]).abs().min()
        print(f"behaviour {tb}: pads {pads.tolist()}, min score gap between ranked beams {float(gaps):.3e}")
        res.update({f"b{tb}_input_ids": batch["input_ids"].numpy(), f"b{tb}_attention_mask": batch["attention_mask"].numpy(),
                    f"b{tb}_sequences": out.sequences.numpy(), f"b{tb}_scores": scores.numpy().astype(np.float64)})
    meta = dict(config=d, model="Qwen3MoeWithTemperature", codebook=CB, num_behavior=NB, beams=BEAMS, weight_seed=WSEED_DEC,
                weight_scale=WSCALE, use_cache=False,
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    if not _ref_loader.reference_available():
        raise SystemExit(f"reference not found under {_ref_loader.REF_ROOT}")
    torch.set_num_threads(8)
    which = sys.argv[1:] or list(CASES) + ["moe_router"] + list(DECODE)
    for n in which:
        if n == "moe_router":
            run_router()
        elif n in DECODE:
            run_decode(n)
        else:
            run_case(n, CASES[n])
