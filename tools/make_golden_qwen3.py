#!/usr/bin/env python3
"""Golden fixtures of the plain Qwen3 baseline (``--backbone Qwen3``), generated from the REAL reference.

Runs the reference's ``Qwen3WithTemperature`` (ref:SeqRec/models/generative/Qwen3/model.py: HF ``Qwen3ForCausalLM`` +
the temperature loss), imported through the shims of ``oracle/_ref_loader.py``, with the weights of the one seeded
recipe in ``tests/helpers/qwen3_weights.py`` (pinned in every fixture by per-tensor fp64 checksums).  The config is the
reference's ``Qwen3-Light`` config.json with the vocabulary resized, as train_SMB_decoder.py does.

  qwen3_small.npz       shrunk shape (hidden 128, 4 layers, 2 / 1 heads, intermediate 256): full logits, the norms'
                        and the embedding's gradients in full, samples of the projections' gradients
  qwen3_full.npz        the Qwen3-Light shape, V = 1041, S = 505, one padded row, sampled tensors
  qwen3_small_bf16.npz  "small" with the forward under torch.autocast("cpu", bfloat16), backward outside it
  decode_qwen3_small.npz  generate() as test_SMB_decoder.py:122-137 calls it (left-padded prompts of different lengths,
                        trie constraint, 6 beams, 4 new tokens): beams, scores and metrics

The Qwen3Session baseline (``--backbone Qwen3Session``): the reference's ``Qwen3SessionWithTemperature``
(ref:SeqRec/models/generative/Qwen3Session/model.py, the same parameters) with the same weights, num_positions = 5 and
model_max_length = 1024 set on the config as train_SMB_decoder.py:369-378 does, items grouped into sessions:

  qwen3_session_small.npz       "small" with LEFT-padded rows, sessions of mean 2.5 items, raw session ids that are not
                                consecutive, and the reference's own dense self mask (_update_session_wise_causal_mask)
  qwen3_session_full.npz        "full" with sessions of mean 4 items
  qwen3_session_small_bf16.npz  "session_small" under torch.autocast("cpu", bfloat16)
  decode_qwen3_session_small.npz  generate() as test_SMB_decoder.py:139-156 calls it (session_ids, extended_session_ids)

As oracle/make_golden.py: every dropout p = 0 and the gradients under ``sdpa_kernel(SDPBackend.MATH)``.

Usage:  python tools/make_golden_qwen3.py [small full small_bf16 decode session_small session_full session_small_bf16
                                          decode_session]     (needs the reference checkout; CPU only)
"""
import contextlib
import functools
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402
import qwen3_weights  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SMALL = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
             intermediate_size=256)
CASES = {
    "small": dict(dims=SMALL, codebook=8, B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=12, wseed=6, full=True),
    "full": dict(dims=dict(), codebook=256, B=4, n_items=101, pad_rows={1: 10}, seed=1, wseed=0, full=False),
    "small_bf16": dict(dims=SMALL, codebook=8, B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=12, wseed=6, full=True, amp=True),
    # Qwen3Session
    "session_small": dict(dims=SMALL, codebook=8, B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=14, wseed=6, full=True,
                          session_mean=2.5, left_pad=True, dense_mask=True),
    "session_full": dict(dims=dict(), codebook=256, B=4, n_items=101, pad_rows={1: 10}, seed=2, wseed=0, full=False,
                         session_mean=4.0),
    "session_small_bf16": dict(dims=SMALL, codebook=8, B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=14, wseed=6, full=True,
                               session_mean=2.5, left_pad=True, amp=True),
}
SESSION_FIELDS = dict(num_positions=5, model_max_length=1024)      # train_SMB_decoder.py:369-378
# decode case: the shape of oracle/make_golden_decode.py's, weights of the recipe scaled so that beam order is decided by
# gaps far above fp32 noise
CB, NB, N_CAT, BEAMS, B_DEC, MAX_HIS, WSEED_DEC, WSCALE = 8, 3, 48, 6, 4, 6, 21, 4.0
METRICS = ["hit@1", "hit@5", "ndcg@5", "recall@5"]


def load_reference(session: bool = False):
    """(reference Qwen3WithTemperature or Qwen3SessionWithTemperature, transformers Qwen3Config)."""
    if not _ref_loader.reference_available():
        raise SystemExit(f"reference not found under {_ref_loader.REF_ROOT}")
    _ref_loader._install_shims()
    for parent in ("SeqRec", "SeqRec.models", "SeqRec.models.generative"):
        if parent not in sys.modules:           # (generative/__init__ imports every backbone: import the leaf module only)
            pkg = types.ModuleType(parent)
            pkg.__path__ = [os.path.join(_ref_loader.REF_ROOT, *parent.split("."))]
            pkg.__spec__ = importlib.machinery.ModuleSpec(parent, None, is_package=True)
            pkg.__spec__.submodule_search_locations = pkg.__path__
            sys.modules[parent] = pkg
    from transformers import Qwen3Config
    if session:
        from SeqRec.models.generative.Qwen3Session.model import Qwen3SessionWithTemperature
        return Qwen3SessionWithTemperature, Qwen3Config
    from SeqRec.models.generative.Qwen3.model import Qwen3WithTemperature
    return Qwen3WithTemperature, Qwen3Config


def reference_config(Cfg, vocab_size, session=False, **dims):
    cfg = Cfg.from_pretrained(os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "Qwen3-Light"))
    for k, v in dims.items():
        setattr(cfg, k, v)
    cfg.vocab_size = vocab_size
    cfg.attention_dropout = 0.0
    if session:
        for k, v in SESSION_FIELDS.items():
            setattr(cfg, k, v)
    return cfg


def config_dict(cfg, session=False):
    keys = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim",
            "intermediate_size", "rms_norm_eps", "initializer_range", "pad_token_id", "tie_word_embeddings")
    if session:
        keys += tuple(SESSION_FIELDS)
    d = {k: getattr(cfg, k) for k in keys}
    rp = getattr(cfg, "rope_parameters", None)
    d["rope_theta"] = float(rp["rope_theta"]) if isinstance(rp, dict) else float(cfg.rope_theta)
    return d


def _as_transformers_4(model):
    """Qwen3SessionWithTemperature (ref model.py:165-180, 279-309) is written against transformers 4.x: its decoder layer
    took ``past_key_value`` and returned a tuple, and generate() passed ``cache_position``; 5.x's layer takes
    ``past_key_values`` and returns the hidden states, and its generate() passes no ``cache_position``.  Two hooks per layer
    and a forward that fills in ``cache_position`` (the cached length onwards, what 4.x passed) give the reference its
    calling convention back: without them the second layer sees one row of the batch, a generation's K/V cache stays empty
    and the generated tokens never leave the prompt's extended ids."""
    def pre(mod, args, kwargs):
        if "past_key_value" in kwargs:
            kwargs["past_key_values"] = kwargs.pop("past_key_value")
        kwargs.pop("output_attentions", None)
        return args, kwargs

    for layer in model.model.layers:
        layer.register_forward_pre_hook(pre, with_kwargs=True)
        layer.register_forward_hook(lambda mod, inp, out: (out,) if torch.is_tensor(out) else out)
    orig_forward = model.forward

    @functools.wraps(orig_forward)
    def forward(*a, **k):
        ids, pkv = k.get("input_ids"), k.get("past_key_values")
        if k.get("cache_position") is None and ids is not None and pkv is not None:
            past = pkv.get_seq_length()
            k["cache_position"] = torch.arange(past, past + ids.shape[1])
        return orig_forward(*a, **k)
    model.forward = forward


def build_model(Model, cfg, sd):
    model = Model(cfg)
    if hasattr(model.model, "_update_session_wise_causal_mask"):
        _as_transformers_4(model)
    model.set_hyper(0.7)
    model.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True)
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr(), "head not tied"
    return model


def left_pad(batch):
    """The padding moved in front of every row (whole items: the in-item mask stays aligned), all tensors with it."""
    am = batch["attention_mask"]
    for b in range(am.shape[0]):
        n = int(am[b].sum())
        for k in batch:
            row = batch[k][b].clone()
            batch[k][b] = torch.cat([row[n:], row[:n]])
    return batch


def run_case(name, spec):
    session = spec.get("session_mean") is not None
    Model, Cfg = load_reference(session)
    cb = spec["codebook"]
    V = synthetic.vocab_size(cb, NB)
    cfg = reference_config(Cfg, V, session, **spec["dims"])
    cd = config_dict(cfg, session)
    sd = qwen3_weights.init_state_dict(cd, seed=spec["wseed"])
    model = build_model(Model, cfg, sd)
    ref_keys = [k for k in model.state_dict().keys()]
    batch = synthetic.make_batch(spec["B"], spec["n_items"], cb, NB, seed=spec["seed"], pad_rows=spec["pad_rows"],
                                 **(dict(session_mean=spec["session_mean"]) if session else {}))
    if spec.get("left_pad"):
        batch = left_pad(batch)
    fwd_in = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"])
    if session:
        fwd_in.update(session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])
    amp = bool(spec.get("amp"))
    autocast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if amp else contextlib.nullcontext
    model.eval()
    with torch.no_grad(), autocast():
        out = model(**fwd_in, output_hidden_states=True, use_cache=False)
        logits_raw = out.logits.float().clone()
        hidden = [h.float().clone() for h in out.hidden_states]
        out_l = model(**fwd_in, labels=batch["labels"], use_cache=False)
        loss_mean = float(out_l.loss)
        logits_scaled = out_l.logits.float().clone()
        n_items_tok = float((batch["labels"][:, 1:] != -100).sum()) * 2.0       # any positive number
        loss_sum = float(model(**fwd_in, labels=batch["labels"], use_cache=False, num_items_in_batch=n_items_tok).loss)
    model.train()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    with sdpa_kernel(SDPBackend.MATH):
        with autocast():
            out_g = model(**fwd_in, labels=batch["labels"], use_cache=False)
        out_g.loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    keys, sums = qwen3_weights.fp64_checksums(sd)
    gkeys = sorted(k for k in grads if k != "lm_head.weight")
    keep = batch["attention_mask"].bool()[:, :, None]
    res = dict(
        input_ids=batch["input_ids"].numpy(), attention_mask=batch["attention_mask"].numpy(),
        actions=batch["actions"].numpy(), labels=batch["labels"].numpy(),
        session_ids=batch["session_ids"].numpy(), extended_session_ids=batch["extended_session_ids"].numpy(),
        loss_mean=np.float64(loss_mean), loss_sum=np.float64(loss_sum), num_items=np.float64(n_items_tok),
        loss_train_mode=np.float64(float(out_g.loss)),
        weight_keys=np.array(keys), weight_checksums=sums,
        reference_state_dict_keys=np.array(ref_keys),
        reference_state_dict_shapes=np.array([json.dumps(list(model.state_dict()[k].shape)) for k in ref_keys]),
        grad_keys=np.array(gkeys),
        grad_norms=np.array([float(grads[k].double().norm()) for k in gkeys]),
        grad_abssum=np.array([float(grads[k].double().abs().sum()) for k in gkeys]),
        global_grad_norm=np.float64(float(torch.sqrt(sum((grads[k].double() ** 2).sum() for k in gkeys)))),
        hidden_sum=np.array([float(h.double().sum()) for h in hidden]),
        hidden_abssum=np.array([float(h.double().abs().sum()) for h in hidden]),
        # (over the kept tokens only: rows before a sequence's first token have no key and their value is a convention)
        hidden_sum_kept=np.array([float((h.double() * keep).sum()) for h in hidden]),
    )
    if amp:
        res["logits_dtype"] = np.array(str(out.logits.dtype))
    if spec.get("dense_mask"):
        # the reference's own self mask (model.py:28-80): True where query i may attend key j
        S = batch["input_ids"].shape[1]
        with torch.no_grad():
            dense = model.model._update_session_wise_causal_mask(
                attention_mask=batch["attention_mask"], input_tensor=torch.zeros(spec["B"], S, 1),
                cache_position=torch.arange(S), past_key_values=None, session_ids=batch["session_ids"])
        res["reference_self_mask"] = (dense[:, 0] == 0).numpy()
    if spec["full"]:
        res["logits_raw"] = logits_raw.numpy()
        res["logits_scaled"] = logits_scaled.numpy()
        # the norms' and the embedding's gradients in full, the projections' sampled as in "full": the fixture stays small
        for k in gkeys:
            g = grads[k]
            if g.dim() == 1 or k == "model.embed_tokens.weight":
                res["grad::" + k] = g.numpy()
            else:
                res["gradsample::" + k] = g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].numpy()
    else:
        res["logits_raw_sample"] = logits_raw[:, ::37, ::53].numpy()
        res["logits_scaled_sample"] = logits_scaled[:, ::37, ::53].numpy()
        res["logits_raw_absmax"] = np.float64(float(logits_raw.abs().max()))
        res["hidden_last_sample"] = hidden[-1][:, ::37, ::16].numpy()
        for k in gkeys:
            g = grads[k]
            if g.dim() == 1:
                res["grad::" + k] = g.numpy()
            else:
                res["gradsample::" + k] = g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].numpy()
    meta = dict(name=name, config=cd, codebook=cb, temperature=0.7, weight_seed=spec["wseed"], batch_seed=spec["seed"],
                n_items=spec["n_items"], pad_rows={str(k): v for k, v in spec["pad_rows"].items()},
                **(dict(session_mean=spec["session_mean"], left_pad=bool(spec.get("left_pad"))) if session else {}),
                autocast="bfloat16" if amp else None,
                model="Qwen3SessionWithTemperature" if session else "Qwen3WithTemperature",
                weights="tests/helpers/qwen3_weights.py::init_state_dict(config, weight_seed)",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__,
                               reference="wzf2000/GAMER", sdpa_backend_for_grads="MATH"))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"qwen3_{name}.npz")
    np.savez_compressed(path, **res)
    print(f"[qwen3_{name}] loss_mean={loss_mean:.7f} loss_sum={loss_sum:.7f} gnorm={float(res['global_grad_norm']):.6f} "
          f"-> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


def run_decode(session: bool = False):
    Model, Cfg = load_reference(session)
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn_by_last_token
    from SeqRec.evaluation.ranking import get_metrics_results, get_topk_results
    V = synthetic.vocab_size(CB, NB)
    cfg = reference_config(Cfg, V, session, **SMALL)
    cd = config_dict(cfg, session)
    sd = qwen3_weights.init_state_dict(cd, seed=WSEED_DEC, scale=WSCALE)
    model = build_model(Model, cfg, sd)
    model.eval()
    model.generation_config.pad_token_id = synthetic.PAD_ID
    catalogue = synthetic.make_catalogue(N_CAT, CB, seed=3)
    all_item_tokens = [synthetic.item_tokens(catalogue, b, CB).tolist() for b in range(NB)]
    last_token_set = set(t[-1] for beh in all_item_tokens for t in beh)
    last_token_set.add(synthetic.PAD_ID)
    keys, sums = qwen3_weights.fp64_checksums(sd)
    res = dict(catalogue=catalogue.numpy(), weight_keys=np.array(keys), weight_checksums=sums)
    orig_forward = model.forward

    @functools.wraps(orig_forward)
    def forward_without_offsets(*a, **k):
        # RoPE is relative, so a row's positions may all shift together; what must not happen is that the generated tokens
        # lose the row's offset: prompt at cumsum(mask) - 1 as generate() builds it, the new token then at L0 + t - 1 for
        # every row (the cache length) instead of kept tokens + t - 1.  The fixture's beams must differ from this.
        # Qwen3Session: the generated tokens must sit at max(extended_session_ids) + t (model.py:293-309); the stand-in
        # drops the extended ids after the prompt, which leaves them at generate()'s padding-offset positions
        # cumsum(mask) - 1.  The fixture's beams must differ from this too.
        ids = k.get("input_ids")
        pkv = k.get("past_key_values")
        past = pkv.get_seq_length() if pkv is not None else 0
        if ids is not None and past > 0:
            if session:
                k.pop("extended_session_ids", None)
            else:
                k["position_ids"] = torch.arange(past, past + ids.shape[1])[None, :].expand(ids.shape[0], -1)
        return orig_forward(*a, **k)
    for tb in range(NB):
        batch = synthetic.make_eval_batch(B_DEC, MAX_HIS, catalogue, tb, CB, NB, min_his=2, seed=40 + tb,
                                          **(dict(session_mean=2.5) if session else {}))
        pads = (batch["attention_mask"] == 0).sum(1).tolist()
        assert len(set(pads)) >= 3, f"behaviour {tb}: the rows' left padding should differ ({pads})"
        trie = Trie(all_item_tokens[tb])
        fn = prefix_allowed_tokens_fn_by_last_token(trie, last_token_set)
        gen_kw = dict(max_new_tokens=4, prefix_allowed_tokens_fn=fn, num_beams=BEAMS, num_return_sequences=BEAMS,
                      output_scores=True, return_dict_in_generate=True, early_stopping=True)
        if session:      # test_SMB_decoder.py:139-156
            gen_kw.update(session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])
        with torch.no_grad():
            out = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], **gen_kw)
            model.forward = forward_without_offsets
            try:
                out_np = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], **gen_kw)
            finally:
                model.forward = orig_forward
        seqs, scores = out.sequences, out.sequences_scores
        differs = bool((out_np.sequences != seqs).any()) or bool((out_np.sequences_scores - scores).abs().max() > 1e-3)
        gen = seqs[:, -4:]
        pred = ["".join(f"<{int(t)}>" for t in row) for row in gen]
        tgt_tok = synthetic.item_tokens(batch["targets"], tb, CB)[:, 1:]
        targets = [["".join(f"<{int(t)}>" for t in row)] for row in tgt_tok]
        topk = get_topk_results(pred, scores, targets, BEAMS)
        metrics = get_metrics_results(topk, METRICS, targets)
        sc = scores.view(B_DEC, BEAMS)
        print(f"behaviour {tb}: left padding {pads}; min score gap {float((sc[:, :-1] - sc[:, 1:]).abs().min()):.3e}; "
              f"positions without the offsets change the result: {differs}; metrics {metrics}")
        res.update({f"b{tb}_input_ids": batch["input_ids"].numpy(), f"b{tb}_attention_mask": batch["attention_mask"].numpy(),
                    f"b{tb}_actions": batch["actions"].numpy(), f"b{tb}_targets": batch["targets"].numpy(),
                    f"b{tb}_sequences": seqs.numpy(), f"b{tb}_scores": scores.numpy().astype(np.float64),
                    f"b{tb}_sequences_no_offsets": out_np.sequences.numpy(),
                    f"b{tb}_scores_no_offsets": out_np.sequences_scores.numpy().astype(np.float64),
                    f"b{tb}_topk": np.array(topk, dtype=np.int8),
                    f"b{tb}_metrics": np.array([metrics[m] for m in METRICS], dtype=np.float64)})
        if session:
            res.update({f"b{tb}_session_ids": batch["session_ids"].numpy(),
                        f"b{tb}_extended_session_ids": batch["extended_session_ids"].numpy()})
    meta = dict(config=cd, model="Qwen3SessionWithTemperature" if session else "Qwen3WithTemperature", codebook=CB, num_behavior=NB, beams=BEAMS, weight_seed=WSEED_DEC,
                weight_scale=WSCALE, metrics=METRICS,
                weights="tests/helpers/qwen3_weights.py::init_state_dict(config, weight_seed, scale=weight_scale)",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__,
                               reference="wzf2000/GAMER"))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "decode_qwen3_session_small.npz" if session else "decode_qwen3_small.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["small", "full", "small_bf16", "decode", "session_small", "session_full", "session_small_bf16",
                             "decode_session"]
    for n in which:
        if n in ("decode", "decode_session"):
            run_decode(session=n == "decode_session")
        else:
            run_case(n, CASES[n])
