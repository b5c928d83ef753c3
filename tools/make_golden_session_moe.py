#!/usr/bin/env python3
"""Golden fixtures of the Qwen3SessionMoe model, generated from the REAL reference.

Runs the reference's ``Qwen3SessionMoeWithTemperature`` (ref:SeqRec/models/generative/Qwen3SessionMoe/model.py) under the
installed transformers 5.x.  The reference constructs this class in no task, so the config is what a task would hand it:
``config/s2s-models/Qwen3Moe/config.json`` with the run-time fields of the Qwen3SessionMulti branch
(train_SMB_decoder.py:321-367) and ``model_max_length``, at the small size of ``moe_small``.  The parameters are Qwen3Moe's,
so the weights come from ``tests/helpers/qwen3moe_weights.py`` (pinned by fp64 checksums); the real class's state-dict key list
and shapes are stored and checked against the recipe's.  Every dropout p = 0, gradients under ``sdpa_kernel(SDPBackend.MATH)``.

Importing model.py needs the shims ``tools/make_golden_qwen3moe.py`` documents (``load_reference_moe``) and nothing else.

Batch of the training cases: B = 3 rows of 9 items (num_positions = 5) plus the eos column, S = 46.  Row 0 has sessions of
1, 2, 4 and 2 items and ends with eos in a session of its own; row 1 has 5 items in sessions of 4 and 1 and is right padded;
row 2 has 8 items in ONE session - every query of it sees only its own item - and is right padded.  Raw session ids neither
start at 0 nor are consecutive; the extended ids are 5 * (session rank) + (token in item), as SMB_dataset.py:194-222 lays
them out.

Generation: as for Qwen3Moe, transformers 5.x's ``Qwen3MoeAttention.forward`` takes the cache as ``past_key_values=`` and the
reference's decoder layer passes ``past_key_value=``, which is ignored - the cache is never filled.  The decode fixture was
therefore made the RE-RUN way: ``generate(use_cache=False)`` runs the whole sequence every step, and a wrapper around the
model's forward appends, for the generated columns, a new last session id and the extended ids max + 1, max + 2, ... per row
(what model.py:688-703 gives a cached step).  By model.py:442-455 a generated token then sees every kept token of the prompt
and, through the in-item block, the generated tokens up to itself: the mask a working cache gives.

  session_moe_small        shipped FFN (SwiGLU experts in every layer, injection layers [0, 1])
  session_moe_pba_small    PBATransformer experts, sparse layers [0, 2]
  session_moe_small_bf16   "session_moe_small" with the forward under torch.autocast("cpu", bfloat16), backward outside it
  decode_session_moe_small generate() re-run as above on left-padded prompts (sessions of mean 2.5 items), 4 beams, 4 new tokens

Usage:  python tools/make_golden_session_moe.py [case ...]     (needs the reference checkout; CPU only)
"""
import contextlib
import functools
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3SessionMoeConfig  # noqa: E402
import make_golden_qwen3moe as moe  # noqa: E402
import qwen3moe_weights as mw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CB, NB, P = moe.CB, moe.NB, synthetic.TOKENS_PER_ITEM
MODEL_MAX_LENGTH = 1024
CASES = {
    "session_moe_small": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), seed=71, wseed=31),
    "session_moe_pba_small": dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2]), seed=72, wseed=32),
    "session_moe_small_bf16": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), seed=71, wseed=31, amp=True),
}
B_TRAIN, N_ITEMS, PAD_ROWS = 3, 9, {1: 4, 2: 1}
# per row: (items per session, raw id of each session)
SESSIONS = [([1, 2, 4, 2], [3, 4, 7, 8]), ([4, 1], [1, 5]), ([8], [2])]
N_CAT, BEAMS, NEW, B_DEC, MAX_HIS, WSEED_DEC, WSCALE = 48, 4, 4, 4, 6, 33, 4.0


def load_reference_session_moe():
    """(Qwen3SessionMoeWithTemperature, transformers' Qwen3MoeConfig) of the reference."""
    _, HFConfig = moe.load_reference_moe()
    mod = importlib.import_module("SeqRec.models.generative.Qwen3SessionMoe.model")
    return mod.Qwen3SessionMoeWithTemperature, HFConfig


def hf_config(HFConfig, ffn: dict):
    cfg = moe.hf_config(HFConfig, True, ffn, P)
    cfg.model_max_length = MODEL_MAX_LENGTH
    return cfg


def our_config(cfg) -> dict:
    d = Qwen3SessionMoeConfig.coerce(cfg).to_dict()
    d.pop("torch_dtype", None)
    return d


def build(ffn: dict, wseed: int, scale: float = 1.0):
    Model, HFConfig = load_reference_session_moe()
    cfg = hf_config(HFConfig, ffn)
    d = our_config(cfg)
    sd = mw.init_state_dict(d, wseed, scale)
    model = Model(cfg)
    model.set_hyper(0.7)
    ref_sd = model.state_dict()
    ref_keys = sorted(k for k in ref_sd if k != "lm_head.weight")
    assert ref_keys == sorted(sd), (set(ref_keys) ^ set(sd))
    for k in ref_keys:
        assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), k
    shapes = [json.dumps(list(ref_sd[k].shape)) for k in ref_keys]
    model.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True)
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr(), "head not tied"
    return model, cfg, d, sd, ref_keys, shapes


def case_batch(seed: int):
    """The synthetic SMB batch with the hand-placed sessions of the module docstring and the eos column."""
    batch = synthetic.make_batch(B_TRAIN, N_ITEMS, CB, NB, seed=seed, pad_rows=PAD_ROWS)
    S0 = N_ITEMS * P
    sess = torch.zeros(B_TRAIN, S0 + 1, dtype=torch.int64)
    ext = torch.zeros(B_TRAIN, S0 + 1, dtype=torch.int64)
    ids = torch.cat([batch["input_ids"], torch.full((B_TRAIN, 1), synthetic.PAD_ID, dtype=torch.int64)], 1)
    am = torch.cat([batch["attention_mask"], torch.zeros(B_TRAIN, 1, dtype=torch.int64)], 1)
    lab = torch.cat([batch["labels"], torch.full((B_TRAIN, 1), -100, dtype=torch.int64)], 1)
    tok = torch.arange(P)
    for b, (sizes, raws) in enumerate(SESSIONS):
        assert sum(sizes) * P == int(batch["attention_mask"][b].sum()), (b, sizes)
        col = 0
        for rank, (n, raw) in enumerate(zip(sizes, raws)):
            sess[b, col:col + n * P] = raw
            ext[b, col:col + n * P] = rank * P + tok.repeat(n)
            col += n * P
        if col == S0:                               # a full row: eos in a session of its own
            ids[b, S0], am[b, S0], lab[b, S0] = synthetic.EOS_ID, 1, synthetic.EOS_ID
            sess[b, S0], ext[b, S0] = raws[-1] + 1, len(sizes) * P
    return dict(input_ids=ids, attention_mask=am, labels=lab, session_ids=sess, extended_session_ids=ext)


def run_case(name, spec):
    model, cfg, d, sd, ref_keys, shapes = build(spec["ffn"], spec["wseed"])
    batch = case_batch(spec["seed"])
    fwd_in = {k: batch[k] for k in ("input_ids", "attention_mask", "session_ids", "extended_session_ids")}
    amp = bool(spec.get("amp"))
    autocast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if amp else contextlib.nullcontext
    B, S = batch["input_ids"].shape
    model.eval()
    with torch.no_grad(), autocast():
        logits_raw = model(**fwd_in, use_cache=False).logits.float().clone()
        out_l = model(**fwd_in, labels=batch["labels"], use_cache=False)
        loss_mean, logits_scaled = float(out_l.loss), out_l.logits.float().clone()
        dense = model.model._update_session_wise_causal_mask(
            attention_mask=batch["attention_mask"], input_tensor=torch.zeros(B, S, 1), cache_position=torch.arange(S),
            past_key_values=None, session_ids=batch["session_ids"])
    allowed = dense[:, 0] == 0                       # True where query i may attend key j
    one = allowed[2, :8 * P, :8 * P]                 # the single-session row: its own item up to itself, nothing else
    own = (torch.arange(8 * P)[:, None] // P == torch.arange(8 * P)[None, :] // P) & torch.ones(8 * P, 8 * P).tril().bool()
    assert bool((one == own).all()), "row 2 is one session: every query sees only its own item"
    model.train()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    with sdpa_kernel(SDPBackend.MATH):
        with autocast():
            out_g = model(**fwd_in, labels=batch["labels"], use_cache=False)
        out_g.loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if k != "lm_head.weight"}
    gkeys = sorted(grads)
    keys, sums = mw.fp64_checksums(sd)
    res = {k: v.numpy() for k, v in batch.items()}
    res.update(reference_self_mask=allowed.numpy(), loss_mean=np.float64(loss_mean),
               loss_train_mode=np.float64(float(out_g.loss)), logits_raw=logits_raw.numpy(),
               logits_scaled=logits_scaled.numpy(), state_dict_keys=np.array(ref_keys), state_dict_shapes=np.array(shapes),
               weight_keys=np.array(keys), weight_checksums=sums, grad_keys=np.array(gkeys),
               grad_norms=np.array([float(grads[k].double().norm()) for k in gkeys]),
               grad_abssum=np.array([float(grads[k].double().abs().sum()) for k in gkeys]),
               global_grad_norm=np.float64(float(torch.sqrt(sum((grads[k].double() ** 2).sum() for k in gkeys)))))
    for k in gkeys:
        g = grads[k]
        if g.dim() == 1:
            res["grad::" + k] = g.numpy()
        else:
            res["gradsample::" + k] = g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].numpy()
    meta = dict(name=name, config=d, codebook=CB, temperature=0.7, weight_seed=spec["wseed"], batch_seed=spec["seed"],
                sessions=SESSIONS, autocast="bfloat16" if amp else None, model="Qwen3SessionMoeWithTemperature",
                weights="tests/helpers/qwen3moe_weights.py::init_state_dict(config, weight_seed)",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__,
                               sdpa_backend_for_grads="MATH"))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **res)
    print(f"[{name}] loss={loss_mean:.7f} gnorm={float(res['global_grad_norm']):.6f} -> {path} "
          f"({os.path.getsize(path) / 1e6:.3f} MB)")


def rerun_forward(model, L0: int):
    """The model's forward for ``generate(use_cache=False)``: the session ids and extended ids of the prompt (what generate()
    keeps passing, one row per beam) grown by the generated columns - a new last session, extended ids max + 1, max + 2, ..."""
    orig = model.forward

    @functools.wraps(orig)
    def forward(*a, **k):
        ids, sid, ext = k["input_ids"], k["session_ids"], k["extended_session_ids"]
        t = ids.shape[1] - L0
        assert sid.shape[1] == L0 and ext.shape[1] == L0 and k.get("past_key_values") is None
        if t:
            k["session_ids"] = torch.cat([sid, (sid.max(1, keepdim=True).values + 1).expand(-1, t)], 1)
            k["extended_session_ids"] = torch.cat([ext, ext.max(1, keepdim=True).values + torch.arange(1, t + 1)[None, :]], 1)
        k.pop("cache_position", None)
        k.pop("position_ids", None)                  # (generate()'s cumsum(mask) - 1; the model takes the extended ids)
        return orig(*a, **k)
    return forward


def run_decode(name="decode_session_moe_small"):
    load_reference_session_moe()
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn_by_last_token
    model, cfg, d, sd, ref_keys, shapes = build(dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3]), WSEED_DEC, WSCALE)
    model.eval()
    model.generation_config.pad_token_id = synthetic.PAD_ID
    catalogue = synthetic.make_catalogue(N_CAT, CB, seed=3)
    all_item_tokens = [synthetic.item_tokens(catalogue, b, CB).tolist() for b in range(NB)]
    last_token_set = set(t[-1] for beh in all_item_tokens for t in beh)
    last_token_set.add(synthetic.PAD_ID)
    keys, sums = mw.fp64_checksums(sd)
    res = dict(catalogue=catalogue.numpy(), state_dict_keys=np.array(ref_keys), weight_keys=np.array(keys),
               weight_checksums=sums)
    L0 = MAX_HIS * P + 1
    model.forward = rerun_forward(model, L0)
    for tb in range(NB):
        batch = synthetic.make_eval_batch(B_DEC, MAX_HIS, catalogue, tb, CB, NB, min_his=2, seed=80 + tb, session_mean=2.5)
        pads = (batch["attention_mask"] == 0).sum(1)
        assert bool((pads % P == 0).all()) and len(set(pads.tolist())) >= 2, pads
        fn = prefix_allowed_tokens_fn_by_last_token(Trie(all_item_tokens[tb]), last_token_set)
        with torch.no_grad():
            out = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"],
                                 session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"],
                                 max_new_tokens=NEW, prefix_allowed_tokens_fn=fn, num_beams=BEAMS, num_return_sequences=BEAMS,
                                 output_scores=True, return_dict_in_generate=True, early_stopping=True, use_cache=False)
        scores = out.sequences_scores
        gaps = (scores.view(B_DEC, BEAMS)[:, :-1] - scores.view(B_DEC, BEAMS)[:, 1:]).abs().min()
        print(f"behaviour {tb}: pads {pads.tolist()}, min score gap between ranked beams {float(gaps):.3e}")
        res.update({f"b{tb}_{k}": batch[k].numpy() for k in ("input_ids", "attention_mask", "session_ids",
                                                            "extended_session_ids")})
        res.update({f"b{tb}_sequences": out.sequences.numpy(), f"b{tb}_scores": scores.numpy().astype(np.float64)})
    meta = dict(config=d, model="Qwen3SessionMoeWithTemperature", codebook=CB, num_behavior=NB, beams=BEAMS, new_tokens=NEW,
                weight_seed=WSEED_DEC, weight_scale=WSCALE, use_cache=False, made="re-run: the whole sequence every step",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    if not _ref_loader.reference_available():
        raise SystemExit(f"reference not found under {_ref_loader.REF_ROOT}")
    torch.set_num_threads(8)
    for n in sys.argv[1:] or list(CASES) + ["decode_session_moe_small"]:
        if n.startswith("decode"):
            run_decode(n)
        else:
            run_case(n, CASES[n])
