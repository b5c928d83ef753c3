#!/usr/bin/env python3
"""Golden fixtures of Qwen3Multi's FFN ablation configurations, generated from the REAL reference.

Runs the reference's ``Qwen3MultiWithTemperature`` / ``Qwen3SessionMultiWithTemperature`` (imported through the shims of
``oracle/_ref_loader.py``) with the switches its config.json carries for the paper's FFN ablations set as
train_SMB_decoder.py:321-360 leaves them: ``mlp_type`` (MyQwen3SparseMLP or PBATransformerSparseMLP), ``sparse_layers_decoder``
(the other layers run one dense MLP over every token) and ``Moe_behavior_only`` (num_experts = 2: behaviour tokens to expert 1,
semantic tokens to index 2, for which no expert exists - their FFN output stays zero).  Weights come from the seeded recipe in
``tests/helpers/ffn_ablation_weights.py`` (pinned by per-tensor fp64 checksums); the reference's state-dict key list is stored
and checked against the recipe's.  Every dropout p = 0, gradients under ``sdpa_kernel(SDPBackend.MATH)``.

  ablate_dense_small      SwiGLU; sparse layers [1, 3]: layer 0 a dense injecting layer, layer 2 a dense cross layer
  ablate_pba_small        PBATransformer; sparse layers [0, 2] (sparse and dense, injecting and cross)
  ablate_behonly_small    SwiGLU, Moe_behavior_only, every layer sparse, num_experts = 2
  ablate_pba_small_bf16   "pba_small" with the forward under torch.autocast("cpu", bfloat16), backward outside it
  ablate_session_small    Qwen3SessionMulti, PBATransformer, sparse layers [1, 3]
  decode_ablate_small     generate() as test_SMB_decoder.py:158-175 calls it: PBATransformer, sparse layers [0, 2],
                          Moe_behavior_only (the generated semantic tokens skip the FFN of the sparse layers)

Usage:  python tools/make_golden_ffn_ablation.py [case ...]     (needs the reference checkout; CPU only)
"""
import contextlib
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
from gamer_amd.config import _DEFAULTS  # noqa: E402
import ffn_ablation_weights as fw  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SMALL = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
             intermediate_size=256, moe_intermediate_size=128, behavior_embedding_dim=64,
             behavior_injection_decoder=[0, 1], cross_attention_decoder=[2, 3])
CASES = {
    "ablate_dense_small": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[1, 3], Moe_behavior_only=False),
                               B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=31, wseed=7),
    "ablate_pba_small": dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2], Moe_behavior_only=False),
                             B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=32, wseed=8),
    "ablate_behonly_small": dict(ffn=dict(mlp_type="Qwen3", sparse_layers_decoder=[0, 1, 2, 3], Moe_behavior_only=True),
                                 B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=33, wseed=9),
    "ablate_pba_small_bf16": dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2], Moe_behavior_only=False),
                                  B=3, n_items=9, pad_rows={1: 4, 2: 1}, seed=32, wseed=8, amp=True),
    "ablate_session_small": dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[1, 3], Moe_behavior_only=False),
                                 B=4, n_items=15, pad_rows={1: 4, 2: 1}, seed=34, wseed=10, session_mean=2.5),
}
DECODE = dict(ffn=dict(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2], Moe_behavior_only=True))
CB, NB, N_CAT, BEAMS, B_DEC, MAX_HIS, WSEED_DEC, WSCALE = 8, 3, 48, 6, 4, 6, 23, 4.0


def build(ffn: dict, session: bool, wseed: int, scale: float = 1.0):
    """(reference model, its config as a plain dict of this project's schema, weights)."""
    Model, Cfg = _ref_loader.load_reference_classes(session=session)
    V, bmaps = synthetic.vocab_size(CB, NB), synthetic.behavior_maps(CB, NB)
    cfg = _ref_loader.reference_config(Cfg, NB, V, bmaps, n_positions=101, **SMALL)
    for k, v in ffn.items():
        setattr(cfg, k, v)
    cfg.num_experts = 2 if cfg.Moe_behavior_only else cfg.num_positions + 1      # train_SMB_decoder.py:349-356
    cfg.dropout_rate = 0.0
    cfg.attention_dropout = 0.0
    d = {k: getattr(cfg, k) for k in _DEFAULTS if hasattr(cfg, k) and k != "torch_dtype"}
    d["behavior_maps"] = {str(k): int(v) for k, v in bmaps.items()}
    sd = fw.init_state_dict(d, wseed, scale)
    model = Model(cfg)
    model.set_hyper(0.7)
    ref_keys = sorted(k for k in model.state_dict() if k != "lm_head.weight")
    assert ref_keys == sorted(sd), (set(ref_keys) ^ set(sd))
    for k, v in model.state_dict().items():
        if k != "lm_head.weight":
            assert tuple(v.shape) == tuple(sd[k].shape), k
    model.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True)
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr(), "head not tied"
    return model, d, sd, ref_keys


def run_case(name, spec):
    session = spec.get("session_mean") is not None
    model, d, sd, ref_keys = build(spec["ffn"], session, spec["wseed"])
    batch = synthetic.make_batch(spec["B"], spec["n_items"], CB, NB, seed=spec["seed"], pad_rows=spec["pad_rows"],
                                 session_mean=spec.get("session_mean"))
    fwd_in = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], actions=batch["actions"],
                  session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])
    amp = bool(spec.get("amp"))
    autocast = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if amp else contextlib.nullcontext
    model.eval()
    with torch.no_grad(), autocast():
        pos, _, _ = model.model.router(batch["input_ids"].clone(), cache_position=torch.arange(batch["input_ids"].shape[1]))
        logits_raw = model(**fwd_in, use_cache=False).logits.float().clone()
        out_l = model(**fwd_in, labels=batch["labels"], use_cache=False)
        loss_mean, logits_scaled = float(out_l.loss), out_l.logits.float().clone()
    model.train()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    with sdpa_kernel(SDPBackend.MATH):
        with autocast():
            out_g = model(**fwd_in, labels=batch["labels"], use_cache=False)
        out_g.loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if k != "lm_head.weight"}
    gkeys = sorted(grads)
    keys, sums = fw.fp64_checksums(sd)
    res = dict(input_ids=batch["input_ids"].numpy(), attention_mask=batch["attention_mask"].numpy(),
               actions=batch["actions"].numpy(), labels=batch["labels"].numpy(),
               session_ids=batch["session_ids"].numpy(), extended_session_ids=batch["extended_session_ids"].numpy(),
               router_position=pos.numpy().astype(np.int16),
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
                autocast="bfloat16" if amp else None,
                model="Qwen3SessionMultiWithTemperature" if session else "Qwen3MultiWithTemperature",
                generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__,
                               sdpa_backend_for_grads="MATH"))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **res)
    print(f"[{name}] loss={loss_mean:.7f} gnorm={float(res['global_grad_norm']):.6f} -> {path} "
          f"({os.path.getsize(path) / 1e6:.3f} MB)")


def run_decode():
    from SeqRec.generation.trie import Trie, prefix_allowed_tokens_fn_by_last_token
    model, d, sd, ref_keys = build(DECODE["ffn"], False, WSEED_DEC, WSCALE)
    model.eval()
    model.generation_config.pad_token_id = synthetic.PAD_ID
    catalogue = synthetic.make_catalogue(N_CAT, CB, seed=3)
    all_item_tokens = [synthetic.item_tokens(catalogue, b, CB).tolist() for b in range(NB)]
    last_token_set = set(t[-1] for beh in all_item_tokens for t in beh)
    last_token_set.add(synthetic.PAD_ID)
    keys, sums = fw.fp64_checksums(sd)
    res = dict(catalogue=catalogue.numpy(), state_dict_keys=np.array(ref_keys), weight_keys=np.array(keys),
               weight_checksums=sums)
    for tb in range(NB):
        batch = synthetic.make_eval_batch(B_DEC, MAX_HIS, catalogue, tb, CB, NB, seed=60 + tb)
        fn = prefix_allowed_tokens_fn_by_last_token(Trie(all_item_tokens[tb]), last_token_set)
        with torch.no_grad():
            out = model.generate(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"],
                                 actions=batch["actions"], max_new_tokens=4, prefix_allowed_tokens_fn=fn, num_beams=BEAMS,
                                 num_return_sequences=BEAMS, output_scores=True, return_dict_in_generate=True,
                                 early_stopping=True)
        scores = out.sequences_scores
        gaps = (scores.view(B_DEC, BEAMS)[:, :-1] - scores.view(B_DEC, BEAMS)[:, 1:]).abs().min()
        print(f"behaviour {tb}: min score gap between ranked beams {float(gaps):.3e}")
        res.update({f"b{tb}_input_ids": batch["input_ids"].numpy(), f"b{tb}_attention_mask": batch["attention_mask"].numpy(),
                    f"b{tb}_actions": batch["actions"].numpy(), f"b{tb}_sequences": out.sequences.numpy(),
                    f"b{tb}_scores": scores.numpy().astype(np.float64)})
    meta = dict(config=d, model="Qwen3MultiWithTemperature", codebook=CB, num_behavior=NB, beams=BEAMS, weight_seed=WSEED_DEC,
                weight_scale=WSCALE, generator=dict(torch=torch.__version__, transformers=__import__("transformers").__version__))
    res["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "decode_ablate_small.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    if not _ref_loader.reference_available():
        raise SystemExit(f"reference not found under {_ref_loader.REF_ROOT}")
    torch.set_num_threads(8)
    which = sys.argv[1:] or list(CASES) + ["decode_ablate_small"]
    for n in which:
        run_decode() if n == "decode_ablate_small" else run_case(n, CASES[n])
