#!/usr/bin/env python3
"""Train-step time and beam-search throughput of Qwen3MoeAction next to Qwen3Moe at the same shape.

Both models have config/s2s-models/Qwen3Moe's architecture (hidden 256, 8 layers, SwiGLU experts in every layer, injection
layers 0-3, no cross attention), five positions per item and FOUR behaviours: Qwen3Moe's sparse layers have 6 experts,
Qwen3MoeAction's (6 - 1) * 4 + 1 = 21.  21 experts x 5 behaviour indices exceed the 64 groups of the (expert, behaviour)
inject table, so Qwen3MoeAction's fp32 forms take the concatenated [T, 320] FFN input; Qwen3Moe is therefore timed twice,
as shipped and with GAMER_SPLIT_INJECT=0 (the same concatenated input, 6 groups): the second leg separates what the input
path costs from what the 21 groups cost.
Train step: ``Engine.train_step`` on one synthetic batch of ``--batch`` x 505 tokens (101 items), the three split3 engines in
the SAME process in alternating blocks of ``--steps`` steps, ``--rounds`` times, after ``--warmup`` untimed steps each, every
step between device events; then the two bf16 engines in the same way.
Evaluation path: ``--users`` users x ``--beams`` beams, history 100 items, 4 new tokens, cached decode in fp32; the users'
target behaviours cycle through all four (a Qwen3MoeAction step then runs four experts), the trie holds the catalogue under
every behaviour token, and both models search the same prompts, alternating, every search between device events after 3
untimed ones.
Every figure is the median with the smallest and largest sample.  Prints one JSON line.

  python tools/bench_moe_action.py --batch 1024 --steps 10 --warmup 3 --rounds 2
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeActionConfig, Qwen3MoeConfig  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from bench_session_moe import alternate  # noqa: E402

ITEMS, NB, MIX = 101, 4, [0.6, 0.25, 0.1, 0.05]


def config(cls):
    return cls(vocab_size=synthetic.vocab_size(256, NB), num_behavior=NB, n_positions=ITEMS, num_positions=5,
               behavior_maps={str(k): v for k, v in synthetic.behavior_maps(256, NB).items()})


def engine(cls, variant, dtype="f32", split_inject=True):
    """An engine with seeded weights; ``split_inject=False``: constructed under GAMER_SPLIT_INJECT=0."""
    old = os.environ.get("GAMER_SPLIT_INJECT")
    if not split_inject:
        os.environ["GAMER_SPLIT_INJECT"] = "0"
    try:
        e = Engine(config(cls), temperature=0.7, variant=variant, dtype=dtype)
    finally:
        if not split_inject:
            os.environ.pop("GAMER_SPLIT_INJECT")
            if old is not None:
                os.environ["GAMER_SPLIT_INJECT"] = old
    e.init_weights(seed=0)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_action.py measures on the GPU; there is none")
    out = dict(metric="Qwen3MoeAction train step and beam search next to Qwen3Moe's at the same shape",
               device=torch.cuda.get_device_name(0), batch=args.batch, tokens=ITEMS * 5, behaviours=NB)
    batch = synthetic.make_batch(args.batch, ITEMS, 256, NB, seed=7, behavior_probs=MIX)
    action = engine(Qwen3MoeActionConfig, "qwen3moe_action")
    moe = engine(Qwen3MoeConfig, "qwen3moe")
    moe_cat = engine(Qwen3MoeConfig, "qwen3moe", split_inject=False)
    out["ffn_experts"] = dict(qwen3moe_action=action.cfg.num_ffn_experts, qwen3moe=moe.cfg.num_ffn_experts)
    out["split_inject"] = dict(qwen3moe_action=action.split_inject, qwen3moe=moe.split_inject, qwen3moe_concat=moe_cat.split_inject)
    out["train_step"] = alternate({"qwen3moe_action_split3": lambda: action.train_step(batch, 5e-4),
                                   "qwen3moe_split3": lambda: moe.train_step(batch, 5e-4),
                                   "qwen3moe_split3_concat_inject": lambda: moe_cat.train_step(batch, 5e-4)},
                                  args.warmup, args.steps, args.rounds, args.batch)
    action.check_inputs()
    del action, moe, moe_cat
    torch.cuda.empty_cache()
    action16 = engine(Qwen3MoeActionConfig, "qwen3moe_action", dtype="bf16")
    moe16 = engine(Qwen3MoeConfig, "qwen3moe", dtype="bf16")
    out["train_step"].update(alternate({"qwen3moe_action_bf16": lambda: action16.train_step(batch, 5e-4),
                                        "qwen3moe_bf16": lambda: moe16.train_step(batch, 5e-4)},
                                       args.warmup, args.steps, args.rounds, args.batch))
    del action16, moe16
    torch.cuda.empty_cache()
    print(json.dumps(out["train_step"]), file=sys.stderr, flush=True)

    his = ITEMS - 1
    cat = synthetic.make_catalogue(20000, 256, seed=3)
    trie = ItemTrie([t for b in range(NB) for t in synthetic.item_tokens(cat, b, 256).tolist()])
    per = [synthetic.make_eval_batch(args.users, his, cat, tb, 256, NB, min_his=his, seed=5, behavior_probs=MIX)
           for tb in range(NB)]
    ev = {k: torch.stack([per[i % NB][k][i] for i in range(args.users)]) for k in ("input_ids", "attention_mask")}
    action = engine(Qwen3MoeActionConfig, "qwen3moe_action")
    moe = engine(Qwen3MoeConfig, "qwen3moe")
    out["beam_search"] = alternate(
        {"qwen3moe_action": lambda: beam_search(action, ev["input_ids"], ev["attention_mask"], None, trie, args.beams, 4),
         "qwen3moe": lambda: beam_search(moe, ev["input_ids"], ev["attention_mask"], None, trie, args.beams, 4)},
        3, max(2, args.steps // 2), args.rounds, args.users)
    out["beam_search"].update(users=args.users, beams=args.beams, history_items=his, target_behaviours=NB)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
