#!/usr/bin/env python3
"""Train-step time and beam-search throughput of Qwen3SessionMoe next to the two driver-line legs it is a subset of.

Train step: ``Engine.train_step`` on one synthetic batch of ``--batch`` x 505 tokens (101 items) with sessions of 4 items
on average and bench.py's behaviour mix - Qwen3SessionMoe (config/s2s-models/Qwen3Moe's architecture: hidden 256, 8 layers,
SwiGLU experts in every layer, injection layers 0-3, no cross attention) in split3 and bf16, and Qwen3SessionMulti in split3,
which is bench.py's ``session_split3_b1024`` leg, in the SAME process: the two split3 engines are timed in alternating
blocks of ``--steps`` steps, ``--rounds`` times, after ``--warmup`` untimed steps each, every step between device events.
Evaluation path: ``--users`` users x ``--beams`` beams, history 100 items, 4 new tokens, cached decode in fp32 -
Qwen3SessionMoe (prompts with sessions of 4 items) next to Qwen3Multi, which is bench.py's ``decode_bs256_beams20`` leg,
alternating in the same way, every search between device events after 3 untimed ones.
Every figure is the median with the smallest and largest sample.  Prints one JSON line.

  python tools/bench_session_moe.py --batch 1024 --steps 10 --warmup 3 --rounds 2
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3SessionMoeConfig, synthetic_config  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402

ITEMS, MIX = 101, [0.7, 0.25, 0.05]


def session_moe_config() -> Qwen3SessionMoeConfig:
    return Qwen3SessionMoeConfig(vocab_size=synthetic.vocab_size(256, 3), num_behavior=3, n_positions=ITEMS, num_positions=5,
                                 model_max_length=1024,
                                 behavior_maps={str(k): v for k, v in synthetic.behavior_maps(256, 3).items()})


def timed(fn, n):
    out = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def summary(ms, per):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return dict(ms=round(med, 2), ms_min=round(ms[0], 2), ms_max=round(ms[-1], 2), per_s=round(per / (med * 1e-3), 1),
                samples=len(ms))


def alternate(legs: dict, warmup: int, steps: int, rounds: int, per: int) -> dict:
    """legs: name -> callable.  Every leg warmed, then ``rounds`` alternating blocks of ``steps`` timed calls each."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k] += timed(fn, steps)
    return {k: summary(v, per) for k, v in ms.items()}


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
        raise SystemExit("bench_session_moe.py measures on the GPU; there is none")
    out = dict(metric="Qwen3SessionMoe train step and beam search next to session_split3_b1024 / decode_bs256_beams20",
               device=torch.cuda.get_device_name(0), batch=args.batch, tokens=ITEMS * 5)
    batch = synthetic.make_batch(args.batch, ITEMS, 256, 3, seed=7, behavior_probs=MIX, session_mean=4.0)
    moe = Engine(session_moe_config(), temperature=0.7, variant="qwen3_session_moe")
    multi = Engine(synthetic_config(n_positions=ITEMS), temperature=0.7, variant="session")
    for e in (moe, multi):
        e.init_weights(seed=0)
    out["train_step"] = alternate({"qwen3_session_moe_split3": lambda: moe.train_step(batch, 5e-4),
                                   "session_split3_b1024": lambda: multi.train_step(batch, 5e-4)},
                                  args.warmup, args.steps, args.rounds, args.batch)
    moe.check_inputs()
    del moe, multi
    torch.cuda.empty_cache()
    moe16 = Engine(session_moe_config(), temperature=0.7, variant="qwen3_session_moe", dtype="bf16")
    moe16.init_weights(seed=0)
    out["train_step"].update(alternate({"qwen3_session_moe_bf16": lambda: moe16.train_step(batch, 5e-4)},
                                       args.warmup, args.steps, args.rounds, args.batch))
    del moe16
    torch.cuda.empty_cache()
    print(json.dumps(out["train_step"]), file=sys.stderr, flush=True)

    his = ITEMS - 1
    cat = synthetic.make_catalogue(20000, 256, seed=3)
    trie = ItemTrie(synthetic.item_tokens(cat, 2, 256).tolist())
    ev = synthetic.make_eval_batch(args.users, his, cat, 2, 256, 3, min_his=his, seed=5, behavior_probs=MIX)
    evs = synthetic.make_eval_batch(args.users, his, cat, 2, 256, 3, min_his=his, seed=5, behavior_probs=MIX, session_mean=4.0)
    moe = Engine(session_moe_config(), temperature=0.7, variant="qwen3_session_moe")
    multi = Engine(synthetic_config(n_positions=ITEMS), temperature=0.7)
    for e in (moe, multi):
        e.init_weights(seed=0)
    out["beam_search"] = alternate(
        {"qwen3_session_moe": lambda: beam_search(moe, evs["input_ids"], evs["attention_mask"], None, trie, args.beams, 4,
                                                  session_ids=evs["session_ids"],
                                                  extended_session_ids=evs["extended_session_ids"]),
         "decode_bs256_beams20": lambda: beam_search(multi, ev["input_ids"], ev["attention_mask"], ev["actions"], trie,
                                                     args.beams, 4)},
        3, max(2, args.steps // 2), args.rounds, args.users)
    out["beam_search"].update(users=args.users, beams=args.beams, history_items=his)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
