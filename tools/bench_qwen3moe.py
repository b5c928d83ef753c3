#!/usr/bin/env python3
"""Train-step time of Qwen3Moe next to Qwen3Multi (same process, same box), and its beam-search throughput.

Qwen3Moe: the shipped architecture of config/s2s-models/Qwen3Moe (hidden 256, 8 layers, SwiGLU experts in every layer,
injection layers 0-3, no cross attention) on the synthetic vocabulary with behaviour tokens; Qwen3Multi: the shipped one.  The
step is ``Engine.train_step`` on synthetic batches of ``--batch`` sequences at two lengths: the MB default ``max_his_len``
= 20 (21 items, 105 tokens) and 101 items (505 tokens); Qwen3Moe in split3 and bf16, Qwen3Multi in split3, medians of
``--steps`` device-event timings after ``--warmup``.  Beam search: ``--users`` users x ``--beams`` beams, history 20 items,
4 new tokens, cached decode (fp32).  Prints one JSON line.

  python tools/bench_qwen3moe.py --batch 1024 --steps 10 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeConfig, synthetic_config  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402


def moe_config(items: int) -> Qwen3MoeConfig:
    return Qwen3MoeConfig(vocab_size=synthetic.vocab_size(256, 3), num_behavior=3, n_positions=items,
                          behavior_maps={str(k): v for k, v in synthetic.behavior_maps(256, 3).items()})


def step_ms(eng, batch, steps, warmup):
    times = []
    for i in range(warmup + steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        eng.train_step(batch, 5e-4)
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(s.elapsed_time(e))
    times.sort()
    return round(times[len(times) // 2], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    args = ap.parse_args()
    out = dict(metric="Qwen3Moe train step (ms) next to Qwen3Multi, and beam-search users/s", batch=args.batch, steps={})
    for items in (21, 101):
        batch = synthetic.make_batch(args.batch, items, 256, 3, seed=7, behavior_probs=[0.7, 0.25, 0.05])
        for name, make in (("qwen3moe_split3", lambda: Engine(moe_config(items), temperature=0.7, variant="qwen3moe")),
                           ("qwen3moe_bf16", lambda: Engine(moe_config(items), temperature=0.7, variant="qwen3moe",
                                                            dtype="bf16")),
                           ("qwen3multi_split3", lambda: Engine(synthetic_config(n_positions=items), temperature=0.7))):
            eng = make()
            eng.init_weights(seed=0)
            out["steps"][f"{name}_seq{items * 5}"] = step_ms(eng, batch, args.steps, args.warmup)
            print(json.dumps({name: out["steps"][f"{name}_seq{items * 5}"], "seq": items * 5}), file=sys.stderr, flush=True)
            del eng
            torch.cuda.empty_cache()
    eng = Engine(moe_config(101), temperature=0.7, variant="qwen3moe")
    eng.init_weights(seed=0)
    cat = synthetic.make_catalogue(20000, 256, seed=3)
    trie = ItemTrie(synthetic.item_tokens(cat, 2, 256).tolist())
    ev = synthetic.make_eval_batch(args.users, 20, cat, 2, 256, 3, min_his=20, seed=5, behavior_probs=[0.7, 0.25, 0.05])
    run = lambda: beam_search(eng, ev["input_ids"], ev["attention_mask"], None, trie, args.beams, 4)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    out["beam_search"] = dict(users_per_s=round(args.users / dt, 1), ms_per_batch=round(dt * 1e3, 2), users=args.users,
                              beams=args.beams, history_items=20)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
