#!/usr/bin/env python3
"""Throughput of the plain Qwen3 baseline (--backbone Qwen3, Qwen3-Light, V = 1041): the train step at batch 1024 x 505
tokens (fp32 split3 and bf16) and trie-constrained beam search at 256 users x 20 beams, plus Qwen3Multi's step on the same
box for comparison; and the same three numbers for the Qwen3Session baseline (--backbone Qwen3Session: sessions of mean
4 items, session-wise masks, RoPE on the extended session ids), keys prefixed ``session_``.

  python tools/bench_qwen3.py [--B 1024] [--steps 10] [--warmup 3] [--users 256] [--beams 20] [--no-multi] [--no-session]

Prints one JSON line.  The step is ``Engine.train_step`` (forward + backward + clip + AdamW), timed with a device
synchronisation around ``--steps`` steps after ``--warmup`` untimed ones.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gamer_amd import synthetic  # noqa: E402
from gamer_amd.config import Qwen3Config, Qwen3SessionConfig, synthetic_config  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402


def time_steps(eng, batch, steps, warmup):
    dev = eng.device
    b = {k: v.to(dev) for k, v in batch.items()}
    for _ in range(warmup):
        eng.train_step(b, lr=1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = eng.train_step(b, lr=1e-4)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dict(ms_per_step=dt * 1e3, sequences_per_s=batch["input_ids"].shape[0] / dt, loss=float(loss))


def release():
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--items", type=int, default=101, help="items per sequence (x 5 tokens)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    ap.add_argument("--his", type=int, default=100)
    ap.add_argument("--catalogue", type=int, default=20000)
    ap.add_argument("--no-multi", dest="multi", action="store_false")
    ap.add_argument("--no-session", dest="session", action="store_false")
    args = ap.parse_args()
    V = synthetic.vocab_size(256, 3)
    cfg = Qwen3Config(vocab_size=V, pad_token_id=synthetic.PAD_ID)
    batch = synthetic.make_batch(args.B, args.items, 256, 3, seed=1)
    cat = synthetic.make_catalogue(args.catalogue, 256, seed=3)
    tb = 2
    trie = ItemTrie(synthetic.item_tokens(cat, tb, 256).tolist())
    out = dict(metric="Qwen3 baseline train step and evaluation", box=torch.cuda.get_device_name(0),
               workload=f"B = {args.B} x S = {batch['input_ids'].shape[1]}, Qwen3-Light, V = {V}")
    for name, kw in (("step_f32_split3", dict(dtype="f32")), ("step_bf16", dict(dtype="bf16"))):
        eng = Engine(cfg, temperature=0.7, variant="qwen3", **kw)
        eng.init_weights(seed=0)
        out[name] = time_steps(eng, batch, args.steps, args.warmup)
        eng = None
        release()
    if args.session:
        scfg = Qwen3SessionConfig(vocab_size=V, pad_token_id=synthetic.PAD_ID, num_positions=5, model_max_length=1024)
        sbatch = synthetic.make_batch(args.B, args.items, 256, 3, seed=1, session_mean=4.0)
        for name, kw in (("session_step_f32_split3", dict(dtype="f32")), ("session_step_bf16", dict(dtype="bf16"))):
            eng = Engine(scfg, temperature=0.7, variant="qwen3_session", **kw)
            eng.init_weights(seed=0)
            out[name] = time_steps(eng, sbatch, args.steps, args.warmup)
            eng = None
            release()
        eng = Engine(scfg, temperature=0.7, variant="qwen3_session")
        eng.init_weights(seed=0)
        eb = synthetic.make_eval_batch(args.users, args.his, cat, tb, 256, 3, min_his=70, seed=5, session_mean=4.0)
        out["session_decode"] = time_decode(eng, eb, trie, args, session_ids=eb["session_ids"],
                                            extended_session_ids=eb["extended_session_ids"])
        eng = None
        release()
    if args.multi:
        eng = Engine(synthetic_config(), temperature=0.7)
        eng.init_weights(seed=0)
        out["qwen3multi_step_f32_split3"] = time_steps(eng, batch, args.steps, args.warmup)
        eng = None
        release()
    # evaluation: prompts of history `his` items + the target behaviour token, left padded; beams constrained to one behaviour
    eng = Engine(cfg, temperature=0.7, variant="qwen3")
    eng.init_weights(seed=0)
    eb = synthetic.make_eval_batch(args.users, args.his, cat, tb, 256, 3, min_his=70, seed=5)
    out["decode"] = time_decode(eng, eb, trie, args)
    print(json.dumps(out))


def time_decode(eng, eb, trie, args, **skw):
    run = lambda: beam_search(eng, eb["input_ids"], eb["attention_mask"], None, trie, args.beams, 4, **skw)   # noqa: E731
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters = 3
    for _ in range(iters):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return dict(users_per_s=args.users / dt, ms_per_batch=dt * 1e3,
                workload=f"{args.users} users x {args.beams} beams, history up to {args.his} items, 4 new tokens, "
                         f"catalogue {args.catalogue} items, fp32 split3, K/V cache")


if __name__ == "__main__":
    main()
