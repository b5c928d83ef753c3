#!/usr/bin/env python3
"""TIGER on the SMB data on one GPU: train step on batches the per-interaction sampler draws, their padding share, and the
per-behaviour evaluation.

A synthetic SMB dataset with long users (``synthetic.write_smb_dataset``: ``--users`` users of 3 - 40 sessions of 1 - 6 interactions,
a 256-entry codebook) is read by t5_mb_data.T5SMBData at the T5 vocabulary; the model is the shipped config (d_model 128, 6 heads of
64, 4 + 4 layers, d_ff 1024, dropout 0.1) resized to it.  Per ``--max_his_len`` and ``--batch``:
  * train step (forward with labels + backward) on ``--steps`` different batches of ``smb_explicit`` samples in a seeded shuffle,
    as train_tiger.run draws them: median time, sequences/s, the batches' widths;
  * the share of the encoder tokens of those batches that is padding (1 - attention_mask.mean()), over ``--pad_batches`` batches:
    the per-interaction sampler mixes a user's first sessions (short or empty histories) with full ones;
  * the collator's time per batch on the host;
and per ``--max_his_len`` and behaviour: test_SMB_decoder's search at ``--eval_users`` users x ``--beams`` beams: users/s.
Medians of device-event timings after ``--warmup``.  Prints one JSON line per row and writes them all to ``--out``.

  python tools/bench_tiger_smb.py --batch 256,1024 --max_his_len 20,100 --steps 8 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import synthetic, t5_mb_data, tiger  # noqa: E402
from gamer_amd.decode import ItemTrie  # noqa: E402

DEV = "cuda:0"
SHIPPED = dict(d_model=128, d_kv=64, d_ff=1024, num_layers=4, num_decoder_layers=4, num_heads=6, dropout_rate=0.1, vocab_size=32128)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_steps(model, samples, coll, B, a):
    order = np.random.RandomState(0).permutation(len(samples))
    chunks = [order[i:i + B] for i in range(0, len(order) - B + 1, B)]
    if len(chunks) < a.warmup + a.steps:
        raise SystemExit(f"{len(samples)} samples give {len(chunks)} batches of {B}; raise --users")
    t0 = time.perf_counter()
    batches = [coll(samples, c) for c in chunks[:a.warmup + a.steps]]
    collate_ms = (time.perf_counter() - t0) / len(batches) * 1e3
    pad = [coll(samples, c)["attention_mask"] for c in chunks[:a.pad_batches]]
    padding = 1.0 - sum(int(m.sum()) for m in pad) / sum(m.numel() for m in pad)
    model.train()

    def step(b):
        for p in model.parameters():
            p.grad = None
        loss, _ = model(b["input_ids"].to(DEV), b["attention_mask"].to(DEV), labels=b["labels"].to(DEV))
        loss.backward()
    for b in batches[:a.warmup]:
        step(b)
    ts = [event_ms(lambda b=b: step(b)) for b in batches[a.warmup:]]
    ms = statistics.median(ts)
    widths = [int(b["input_ids"].shape[1]) for b in batches[a.warmup:]]
    return dict(step_ms=round(ms, 3), sequences_per_s=round(B / ms * 1e3, 1), widths=[min(widths), max(widths)],
                padding_share=round(padding, 4), padding_batches=len(pad), collate_ms=round(collate_ms, 3))


def bench_eval(model, data, coll, max_his_len, a):
    base = data.samples("test", max_his_len)
    out = {}
    for b in data.behaviors:
        sub = base.filter_by_behavior(b)
        n = min(len(sub), a.eval_users)
        inputs, _ = coll.test(sub, range(n))
        ids, am = inputs["input_ids"].to(DEV), inputs["attention_mask"].to(DEV)
        trie = ItemTrie(data.trie_sequences(b, 0), device=DEV, pad_token_id=0)
        prefix = torch.tensor([0, data.behavior_token_ids[b]])
        run = lambda: tiger.beam_search(model, ids, am, trie, a.beams, data.sole_item_len, decoder_prefix=prefix)
        run()
        ms = statistics.median(event_ms(run) for _ in range(max(2, a.steps // 2)))
        out[b] = dict(users=n, width=int(ids.shape[1]), beam_ms=round(ms, 2), users_per_s=round(n / ms * 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="256,1024")
    ap.add_argument("--max_his_len", default="20,100")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pad_batches", type=int, default=30)
    ap.add_argument("--users", type=int, default=1200)
    ap.add_argument("--items", type=int, default=5000)
    ap.add_argument("--eval_users", type=int, default=256)
    ap.add_argument("--beams", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tiger_smb_bench.json"))
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_smb_dataset(tmp, "Bench", n_users=a.users, n_items=a.items, codebook=256, max_sessions=40, max_per_session=6,
                                    min_sessions=3, seed=0)
        data = t5_mb_data.T5SMBData(tmp, "Bench", "smb_explicit")
        coll = t5_mb_data.EncDecCollator(1024, data.token_count)
        torch.manual_seed(0)
        model = tiger.TIGER(tiger.TigerConfig(**SHIPPED))
        model.resize_token_embeddings(data.vocab_size)
        model.to(DEV)
        for H in (int(x) for x in a.max_his_len.split(",")):
            samples = data.samples("train", H)
            hist = samples.n_history // data.token_count
            for B in (int(x) for x in a.batch.split(",")):
                row = dict(kind="train_step", task="smb_explicit", max_his_len=H, batch=B, samples=len(samples), vocabulary=data.vocab_size,
                           mean_history_items=round(float(hist.mean()), 2), **bench_steps(model, samples, coll, B, a))
                rows.append(row)
                print(json.dumps(row), flush=True)
            row = dict(kind="evaluation", max_his_len=H, beams=a.beams, behaviors=bench_eval(model, data, coll, H, a))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
