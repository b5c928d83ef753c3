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

``--pack_rows both`` times the padded and the packed form (``TIGER.forward(packed=True)``, the encoder side without the padding
tokens) on the same batches in one process, alternating batch by batch, and the same for the evaluation; per form it reports the step
time, the peak memory of a step, the encoder tokens per batch, and one encoder layer's self attention (forward + backward, the fused
kernels alone) at the first timed batch's lengths.  ``on`` times the packed form alone.  The rows then go to
profiles/tiger_packed_bench.json.

  python tools/bench_tiger_smb.py --batch 256,1024 --max_his_len 20,100 --steps 8 --warmup 3
  python tools/bench_tiger_smb.py --pack_rows both
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

from gamer_amd import ops, synthetic, t5_mb_data, tiger  # noqa: E402
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


def forms(a):
    return {"off": ("padded",), "on": ("packed",), "both": ("padded", "packed")}[a.pack_rows]


def pack_kw(form, mask):
    """the lengths from the collated mask on the host, as train_tiger.run takes them"""
    return dict(packed=True, lengths=tiger.packed_lengths(mask)) if form == "packed" else {}


def bench_attention(lengths, S, form, a, h=SHIPPED["num_heads"], d=SHIPPED["d_kv"]):
    """one encoder layer's self attention, forward + backward with the bias and dropout 0.1, the fused kernels alone: median ms"""
    B, I = lengths.numel(), h * d
    off = ops.T5Offsets.from_lengths(lengths, DEV)
    T = off.total if form == "packed" else B * S
    long = S > ops.T5_MAX_S
    qkv, d_o = torch.randn(T, 3 * I, device=DEV) * 0.3, torch.randn(T, I, device=DEV)
    dqkv, o, lse = torch.empty_like(qkv), torch.empty(T, I, device=DEV), torch.empty(h * T, device=DEV)
    rel, slabs = torch.randn(h, 2 * S - 1, device=DEV), torch.empty(ops.t5_n_slab(B, h), h, 2 * S - 1, device=DEV)
    keep = (torch.arange(S)[None, :] < lengths[:, None]).to(torch.uint8).to(DEV)
    q, k, v = qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:]
    dq, dk, dv = dqkv[:, :I], dqkv[:, I:2 * I], dqkv[:, 2 * I:]
    if form == "packed":
        fwd, bwd = (ops.t5_attn_long_packed_fwd, ops.t5_attn_long_packed_bwd) if long else (ops.t5_attn_packed_fwd, ops.t5_attn_packed_bwd)
        where = (off, off)
    else:
        fwd, bwd = (ops.t5_attn_long_fwd, ops.t5_attn_long_bwd) if long else (ops.t5_attn_fwd, ops.t5_attn_bwd)
        where = (keep,)

    def run():
        fwd(q, k, v, rel, *where, B, S, S, h, d, False, 0.1, 3, o, lse)
        bwd(q, k, v, rel, *where, B, S, S, h, d, False, 0.1, 3, d_o, lse, dq, dk, dv, slabs)
    for _ in range(a.warmup):
        run()
    return round(statistics.median(event_ms(run) for _ in range(a.steps)), 3)


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

    def step(b, form):
        for p in model.parameters():
            p.grad = None
        loss, _ = model(b["input_ids"].to(DEV), b["attention_mask"].to(DEV), labels=b["labels"].to(DEV), **pack_kw(form, b["attention_mask"]))
        loss.backward()
    for b in batches[:a.warmup]:
        for form in forms(a):
            step(b, form)
    ts, peak = {f: [] for f in forms(a)}, {f: 0 for f in forms(a)}
    for b in batches[a.warmup:]:                                              # the forms alternate on the same batch
        for form in forms(a):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ts[form].append(event_ms(lambda: step(b, form)))
            peak[form] = max(peak[form], torch.cuda.max_memory_allocated())
    widths = [int(b["input_ids"].shape[1]) for b in batches[a.warmup:]]
    common = dict(widths=[min(widths), max(widths)], padding_share=round(padding, 4), padding_batches=len(pad), collate_ms=round(collate_ms, 3))
    if a.pack_rows == "off":
        ms = statistics.median(ts["padded"])
        return dict(step_ms=round(ms, 3), sequences_per_s=round(B / ms * 1e3, 1), **common)
    timed = batches[a.warmup:]
    tokens = dict(padded=round(sum(b["attention_mask"].numel() for b in timed) / len(timed), 1),
                  packed=round(sum(int(b["attention_mask"].sum()) for b in timed) / len(timed), 1))
    first = timed[0]["attention_mask"]
    out = dict(common, encoder_tokens_per_batch=tokens)
    for form in forms(a):
        ms = statistics.median(ts[form])
        out[form] = dict(step_ms=round(ms, 3), sequences_per_s=round(B / ms * 1e3, 1), peak_memory_mb=round(peak[form] / 2 ** 20, 1),
                         self_attention_fwd_bwd_ms=bench_attention(tiger.packed_lengths(first), first.shape[1], form, a))
    return out


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
        run = lambda form: tiger.beam_search(model, ids, am, trie, a.beams, data.sole_item_len, decoder_prefix=prefix,
                                             **pack_kw(form, inputs["attention_mask"]))
        ts = {f: [] for f in forms(a)}
        for form in forms(a):
            run(form)
        for _ in range(max(2, a.steps // 2)):                                     # the forms alternate
            for form in forms(a):
                ts[form].append(event_ms(lambda: run(form)))
        out[b] = dict(users=n, width=int(ids.shape[1]))
        if a.pack_rows == "off":
            ms = statistics.median(ts["padded"])
            out[b].update(beam_ms=round(ms, 2), users_per_s=round(n / ms * 1e3, 1))
        else:
            out[b]["encoder_tokens"] = dict(padded=int(am.numel()), packed=int(am.sum()))
            for form in forms(a):
                ms = statistics.median(ts[form])
                out[b][form] = dict(beam_ms=round(ms, 2), users_per_s=round(n / ms * 1e3, 1))
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
    ap.add_argument("--pack_rows", choices=("off", "on", "both"), default="off")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "tiger_smb_bench.json" if a.pack_rows == "off" else "tiger_packed_bench.json")
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
