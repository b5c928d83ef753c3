#!/usr/bin/env python3
"""SASRec on one GPU: train step, the catalogue head against a materialised composition, and top-10 ranking.

  * train step (``calculate_loss`` + backward + ``gamer_adamw``-free: forward and backward only) of the reference's shipped
    config (hidden 128, 2 layers, 2 heads, inner 256, dropout 0.5) at batch ``--batch`` x 20 on synthetic catalogues;
  * the head alone at R = ``--batch`` rows, H = 128: gamer_catalog_ce_fwd + _bwd against torch.matmul + F.cross_entropy
    + the two gradient GEMMs (autograd) in the same process, time and peak allocated memory;
  * evaluation: users/s of top-10 full ranking (gamer_catalog_topk) against materialised scores + torch.topk.
Medians of ``--steps`` device-event timings after ``--warmup``.  Prints one JSON line.

  python tools/bench_sasrec.py --batch 4096 --steps 10 --warmup 3 --items 16384,100000,1000000
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import ops, rec_common  # noqa: E402
from gamer_amd.sasrec import SASRec, SASRecConfig  # noqa: E402

DEV = "cuda:0"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def peak(fn, reset):
    fn()
    reset()                                           # (drop the gradients of the warm-up call before the baseline)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seq", type=int, default=20)
    ap.add_argument("--items", default="16384,100000,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=4096)
    a = ap.parse_args()
    R, S = a.batch, a.seq
    out = dict(batch=R, seq=S, hidden=128)
    for V in [int(x) for x in a.items.split(",")]:
        key = f"items_{V}"
        g = torch.Generator().manual_seed(V)
        torch.manual_seed(0)
        model = SASRec(SASRecConfig(), V, S).to(DEV).train()
        inter = dict(inputs=torch.randint(1, V + 1, (R, S), generator=g).to(DEV), seq_len=torch.full((R,), S, device=DEV),
                     target=torch.randint(1, V + 1, (R,), generator=g).to(DEV))

        def step():
            model.zero_grad(set_to_none=True)
            model.calculate_loss(inter).backward()
        ms = timed(step, a.steps, a.warmup)
        r = dict(step_ms=round(ms, 3), sequences_per_s=round(R / ms * 1e3, 1), step_peak_mib=round(peak(step, lambda: model.zero_grad(set_to_none=True)), 1))
        # the head alone
        h = (torch.randn(R, 128, generator=g) * 0.3).to(DEV).requires_grad_(True)
        E = model.item_embedding.weight.detach().clone().requires_grad_(True)
        rows = torch.arange(R, device=DEV)

        def fused():
            E.grad = None
            h.grad = None
            rec_common.CatalogCEFn.apply(h, rows, E, inter["target"]).backward()

        def drop():
            E.grad = None
            h.grad = None

        def materialised():
            E.grad = None
            h.grad = None
            F.cross_entropy(torch.matmul(h, E.t()), inter["target"]).backward()
        r["head_fused_ms"] = round(timed(fused, a.steps, a.warmup), 3)
        r["head_fused_peak_mib"] = round(peak(fused, drop), 1)
        try:
            r["head_materialised_ms"] = round(timed(materialised, a.steps, a.warmup), 3)
            r["head_materialised_peak_mib"] = round(peak(materialised, drop), 1)
        except torch.cuda.OutOfMemoryError:
            r["head_materialised_ms"] = "out of memory"
        # evaluation: top-10 over the whole table
        U = a.eval_users
        hu = (torch.randn(U, 128, generator=g) * 0.3).to(DEV)
        Ed = E.detach()
        t_fused = timed(lambda: ops.catalog_topk(hu, Ed, 10), a.steps, a.warmup)

        def topk_mat():
            torch.topk(torch.matmul(hu, Ed.t()), 10, dim=1)
        t_mat = timed(topk_mat, a.steps, a.warmup)
        r["topk_fused_users_per_s"] = round(U / t_fused * 1e3, 1)
        r["topk_materialised_users_per_s"] = round(U / t_mat * 1e3, 1)
        out[key] = r
        del model, E, h, hu, Ed
        torch.cuda.empty_cache()
    # the item-embedding gradient at the step's token count: uniform ids against a skewed batch (one item in a quarter of the
    # tokens, the rest Zipf(1.2)): gamer_embedding_bwd_large ranks a segment of n tokens in n steps per token
    g = torch.Generator().manual_seed(9)
    T, V = R * S, 1_000_000
    dx = torch.randn(T, 128, device=DEV)
    dW = torch.zeros(V + 1, 128, device=DEV)
    uni = torch.randint(1, V + 1, (T,), generator=g).to(DEV)
    zipf = torch.from_numpy(__import__("numpy").random.default_rng(9).zipf(1.2, T) % V + 1).to(DEV)
    zipf[::4] = 7
    for name, ids in (("uniform", uni), ("skewed", zipf)):
        out[f"emb_grad_{name}_ms"] = round(timed(lambda: ops.embedding_bwd_large(ids, dx, 0, dW), a.steps, a.warmup), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
