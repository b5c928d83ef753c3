#!/usr/bin/env python3
"""GRU4Rec on one GPU: train step, the recurrence against torch.nn.GRU, and top-10 ranking.

  * train step (``calculate_loss`` + backward, no optimizer) of the reference's shipped config (E 64, H 128, 1 layer,
    dropout 0.3) at batch ``--batch`` x ``--seq`` (full-length rows) on synthetic catalogues of ``--items`` items, with the
    recurrence's share (gamer_gru_fwd + the input GEMM, gamer_gru_bwd + its three GEMMs) timed on its own;
  * the GRU layer alone, forward + backward with the weight and input gradients: gamer_gru_fwd / _bwd and their GEMMs against
    torch.nn.GRU(bias=False) in fp32 (MIOpen) on the same tensors in the same process;
  * evaluation: users/s of top-10 full ranking (``full_sort_topk``) at ``--rank_items`` items.
Medians of ``--steps`` device-event timings after ``--warmup``.  Prints one JSON line.

  python tools/bench_gru4rec.py --batch 4096 --steps 10 --warmup 3 --items 16384,100000,1000000
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig, _GRULayerFn  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seq", type=int, default=20)
    ap.add_argument("--items", default="16384,100000,1000000")
    ap.add_argument("--rank_items", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, L = a.batch, a.seq
    cfg = GRU4RecConfig()
    E, H = cfg.embedding_size, cfg.hidden_size
    out = dict(metric="gru4rec", batch=B, seq=L, embedding_size=E, hidden_size=H, steps=a.steps, warmup=a.warmup)
    g = torch.Generator().manual_seed(0)

    # ---- train step -------------------------------------------------------------------------------------------------------
    for V in [int(v) for v in a.items.split(",")]:
        torch.manual_seed(0)
        model = GRU4Rec(cfg, V - 1).to(DEV).train()
        inter = dict(inputs=torch.randint(1, V, (B, L), generator=g).to(DEV), seq_len=torch.full((B,), L, device=DEV),
                     target=torch.randint(1, V, (B,), generator=g).to(DEV))

        def step():
            model.zero_grad(set_to_none=True)
            model.calculate_loss(inter).backward()
        out[f"train_step_ms_{V}"] = round(timed(step, a.steps, a.warmup), 3)
        del model
        torch.cuda.empty_cache()

    # ---- the GRU layer alone against torch.nn.GRU (MIOpen, fp32) ------------------------------------------------------------
    x = torch.randn(B, L, E, generator=g).to(DEV)
    dy = torch.randn(B, L, H, generator=g).to(DEV)
    ref = torch.nn.GRU(E, H, bias=False, batch_first=True).to(DEV)
    w_ih, w_hh = ref.weight_ih_l0.detach().clone().requires_grad_(True), ref.weight_hh_l0.detach().clone().requires_grad_(True)
    lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
    xg = x.clone().requires_grad_(True)

    def ours_fwd():
        with torch.no_grad():
            _GRULayerFn.apply(x, w_ih, w_hh, lens, False)

    def ours():
        xg.grad = w_ih.grad = w_hh.grad = None
        _GRULayerFn.apply(xg, w_ih, w_hh, lens, True).backward(dy)

    def torch_fwd():
        with torch.no_grad():
            ref(x)

    def torch_gru():
        xg.grad = None
        ref.zero_grad(set_to_none=True)
        ref(xg)[0].backward(dy)
    out["gru_fwd_ms"] = round(timed(ours_fwd, a.steps, a.warmup), 3)
    out["gru_fwd_bwd_ms"] = round(timed(ours, a.steps, a.warmup), 3)
    out["torch_gru_fwd_ms"] = round(timed(torch_fwd, a.steps, a.warmup), 3)
    out["torch_gru_fwd_bwd_ms"] = round(timed(torch_gru, a.steps, a.warmup), 3)
    out["gru_speedup_vs_torch"] = round(out["torch_gru_fwd_bwd_ms"] / out["gru_fwd_bwd_ms"], 2)

    # ---- evaluation: top-10 ranking ---------------------------------------------------------------------------------------
    V = a.rank_items
    torch.manual_seed(0)
    model = GRU4Rec(cfg, V - 1).to(DEV).eval()
    inter = dict(inputs=torch.randint(1, V, (B, L), generator=g).to(DEV), seq_len=torch.randint(1, L + 1, (B,), generator=g).to(DEV))
    ms = timed(lambda: model.full_sort_topk(inter, 10), a.steps, a.warmup)
    out[f"rank_top10_users_per_s_{V}"] = round(B / (ms / 1e3))
    out["rank_top10_ms"] = round(ms, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
