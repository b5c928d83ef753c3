#!/usr/bin/env python3
"""The RQ-VAE item tokenizer on one GPU: the train step of the shipped configuration and where its time goes, and tokenisation.

  * train step (forward, ``compute_loss``, backward, AdamW) at batch ``--batch`` x 768 through layers [2048, 1024, 512, 256, 128,
    64], e_dim 32, codebooks [256] * 4, sk_epsilons [0, 0, 0, 0.003], alpha 0.2, beta 1e-4 on synthetic embeddings;
  * the same step by part: the two MLPs forward + backward; the quantiser (gamer_rvq_fwd + gamer_rvq_bwd on all four levels by
    argmin) against the same maths as torch ops with autograd on the same GPU (what the reference launches per level: distance
    matrix, argmin, gather, two MSE losses, the straight-through sum); Sinkhorn (centring + 50 fp64 iterations + argmax on a
    [batch, 256] matrix); the host sampling of positives (the device-to-host copy of the indices + ``random.choice``);
  * tokenisation: items/s of ``get_indices(use_sk=False)`` over ``--items`` items in batches of 1024.
Medians of ``--steps`` timings after ``--warmup`` (device events; a host clock around a synchronise for the host part).  Prints
one JSON line.

  python tools/bench_rqvae.py --batch 1024 --steps 8 --warmup 3 --items 100000
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import ops, rqvae  # noqa: E402
from gamer_amd.rqvae import RQVAE  # noqa: E402

DEV = "cuda:0"
IN_DIM, LAYERS, E_DIM, KS = 768, [2048, 1024, 512, 256, 128, 64], 32, [256] * 4


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


def host_timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def torch_quantiser(z, Es):
    """the reference's per-level composition as device torch ops, forward + backward"""
    z = z.detach().requires_grad_(True)
    res, xq, losses = z, 0, []
    for E in Es:
        d = torch.sum(res ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1, keepdim=True).t() - 2 * torch.matmul(res, E.t())
        e = F.embedding(torch.argmin(d, dim=-1), E)
        losses.append(F.mse_loss(e, res.detach()) + 0.25 * F.mse_loss(e.detach(), res))
        x_res = res + (e - res).detach()
        res, xq = res - x_res, xq + x_res
    (torch.stack(losses).mean() + xq.sum()).backward()
    return xq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=100000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rqvae needs the GPU"
    B = a.batch
    torch.manual_seed(0)
    random.seed(0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, IN_DIM, generator=g).to(DEV)
    cf = torch.randn(B, E_DIM, generator=g).numpy()
    model = RQVAE(in_dim=IN_DIM, num_emb_list=KS, e_dim=E_DIM, layers=LAYERS, sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50,
                  alpha=0.2, beta=1e-4, cf_embedding=cf, cluster_backend="sklearn").to(DEV).train()
    for q in model.rq.vq_layers:                           # codes of the latents' size, so that the levels are not degenerate
        q.embedding.weight.data.normal_(0.0, 0.05)
    labels = {str(l): [j % 10 for j in range(k)] for l, k in enumerate(KS)}
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    rows = torch.arange(B)

    def step():
        opt.zero_grad()
        out, rq_loss, _, dense = model(x, labels)
        loss = model.compute_loss(out, rq_loss, rows, dense, xs=x)[0]
        loss.backward()
        opt.step()

    res = dict(batch=B, steps=a.steps, warmup=a.warmup)
    res["step_ms"] = timed(step, a.steps, a.warmup)

    # the parts
    def mlps():
        xi = x.clone().requires_grad_(True)
        z = model.encoder(xi)
        out = model.decoder(z)
        out.backward(torch.ones_like(out))
    res["mlp_fwd_bwd_ms"] = timed(mlps, a.steps, a.warmup)

    z = model.encoder(x).detach()
    Es = [q.embedding.weight.detach().clone().requires_grad_(True) for q in model.rq.vq_layers]
    off = model.rq._offsets()

    def kernels():
        zi = z.clone().requires_grad_(True)
        E = torch.cat(Es)
        xq, lv, _ = rqvae.RVQFn.apply(zi, E, off, [0.0] * 4, 50)
        (lv.mean() + xq.sum()).backward()
    res["quantiser_kernels_ms"] = timed(kernels, a.steps, a.warmup)
    res["quantiser_torch_ms"] = timed(lambda: torch_quantiser(z, Es), a.steps, a.warmup)

    # the bare launches, without autograd's bookkeeping and the torch.cat
    E = torch.cat([e.detach() for e in Es])
    f32 = dict(dtype=torch.float32, device=DEV)
    idx, xq, rs = torch.empty(B, 4, dtype=torch.int32, device=DEV), torch.empty(B, E_DIM, **f32), torch.empty(B, E_DIM, **f32)
    rl, sums, dz, dE = torch.empty(4, B, E_DIM, **f32), torch.zeros(4, **f32), torch.empty(B, E_DIM, **f32), torch.empty_like(E)
    gl, gx = torch.ones(4, **f32), torch.ones(B, E_DIM, **f32)
    res["rvq_fwd_launch_ms"] = timed(lambda: ops.rvq_fwd(z, E, off, [0] * 4, 0, 4, idx, xq, rs, rl, None, sums), a.steps, a.warmup)
    res["rvq_bwd_launch_ms"] = timed(lambda: ops.rvq_bwd(idx, rl, E, off, gx, gl, 0.25, dz, dE), a.steps, a.warmup)

    d = torch.rand(B, 256, device=DEV)
    res["sinkhorn_ms"] = timed(lambda: rqvae.sinkhorn_indices(d, 0.003, 50), a.steps, a.warmup)

    ids = torch.randint(0, 256, (B, 4), device=DEV)

    def sample():
        host = ids.cpu().tolist()
        for l in range(4):
            rqvae.sample_positives([r[l] for r in host], labels[str(l)], l)
    res["positives_host_ms"] = host_timed(sample, a.steps, a.warmup)

    # tokenisation
    model.eval()
    items = torch.randn(a.items, IN_DIM, generator=g).to(DEV)

    def tokenise():
        for s in range(0, a.items, 1024):
            model.get_indices(items[s:s + 1024], None, use_sk=False)
    orig_beta, model.rq.beta = model.rq.beta, 0.0                        # (no labels: nothing to draw)
    ms = host_timed(tokenise, max(2, a.steps // 2), 1)
    model.rq.beta = orig_beta
    res["tokenise_items"] = a.items
    res["tokenise_items_per_s"] = a.items / (ms * 1e-3)
    res = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
