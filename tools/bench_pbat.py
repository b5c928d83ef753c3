#!/usr/bin/env python3
"""PBAT on one GPU: train step, the fused Wasserstein attention and the head against torch compositions of the reference's
formulation, and the share of the step that still runs as torch ops.

  * train step (``calculate_loss`` + backward) of the reference's shipped config (hidden 64, 2 layers, 2 heads, inner 256,
    dropout 0.2, mask_ratio 0.2) with 4 behaviours at batch ``--batch`` x ``--seq`` on synthetic catalogues (full-length rows,
    uniform types, 1000 users): time, sequences/s, peak allocated memory, M (masked rows);
  * one layer's attention, forward + backward with every gradient, at ``--attn_batch`` rows: gamer_pbat_attn_fwd / _bwd + the slab
    reductions against a torch composition that, like the reference, forms the four fused [B, h, L, L, d] tensors and the two
    gathered relation tensors and lets autograd differentiate them; time and peak allocated memory of each;
  * the head on M rows: gamer_wass_rows / _table + the biased catalogue cross entropy (forward + backward) against the
    materialised [M, V] distances of ``wasserstein_distance_matmul`` + ``cross_entropy``;
  * the torch-op share: the pre-encoder block (user x behaviour SAGP, pairwise distances, relation scaling) and the final SAGP
    with ``WPub`` on the M rows, forward + backward, timed on their own, over the step's time.
Medians of ``--steps`` device-event timings after ``--warmup``.  Prints one JSON line per (batch, seq, items).

  python tools/bench_pbat.py --batch 4096 --seq 20,50 --steps 10 --warmup 3 --items 16384,100000
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import ops, pbat, rec_common  # noqa: E402
from gamer_amd.pbat import PBAT, PBATConfig  # noqa: E402

DEV = "cuda:0"
NB, N_USERS, EPS = 4, 1000, 1e-24


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


def peak(fn, reset=lambda: None):
    fn()
    reset()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def _tri(m1, m2, m3, c1, c2, c3):
    c1, c2, c3 = c1.clamp(min=EPS), c2.clamp(min=EPS), c3.clamp(min=EPS)
    cov = 1.0 / (1.0 / c1 + 1.0 / c2 + 1.0 / c3)
    return cov * (m1 / c1 + m2 / c2 + m3 / c3), cov


def _wass(m1, c1, m2, c2):
    mean = (m1 ** 2).sum(-1) + (m2 ** 2).sum(-1) - 2 * (m1 * m2).sum(-1)
    return mean + c1.sum(-1) + c2.sum(-1) - 2 * (torch.sqrt(c1.clamp(min=EPS)) * torch.sqrt(c2.clamp(min=EPS))).sum(-1)


def attention_pair(B, L, h, d, b, g):
    """(fused, materialised, reset): the same attention both ways, every gradient produced"""
    H, NT = h * d, b + 1
    NP = NT * NT
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(DEV)
    cov = lambda *s: (F.elu(torch.randn(*s, generator=g)) + 1).to(DEV)
    pm_all, pc_all = rnd(B * L, 3 * H), cov(B * L, 3 * H)
    rel_m, rel_c, pos_m, pos_c = rnd(B, NP, H), cov(B, NP, H), rnd(L, H), cov(L, H)
    W = tuple(rnd(d) * 0.2 if i % 2 else rnd(d, d) / math.sqrt(d) for i in range(8))
    types = torch.randint(1, b + 1, (B, L), generator=g)
    t32, tl = types.to(torch.int32).to(DEV), types.to(DEV)
    keep = torch.ones(B, L, dtype=torch.int32, device=DEV)
    do = torch.randn(2, B * L, H, generator=g).to(DEV)
    scale = math.sqrt(1.0 / d)
    sl = lambda x: (x[:, :H], x[:, H:2 * H], x[:, 2 * H:])

    def fused():
        (q1, k1, v1), (q2, k2, v2) = sl(pm_all), sl(pc_all)
        proj = (q1, q2, k1, k2, v1, v2)
        o = torch.empty(2, B * L, H, device=DEV)
        S, lse = torch.empty(B, h, L, NT, device=DEV), torch.empty(B, h, L, device=DEV)
        args = (proj, rel_m, rel_c, pos_m, pos_c, W, t32, keep, B, L, h, d, b, scale, 0.0, 1)
        ops.pbat_attn_fwd(*args, o[0], o[1], S, lse)
        dpm, dpc = torch.empty(B * L, 3 * H, device=DEV), torch.empty(B * L, 3 * H, device=DEV)
        (a1, b1, c1), (a2, b2, c2) = sl(dpm), sl(dpc)
        drm, drc = torch.empty(B, NP, H, device=DEV), torch.empty(B, NP, H, device=DEV)
        n = ops.pbat_n_partial(B, h)
        wpart, ppart = torch.zeros(n, h, 4 * (d * d + d), device=DEV), torch.zeros(n, h, 4, L, d, device=DEV)
        ops.pbat_attn_bwd(*args, S, lse, do[0], do[1], (a1, a2, b1, b2, c1, c2), drm, drc, wpart, ppart)
        rec_common.colsum(wpart.view(n * h, -1))
        rec_common.colsum(ppart.view(n, -1))
        return o

    leaves = [t.clone().requires_grad_(True) for t in (pm_all, pc_all, rel_m, rel_c, pos_m, pos_c, *W)]

    def materialised(backward=True):
        xm, xc, rm, rc, pm, pc, wq1, bq1, wq2, bq2, wk1, bk1, wk2, bk2 = leaves
        heads = lambda t: t.reshape(B, L, h, d).permute(0, 2, 1, 3)
        (q1, k1, v1), (q2, k2, v2) = (tuple(heads(x) for x in sl(xm)), tuple(heads(x) for x in sl(xc)))
        bi = torch.arange(B, device=DEV)[:, None, None]
        Rm = rm.view(B, NT, NT, h, d)[bi, tl[:, :, None], tl[:, None, :]].permute(0, 3, 1, 2, 4)       # [B, h, L, L, d]
        Rc = rc.view(B, NT, NT, h, d)[bi, tl[:, :, None], tl[:, None, :]].permute(0, 3, 1, 2, 4)
        pmh, pch = pm.view(L, h, d).permute(1, 0, 2), pc.view(L, h, d).permute(1, 0, 2)
        pcb = pch[None, :, :, None, :]
        fQm, fQc = _tri(q1[:, :, :, None, :], Rm @ wq1.t() + bq1, (pmh @ wq2.t() + bq2)[None, :, :, None, :], q2[:, :, :, None, :], Rc, pcb)
        fKm, fKc = _tri(k1[:, :, :, None, :], Rm @ wk1.t() + bk1, (pmh @ wk2.t() + bk2)[None, :, :, None, :], k2[:, :, :, None, :], Rc, pcb)
        p = torch.softmax(-_wass(fQm, fQc, fKm, fKc) * scale, -1)
        out = torch.stack([(p @ v1).permute(0, 2, 1, 3).reshape(B * L, H), (p @ v2).permute(0, 2, 1, 3).reshape(B * L, H)])
        if backward:
            out.backward(do)
        return out

    def reset():
        for t in leaves:
            t.grad = None
    return fused, materialised, reset


def head_pair(M, H, V, g):
    """(fused, materialised, reset): the cross entropy over the distances to V items, forward + backward to hm, hc, E_m, E_c"""
    hm, hc = torch.randn(M, H, generator=g).to(DEV), torch.randn(M, H, generator=g).to(DEV)
    Em, Ec = (0.5 * torch.randn(V + 1, H, generator=g)).to(DEV), torch.randn(V + 1, H, generator=g).to(DEV)
    target = torch.randint(1, V, (M,), generator=g).to(DEV)
    rows = torch.arange(M, device=DEV)

    def fused():
        f32 = dict(dtype=torch.float32, device=DEV)
        x, a, E2, c = torch.empty(M, 2 * H, **f32), torch.empty(M, **f32), torch.empty(V, 2 * H, **f32), torch.empty(V, **f32)
        ops.wass_rows_fwd(hm, hc, x, a)
        ops.wass_table_fwd(Em, Ec, V, E2, c)
        lse, loss, bad = torch.empty(M, **f32), torch.empty((), **f32), torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.catalog_ce_bias_fwd(x, rows, E2, c, target, lse, loss, bad, V)
        dE2, dx, dc = torch.zeros(V, 2 * H, **f32), torch.zeros(M, 2 * H, **f32), torch.empty(V, **f32)
        ops.catalog_ce_bias_bwd(x, rows, E2, c, target, lse, torch.ones((), **f32), 1.0 / M, dE=dE2, dh=dx, dbias=dc, V=V)
        dhm, dhc, dEm, dEc = torch.empty(M, H, **f32), torch.empty(M, H, **f32), torch.zeros(V + 1, H, **f32), torch.zeros(V + 1, H, **f32)
        ops.wass_rows_bwd(hm, hc, dx, None, dhm, dhc)
        ops.wass_table_bwd(Em, Ec, V, dE2, dc, dEm, dEc)
        return loss

    leaves = [t.clone().requires_grad_(True) for t in (hm, hc, Em, Ec)]

    def materialised():
        a, b, em, ec = leaves
        m2, c2 = em[:V], F.elu(ec[:V]) + 1                                           # (wasserstein_distance_matmul: [M, V] only)
        dist = -2 * a @ m2.t() + (a ** 2).sum(-1, keepdim=True) + (m2 ** 2).sum(-1)[None] + b.sum(-1, keepdim=True) + c2.sum(-1)[None] \
            - 2 * torch.sqrt(b.clamp(min=EPS)) @ torch.sqrt(c2.clamp(min=EPS)).t()
        loss = F.cross_entropy(dist, target)
        loss.backward()
        return loss

    def reset():
        for t in leaves:
            t.grad = None
    return fused, materialised, reset


def torch_share(model, inter, M, steps, warmup):
    """ms of the pre-encoder block and of the final SAGP with WPub on M rows, forward + backward, on their own"""
    H, b = model.hidden_size, model.n_behaviors
    users = inter["uid"]

    def pre():
        P_m, P_c, R_m, R_c = model._user_behavior(users)
        (P_m.sum() + P_c.sum() + R_m.sum() + R_c.sum()).backward()
    g = torch.Generator().manual_seed(3)
    om, oc = torch.randn(M, H, generator=g).to(DEV).requires_grad_(True), (torch.rand(M, H, generator=g) + 0.5).to(DEV).requires_grad_(True)
    pm, pc = torch.randn(M, H, generator=g).to(DEV).requires_grad_(True), (torch.rand(M, H, generator=g) + 0.5).to(DEV).requires_grad_(True)

    def final():
        a, c = pbat.sagp(om, model.WPub(pm), oc, pc)
        (a.sum() + c.sum()).backward()
    return timed(pre, steps, warmup), timed(final, steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--attn_batch", type=int, default=1024)
    ap.add_argument("--seq", default="20,50")
    ap.add_argument("--items", default="16384,100000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg = PBATConfig()
    h, d = cfg.n_heads, cfg.hidden_size // cfg.n_heads
    for S in (int(s) for s in a.seq.split(",")):
        g = torch.Generator().manual_seed(S)
        fused, mat, reset = attention_pair(a.attn_batch, S, h, d, NB, g)
        with torch.no_grad():
            err = float((fused() - mat(backward=False)).abs().max())
        att = dict(batch=a.attn_batch, fused_ms=timed(fused, a.steps, a.warmup), torch_ms=timed(lambda: (reset(), mat()), a.steps, a.warmup),
                   fused_peak_mib=peak(fused), torch_peak_mib=peak(mat, reset), max_abs_diff=err)
        del fused, mat, reset
        torch.cuda.empty_cache()
        for V in (int(v) for v in a.items.split(",")):
            torch.manual_seed(0)
            model = PBAT(cfg, V, N_USERS, S, NB).to(DEV)
            model.train()
            inter = dict(inputs=torch.randint(1, V + 1, (a.batch, S), generator=g).to(DEV),
                         behaviors=torch.randint(1, NB + 1, (a.batch, S), generator=g).to(DEV),
                         uid=torch.randint(1, N_USERS + 1, (a.batch,), generator=g).to(DEV))
            Ms = []

            def step():
                for p in model.parameters():
                    p.grad = None
                model.calculate_loss(inter).backward()
                Ms.append(model.last_masked_count)
            ms = timed(step, a.steps, a.warmup)
            pk = peak(step)
            M = int(statistics.median(Ms))
            pre_ms, final_ms = torch_share(model, inter, M, a.steps, a.warmup)
            hf, hmat, hreset = head_pair(M, cfg.hidden_size, V + 1, g)
            head = dict(M=M, fused_ms=timed(hf, a.steps, a.warmup), fused_peak_mib=peak(hf))
            if M * (V + 1) * 4 * 6 < 100 * 2**30:                             # (the composition holds several [M, V] tensors)
                head.update(torch_ms=timed(lambda: (hreset(), hmat()), a.steps, a.warmup), torch_peak_mib=peak(hmat, hreset))
            print(json.dumps(dict(batch=a.batch, seq=S, items=V, step_ms=ms, seq_per_s=a.batch / ms * 1e3, peak_mib=pk, M=M,
                                  attention=att, head=head, pre_encoder_ms=pre_ms, final_sagp_ms=final_ms,
                                  torch_op_share=(pre_ms + final_ms) / ms)), flush=True)
            del model, hf, hmat, hreset
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
