#!/usr/bin/env python3
"""MBSTR on one GPU: train step, the behaviour attention and the behaviour FFN against torch compositions of the reference's
formulation, and top-10 ranking.

  * train step (``calculate_loss`` + backward) of the reference's shipped config (hidden 64, 2 layers, 2 heads, inner 256,
    dropout 0.2, mask_ratio 0.2, all four behaviour switches on) with 4 behaviours at batch ``--batch`` x ``--seq`` on synthetic
    catalogues (full-length rows, uniform types): time, sequences/s, peak allocated memory, M (median masked rows);
  * one attention (mix, scores, softmax, dropout-free context; forward + backward with every gradient) on the same q / k / v:
    gamer_mbs_mix_fwd/_bwd + gamer_mbs_attn_fwd/_bwd + the slab reductions against a torch composition that, like the
    reference, forms the [B, h, L, L, b b + 1] score tensor and the one-hot of the pair index and lets autograd differentiate
    them; time and peak allocated memory of each;
  * the behaviour FFN forward + backward: two grouped GEMMs over the rows sorted by type (each row through its own expert)
    against all experts on all rows followed by the one-hot selection, as the reference runs it;
  * evaluation: users/s of top-10 full ranking (``full_sort_topk``: encoder + CGC head + gamer_catalog_topk).
Medians of ``--steps`` device-event timings after ``--warmup``.  Prints one JSON line per (batch, seq).

  python tools/bench_mbstr.py --batch 4096 --seq 20,50 --steps 10 --warmup 3 --items 16384,100000,1000000
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

from gamer_amd import layer_blocks, mbstr, ops, rec_common  # noqa: E402
from gamer_amd.mbstr import MBSTR, MBSTRConfig  # noqa: E402

DEV = "cuda:0"
NB = 4


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
    reset()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def attention_pair(B, L, h, d, b, g):
    """(fused, materialised, reset): the same attention both ways, every gradient produced"""
    H, C = h * d, b * b + 1
    qkv = (torch.randn(B * L, 3 * H, generator=g) * 0.5).to(DEV)
    types = torch.randint(1, b + 1, (B, L), generator=g)
    W1, W2 = ((torch.randn(b, h, d, d, generator=g) / math.sqrt(d)).to(DEV) for _ in range(2))
    a1, a2 = (torch.randn(C, b, h, generator=g).to(DEV) for _ in range(2))
    rel = (torch.randn(C, 32, h, generator=g) * 0.5).to(DEV)
    bucket = mbstr.relative_position_buckets(L, 32, 40).to(DEV)
    d_o = torch.randn(B * L, H, generator=g).to(DEV)
    t32, tl_all = types.to(torch.int32).to(DEV), types.to(DEV)
    scale = math.sqrt(1.0 / d)
    q_, k_, v_ = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]

    def fused():
        w1m, w2m = torch.empty(C, h, d, d, device=DEV), torch.empty(C, h, d, d, device=DEV)
        ops.mbs_mix_fwd(W1, a1, w1m)
        ops.mbs_mix_fwd(W2, a2, w2m)
        o, lse = torch.empty(B * L, H, device=DEV), torch.empty(B, h, L, device=DEV)
        ops.mbs_attn_fwd(q_, k_, v_, t32, w1m, w2m, rel, bucket, B, L, h, d, b, scale, 0.0, 1, o, lse)
        n = ops.mbs_n_partial(B, h, d, b)
        dqkv = torch.zeros(B * L, 3 * H, device=DEV)
        p1, p2 = torch.zeros(n, C, h, d, d, device=DEV), torch.zeros(n, C, h, d, d, device=DEV)
        pr = torch.zeros(n, C, 2 * L - 1, h, device=DEV)
        ops.mbs_attn_bwd(q_, k_, v_, t32, w1m, w2m, rel, bucket, B, L, h, d, b, scale, 0.0, 1, o, d_o, lse, dqkv[:, :H],
                         dqkv[:, H:2 * H], dqkv[:, 2 * H:], p1, p2, pr)
        dw1m, dw2m = rec_common.colsum(p1.view(n, -1)).view(C, h, d, d), rec_common.colsum(p2.view(n, -1)).view(C, h, d, d)
        dW1, dW2, da1, da2 = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(a1), torch.empty_like(a2)
        ops.mbs_mix_bwd(W1, a1, dw1m, dW1, da1)
        ops.mbs_mix_bwd(W2, a2, dw2m, dW2, da2)
        drel = torch.empty_like(rel)
        ops.mbs_bias_fold(rec_common.colsum(pr.view(n, -1)).view(C, 2 * L - 1, h), bucket, drel)
        return o

    leaves = [t.clone().requires_grad_(True) for t in (qkv, W1, a1, W2, a2, rel)]

    def materialised(r0=0, r1=B, backward=True):
        """rows r0 .. r1 of the batch (the whole batch when timed; slices for the comparison of the values)"""
        x, w1, al1, w2, al2, r = leaves
        B = r1 - r0
        x, tl = x[r0 * L:r1 * L], tl_all[r0:r1]
        heads = lambda t: t.reshape(B, L, h, d).permute(0, 2, 1, 3)
        q, k, v = heads(x[:, :H]), heads(x[:, H:2 * H]), heads(x[:, 2 * H:])
        pair = (tl[:, :, None] - 1) * b + tl[:, None, :]                                        # (no padding in this batch)
        idx = pair[:, None, :, :, None].expand(-1, h, -1, -1, -1)
        w1m = torch.einsum("bhmn,Cbh->Chmn", w1, torch.softmax(al1, 1))
        every = torch.einsum("BhQm,Chmn,BhKn->BhQKC", q, w1m, k)                                # [B, h, L, L, C]
        score = every.gather(4, idx)[..., 0] * scale
        pos = bucket.long()[torch.arange(L, device=DEV)[None, :] - torch.arange(L, device=DEV)[:, None] + L - 1]
        tables = r[:, pos].permute(3, 1, 2, 0)[None].expand(B, -1, -1, -1, -1)                  # [B, h, L, L, C]
        score = score + tables.gather(4, idx)[..., 0]
        p = torch.softmax(score, -1)
        onehot = F.one_hot(pair[:, None], C).expand(-1, h, -1, -1, -1).float()                  # [B, h, L, L, C]
        w2m = torch.einsum("bhmn,Cbh->Chmn", w2, torch.softmax(al2, 1))
        ctx = torch.einsum("BhQK,BhQKC,Chnm,BhKn->BhQm", p, onehot, w2m, v)
        out = ctx.permute(0, 2, 1, 3).reshape(B * L, H)
        if backward:
            out.backward(d_o[r0 * L:r1 * L])
        return out

    def reset():
        for t in leaves:
            t.grad = None
    return fused, materialised, reset


def ffn_pair(B, L, H, dff, b, g):
    T = B * L
    x = (torch.randn(T, H, generator=g) * 0.5).to(DEV)
    dy = torch.randn(T, H, generator=g).to(DEV)
    types = torch.randint(1, b + 1, (B, L), generator=g).to(torch.int32).to(DEV)
    w1, b1 = (torch.randn(b, dff, H, generator=g) * 0.1).to(DEV), (torch.randn(b, dff, generator=g) * 0.1).to(DEV)
    w2, b2 = (torch.randn(b, H, dff, generator=g) * 0.1).to(DEV), (torch.randn(b, H, generator=g) * 0.1).to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    relu = ops.ACTIVATIONS["relu"]

    def grouped():
        with ops.f32_matmul("f32"):
            lists = layer_blocks._TypeLists(types, b)
            perm, grp = lists.perm, dict(groups=b, group_offsets=lists.offsets[1:])
            xa = layer_blocks._with_ones(x.index_select(0, perm))
            w1a, w2a = layer_blocks._aug_weights(w1, b1), layer_blocks._aug_weights(w2, b2)
            pre = torch.zeros(T, dff, **f32)
            ops.linear_fwd(xa, H + 4, w1a, H + 4, pre, dff, T, dff, H + 4, strideB=dff * (H + 4), **grp)
            a1 = torch.empty(T, dff, **f32)
            ops.bias_act_fwd(pre, torch.zeros(dff, **f32), relu, a1)
            a1a = layer_blocks._with_ones(a1)
            ys = torch.zeros(T, H, **f32)
            ops.linear_fwd(a1a, dff + 4, w2a, dff + 4, ys, H, T, H, dff + 4, strideB=H * (dff + 4), **grp)
            y = torch.empty(T, H, **f32)
            y.index_copy_(0, perm, ys)
            dys = dy.index_select(0, perm)
            dw2a, dw1a = torch.zeros_like(w2a), torch.zeros_like(w1a)
            ops.linear_wgrad(dys, H, a1a, dff + 4, dw2a, dff + 4, T, H, dff + 4, strideC=H * (dff + 4), **grp)
            da1 = torch.zeros(T, dff, **f32)
            ops.gemm(dys, H, 1, w2a, 1, dff + 4, da1, dff, T, dff, H, strideB=H * (dff + 4), **grp)
            ops.bias_act_bwd(pre, da1, relu, da1, torch.empty(256, dff, **f32))
            ops.linear_wgrad(da1, dff, xa, H + 4, dw1a, H + 4, T, dff, H + 4, strideC=dff * (H + 4), **grp)
            dxs = torch.zeros(T, H, **f32)
            ops.gemm(da1, dff, 1, w1a, 1, H + 4, dxs, H, T, H, dff, strideB=dff * (H + 4), **grp)
            dx = torch.empty(T, H, **f32)
            dx.index_copy_(0, perm, dxs)
            return y

    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    onehot = F.one_hot(types.long().view(T), b + 1).float()

    def all_then_select():
        xx, a, ab, c, cb = leaves
        outs = [torch.zeros_like(xx)] + [F.linear(torch.relu(F.linear(xx, a[i], ab[i])), c[i], cb[i]) for i in range(b)]
        y = torch.einsum("bTH,Tb->TH", torch.stack(outs), onehot)
        y.backward(dy)
        return y

    def reset():
        for t in leaves:
            t.grad = None
    return grouped, all_then_select, reset


def bench(B, S, items, a):
    cfg = MBSTRConfig()
    H, h = cfg.hidden_size, cfg.n_heads
    out = dict(batch=B, seq=S, hidden=H, heads=h, layers=cfg.n_layers, behaviours=NB)
    g = torch.Generator().manual_seed(S)
    fused, mat, reset = attention_pair(B, S, h, H // h, NB, g)
    # values: the fused output against the composition evaluated 256 rows at a time (tensors of a size torch's einsum is used at
    # every day) and against the composition on the whole batch, as it is timed
    o = fused()
    with torch.no_grad():
        err = max(float((o[r0 * S:(r0 + 256) * S] - mat(r0, min(B, r0 + 256), False)).abs().max()) for r0 in range(0, B, 256))
    err_whole = float((o - mat().detach()).abs().max())
    reset()
    att = dict(max_abs_diff_whole_batch_composition=err_whole, fused_ms=round(timed(fused, a.steps, a.warmup), 3), fused_peak_mib=round(peak(fused, reset), 1), max_abs_diff=err)
    try:
        att["materialised_ms"] = round(timed(mat, a.steps, a.warmup), 3)
        att["materialised_peak_mib"] = round(peak(mat, reset), 1)
    except torch.cuda.OutOfMemoryError:
        att["materialised_ms"] = "out of memory"
    reset()
    out["attention_fwd_bwd"] = att
    del fused, mat, reset
    torch.cuda.empty_cache()
    grouped, dense, reset = ffn_pair(B, S, H, cfg.inner_size, NB, g)
    err = float((grouped() - dense().detach()).abs().max())
    reset()
    out["ffn_fwd_bwd"] = dict(grouped_ms=round(timed(grouped, a.steps, a.warmup), 3), grouped_peak_mib=round(peak(grouped, reset), 1),
                              all_experts_then_select_ms=round(timed(dense, a.steps, a.warmup), 3),
                              all_experts_then_select_peak_mib=round(peak(dense, reset), 1), max_abs_diff=err)
    del grouped, dense, reset
    torch.cuda.empty_cache()
    for n_items in items:
        g = torch.Generator().manual_seed(n_items)
        torch.manual_seed(0)
        model = MBSTR(cfg, n_items, S, NB).to(DEV).train()
        inter = dict(inputs=torch.randint(1, n_items + 1, (B, S), generator=g).to(DEV),
                     behaviors=torch.randint(1, NB + 1, (B, S), generator=g).to(DEV), seq_len=torch.full((B,), S, device=DEV))
        counts = []

        def step():
            model.zero_grad(set_to_none=True)
            model.calculate_loss(inter).backward()
            counts.append(model.last_masked_count)
        ms = timed(step, a.steps, a.warmup)
        r = dict(step_ms=round(ms, 3), sequences_per_s=round(B / ms * 1e3, 1), masked_rows=int(statistics.median(counts)),
                 step_peak_mib=round(peak(step, lambda: model.zero_grad(set_to_none=True)), 1))
        model.eval()
        ev = dict(inter, inputs=inter["inputs"].clone())
        ev["inputs"][:, -1] = n_items + 1
        U = min(B, a.eval_users)
        ev = {k: v[:U] for k, v in ev.items()}
        r["topk_users_per_s"] = round(U / timed(lambda: model.full_sort_topk(ev, 10), a.steps, a.warmup) * 1e3, 1)
        out[f"items_{n_items}"] = r
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="4096")
    ap.add_argument("--seq", default="20,50")
    ap.add_argument("--items", default="16384,100000,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval_users", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mbstr.py needs the GPU")
    items = [int(x) for x in a.items.split(",")]
    for B in [int(x) for x in a.batch.split(",")]:
        for S in [int(x) for x in a.seq.split(",")]:
            print(json.dumps(bench(B, S, items, a)), flush=True)
    # the kernels' limits (L 128, head size 64, 4 heads, 8 behaviours): the fused attention alone; the composition's
    # [B, h, L, L, 65] tensors would take 17 GB each at this batch
    Bl = 1024
    fused, _, _ = attention_pair(Bl, 128, 4, 64, 8, torch.Generator().manual_seed(7))
    print(json.dumps(dict(limit_shape=dict(batch=Bl, seq=128, heads=4, head_size=64, behaviours=8, slabs=ops.mbs_n_partial(Bl, 4, 64, 8),
                                           fused_fwd_bwd_ms=round(timed(fused, a.steps, a.warmup), 3)))), flush=True)


if __name__ == "__main__":
    main()
