#!/usr/bin/env python3
"""MBHT on one GPU: the train step, and each fused piece forward + backward against the torch composition of the same mathematics.

  * train step (``calculate_loss`` + backward) of the reference's shipped config (hidden 64, 2 layers, 2 heads, inner 256, dropout
    0.5, scales [5, 4, 20], hyper_len 6, both switches on) at batch ``--batch`` x L = 40 (max_his_len 39) on synthetic catalogues:
    time, sequences/s, peak allocated memory; and users/s of top-10 ranking (``full_sort_topk``);
  * linear attention: gamer_msa_linear_fwd / _bwd + the slab reduction against the masked, transposed, twice projected composition
    of LinearAttention.forward under autograd;
  * seq-mix: gamer_seq_mix_fwd / _bwd against cat + transpose + Linear + transpose;
  * graph build: gamer_hg_build_fwd / _bwd against the reference's per-row construction (a Python walk over the batch and
    torch.block_diag), timed at ``--graph_batch`` rows, where the block-diagonal matrix still fits;
  * two graph convolutions + readout: gamer_hg_conv_fwd / _bwd twice and gamer_hg_readout_fwd / _bwd on the padded [B, L, L] layout
    against the block-diagonal matmuls and the Python readout loop, at ``--graph_batch`` rows.
Medians of ``--steps`` device-event timings after ``--warmup``.  There is no time threshold: the tool prints one JSON line per
(batch, items) and names every piece that is slower than its torch counterpart.

  python tools/bench_mbht.py --batch 1024,4096 --items 16384,100000 --steps 10 --warmup 3
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import mbht, ops, rec_common  # noqa: E402
from gamer_amd.mbht import MBHT, MBHTConfig  # noqa: E402

DEV = "cuda:0"
NB, L, MAX_HIS = 4, 40, 39


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


def batch_rows(B, n_items, g):
    lens = torch.randint(5, MAX_HIS + 1, (B,), generator=g)
    items = torch.randint(1, n_items + 1, (B, MAX_HIS), generator=g) * (torch.arange(MAX_HIS)[None] < lens[:, None])
    types = torch.randint(1, NB + 1, (B, MAX_HIS), generator=g) * (items != 0)
    return dict(inputs=items.to(DEV), behaviors=types.to(DEV), target=torch.randint(1, n_items + 1, (B,), generator=g).to(DEV),
                behavior=torch.full((B,), NB).to(DEV))


def linear_attention_pair(B, h, d, c, g):
    H = h * d
    qkv = (torch.randn(B * L, 3 * H, generator=g) * 0.5).to(DEV)
    keep = (torch.arange(L)[None] < torch.randint(5, L + 1, (B, 1), generator=g)).to(torch.int32).to(DEV)
    Ew, Fw = (torch.randn(c, L, generator=g) * 0.3).to(DEV), (torch.randn(c, L, generator=g) * 0.3).to(DEV)
    Eb, Fb = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    d_o = torch.randn(B * L, H, generator=g).to(DEV)
    scale = math.sqrt(1.0 / d)

    def fused():
        o, lse = torch.empty(B * L, H, device=DEV), torch.empty(B, h, L, device=DEV)
        ops.msa_linear_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, 0.0, 1, o, lse)
        dqkv = torch.empty(B * L, 3 * H, device=DEV)
        part = torch.zeros(ops.msa_n_partial(B, h), 2 * c * L + 2 * c, device=DEV)
        ops.msa_linear_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], keep, Ew, Eb, Fw, Fb, B, L, h, d, scale, 0.0, 1, d_o, lse,
                           dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], part)
        rec_common.colsum(part)
        return o
    leaves = [t.clone().requires_grad_(True) for t in (qkv, Ew, Eb, Fw, Fb)]

    def composed():
        x, ew, eb, fw, fb = leaves
        heads = lambda t: t.reshape(B, L, h, d).permute(0, 2, 1, 3)
        q, k, v = heads(x[:, :H]), heads(x[:, H:2 * H]), heads(x[:, 2 * H:])
        m = keep.float()[:, None, :, None]
        v = torch.nn.functional.linear((v * m).transpose(2, 3), ew, eb).transpose(2, 3)
        k = torch.nn.functional.linear((k * m).transpose(2, 3), fw, fb).transpose(2, 3)
        p = torch.softmax(q @ k.transpose(-2, -1) * scale, -1)
        o = (p @ v).permute(0, 2, 1, 3).reshape(B * L, H)
        o.backward(d_o)
        for t in leaves:
            t.grad = None
        return o
    return fused, composed


def seq_mix_pair(B, H, s1, s2, g):
    lens = [L, L // s1, L // s2]
    xs = [torch.randn(B, n, H, generator=g).to(DEV) for n in lens]
    W, bias = (torch.randn(L, sum(lens), generator=g) * 0.2).to(DEV), torch.zeros(L, device=DEV)
    dy = torch.randn(B, L, H, generator=g).to(DEV)

    def fused():
        y = torch.empty(B, L, H, device=DEV)
        ops.seq_mix_fwd(xs, W, bias, y)
        dxs = [torch.empty_like(x) for x in xs]
        part = torch.zeros(ops.seq_mix_n_partial(B, L, sum(lens)), L * sum(lens) + L, device=DEV)
        ops.seq_mix_bwd(xs, W, dy, dxs, part)
        rec_common.colsum(part)
        return y
    leaves = [t.clone().requires_grad_(True) for t in xs + [W, bias]]

    def composed():
        y = torch.nn.functional.linear(torch.cat(leaves[:3], 1).transpose(1, 2), leaves[3], leaves[4]).transpose(1, 2)
        y.backward(dy)
        for t in leaves:
            t.grad = None
        return y
    return fused, composed


def graph_pairs(B, H, K, n_items, g):
    """(build fused, build composed, conv + readout fused, conv + readout composed) on the same rows"""
    model = MBHT(MBHTConfig(hidden_size=H, scales=[5, 4, 20], hyper_len=K), n_items, MAX_HIS, NB, NB).to(DEV)
    inter = batch_rows(B, n_items, g)
    masked, pos_items, masked_index, _ = model.reconstruct_train_data(inter["inputs"], inter["behaviors"], inter["target"],
                                                                      inter["behavior"], seed=1)
    xm = (torch.randn(n_items + 2, H, generator=g) * 0.3 + 0.5).to(DEV)[masked].contiguous()
    items32, n_obj = masked.to(torch.int32).contiguous(), torch.count_nonzero(masked, 1).to(torch.int32)
    dG = torch.randn(B, L, L, generator=g).to(DEV)
    x = torch.randn(B, L, H, generator=g).to(DEV)
    dy = torch.randn(B, L, H, generator=g).to(DEV)
    pos = masked_index.to(torch.int32).contiguous()
    G, sel = torch.empty(B, L, L, device=DEV), torch.empty(B, L, K, dtype=torch.int32, device=DEV)
    ops.hg_build_fwd(xm, items32, model.mask_token, K, G, sel)

    def build_fused():
        ops.hg_build_fwd(xm, items32, model.mask_token, K, G, sel)
        dxm = torch.empty(B, L, H, device=DEV)
        ops.hg_build_bwd(xm, items32, sel, G, dG, model.mask_token, dxm)
        return G
    leaf = xm.clone().requires_grad_(True)
    ns = n_obj.tolist()

    def build_composed():
        z = torch.nn.functional.normalize(leaf)
        sim = z @ z.transpose(1, 2)
        sim = torch.where(sim < 0, torch.full_like(sim, 0.01), sim)
        Gs = []
        for b in range(B):
            n = ns[b]
            s = masked[b, :n]
            val, idx = torch.topk(sim[b, :n, :n], min(K, n), sorted=False)
            tok = s[idx]
            own = s[:, None].expand_as(tok)
            hit = tok == model.mask_token
            tok, val = torch.where(hit, own, tok), torch.where(hit, torch.ones_like(val), val)
            uniq, counts = torch.unique(s, return_counts=True)
            multi = uniq[(counts > 1) & (uniq != model.mask_token)]
            Hm = torch.zeros(n, len(uniq) + len(multi), device=DEV)
            live = s != model.mask_token
            col = (tok[:, :, None] == uniq[None, None, :]).long().argmax(-1)
            rows = live.nonzero()[:, 0].repeat_interleave(val.shape[1])
            Hm[rows, col[live].flatten()] = val[live].flatten()
            Hm[(s[:, None] == uniq[None, :]).nonzero(as_tuple=True)] = 1.0
            if len(multi):
                mm = s[:, None] == multi[None, :]
                Hm[mm.any(1), len(uniq) + mm.long().argmax(1)[mm.any(1)]] = 1.0
            Gs.append((Hm / Hm.sum(1, keepdim=True)) @ (Hm / Hm.sum(0, keepdim=True)).t())
        big = torch.block_diag(*Gs)
        big.backward(torch.ones_like(big))
        leaf.grad = None
        return big

    def tail_fused():
        y1, y2, r = torch.empty(B, L, H, device=DEV), torch.empty(B, L, H, device=DEV), torch.empty(B, L, H, device=DEV)
        ops.hg_conv_fwd(G, x, y1)
        ops.hg_conv_fwd(G, y1, y2)
        ops.hg_readout_fwd((y1 + y2) / 2, pos, n_obj, r)
        dh = torch.empty(B, L, H, device=DEV)
        ops.hg_readout_bwd(dy, pos, n_obj, dh)
        d2, dG2, d1, dG1 = torch.empty_like(x), torch.empty_like(G), torch.empty_like(x), torch.empty_like(G)
        ops.hg_conv_bwd(G, y1, dh / 2, d2, dG2)
        ops.hg_conv_bwd(G, x, d2 + dh / 2, d1, dG1)
        return r
    big = torch.block_diag(*[G[b, :n, :n] for b, n in enumerate(ns)]).requires_grad_(True)
    flat = torch.cat([x[b, :n] for b, n in enumerate(ns)]).requires_grad_(True)
    poss = pos.tolist()

    def tail_composed():
        x1 = big @ flat
        x2 = big @ x1
        emb = (x1 + x2) / 2
        outs, start = [], 0
        for b, n in enumerate(ns):
            e = torch.cat([emb[start:start + n], torch.zeros(L - n, H, device=DEV)])
            start += n
            for p in poss[b]:
                if p == 0:
                    continue
                end = p + 6 if p + 6 < n else n - 1
                e[p] = torch.cat((e[max(p - 10, 0):p], e[p + 1:end])).mean(0)
            outs.append(e)
        out = torch.stack(outs)
        out.backward(dy)
        big.grad = flat.grad = None
        return out
    return build_fused, build_composed, tail_fused, tail_composed, int(sum(ns))


def bench(B, n_items, a):
    cfg = MBHTConfig(hidden_size=64, scales=[5, 4, 20])
    g = torch.Generator().manual_seed(B)
    model = MBHT(cfg, n_items, MAX_HIS, NB, NB).to(DEV).train()
    inter = batch_rows(B, n_items, g)

    def step():
        for p in model.parameters():
            p.grad = None
        model.calculate_loss(inter).backward()
    out = dict(batch=B, L=L, items=n_items, hidden=cfg.hidden_size, layers=cfg.n_layers, hyper_len=cfg.hyper_len)
    ms = timed(step, a.steps, a.warmup)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    out["step"] = dict(ms=round(ms, 3), seq_per_s=round(B / ms * 1e3), peak_mib=round((torch.cuda.max_memory_allocated() - base) / 2**20, 1))
    model.eval()
    ev = timed(lambda: model.full_sort_topk(inter, 10), a.steps, a.warmup)
    out["top10"] = dict(ms=round(ev, 3), users_per_s=round(B / ev * 1e3))
    pieces = {}
    f, c = linear_attention_pair(B, cfg.n_heads, cfg.hidden_size // cfg.n_heads, cfg.scales[0], g)
    pieces["linear_attention"] = (f, c, B)
    f, c = seq_mix_pair(B, cfg.hidden_size, cfg.scales[1], cfg.scales[2], g)
    pieces["seq_mix"] = (f, c, B)
    GB = min(B, a.graph_batch)
    bf, bc, tf_, tc, total = graph_pairs(GB, cfg.hidden_size, cfg.hyper_len, n_items, g)
    pieces["graph_build"] = (bf, bc, GB)
    pieces["graph_conv_x2_readout"] = (tf_, tc, GB)
    slower = []
    for name, (f, c, rows) in pieces.items():
        fm, cm = timed(f, a.steps, a.warmup), timed(c, max(2, a.steps // 3), 1)
        pieces[name] = dict(rows=rows, fused_ms=round(fm, 3), torch_ms=round(cm, 3))
        if fm > cm:
            slower.append(name)
    out.update(pieces=pieces, block_diag_mib_at_graph_batch=round(total * total * 4 / 2**20, 1), slower_than_torch=slower)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1024,4096")
    ap.add_argument("--items", default="16384,100000")
    ap.add_argument("--graph_batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from gamer_amd import build
    build.build()
    for B in (int(x) for x in a.batch.split(",")):
        for n in (int(x) for x in a.items.split(",")):
            bench(B, n, a)


if __name__ == "__main__":
    main()
