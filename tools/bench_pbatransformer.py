#!/usr/bin/env python3
"""PBATransformer's train step on one GPU, against the same step without the fused activation and against TIGER.

The model has the shipped config's dimensions (d_model 256, 6 heads of 64, d_ff 512, 4 + 4 layers, the encoder dense, the decoder
sparse in all four layers, injection in layers 0 and 1 of both stacks, behaviour dim 64, dropout 0.1) with num_positions 5 and 4
behaviours at the T5 vocabulary; a batch holds ``--batch`` (256) users with histories of 1 .. ``--history`` (20) items, rows of
``history * 5 + 1`` tokens, right-padded.  Per ``--model``:
  fused       the model as it ships: gamer_relu_tbl_fwd / _bwd, the injection as a table
  three_pass  the same model with the feed-forward layer's activation as TIGER runs it - gamer_bias_act (zero bias), a dropout pass,
              and their backward pair - on a MATERIALISED [T, d_model + behaviour_dim] concatenation: wi runs at K = 320, the
              behaviour columns' input gradient is formed and scattered into the embedding gradient
  tiger       TIGER at the same dimensions on the same ids (a dense ReLU feed-forward layer, no routing)
it reports the median ms per step (forward with labels + backward, device events after ``--warmup``) with the smallest and the
largest, sequences/s, and the share of
the step inside the feed-forward layers (from the input permutation to the output permutation, both directions; device events
around them, summed over the eight layers).  A model may be named more than once: the forms then alternate in one process.  Prints
one JSON line per run and writes them to ``--out`` (profiles/pbatransformer_bench.json).

  python tools/bench_pbatransformer.py --model fused,three_pass,tiger,fused,three_pass,tiger --steps 20 --warmup 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gamer_amd import ops, tiger  # noqa: E402
from gamer_amd.layer_blocks import _N_PARTIAL, _dropout_bwd, dropout_fwd  # noqa: E402

DEV = "cuda:0"
P, BEHAVIOURS, VOCAB = 5, (32100, 32101, 32102, 32103), 32128
DIMS = dict(d_model=256, d_kv=64, d_ff=512, num_layers=4, num_decoder_layers=4, num_heads=6, dropout_rate=0.1, vocab_size=VOCAB)
PBA = dict(DIMS, behavior_injection=True, behavior_embedding_dim=64, num_positions=P, num_behavior=len(BEHAVIOURS), n_positions=20,
           sparse_layers_encoder=[], sparse_layers_decoder=[0, 1, 2, 3], behavior_injection_encoder=[0, 1],
           behavior_injection_decoder=[0, 1], behavior_maps={t: i for i, t in enumerate(BEHAVIOURS)})


def batch(B, history, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, history * P + 1, dtype=torch.int64)
    labels = torch.empty(B, P + 1, dtype=torch.int64)

    def items(n):
        rows = torch.randint(2, 32100, (n, P), generator=g)
        rows[:, 0] = torch.tensor(BEHAVIOURS)[torch.randint(0, len(BEHAVIOURS), (n,), generator=g)]
        return rows
    for r in range(B):
        n = int(torch.randint(1, history + 1, (1,), generator=g))
        ids[r, :n * P] = items(n).reshape(-1)
        ids[r, n * P] = 1
        labels[r, :P], labels[r, P] = items(1)[0], 1
    return ids.to(DEV), (ids != 0).long().to(DEV), labels.to(DEV)


# ---- the three-pass form of the feed-forward layer (this tool's baseline, not the model's path) ----------------------------------
def three_pass(pb):
    zero = {}

    def fwd(n2, W1, W2, Eb, lists, p, seed):
        T, D = n2.shape
        E, dff, Kw = W1.shape
        grp = pb._grp(lists) if lists is not None else {}
        xs = n2 if lists is None else n2.index_select(0, lists.perm)
        beh = None
        if Eb is not None:
            beh = torch.remainder(lists.gid, Eb.shape[0]).long()
            xs = torch.cat([xs, Eb.index_select(0, beh)], 1).contiguous()            # the [T, d_model + behaviour_dim] concatenation
        K = xs.shape[1]
        pre = torch.zeros(T, dff, device=n2.device)
        ops.linear_fwd(xs, K, W1, Kw, pre, dff, T, dff, K, strideB=dff * Kw, **grp)
        act = torch.empty_like(pre)
        if dff not in zero:
            zero[dff] = torch.zeros(dff, device=n2.device)
        ops.bias_act_fwd(pre, zero[dff], ops.ACTIVATIONS["relu"], act)
        actd = dropout_fwd(act, p, seed)
        outs = torch.zeros(T, D, device=n2.device)
        ops.linear_fwd(actd, dff, W2, dff, outs, D, T, D, dff, strideB=D * dff, **grp)
        if lists is None:
            return outs, (xs, pre, actd, beh)
        out = torch.empty_like(outs)
        out.index_copy_(0, lists.perm, outs)
        return out, (xs, pre, actd, beh)

    def bwd(df, saved, W1, W2, Eb, lists, p, seed):
        xs, pre, actd, beh = saved
        T, D = df.shape
        E, dff, Kw = W1.shape
        K = xs.shape[1]
        grp = pb._grp(lists) if lists is not None else {}
        dfs = df if lists is None else df.index_select(0, lists.perm)
        dW1, dW2 = torch.zeros_like(W1), torch.zeros_like(W2)
        ops.linear_wgrad(dfs, D, actd, dff, dW2, dff, T, D, dff, strideC=D * dff, **grp)
        dactd = torch.zeros(T, dff, device=df.device)
        ops.linear_dgrad(dfs, D, W2, dff, dactd, dff, T, D, dff, strideB=D * dff, **grp)
        dact = _dropout_bwd(dactd, dff, p, seed)
        ops.bias_act_bwd(pre, dact, ops.ACTIVATIONS["relu"], dact, torch.empty(_N_PARTIAL, dff, device=df.device))
        ops.linear_wgrad(dact, dff, xs, K, dW1, Kw, T, dff, K, strideC=dff * Kw, **grp)
        dxs = torch.zeros(T, K, device=df.device)
        ops.linear_dgrad(dact, dff, W1, Kw, dxs, K, T, dff, K, strideB=dff * Kw, **grp)
        dEb = None
        if Eb is not None:
            dEb = torch.zeros_like(Eb).index_add_(0, beh, dxs[:, D:])
        if lists is None:
            return dxs, dW1, dW2, dEb
        dn2 = torch.empty(T, D, device=df.device)
        dn2.index_copy_(0, lists.perm, dxs[:, :D])
        return dn2, dW1, dW2, dEb
    return fwd, bwd


class _Spans:
    """device events around every call of the wrapped functions; ``total()`` after a synchronize"""

    def __init__(self):
        self.pairs = []

    def wrap(self, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.pairs.append((e0, e1))
            return out
        return timed

    def total(self):
        ms = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return ms


def bench(kind, a):
    torch.manual_seed(0)
    spans = _Spans()
    if kind == "tiger":
        model = tiger.TIGER(tiger.TigerConfig(**DIMS))
    else:
        from gamer_amd import pbatransformer as pb
        model = pb.PBATransformerForConditionalGeneration(pb.PBATransformerConfig(**PBA))
        if not hasattr(pb, "_shipped_ffn"):
            pb._shipped_ffn = (pb.ffn_fwd, pb.ffn_bwd)
        fwd, bwd = three_pass(pb) if kind == "three_pass" else pb._shipped_ffn
        pb.ffn_fwd, pb.ffn_bwd = spans.wrap(fwd), spans.wrap(bwd)
    model.to(DEV).train()
    batches = [batch(a.batch, a.history, s) for s in range(a.warmup + a.steps)]
    ts, ffn = [], []
    for i, (ids, am, labels) in enumerate(batches):
        for p in model.parameters():
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss, _ = model(ids, am, labels=labels)
        loss.backward()
        e1.record()
        e1.synchronize()
        inside = spans.total()
        if i >= a.warmup:
            ts.append(e0.elapsed_time(e1))
            ffn.append(inside)
    if hasattr(model, "check_inputs"):
        model.check_inputs()
    ms = statistics.median(ts)
    row = dict(model=kind, batch=a.batch, history=a.history, encoder_tokens=int(batches[0][0].shape[1]), step_ms=round(ms, 3),
               sequences_per_s=round(a.batch / ms * 1e3, 1), spread_ms=[round(min(ts), 3), round(max(ts), 3)], loss=round(float(loss.detach()), 4))
    if kind != "tiger":
        row.update(ffn_ms=round(statistics.median(ffn), 3), ffn_share=round(statistics.median(f / t for f, t in zip(ffn, ts)), 4))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fused,three_pass,tiger")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pbatransformer_bench.json"))
    a = ap.parse_args()
    rows = []
    for kind in a.model.split(","):
        if kind not in ("fused", "three_pass", "tiger"):
            raise SystemExit(f"--model {kind}: fused, three_pass or tiger")
        rows.append(bench(kind, a))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
