"""``python -m gamer_amd.train_rec``: train and test SASRec or GRU4Rec on session-wise multi-behaviour data (``train_SMB_rec``).

Mirrors ``TrainSMBRec.invoke`` (ref:SeqRec/tasks/train_SMB_rec.py) and ``SMBRec.Trainer`` (ref:SeqRec/trainers/SMBRec.py):
evaluate before training, then per epoch a shuffled pass over the training samples and an evaluation on the target
behaviour's validation set; the best model by the last metric goes to ``best_model.pth`` (patience as the reference).  The
step is AdamW (betas 0.9 / 0.999, eps 1e-8, decay on every parameter, no clipping) on ``gamer_adamw``.  Test: every
behaviour of the test split plus the "Merged Behavior" entry weighted by the behaviours' sample counts, written to
``result-{test_task}.json`` in the reference's layout.  Ranking uses the model's ``full_sort_topk`` with K = the largest k of
``--metrics``.  ``--base_model`` defaults to ``./config/dis-models/{backbone}``, as the reference's launcher sets it.  Single
device, no wandb.

``run`` is that loop with the model class, the config class and the data functions as arguments: ``main`` here calls it with the
``smb_dis`` data layer, ``python -m gamer_amd.train_bert4rec`` with BERT4Rec and ``smb_dis_target_data``.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

from . import ops, smb_dis_data
from .gru4rec import GRU4Rec, GRU4RecConfig
from .metrics import topk_rank_metrics
from .sasrec import SASRec, SASRecConfig

DEFAULT_METRICS = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10"
BACKBONES = {"SASRec": (SASRec, SASRecConfig), "GRU4Rec": (GRU4Rec, GRU4RecConfig)}


def parse_args(argv=None, prog="python -m gamer_amd.train_rec", backbone="SASRec", backbones=None, tasks="smb_dis",
               test_task="smb_dis"):
    """The command's arguments; a command of another backbone family (train_bert4rec) passes its own defaults and names."""
    backbones = BACKBONES if backbones is None else backbones
    ap = argparse.ArgumentParser(prog=prog)
    ap.add_argument("--backbone", default=backbone)
    ap.add_argument("--base_model", default=None, help="default: ./config/dis-models/{backbone}")
    ap.add_argument("--data_path", default="./data")
    ap.add_argument("--dataset", default="Retail_Beh")
    ap.add_argument("--tasks", default=tasks)
    ap.add_argument("--test_task", default=test_task)
    ap.add_argument("--max_his_len", type=int, default=20)
    ap.add_argument("--optim", default="adamw")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--learning_rate", type=float, default=5e-4)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--patience", type=int, default=20)
    ap.add_argument("--metrics", default=DEFAULT_METRICS)
    ap.add_argument("--output_dir", default="./checkpoint/SMB-recommender")
    ap.add_argument("--result_dir", default="./results")
    ap.add_argument("--only_test", action="store_true")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)
    if a.backbone not in backbones:
        raise NotImplementedError(f"--backbone {a.backbone}: only {', '.join(backbones)} run on the HIP path")
    if a.base_model is None:
        a.base_model = f"./config/dis-models/{a.backbone}"
    if a.optim.lower() != "adamw":
        raise NotImplementedError(f"--optim {a.optim}: only adamw (gamer_adamw) runs on the HIP path")
    return a


class AdamW:
    """torch.optim.AdamW's update (decay on every parameter, no clipping) with gamer_adamw, one launch pair per tensor."""

    def __init__(self, params, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
        self.params = [p for p in params if p.requires_grad]
        self.lr, self.wd, self.betas, self.eps, self.step_n = lr, weight_decay, betas, eps, 0
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        dev = self.params[0].device
        self.partial = torch.empty(64, dtype=torch.float32, device=dev)
        self.norm = torch.empty(1, dtype=torch.float32, device=dev)

    def step(self):
        self.step_n += 1
        for p, m, v in zip(self.params, self.m, self.v):
            if p.grad is None:          # (a parameter no loss reaches: torch's AdamW skips it too)
                continue
            g = p.grad.contiguous()
            ops.sumsq(g, self.partial)
            ops.adamw(p.data, g, m, v, p.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_n, 0.0,
                      1.0, self.partial, self.norm)


def _to(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def evaluate(model, data, batch_size, metrics, dev, collate=smb_dis_data.collate):
    """mean of every metric over the samples of ``data`` (valid / test: lists of targets)"""
    model.eval()
    K = max(int(m.split("@")[1]) for m in metrics)
    vals = {m: [] for m in metrics}
    with torch.no_grad():
        for i in range(0, len(data.samples), batch_size):
            batch, targets = collate(data.samples[i:i + batch_size], test=True)
            idx, _ = model.full_sort_topk(_to(batch, dev), K)
            for m, v in topk_rank_metrics(idx.cpu().numpy(), targets, metrics).items():
                vals[m].extend(v)
    return {m: float(np.mean(v)) for m, v in vals.items()}


def run(a, model_cls, config_cls, load_train_valid, load_test, collate, tag="train_rec", train_target_only=False,
        test_target_only=False, pass_target_behavior_id=False, pass_n_users=False):
    """The loop of ``TrainSMBRec.invoke`` for the parsed arguments ``a``: the model and config classes, the data functions
    (train / valid loader, test loader, collate) and the tag of the printed lines are the command's (train_rec, train_bert4rec).
    The three flags are what the reference does for MBHT alone: train on the target behaviour's rows only, test the target
    behaviour only (the merged entry then equals it), and give the model ``target_behavior_id = target_behavior_index + 1``.
    ``pass_n_users`` gives the model ``n_users`` (PBAT, whose data functions put ``uid`` into the batches)."""
    random.seed(a.seed)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    dev = torch.device("cuda")
    metrics = a.metrics.split(",")
    os.makedirs(a.output_dir, exist_ok=True)
    config = config_cls.from_pretrained(a.base_model)
    trains, valid = load_train_valid(a.data_path, a.dataset, a.max_his_len, a.tasks)
    valid = valid.filter_by_behavior(valid.target_behavior)
    first = trains[0]
    # (n_behaviors: read by the behaviour-aware backbones; the others take it in **kwargs)
    extra = dict(target_behavior_id=first.target_behavior_index + 1) if pass_target_behavior_id else {}
    if pass_n_users:
        extra["n_users"] = first.num_users
    model = model_cls(config, n_items=first.num_items, max_his_len=a.max_his_len, n_behaviors=len(first.behaviors), **extra).to(dev)
    ckpt = os.path.join(a.output_dir, "best_model.pth")
    if not a.only_test:
        if train_target_only:
            trains = [t.filter_by_behavior(t.target_behavior) for t in trains]
        train_samples = [s for t in trains for s in t.samples]
        opt = AdamW(model.parameters(), a.learning_rate, a.weight_decay)
        g = torch.Generator().manual_seed(a.seed)
        best = evaluate(model, valid, a.batch_size, metrics, dev, collate)[metrics[-1]]
        print(f"[{tag}] before training: {metrics[-1]} {best:.4f}", flush=True)
        patience, saved = 0, False
        for epoch in range(a.epochs):
            model.train()
            order = torch.randperm(len(train_samples), generator=g).tolist()
            losses = []
            for i in range(0, len(order), a.batch_size):
                batch = _to(collate([train_samples[j] for j in order[i:i + a.batch_size]]), dev)
                for p in model.parameters():
                    p.grad = None
                loss = model.calculate_loss(batch)
                loss.backward()
                opt.step()
                losses.append(loss.detach())
            loss = float(torch.stack(losses).mean())
            res = evaluate(model, valid, a.batch_size, metrics, dev, collate)
            print(f"[{tag}] epoch {epoch + 1}/{a.epochs} loss {loss:.4f} " +
                  " ".join(f"{m} {v:.4f}" for m, v in res.items()), flush=True)
            if res[metrics[-1]] > best:
                best, patience, saved = res[metrics[-1]], 0, True
                torch.save(model.state_dict(), ckpt)
            else:
                patience += 1
                if patience >= a.patience:
                    print(f"[{tag}] early stopping on epoch {epoch + 1}", flush=True)
                    break
        if not saved:
            # no epoch beat the evaluation before training: the reference's test step would fail on the missing file; the
            # last model is tested instead
            torch.save(model.state_dict(), ckpt)
    test = load_test(a.data_path, a.dataset, a.max_his_len, a.test_task)
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    results, merged, total = [], {m: 0.0 for m in metrics}, 0
    for b in first.behaviors:
        if test_target_only and b != first.target_behavior:
            continue
        part = test.filter_by_behavior(b)
        r = evaluate(model, part, a.batch_size, metrics, dev, collate) if len(part) else {m: float("nan") for m in metrics}
        r["eval_type"] = f"Behavior {b}"
        results.append(r)
        for m in metrics:
            merged[m] += r[m] * len(part) if len(part) else 0.0
        total += len(part)
    for m in metrics:
        merged[m] /= total
    merged["eval_type"] = "Merged Behavior"
    results.append(merged)
    os.makedirs(a.result_dir, exist_ok=True)
    out = os.path.join(a.result_dir, f"result-{a.test_task}.json")
    with open(out, "w") as f:
        json.dump(results, f, indent=4)
    print(f"[{tag}] results saved to {out}", flush=True)
    return results


def main(argv=None):
    a = parse_args(argv)
    return run(a, *BACKBONES[a.backbone], smb_dis_data.load_train_valid, smb_dis_data.load_test, smb_dis_data.collate)


if __name__ == "__main__":
    main(sys.argv[1:])
