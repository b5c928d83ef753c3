"""``python -m gamer_amd.train_tiger``: train and test TIGER, the default backbone of ``train_decoder``, on the HIP engine.

Mirrors ``TrainDecoder.invoke`` (ref:SeqRec/tasks/train_decoder.py) for ``--backbone TIGER --tasks seqrec`` and, with
``--only_test`` or after training, ``TestDecoder`` (ref:SeqRec/tasks/test_decoder.py):
  data       seqrec_data.SeqRecData / EncoderDecoderCollator: the T5 vocabulary plus the sorted index tokens, leave-last-two-out
  model      tiger.TIGER at ``--base_model``'s config.json, ``resize_token_embeddings`` to the grown vocabulary, ``--temperature``
  training   HF Trainer's step: AdamW (betas 0.9 / 0.999, eps 1e-8, no decay on the layer norms) with the gradient clipped at norm
             1.0, on gamer_adamw over one flat parameter buffer; ``--lr_scheduler_type cosine`` with ``--warmup_ratio``
             (gamer_amd/schedule.py); the evaluation loss on the validation split after every epoch; the best model by evaluation
             loss goes to ``best_model.pth`` (a state dict the reference class loads); ``--patience`` as EarlyStoppingCallback
  testing    a trie over all items ([decoder_start] + item tokens + </s>), tiger.beam_search with ``--num_beams``, then
             metrics.py (hit / ndcg / recall @ k) averaged over the test samples, written to ``--results_file``;
             ``--eval_mode exact | sampled`` (tiger_eval.py; also on train_tiger_smb, train_tiger_mb and train_pbatransformer) ranks
             the target by tiger.score_items among all items, or among itself + ``--eval_num_neg`` sampled negatives, at any k
Single device.  ``--fp16``, ``--bf16``, ``--deepspeed`` and ``--resume_from_checkpoint`` are refused by name; gradient accumulation
is not built (``--per_device_batch_size`` is the step's batch).  ``--pack_rows`` (default off) runs the encoder side of training,
of the evaluation loss and of the test on the rows' own tokens, without the padding tokens (tiger.TIGER.forward(packed=True))."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

from . import ops, schedule, tiger, tiger_eval
from .decode import ItemTrie
from .metrics import get_metrics_results, get_topk_results
from .seqrec_data import EncoderDecoderCollator, SeqRecData, T5_EOS_ID

DEFAULT_METRICS = "hit@1,hit@5,hit@10,ndcg@5,ndcg@10"


def add_pack_rows(ap):
    ap.add_argument("--pack_rows", action="store_true",
                    help="run the encoder side on the rows' own tokens, without the padding tokens (tiger.TIGER.forward(packed=True))")


def pack_kwargs(a, batch):
    """the ``packed`` / ``lengths`` arguments of a collated batch: the lengths are read from the mask on the host, before the upload"""
    if not getattr(a, "pack_rows", False):
        return {}
    return dict(packed=True, lengths=tiger.packed_lengths(batch["attention_mask"]))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gamer_amd.train_tiger")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--backbone", default="TIGER")
    ap.add_argument("--base_model", default="./config/s2s-models/TIGER")
    ap.add_argument("--output_dir", default="./checkpoint/decoder")
    ap.add_argument("--data_path", default="./data")
    ap.add_argument("--tasks", default="seqrec")
    ap.add_argument("--dataset", default="Instruments")
    ap.add_argument("--index_file", default=".index.json")
    ap.add_argument("--max_his_len", type=int, default=20)
    ap.add_argument("--optim", default="adamw_torch")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--learning_rate", type=float, default=5e-4)
    ap.add_argument("--per_device_batch_size", type=int, default=256)
    ap.add_argument("--model_max_length", type=int, default=512)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--warmup_ratio", type=float, default=0.1)
    ap.add_argument("--lr_scheduler_type", default="cosine")
    ap.add_argument("--patience", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--resume_from_checkpoint", default=None)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--deepspeed", default=None)
    ap.add_argument("--only_test", action="store_true")
    ap.add_argument("--num_beams", type=int, default=20)
    ap.add_argument("--test_batch_size", type=int, default=32)
    ap.add_argument("--metrics", default=DEFAULT_METRICS)
    ap.add_argument("--results_file", default="./results/test-decoder.json")
    add_pack_rows(ap)
    tiger_eval.add_eval_flags(ap)
    a = ap.parse_args(argv)
    for name in ("fp16", "bf16", "deepspeed", "resume_from_checkpoint"):
        if getattr(a, name):
            raise NotImplementedError(f"--{name} is not supported by train_tiger (fp32, single device, training from the start)")
    if a.backbone != "TIGER":
        raise NotImplementedError(f"--backbone {a.backbone}: train_tiger trains TIGER")
    if a.tasks != "seqrec":
        raise NotImplementedError(f"--tasks {a.tasks}: only seqrec")
    if a.lr_scheduler_type != "cosine":
        raise NotImplementedError(f"--lr_scheduler_type {a.lr_scheduler_type}: only cosine (gamer_amd/schedule.py)")
    if a.optim not in ("adamw_torch", "adamw"):
        raise NotImplementedError(f"--optim {a.optim}: only AdamW (gamer_adamw)")
    if not 1 <= a.model_max_length <= tiger.MAX_LONG_ENCODER_LEN:
        raise NotImplementedError(f"--model_max_length {a.model_max_length}: the encoder runs at most {tiger.MAX_LONG_ENCODER_LEN} tokens "
                                  f"on the HIP path (tiger.MAX_LONG_ENCODER_LEN)")
    return a


class FlatAdamW:
    """HF Trainer's update on gamer_adamw: the parameters become views of one flat buffer, the decayed ones first (every weight but
    the layer norms'), so that one launch pair clips by the global norm and steps every tensor."""

    def __init__(self, model, weight_decay, max_norm=1.0, betas=(0.9, 0.999), eps=1e-8):
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        self.params = [p for n, p in named if "layer_norm" not in n] + [p for n, p in named if "layer_norm" in n]
        self.n_decay = sum(p.numel() for n, p in named if "layer_norm" not in n)
        dev = self.params[0].device
        self.flat = torch.cat([p.data.reshape(-1) for p in self.params]).contiguous()
        off = 0
        for p in self.params:
            p.data = self.flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self.grad = torch.zeros_like(self.flat)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.wd, self.max_norm, self.betas, self.eps, self.step_n = weight_decay, max_norm, betas, eps, 0
        self.partial = torch.empty(256, dtype=torch.float32, device=dev)
        self.norm = torch.empty(1, dtype=torch.float32, device=dev)

    def step(self, lr):
        self.step_n += 1
        off = 0
        for p in self.params:
            n = p.numel()
            if p.grad is None:
                self.grad[off:off + n].zero_()
            else:
                self.grad[off:off + n].copy_(p.grad.reshape(-1))
            off += n
        ops.sumsq(self.grad, self.partial)
        ops.adamw(self.flat, self.grad, self.m, self.v, self.n_decay, lr, self.betas[0], self.betas[1], self.eps, self.wd, self.step_n,
                  self.max_norm, 1.0, self.partial, self.norm)


def _batches(samples, collator, batch_size, order=None):
    order = list(range(len(samples))) if order is None else order
    for i in range(0, len(order), batch_size):
        yield collator(samples, order[i:i + batch_size])


def eval_loss(model, samples, collator, batch_size, dev, a=None):
    """the evaluation loss as HF's Trainer reports it: the mean over the batches of the batch's loss"""
    model.eval()
    losses = []
    with torch.no_grad():
        for b in _batches(samples, collator, batch_size):
            loss, _ = model(b["input_ids"].to(dev), b["attention_mask"].to(dev), labels=b["labels"].to(dev), want_logits=False,
                            **pack_kwargs(a, b))
            losses.append(loss)
    return float(torch.stack(losses).mean())


def test(model, data, collator, a, dev):
    """test_decoder.py's loop: beams over the trie of all items, hit / ndcg against the held-out item"""
    metrics = a.metrics.split(",")
    c = model.config
    item_toks = [data.item_tok[data.item_ptr[i]:data.item_ptr[i + 1]].tolist() for i in range(len(data.item_ptr) - 1)]
    lens = {len(t) for t in item_toks}
    if len(lens) != 1:
        raise NotImplementedError("train_tiger: the items of the index file must all have the same number of tokens")
    item_len = lens.pop()
    trie = ItemTrie([[c.decoder_start_token_id] + t + [T5_EOS_ID] for t in item_toks], device=dev, pad_token_id=c.pad_token_id)
    samples = data.samples("test", a.max_his_len)
    totals, n = {m: 0.0 for m in metrics}, 0
    model.eval()
    if tiger_eval.ranked(a):
        return test_ranked(model, samples, collator, a, dev, item_toks, metrics)
    for b in _batches(samples, collator, a.test_batch_size):
        seqs, scores = tiger.beam_search(model, b["input_ids"].to(dev), b["attention_mask"].to(dev), trie, a.num_beams, item_len + 1,
                                         **pack_kwargs(a, b))
        pred = seqs[:, 1:1 + item_len].cpu().tolist()
        labels = b["labels"][:, :item_len].tolist()
        targets = [[row] for row in labels]
        topk = get_topk_results(pred, scores.cpu().tolist(), targets, a.num_beams)
        for m, v in get_metrics_results(topk, metrics, targets).items():
            totals[m] += v
        n += len(targets)
    return {m: totals[m] / max(n, 1) for m in metrics}


def test_ranked(model, samples, collator, a, dev, item_toks, metrics):
    """--eval_mode exact / sampled: the held-out item ranked by tiger.score_items among all distinct items of the index file, or
    among itself + --eval_num_neg negatives drawn outside the sample's history; the scored tokens are the beam search's (item +
    </s>)"""
    catalogue = tiger_eval.distinct_rows(item_toks)
    index = {tuple(r): i for i, r in enumerate(catalogue.tolist())}
    row_of = [index[tuple(t)] for t in item_toks]                                 # item row of the data layer -> catalogue row
    items = torch.cat([catalogue, torch.full((len(catalogue), 1), T5_EOS_ID, dtype=torch.int64)], 1)
    generator = torch.Generator().manual_seed(a.seed)
    totals, n = {m: 0.0 for m in metrics}, 0
    for i in range(0, len(samples), a.test_batch_size):
        sel = list(range(i, min(i + a.test_batch_size, len(samples))))
        b = collator(samples, sel)
        ids, am, kw = b["input_ids"].to(dev), b["attention_mask"].to(dev), pack_kwargs(a, b)
        tg = [[row_of[int(samples.target[s])]] for s in sel]
        hist = [{row_of[int(j)] for j in samples.hist[samples.ptr[s]:samples.ptr[s + 1]]} for s in sel]
        targets = [[catalogue[t[0]].tolist()] for t in tg]
        sums, _, _ = tiger_eval.rank_batch(lambda it: tiger.score_items(model, ids, am, it, **kw), items, a.eval_mode, tg, hist, targets,
                                           metrics, a.eval_num_neg, generator)
        for m in metrics:
            totals[m] += sums[m]
        n += len(sel)
    return {m: totals[m] / max(n, 1) for m in metrics}


def run(a, tag, data, collator, test_fn, make_model=None):
    """The train-and-test loop of the TIGER commands (train_tiger, train_tiger_smb, train_tiger_mb).  ``data``: ``vocab_size`` and
    ``samples(mode, max_his_len)``; ``collator(samples, index)`` -> input_ids / attention_mask / labels; ``test_fn(model, data,
    collator, a, dev)`` -> (what goes to ``--results_file``, its one-line summary).  ``a.gradient_accumulation_steps`` (where the
    command has the flag) micro-batches share one update, each weighing 1 / steps as HF's Trainer scales them; the last group of an
    epoch may be shorter.  ``make_model(a, data)``: another backbone with TIGER's surface (train_pbatransformer), on the CPU with its
    vocabulary sized; a model with ``check_inputs()`` has it called after every epoch."""
    random.seed(a.seed)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    dev = torch.device("cuda")
    os.makedirs(a.output_dir, exist_ok=True)
    if make_model is None:
        config = tiger.TigerConfig.from_pretrained(a.base_model)
        model = tiger.TIGER(config)
        model.set_hyper(a.temperature)
        model.resize_token_embeddings(data.vocab_size)
    else:
        model = make_model(a, data)
    model.to(dev)
    ckpt = os.path.join(a.output_dir, "best_model.pth")
    accum = getattr(a, "gradient_accumulation_steps", 1)
    if not a.only_test:
        train, valid = data.samples("train", a.max_his_len), data.samples("valid", a.max_his_len)
        batches_per_epoch = (len(train) + a.per_device_batch_size - 1) // a.per_device_batch_size
        steps_per_epoch = (batches_per_epoch + accum - 1) // accum
        total = steps_per_epoch * a.epochs
        warmup = schedule.warmup_steps_for(total, a.warmup_ratio)
        opt = FlatAdamW(model, a.weight_decay)
        g = torch.Generator().manual_seed(a.seed)
        best, patience, step = float("inf"), 0, 0
        print(f"[{tag}] {len(train)} training samples, {len(valid)} validation samples, vocabulary {data.vocab_size}", flush=True)
        for epoch in range(a.epochs):
            model.train()
            losses = []
            order = torch.randperm(len(train), generator=g).tolist()
            for n, b in enumerate(_batches(train, collator, a.per_device_batch_size, order)):
                if n % accum == 0:
                    for p in model.parameters():
                        p.grad = None
                loss, _ = model(b["input_ids"].to(dev), b["attention_mask"].to(dev), labels=b["labels"].to(dev), **pack_kwargs(a, b))
                (loss if accum == 1 else loss / accum).backward()
                losses.append(loss.detach())
                if (n + 1) % accum == 0 or n + 1 == batches_per_epoch:
                    opt.step(schedule.cosine_with_warmup(step, a.learning_rate, warmup, total))
                    step += 1
            if hasattr(model, "check_inputs"):
                model.check_inputs()
            ev = eval_loss(model, valid, collator, a.per_device_batch_size, dev, a)
            print(f"[{tag}] epoch {epoch + 1}/{a.epochs} loss {float(torch.stack(losses).mean()):.4f} eval_loss {ev:.4f}", flush=True)
            if ev < best:
                best, patience = ev, 0
                torch.save(model.state_dict(), ckpt)
            else:
                patience += 1
                if patience >= a.patience:
                    print(f"[{tag}] early stopping on epoch {epoch + 1}", flush=True)
                    break
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    results, line = test_fn(model, data, collator, a, dev)
    results = tiger_eval.tag_results(results, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.results_file)), exist_ok=True)
    with open(a.results_file, "w") as f:
        json.dump(results, f, indent=4)
    print(f"[{tag}] {line}; results saved to {a.results_file}", flush=True)
    return results


def _test_and_line(model, data, collator, a, dev):
    results = test(model, data, collator, a, dev)
    return results, " ".join(f"{m} {v:.4f}" for m, v in results.items())


def main(argv=None):
    a = parse_args(argv)
    data = SeqRecData(a.data_path, a.dataset, a.index_file)
    return run(a, "train_tiger", data, EncoderDecoderCollator(data, a.model_max_length), _test_and_line)


if __name__ == "__main__":
    main(sys.argv[1:])
