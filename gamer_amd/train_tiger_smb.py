"""``python -m gamer_amd.train_tiger_smb``: train and test TIGER on the session-wise multi-behaviour (SMB) data on the HIP engine.

Mirrors ``TrainSMBDecoder.invoke`` (ref:SeqRec/tasks/train_SMB_decoder.py) for ``--backbone TIGER`` and, with ``--only_test`` or after
training, ``TestSMBDecoder`` (ref:SeqRec/tasks/test_SMB_decoder.py:90-302):
  data       t5_mb_data.T5SMBData / EncDecCollator: the T5 vocabulary + the sorted index and behaviour tokens; ``--tasks``
             smb_explicit (one sample per interaction) or smb_explicit_decoder[_N] (one sequence per user + N thinned copies)
  training   train_tiger.run: the loop of ``python -m gamer_amd.train_tiger`` with ``--gradient_accumulation_steps``
  testing    per behaviour b (all of them, or ``--behaviors``): the users with a b interaction in their last session; the decoder
             starts from [decoder_start, <behavior_b>] and searches ``--num_beams`` beams over the trie of b's items for the item's
             tokens (no </s> step); hit / recall / ndcg against the user's b targets (metrics.py), "Avg. Duplicate Ratio" (the share
             of a user's distinct predicted items that the history holds), and the merged row weighted by the sample counts
``--model_max_length`` is taken as given (the reference's default, 1024, only cuts rows); what is refused at parse time is a
``--max_his_len`` whose longest row, max_his_len x (item tokens + behaviour token) + 1, exceeds tiger.MAX_LONG_ENCODER_LEN while
``--model_max_length`` does not cut it to that length.
Single device, fp32; ``--fp16``, ``--bf16``, ``--deepspeed`` and ``--resume_from_checkpoint`` are refused by name."""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import t5_mb_data, tiger, tiger_eval
from .decode import ItemTrie
from .metrics import get_metrics_results, get_topk_results

DEFAULT_METRICS = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10"


def add_train_flags(ap, model_max_length: int):
    """the flags of parse_global_args, parse_dataset_args and the train_SMB_decoder / train_MB_decoder parsers, their defaults"""
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
    ap.add_argument("--gradient_accumulation_steps", type=int, default=2)
    ap.add_argument("--logging_step", type=int, default=30)
    ap.add_argument("--model_max_length", type=int, default=model_max_length)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--resume_from_checkpoint", default=None)
    ap.add_argument("--warmup_ratio", type=float, default=0.1)
    ap.add_argument("--lr_scheduler_type", default="cosine")
    ap.add_argument("--save_and_eval_strategy", default="epoch")
    ap.add_argument("--save_and_eval_steps", type=int, default=1000)
    ap.add_argument("--patience", type=int, default=20)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--deepspeed", default=None)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--wandb_run_name", default="default")
    from .train_tiger import add_pack_rows
    add_pack_rows(ap)
    tiger_eval.add_eval_flags(ap)


def check_train_flags(a, prog: str, backbone: str = "TIGER"):
    for name in ("fp16", "bf16", "deepspeed", "resume_from_checkpoint"):
        if getattr(a, name):
            raise NotImplementedError(f"--{name} is not supported by {prog} (fp32, single device, training from the start)")
    if a.backbone != backbone:
        raise NotImplementedError(f"--backbone {a.backbone}: {prog} trains {backbone}")
    if a.lr_scheduler_type != "cosine":
        raise NotImplementedError(f"--lr_scheduler_type {a.lr_scheduler_type}: only cosine (gamer_amd/schedule.py)")
    if a.optim not in ("adamw_torch", "adamw"):
        raise NotImplementedError(f"--optim {a.optim}: only AdamW (gamer_adamw)")
    if a.save_and_eval_strategy != "epoch":
        raise NotImplementedError(f"--save_and_eval_strategy {a.save_and_eval_strategy}: the model is evaluated and saved per epoch")
    if a.gradient_accumulation_steps < 1 or a.model_max_length < 1:
        raise ValueError("--gradient_accumulation_steps and --model_max_length must be at least 1")


def check_row_limit(max_his_len: int, token_count: int, model_max_length: int):
    """the longest row a layout can produce (max_his_len items + </s>, cut to model_max_length) against the encoder's limit"""
    limit = tiger.MAX_LONG_ENCODER_LEN
    if model_max_length <= limit:
        return
    if max_his_len <= 0 or t5_mb_data.max_row_tokens(max_his_len, token_count) > limit:
        rows = "unbounded" if max_his_len <= 0 else f"up to {max_his_len} x {token_count} + 1 = {t5_mb_data.max_row_tokens(max_his_len, token_count)}"
        raise NotImplementedError(f"--max_his_len {max_his_len}: encoder rows of {rows} tokens (--model_max_length {model_max_length} does not "
                                  f"cut them); TIGER's encoder runs at most {limit} tokens on the HIP path (tiger.MAX_LONG_ENCODER_LEN), the "
                                  f"largest --max_his_len that fits at {token_count} tokens per item is "
                                  f"{t5_mb_data.largest_max_his_len(limit, token_count)}")


def parse_args(argv=None, token_count: int = 5):
    """``token_count``: tokens per history item (4 index tokens + the behaviour token in the shipped index files); main() checks
    the row limit again with the dataset's own count"""
    ap = argparse.ArgumentParser(prog="python -m gamer_amd.train_tiger_smb")
    add_train_flags(ap, 1024)
    ap.add_argument("--only_test", action="store_true")
    ap.add_argument("--num_beams", type=int, default=20)
    ap.add_argument("--test_batch_size", type=int, default=16)
    ap.add_argument("--metrics", default=DEFAULT_METRICS)
    ap.add_argument("--results_file", default="./results/test.json")
    ap.add_argument("--test_task", default="smb_explicit")
    ap.add_argument("--behaviors", nargs="+", default=None)
    a = ap.parse_args(argv)
    check_train_flags(a, "train_tiger_smb")
    if a.tasks == "seqrec":
        raise NotImplementedError("--tasks seqrec: python -m gamer_amd.train_tiger trains it; train_tiger_smb takes smb_explicit or "
                                  "smb_explicit_decoder[_N]")
    t5_mb_data._smb_kind(a.tasks)
    a.test_task = t5_mb_data.check_smb_test_task(a.test_task)
    check_row_limit(a.max_his_len, token_count, a.model_max_length)
    return a


def duplicate_ratio(pred_items: Sequence[Sequence[int]], history_items: Sequence[Sequence[int]]) -> float:
    """test_SMB_decoder.py:218-223 for one user: the share of the distinct predicted items that occur in the history"""
    out = {tuple(int(t) for t in it) for it in pred_items}
    hist = {tuple(int(t) for t in it) for it in history_items}
    return len(out & hist) / len(out) if out else 0


def merge_rows(rows: List[Dict[str, float]], counts: Sequence[int], metrics: Sequence[str]) -> Dict[str, float]:
    """test_SMB_decoder.py:287-304: the per-behaviour rows weighted by their sample counts"""
    merged = {m: 0.0 for m in metrics}
    total = 0
    for row, n in zip(rows, counts):
        for m in metrics:
            merged[m] += row[m] * n
        total += n
    for m in merged:
        merged[m] /= total
    merged["eval_type"] = "Merged Behavior"
    return merged


def test_behavior(model, data, samples, collator, a, dev, behavior: str) -> Dict[str, float]:
    """test_single_behavior (test_SMB_decoder.py:90-285) on ``samples`` = test_samples.filter_by_behavior(behavior)"""
    from .train_tiger import pack_kwargs
    metrics = a.metrics.split(",")
    c = model.config
    K = data.sole_item_len
    trie = ItemTrie(data.trie_sequences(behavior, c.decoder_start_token_id), device=dev, pad_token_id=c.pad_token_id)
    prefix = torch.tensor([c.decoder_start_token_id, data.behavior_token_ids[behavior]], dtype=torch.int64)
    totals, ratios, n = {m: 0.0 for m in metrics}, [], 0
    if tiger_eval.ranked(a):
        # --eval_mode exact / sampled: the behaviour's catalogue (or the targets + negatives outside the history) scored by
        # tiger.score_items on the tokens the search generates; the duplicate ratio is that of the num_beams best candidates
        catalogue = tiger_eval.distinct_rows(data.smb.candidate_tokens(behavior)[:, 1:])
        index = {tuple(r): j for j, r in enumerate(catalogue.tolist())}
        generator = torch.Generator().manual_seed(a.seed)
    for i in range(0, len(samples), a.test_batch_size):
        inputs, targets = collator.test(samples, range(i, min(i + a.test_batch_size, len(samples))))
        if tiger_eval.ranked(a):
            ids, am, kw = inputs["input_ids"].to(dev), inputs["attention_mask"].to(dev), pack_kwargs(a, inputs)
            hist = [set(tiger_eval.rows_to_items(index, h)) for h in inputs["inters_item_list"]]
            sums, _, best = tiger_eval.rank_batch(lambda it: tiger.score_items(model, ids, am, it, decoder_prefix=prefix, **kw), catalogue,
                                                  a.eval_mode, [tiger_eval.rows_to_items(index, t, strict=True) for t in targets], hist, targets,
                                                  metrics, a.eval_num_neg, generator, top=a.num_beams)
            for m in metrics:
                totals[m] += sums[m]
            ratios += [len(set(r) & h) / len(set(r)) if r else 0 for r, h in zip(best, hist)]
            n += len(targets)
            continue
        # the trie's sequences end with </s>; the search stops after the item's tokens (max_new_tokens = sole_item_len)
        seqs, scores = tiger.beam_search(model, inputs["input_ids"].to(dev), inputs["attention_mask"].to(dev), trie, a.num_beams, K,
                                         decoder_prefix=prefix, **pack_kwargs(a, inputs))
        pred = seqs[:, 2:2 + K].cpu().tolist()
        topk = get_topk_results(pred, scores.cpu().tolist(), targets, a.num_beams)
        for m, v in get_metrics_results(topk, metrics, targets).items():
            totals[m] += v
        for b, hist in enumerate(inputs["inters_item_list"]):
            ratios.append(duplicate_ratio(pred[b * a.num_beams:(b + 1) * a.num_beams], hist))
        n += len(targets)
    res = {m: totals[m] / n for m in metrics}
    res["Avg. Duplicate Ratio"] = float(np.mean(ratios))
    return res


def test(model, data, collator, a, dev):
    """TestSMBDecoder.test: one row per behaviour and the merged row -> (rows, the merged row as text)"""
    metrics = a.metrics.split(",")
    base = data.samples("test", a.max_his_len)
    behaviors = a.behaviors if a.behaviors is not None else data.behaviors
    for b in behaviors:
        if b not in data.behaviors:
            raise ValueError(f"Behavior '{b}' is not in the dataset behaviors: {data.behaviors}")
    model.eval()
    rows, counts = [], []
    for b in behaviors:
        samples = base.filter_by_behavior(b)
        if len(samples) == 0:
            raise ValueError(f"behaviour {b}: no test sample (the reference divides by zero here)")
        row = test_behavior(model, data, samples, collator, a, dev, b)
        row["eval_type"] = f"Behavior {b}"
        row["collision_info"] = data.collision_info(samples)
        rows.append(row)
        counts.append(len(samples))
        print(f"[train_tiger_smb] behaviour {b}: {len(samples)} samples " + " ".join(f"{m} {row[m]:.4f}" for m in metrics[:2])
              + f" duplicate ratio {row['Avg. Duplicate Ratio']:.4f}", flush=True)
    merged = merge_rows(rows, counts, metrics)
    return rows + [merged], "merged " + " ".join(f"{m} {merged[m]:.4f}" for m in metrics)


def main(argv=None):
    from . import train_tiger
    a = parse_args(argv)
    data = t5_mb_data.T5SMBData(a.data_path, a.dataset, a.tasks, a.index_file, a.base_model)
    check_row_limit(a.max_his_len, data.token_count, a.model_max_length)
    collator = t5_mb_data.EncDecCollator(a.model_max_length, data.token_count)
    return train_tiger.run(a, "train_tiger_smb", data, collator, test)


if __name__ == "__main__":
    main(sys.argv[1:])
