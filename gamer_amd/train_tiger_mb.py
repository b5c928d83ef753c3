"""``python -m gamer_amd.train_tiger_mb``: train and test TIGER on the plain multi-behaviour (MB) data on the HIP engine.

Mirrors ``TrainMBDecoder.invoke`` (ref:SeqRec/tasks/train_MB_decoder.py) for ``--backbone TIGER`` and, with ``--only_test`` or after
training, the target-behaviour evaluation of ``TestMBDecoder`` (ref:SeqRec/tasks/test_MB_decoder.py, EvaluationType.TARGET_BEHAVIOR):
  data       t5_mb_data.T5MBData / EncDecCollator; ``--tasks`` one of mb_data.TASKS (mb_explicit_decoder_N for augmentation)
  training   train_tiger.run: the loop of ``python -m gamer_amd.train_tiger`` with ``--gradient_accumulation_steps``
  testing    ``--test_task`` mb, mb_explicit or mb_explicit_filter (default: the one that matches ``--tasks``; the decoder tasks
             are tested on mb_explicit_filter, the set they are validated on): the users whose last interaction has the target
             behaviour; the decoder starts from [decoder_start, <behavior_target>] ([decoder_start] alone for ``mb``) and searches
             the trie of the target behaviour's items until </s>; hit / ndcg against the held-out item (metrics.py)
The reference's other two evaluation types (behaviour specific, behaviour item) and ``--filter`` are not built; a task whose
behaviour token follows the item (mb_explicit_back) trains and validates but has no evaluation: the decoder prefix above cannot
name its behaviour, so ``--only_test`` is refused for it and its results file holds an empty list (the command says so).
``--max_his_len`` is refused at parse time when its longest row exceeds tiger.MAX_LONG_ENCODER_LEN and ``--model_max_length`` (default
512 here) does not cut it.  Single device, fp32; ``--fp16``,
``--bf16``, ``--deepspeed`` and ``--resume_from_checkpoint`` are refused by name."""
from __future__ import annotations

import argparse
import sys

import torch

from . import mb_data, t5_mb_data, tiger, tiger_eval
from .decode import ItemTrie
from .metrics import get_metrics_results, get_topk_results
from .train_tiger import pack_kwargs
from .train_tiger_smb import add_train_flags, check_row_limit, check_train_flags

DEFAULT_METRICS = "hit@1,hit@5,hit@10,ndcg@5,ndcg@10"


def default_test_task(task: str) -> str:
    kind, first, filt, _, decoder = mb_data._task_kind(task)
    if kind == "plain":
        return "mb"
    if not first:
        raise NotImplementedError(f"--tasks {task}: the behaviour token follows the item, which the target-behaviour evaluation's decoder "
                                  "prefix [decoder_start, <behavior>] cannot express; no evaluation for this task")
    return "mb_explicit_filter" if filt or decoder else "mb_explicit"


def parse_args(argv=None, item_tokens: int = 4):
    """``item_tokens``: index tokens per item (4 in the shipped index files); main() checks the row limit again with the
    dataset's own count"""
    ap = argparse.ArgumentParser(prog="python -m gamer_amd.train_tiger_mb")
    add_train_flags(ap, 512)
    ap.add_argument("--only_test", action="store_true")
    ap.add_argument("--num_beams", type=int, default=20)
    ap.add_argument("--test_batch_size", type=int, default=16)
    ap.add_argument("--metrics", default=DEFAULT_METRICS)
    ap.add_argument("--results_file", default="./results/test.json")
    ap.add_argument("--test_task", default=None)
    ap.add_argument("--filter", action="store_true")
    a = ap.parse_args(argv)
    check_train_flags(a, "train_tiger_mb")
    if a.filter:
        raise NotImplementedError("--filter (dropping the test samples whose target collides) is not built")
    if a.tasks == "seqrec":
        raise NotImplementedError(f"--tasks seqrec: python -m gamer_amd.train_tiger trains it; train_tiger_mb takes one of {mb_data.TASKS}")
    kind = mb_data._task_kind(a.tasks)
    if a.test_task is None:
        if kind[0] == "explicit" and not kind[1]:
            if a.only_test:
                default_test_task(a.tasks)
        else:
            a.test_task = default_test_task(a.tasks)
    elif a.test_task.lower() not in t5_mb_data.MB_TEST_TASKS:
        raise NotImplementedError(f"--test_task {a.test_task}: one of {t5_mb_data.MB_TEST_TASKS}")
    else:
        a.test_task = a.test_task.lower()
        if (mb_data._task_kind(a.test_task)[0] == "explicit") != (kind[0] == "explicit"):
            raise ValueError(f"--test_task {a.test_task} and --tasks {a.tasks} do not share a vocabulary (behaviour tokens)")
    check_row_limit(a.max_his_len, item_tokens + (1 if kind[0] == "explicit" else 0), a.model_max_length)
    return a


def test(model, data, collator, a, dev):
    """test_single_type(..., EvaluationType.TARGET_BEHAVIOR) -> ([the "Target Behavior" row], its text)"""
    metrics = a.metrics.split(",")
    if a.test_task is None:
        return [], f"no evaluation for --tasks {a.tasks} (the behaviour token follows the item)"
    c = model.config
    td = t5_mb_data.T5MBData(a.data_path, a.dataset, a.test_task, a.index_file, a.base_model)
    if td.tokens.vocab != data.tokens.vocab:
        raise ValueError(f"--test_task {a.test_task} and --tasks {a.tasks} do not share a vocabulary")
    samples = td.test_samples(a.max_his_len, td.target_behavior)
    if len(samples) == 0:
        raise ValueError(f"no test sample of the target behaviour {td.target_behavior}")
    trie = ItemTrie(td.trie_sequences(td.target_behavior, c.decoder_start_token_id), device=dev, pad_token_id=c.pad_token_id)
    prefix = torch.tensor(td.decoder_prefix(c.decoder_start_token_id), dtype=torch.int64)
    P, K = len(prefix), td.token_count
    steps = 1 + K + 1 - P                                                     # the rest of the item + </s>
    totals, n = {m: 0.0 for m in metrics}, 0
    model.eval()
    if tiger_eval.ranked(a):
        # --eval_mode exact / sampled: the target behaviour's catalogue (rows as the targets hold them, behaviour token included;
        # the history is matched on the item tokens alone: its items carry their own behaviours) scored by tiger.score_items on
        # the tokens the search generates, the rest of the row after the prefix + </s>
        catalogue = tiger_eval.distinct_rows(r[1:-1] for r in td.trie_sequences(td.target_behavior, c.decoder_start_token_id))
        index = {tuple(r): j for j, r in enumerate(catalogue.tolist())}
        by_item = {r[P - 1:]: j for r, j in index.items()}
        items = torch.cat([catalogue[:, P - 1:], torch.full((len(catalogue), 1), t5_mb_data.T5_EOS_ID, dtype=torch.int64)], 1)
        generator = torch.Generator().manual_seed(a.seed)
    for i in range(0, len(samples), a.test_batch_size):
        inputs, targets = collator.test(samples, range(i, min(i + a.test_batch_size, len(samples))))
        if tiger_eval.ranked(a):
            ids, am, kw = inputs["input_ids"].to(dev), inputs["attention_mask"].to(dev), pack_kwargs(a, inputs)
            hist = [set(tiger_eval.rows_to_items(by_item, tiger_eval.history_rows(samples, s, K, P - 1)))
                    for s in range(i, min(i + a.test_batch_size, len(samples)))]
            sums, _, _ = tiger_eval.rank_batch(lambda it: tiger.score_items(model, ids, am, it, decoder_prefix=prefix, **kw), items,
                                               a.eval_mode, [tiger_eval.rows_to_items(index, t, strict=True) for t in targets], hist, targets,
                                               metrics, a.eval_num_neg, generator)
            for m in metrics:
                totals[m] += sums[m]
            n += len(targets)
            continue
        seqs, scores = tiger.beam_search(model, inputs["input_ids"].to(dev), inputs["attention_mask"].to(dev), trie, a.num_beams, steps,
                                         decoder_prefix=prefix, **pack_kwargs(a, inputs))
        pred = seqs[:, 1:1 + K].cpu().tolist()
        topk = get_topk_results(pred, scores.cpu().tolist(), targets, a.num_beams)
        for m, v in get_metrics_results(topk, metrics, targets).items():
            totals[m] += v
        n += len(targets)
    row = {m: totals[m] / n for m in metrics}
    line = f"target behaviour {td.target_behavior}: {n} samples " + " ".join(f"{m} {row[m]:.4f}" for m in metrics)
    row["eval_type"] = "Target Behavior"
    row["collision_info"] = td.collision_info(samples)
    return [row], line


def main(argv=None):
    from . import train_tiger
    a = parse_args(argv)
    data = t5_mb_data.T5MBData(a.data_path, a.dataset, a.tasks, a.index_file, a.base_model)
    check_row_limit(a.max_his_len, data.token_count, a.model_max_length)
    return train_tiger.run(a, "train_tiger_mb", data, t5_mb_data.EncDecCollator(a.model_max_length), test)


if __name__ == "__main__":
    main(sys.argv[1:])
