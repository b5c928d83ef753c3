"""Real-data ingestion for the MB decoder path (plain multi-behaviour data, ``train_MB_decoder``): the reference's datasets +
tokenizer + collator restated as a pre-tokeniser that emits id tensors directly, bit for bit (``tests/test_mb_data.py``
against ``tests/golden/mb_data_small.npz``, generated from the real classes by ``tools/make_golden_mb_data.py``).

Reference behaviour restated:
  on-disk format            ref:SeqRec/datasets/MB_dataset.py:56-74 (``<name>.MB.inter.json`` user -> item ids,
                            ``.MB.behavior.json`` user -> behaviour names, ``.behavior_level.json``, the index file);
                            the target behaviour is the only one of the highest level
  samples                   MB_dataset.py:94-148 (train: every prefix of the interactions before the last two; valid: the
                            second-to-last interaction; the history is the ``max_his_len`` items before the target,
                            ``filter_target`` drops repeats of the target item at a lower behaviour level)
  item strings              MBDataset (item tokens only), MBExplicitDataset (behaviour token first, or last for
                            ``mb_explicit_back``), MBExplicitDatasetForDecoder (one full sequence per user plus ``augment``
                            down-sampled copies, numpy's stream seeded with 42, MB_dataset.py:282-341)
  tasks                     ref:SeqRec/datasets/loading_MB.py:9-135 (one task; the validation set each task pairs with)
  vocabulary                MB_dataset.py:150-161 + train_MB_decoder.py:251 (``tokenizer.add_tokens(sorted(new))`` on top of
                            ref:config/s2s-models/Qwen3Moe/vocab.json, which is Qwen3Multi's)
  collator                  ref:SeqRec/datasets/collator.py:47-107 with ``only_train_response = not
                            isinstance(dataset, MBExplicitDatasetForDecoder)`` (train_MB_decoder.py:260-263): right
                            padding, pad -> -100, no behaviour token ignored, the history masked with
                            ``only_train_response`` and in validation batches
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .data import IGNORE_INDEX, PAD_TOKEN, TokenTable, _pad_batch

TASKS = ("mb", "mb_explicit", "mb_explicit_filter", "mb_explicit_decoder", "mb_explicit_back")


@dataclass
class MBSamples:
    """Samples in flat (CSR) form: sample n owns ``tokens[ptr[n]:ptr[n+1]]`` (history + target item), of which the first
    ``n_history[n]`` are the history."""
    mode: str
    ptr: np.ndarray
    tokens: np.ndarray
    n_history: np.ndarray
    behavior: list

    def __len__(self) -> int:
        return len(self.ptr) - 1


def _task_kind(task: str):
    """(dataset kind, behaviour first, filter_target, augment, decoder) of one loading_MB.py task."""
    t = task.lower()
    if t == "mb":
        return "plain", True, False, None, False
    if t == "mb_explicit":
        return "explicit", True, False, None, False
    if t == "mb_explicit_filter":
        return "explicit", True, True, None, False
    if t.startswith("mb_explicit_decoder"):
        if t == "mb_explicit_decoder":
            return "explicit", True, True, None, True
        if not t.startswith("mb_explicit_decoder_"):
            raise ValueError(f"invalid task {task!r} for multi-behavior explicit decoder")
        augment = int(t.split("_")[3])
        if augment < 1:
            raise ValueError("augment must be greater than or equal to 1")
        return "explicit", True, True, augment, True
    if t == "mb_explicit_back":
        return "explicit", False, False, None, False
    raise NotImplementedError(f"task {task!r}: one of {TASKS} (mb_explicit_decoder_N for augmentation)")


class MBData:
    """One dataset directory in the reference's MB format, read for one task (``load_MB_datasets`` with one task)."""

    def __init__(self, data_path: str, dataset: str, task: str, index_file: str = ".index.json",
                 base_vocab: Optional[Dict[str, int]] = None, pad_token: str = PAD_TOKEN):
        d = os.path.join(data_path, dataset)

        def load(suffix):
            with open(os.path.join(d, dataset + suffix)) as f:
                return json.load(f)
        self.task = task.lower()
        self.kind, self.behavior_first, self.filter_target, self.augment, self.decoder = _task_kind(task)
        self.inters: Dict[str, List[int]] = load(".MB.inter.json")
        self.history_behaviors: Dict[str, List[str]] = load(".MB.behavior.json")
        self.indices: Dict[str, List[str]] = load(index_file)
        if not os.path.exists(os.path.join(d, dataset + ".behavior_level.json")):
            raise FileNotFoundError(f"Behavior level file {d}/{dataset}.behavior_level.json does not exist.")
        self.behavior_level: Dict[str, int] = load(".behavior_level.json")
        top = max(self.behavior_level.values())
        targets = [b for b, lv in self.behavior_level.items() if lv == top]
        if len(targets) != 1:
            raise ValueError(f"Expected exactly one target behavior with max level, but found {len(targets)}: {targets}")
        self.target_behavior = targets[0]
        self.max_behavior_level = top
        self.behaviors = list(self.behavior_level)
        new = {t for idx in self.indices.values() for t in idx}
        if self.kind == "explicit":
            new |= {self.behavior_token(b) for b in self.behaviors}
        self.new_tokens = sorted(new)
        self.tokens = TokenTable(self.new_tokens, base_vocab, pad_token)
        self.item_ids = {k: np.array([self.tokens[t] for t in v], dtype=np.int64) for k, v in self.indices.items()}
        self.behavior_token_ids = ({b: self.tokens[self.behavior_token(b)] for b in self.behaviors}
                                   if self.kind == "explicit" else {})
        # tokens per item as the model sees them (train_MB_decoder.py:326-352: the tokenized behaviour item)
        self.token_count = len(next(iter(self.indices.values()))) + (1 if self.kind == "explicit" else 0)

    @staticmethod
    def behavior_token(behavior: str) -> str:
        return f"<behavior_{behavior}>"

    @property
    def use_behavior_token(self) -> bool:
        """train_MB_decoder.py:339-342: the target behaviour's item carries a behaviour token."""
        return self.kind == "explicit"

    def _item(self, item: int, behavior: str) -> np.ndarray:
        ids = self.item_ids[str(item)]
        if self.kind != "explicit":
            return ids
        b = np.array([self.behavior_token_ids[behavior]], dtype=np.int64)
        return np.concatenate([b, ids] if self.behavior_first else [ids, b])

    def _history(self, items: List[int], behaviors: List[str], max_his_len: int, filter_target: bool) -> List[np.ndarray]:
        """BaseMBDataset._get_inters (MB_dataset.py:94-108) as item rows."""
        target_item, target_behavior = items[-1], behaviors[-1]
        if max_his_len > 0:
            items, behaviors = items[-(max_his_len + 1):-1], behaviors[-(max_his_len + 1):-1]
        if filter_target:
            keep = [i for i in range(len(items)) if items[i] != target_item or
                    self.behavior_level[behaviors[i]] >= self.behavior_level[target_behavior]]
            items, behaviors = [items[i] for i in keep], [behaviors[i] for i in keep]
        return [self._item(i, b) for i, b in zip(items, behaviors)]

    def _augment(self, rng: np.random.RandomState, items: List[int], behaviors: List[str]):
        """MBExplicitDatasetForDecoder._augment_interactions (MB_dataset.py:282-318)."""
        if not self.augment:
            return [items], [behaviors]
        ratios = np.arange(1, self.augment + 1) / self.augment
        by_beh = {b: [i for i, x in enumerate(behaviors) if x == b] for b in self.behavior_level}
        out_i, out_b = [items], [behaviors]
        for ratio in ratios:
            if ratio == 0:
                continue
            drop = []
            for b, level in self.behavior_level.items():
                if level == self.max_behavior_level or not by_beh.get(b):
                    continue
                n = int(len(by_beh[b]) * (ratio / (level + 1)))
                if n > 0:
                    drop.extend(rng.choice(by_beh[b], n, replace=False).tolist())
            mask = np.ones(len(items), dtype=bool)
            mask[drop] = False
            ki = np.array(items)[mask].tolist()
            kb = np.array(behaviors)[mask].tolist()
            if len(ki) < 2:
                continue
            out_i.append(ki)
            out_b.append(kb)
        return out_i, out_b

    def _build(self, mode: str, rows) -> MBSamples:
        lens, parts, nh, beh = [0], [], [], []
        for hist, target, b in rows:
            seq = hist + [target]
            parts.extend(seq)
            lens.append(sum(len(x) for x in seq))
            nh.append(sum(len(x) for x in hist))
            beh.append(b)
        tok = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        return MBSamples(mode, np.cumsum(lens).astype(np.int64), tok.astype(np.int64), np.array(nh, np.int64), beh)

    def train_samples(self, max_his_len: int) -> MBSamples:
        """The task's training set (loading_MB.py:16-78)."""
        rows = []
        if self.decoder:
            rng = np.random.RandomState(42)           # set_seed(42): numpy's global stream (MB_dataset.py:321)
            for uid in self.inters:
                items, behaviors = self.inters[uid][:-2], self.history_behaviors[uid][:-2]
                for it, bs in zip(*self._augment(rng, items, behaviors)):
                    rows.append((self._history(it, bs, max_his_len, True), self._item(it[-1], bs[-1]), bs[-1]))
        else:
            for uid in self.inters:
                items, behaviors = self.inters[uid][:-2], self.history_behaviors[uid][:-2]
                for i in range(1, len(items)):
                    rows.append((self._history(items[:i + 1], behaviors[:i + 1], max_his_len, self.filter_target),
                                 self._item(items[i], behaviors[i]), behaviors[i]))
        return self._build("train", rows)

    def valid_samples(self, max_his_len: int) -> MBSamples:
        """The validation set load_MB_datasets pairs with the task (loading_MB.py:80-135): the decoder tasks validate on
        MBExplicitDataset with filter_target."""
        rows = []
        for uid in self.inters:
            items, behaviors = self.inters[uid], self.history_behaviors[uid]
            rows.append((self._history(items[:-1], behaviors[:-1], max_his_len, self.filter_target),
                         self._item(items[-2], behaviors[-2]), behaviors[-2]))
        return self._build("valid", rows)

    @property
    def only_train_response(self) -> bool:
        """train_MB_decoder.py:261: the loss covers the target item only, except for MBExplicitDatasetForDecoder."""
        return not self.decoder


class MBCollator:
    """DecoderOnlyCollator (collator.py:47-107) on MB id arrays: no behaviour token is ignored in the labels."""

    def __init__(self, data: MBData, model_max_length: int = 1024):
        self.data = data
        self.pad_id = data.tokens.pad_id
        self.model_max_length = model_max_length

    def train(self, samples: MBSamples, index: Sequence[int], only_train_response: Optional[bool] = None
              ) -> Dict[str, torch.Tensor]:
        """Right padding; labels = ids with pad -> -100; the history is masked as well with ``only_train_response``
        (default: the task's, train_MB_decoder.py:261) and in a validation batch."""
        if only_train_response is None:
            only_train_response = self.data.only_train_response
        sel = np.asarray(index, dtype=np.int64)
        ids, lens, L = _pad_batch(samples.ptr, samples.tokens, sel, self.pad_id, False, np.int64)
        if L > self.model_max_length:
            raise ValueError(f"sequence of {L} tokens exceeds model_max_length={self.model_max_length} "
                             "(the reference truncates silently; lower max_his_len instead)")
        am = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        labels = ids.copy()
        labels[ids == self.pad_id] = IGNORE_INDEX
        if samples.mode == "valid" or only_train_response:
            labels[np.arange(L)[None, :] < samples.n_history[sel][:, None]] = IGNORE_INDEX
        res = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(am), "labels": torch.from_numpy(labels)}
        res["behavior"] = [samples.behavior[n] for n in sel]
        res["split"] = samples.mode
        return res


def qwen3moe_config(data: MBData, max_his_len: int, base_model: Optional[str] = None, config_cls=None, **overrides):
    """The config of ``--backbone Qwen3Moe`` (train_MB_decoder.py:251-252, 326-362): config.json (``base_model`` DIR, or this
    project's copy of the reference's defaults) with the tokenizer's vocabulary, behaviour token id -> index in
    ``behaviors`` order, behaviour tokens or not, tokens per item, the routing mode's expert count, n_positions =
    max_his_len + 1.  ``mb_explicit_back`` is refused: its behaviour token ends the item, and the router reads behaviour
    tokens at item starts (router.py:97-120).  ``config_cls``: a subclass of ``Qwen3MoeConfig`` (``--backbone Qwen3MoeAction``)."""
    from .config import Qwen3MoeConfig, apply_mb_runtime_fields
    config_cls = config_cls or Qwen3MoeConfig
    if data.kind == "explicit" and not data.behavior_first:
        raise ValueError("task mb_explicit_back puts the behaviour token last; the Qwen3Moe router reads behaviour tokens "
                         "at item starts - use --backbone Qwen3 for this task")
    cfg = config_cls.from_pretrained(base_model) if base_model else config_cls()
    cfg.vocab_size, cfg.pad_token_id = len(data.tokens), data.tokens.pad_id
    for k, v in overrides.items():
        setattr(cfg, k, v)
    bmaps = {data.behavior_token_ids[b]: i for i, b in enumerate(data.behaviors)} if data.use_behavior_token else {}
    return apply_mb_runtime_fields(cfg, len(bmaps), bmaps, data.use_behavior_token, data.token_count, max_his_len)
