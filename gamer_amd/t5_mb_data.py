"""The SMB and MB multi-behaviour data of ``train_SMB_decoder`` / ``train_MB_decoder`` for the encoder-decoder backbone (TIGER): the
T5 vocabulary on top of data.SMBData / mb_data.MBData and the reference's encoder-decoder collators on id arrays, bit for bit
(``tests/test_tiger_smb_data.py`` / ``tests/test_tiger_mb_data.py`` against fixtures that ``tools/make_golden_tiger_smb.py`` generates
from the real datasets, ``T5Tokenizer(legacy=True)`` and collators).

Reference behaviour restated:
  vocabulary        ``T5Tokenizer`` of ref:config/s2s-models/TIGER (32,100 entries: <pad> 0, </s> 1, <unk> 2, the pieces, 100
                    <extra_id_*>) + ``add_tokens(first_dataset.get_new_tokens())`` (train_SMB_decoder.py:251): ids 32100, 32101, ...
                    in sorted order, the behaviour tokens among them for the explicit datasets.  A new token that is already a
                    piece would keep the piece's id in the reference and shift every id after it; it is refused here.
  train / valid     ref:SeqRec/datasets/collator.py:7-44 (``EncoderDecoderCollator``): input_ids = the history's tokens + </s>,
                    labels = the target's tokens + </s>, each cut to the first ``model_max_length - 1`` tokens + </s>, right-padded
                    with 0 to the batch's longest row; pad positions of the labels -> -100; an empty history is the row [</s>]
  test              collator.py:110-146 (``EncoderDecoderTestCollator``): the encoder inputs, the target items per sample, the
                    behaviours, and for SMB the history's items without behaviour tokens (test_SMB_decoder.py:215-223)
  SMB tasks         ref:SeqRec/datasets/loading_SMB.py: training ``smb_explicit`` (SMBExplicitDataset, one sample per interaction)
                    and ``smb_explicit_decoder[_N]`` (SMBExplicitDatasetForDecoder, one sequence per user + N thinned copies), both
                    validated on SMBExplicitDataset; test task ``smb_explicit``.  The others need layouts data.SMBData does not
                    hold (no leading behaviour token, thinned evaluation histories) and are refused by name.
  MB tasks          ref:SeqRec/datasets/loading_MB.py: the five of mb_data.TASKS (+ ``mb_explicit_decoder_N``); test tasks ``mb``,
                    ``mb_explicit``, ``mb_explicit_filter`` (MB_dataset.py:145-156: the last interaction given everything before)
Collation slices the flat arrays of a sample set at once (no loop over the items of a row)."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .data import IGNORE_INDEX, SMBData, SampleSet
from .mb_data import MBData, MBSamples
from .seqrec_data import T5_BASE_VOCAB, T5_EOS_ID, T5_PAD_ID

T5_PAD_TOKEN = "<pad>"
SMB_TRAIN_TASKS = ("smb_explicit", "smb_explicit_decoder")            # (+ smb_explicit_decoder_N)
SMB_TEST_TASKS = ("smb_explicit",)
SMB_REFUSED_TRAIN = ("smb", "smb_explicit_back", "smb_augment_")
SMB_REFUSED_TEST = ("smb", "smb_explicit_back", "smb_augment_", "smb_explicit_valid", "smb_valid_augment_", "smb_drop_gt")
MB_TEST_TASKS = ("mb", "mb_explicit", "mb_explicit_filter")


def t5_base_vocab(base_model: Optional[str] = None) -> Dict[str, int]:
    """token -> id of the 32,100-entry T5 vocabulary.  With ``base_model``/tokenizer.json (what the reference ships next to
    config.json) the real pieces, so that a new token that is already a piece is found; otherwise the special tokens under their
    names (<pad>, </s>, <unk>, <extra_id_0..99> from the top down) and a placeholder for every other id."""
    path = os.path.join(base_model, "tokenizer.json") if base_model else None
    if path and os.path.exists(path):
        with open(path) as f:
            tj = json.load(f)
        vocab = {piece: i for i, (piece, _) in enumerate(tj["model"]["vocab"])}
        for t in tj.get("added_tokens", []):
            vocab.setdefault(t["content"], t["id"])
        if len(vocab) != T5_BASE_VOCAB or vocab.get(T5_PAD_TOKEN) != T5_PAD_ID or vocab.get("</s>") != T5_EOS_ID:
            raise ValueError(f"{path}: expected the T5 vocabulary of {T5_BASE_VOCAB} entries with <pad> = 0 and </s> = 1, got "
                             f"{len(vocab)} entries")
        return vocab
    vocab = {f"<t5_piece_{i}>": i for i in range(T5_BASE_VOCAB)}
    named = {T5_PAD_TOKEN: T5_PAD_ID, "</s>": T5_EOS_ID, "<unk>": 2}
    named.update({f"<extra_id_{k}>": T5_BASE_VOCAB - 1 - k for k in range(100)})
    for t, i in named.items():
        del vocab[f"<t5_piece_{i}>"]
        vocab[t] = i
    return vocab


def _check_new_tokens(new_tokens: Sequence[str], base: Dict[str, int]):
    taken = [t for t in new_tokens if t in base]
    if taken:
        raise ValueError(f"new tokens that are already T5 pieces: {taken[:5]} (add_tokens would keep their ids and shift the rest)")


def max_row_tokens(max_his_len: int, token_count: int) -> int:
    """the longest encoder row of a layout: ``max_his_len`` items of ``token_count`` tokens + </s>"""
    return max_his_len * token_count + 1


def largest_max_his_len(limit: int, token_count: int) -> int:
    return (limit - 1) // token_count


def _smb_kind(task: str):
    """(per interaction, augment) of one supported training task; NotImplementedError naming a refused one"""
    t = task.lower()
    if t == "smb_explicit":
        return True, None
    if t == "smb_explicit_decoder":
        return False, None
    if t.startswith("smb_explicit_decoder_"):
        return False, int(t.split("_")[3])
    if t in SMB_REFUSED_TRAIN or t.startswith("smb_augment_"):
        raise NotImplementedError(f"--tasks {task}: not built for TIGER (refused: smb, smb_explicit_back, smb_augment_*; data.SMBData "
                                  f"holds the layout with a leading behaviour token only); one of {SMB_TRAIN_TASKS} or smb_explicit_decoder_N")
    raise NotImplementedError(f"--tasks {task}: one of {SMB_TRAIN_TASKS} or smb_explicit_decoder_N")


def check_smb_test_task(task: str) -> str:
    t = task.lower()
    if t in SMB_TEST_TASKS:
        return t
    if t in SMB_REFUSED_TEST or t.startswith(("smb_augment_", "smb_valid_augment_")):
        raise NotImplementedError(f"--test_task {task}: not built for TIGER (refused: smb, smb_explicit_back, smb_augment_*, "
                                  f"smb_explicit_valid, smb_valid_augment_*, smb_drop_gt); only {SMB_TEST_TASKS[0]}")
    raise NotImplementedError(f"--test_task {task}: only {SMB_TEST_TASKS[0]}")


class T5SMBData:
    """One SMB dataset directory at the T5 vocabulary, read for one training task (``load_SMB_datasets`` with one task)."""

    def __init__(self, data_path: str, dataset: str, task: str = "smb_explicit", index_file: str = ".index.json",
                 base_model: Optional[str] = None):
        self.task = task.lower()
        self.per_interaction, self.augment = _smb_kind(task)
        base = t5_base_vocab(base_model)
        self.smb = SMBData(data_path, dataset, index_file, base_vocab=base, pad_token=T5_PAD_TOKEN)
        _check_new_tokens(self.smb.new_tokens, base)
        self.new_tokens = self.smb.new_tokens
        self.tokens = self.smb.tokens
        self.vocab_size = len(self.tokens)
        self.behaviors = self.smb.behaviors
        self.behavior_token_ids = self.smb.behavior_token_ids
        self.sole_item_len, self.token_count = self.smb.sole_item_len, self.smb.token_count

    def samples(self, mode: str, max_his_len: int) -> SampleSet:
        if mode == "train":
            if self.per_interaction:
                return self.smb.train_samples_per_interaction(max_his_len)
            return self.smb.train_samples(max_his_len, self.augment)
        if mode == "valid":
            return self.smb.valid_samples(max_his_len)
        if mode == "test":
            return self.smb.test_samples(max_his_len)
        raise NotImplementedError(mode)

    def trie_sequences(self, behavior: str, decoder_start: int = T5_PAD_ID) -> List[List[int]]:
        """test_SMB_decoder.py:496-499: [decoder_start] + <behavior><item tokens> + </s> of every distinct item"""
        return [[decoder_start] + row + [T5_EOS_ID] for row in self.smb.candidate_tokens(behavior).tolist()]

    def collision_info(self, samples: SampleSet) -> Dict[str, float]:
        """check_collision_items (test_SMB_decoder.py:66-88): the items whose token string another item has too"""
        seen, coll = set(), set()
        for toks in self.smb._indices.values():
            row = tuple(self.tokens[t] for t in toks)
            (coll if row in seen else seen).add(row)
        hits = sum(1 for tg in samples.targets for item in tg.tolist() if tuple(item) in coll)
        n = len(samples)
        return {"total": n, "collision_items": len(coll), "collision_samples": hits, "collision_ratio": hits / n if n else 0.0}


class T5MBData:
    """One MB dataset directory at the T5 vocabulary, read for one task (``load_MB_datasets`` with one task)."""

    def __init__(self, data_path: str, dataset: str, task: str = "mb_explicit", index_file: str = ".index.json",
                 base_model: Optional[str] = None):
        base = t5_base_vocab(base_model)
        self.mb = MBData(data_path, dataset, task, index_file, base_vocab=base, pad_token=T5_PAD_TOKEN)
        _check_new_tokens(self.mb.new_tokens, base)
        self.task = self.mb.task
        self.new_tokens = self.mb.new_tokens
        self.tokens = self.mb.tokens
        self.vocab_size = len(self.tokens)
        self.behaviors = self.mb.behaviors
        self.target_behavior = self.mb.target_behavior
        self.behavior_token_ids = self.mb.behavior_token_ids
        self.token_count = self.mb.token_count

    def samples(self, mode: str, max_his_len: int) -> MBSamples:
        if mode == "train":
            return self.mb.train_samples(max_his_len)
        if mode == "valid":
            return self.mb.valid_samples(max_his_len)
        if mode == "test":
            return self.test_samples(max_his_len)
        raise NotImplementedError(mode)

    def test_samples(self, max_his_len: int, behavior: Optional[str] = None) -> MBSamples:
        """BaseMBDataset._process_test_data (MB_dataset.py:145-156): the last interaction given everything before it; with
        ``behavior`` only the users whose last interaction has it (filter_by_behavior)."""
        d = self.mb
        if d.task not in MB_TEST_TASKS:
            raise NotImplementedError(f"test task {d.task}: one of {MB_TEST_TASKS}")
        rows = []
        for uid in d.inters:
            items, behaviors = d.inters[uid], d.history_behaviors[uid]
            if behavior is not None and behaviors[-1] != behavior:
                continue
            rows.append((d._history(items, behaviors, max_his_len, d.filter_target), d._item(items[-1], behaviors[-1]), behaviors[-1]))
        return d._build("test", rows)

    def trie_sequences(self, behavior: str, decoder_start: int = T5_PAD_ID) -> List[List[int]]:
        """test_MB_decoder.py:345-348: [decoder_start] + the behaviour's item tokens + </s> of every distinct item"""
        d = self.mb
        rows = {tuple(d._item(int(k), behavior).tolist()) for k in d.indices}
        return [[decoder_start] + list(r) + [T5_EOS_ID] for r in sorted(rows)]

    def decoder_prefix(self, decoder_start: int = T5_PAD_ID) -> List[int]:
        """test_MB_decoder.py:109-111 for the target behaviour: [decoder_start] + its behaviour token (none for ``mb``)"""
        d = self.mb
        return [decoder_start] + ([d.behavior_token_ids[d.target_behavior]] if d.kind == "explicit" else [])

    def collision_info(self, samples: MBSamples) -> Dict[str, float]:
        d = self.mb
        seen, coll = set(), set()
        for toks in d.indices.values():
            s = "".join(toks)
            (coll if s in seen else seen).add(s)
        coll_rows = {tuple(d.item_ids[k].tolist()) for k, toks in d.indices.items() if "".join(toks) in coll}
        n_item = len(next(iter(d.indices.values())))
        hits = 0
        for n in range(len(samples)):
            tgt = samples.tokens[samples.ptr[n] + samples.n_history[n]:samples.ptr[n + 1]].tolist()
            item = tgt[1:] if d.kind == "explicit" and d.behavior_first else tgt[:n_item]
            hits += tuple(item) in coll_rows
        n = len(samples)
        return {"total": n, "collision_items": len(coll), "collision_samples": hits, "collision_ratio": hits / n if n else 0.0}


def _eos_rows(flat: np.ndarray, start: np.ndarray, lens: np.ndarray, max_len: int) -> np.ndarray:
    """rows ``flat[start[r]:start[r] + lens[r]]`` cut to max_len - 1 tokens, each followed by </s>, right-padded with 0"""
    lens = np.minimum(lens, max_len - 1).astype(np.int64)
    L = int(lens.max()) + 1 if len(lens) else 1
    out = np.full((len(lens), L), T5_PAD_ID, dtype=np.int64)
    col = np.arange(L)[None, :]
    m = col < lens[:, None]
    out[m] = flat[(start[:, None] + col)[m]]
    out[np.arange(len(lens)), lens] = T5_EOS_ID
    return out


class EncDecCollator:
    """EncoderDecoderCollator / EncoderDecoderTestCollator on the flat arrays of a SampleSet or MBSamples."""

    def __init__(self, model_max_length: int = 1024, token_count: Optional[int] = None):
        if model_max_length < 1:
            raise ValueError("model_max_length must be at least 1")
        self.max_len = int(model_max_length)
        self.token_count = token_count

    def __call__(self, samples, index: Sequence[int]) -> Dict[str, object]:
        """collator.py:13-44.  ``samples`` of mode train / valid: tokens = history + target."""
        if samples.mode not in ("train", "valid"):
            raise ValueError("EncDecCollator(samples, index) collates training and validation samples; use .test for test samples")
        sel = np.asarray(index, dtype=np.int64)
        start, nh = samples.ptr[sel], samples.n_history[sel]
        ids = _eos_rows(samples.tokens, start, nh, self.max_len)
        labels = _eos_rows(samples.tokens, start + nh, samples.ptr[sel + 1] - start - nh, self.max_len)
        labels[labels == T5_PAD_ID] = IGNORE_INDEX
        return {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy((ids != T5_PAD_ID).astype(np.int64)),
                "labels": torch.from_numpy(labels), "split": samples.mode, "behavior": [samples.behavior[n] for n in sel]}

    def test(self, samples, index: Sequence[int]):
        """collator.py:116-146 -> (inputs, targets).  SMB test samples (tokens = the history): targets[b] = the token rows of
        the sample's target items, inputs["inters_item_list"][b] = the history's item rows without behaviour tokens.  MB test
        samples (tokens = history + target): targets[b] = [the target's tokens]."""
        sel = np.asarray(index, dtype=np.int64)
        start, nh = samples.ptr[sel], samples.n_history[sel]
        ids = _eos_rows(samples.tokens, start, nh, self.max_len)
        inputs = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy((ids != T5_PAD_ID).astype(np.int64)),
                  "behavior": [samples.behavior[n] for n in sel]}
        if getattr(samples, "targets", None) is not None:
            tc = self.token_count
            if tc is None:
                raise ValueError("EncDecCollator.test on SMB samples needs token_count (behaviour token + item tokens)")
            inputs["inters_item_list"] = [samples.tokens[a:a + h].reshape(-1, tc)[:, 1:] for a, h in zip(start, nh)]
            targets = [samples.targets[n] for n in sel]
        else:
            targets = [samples.tokens[a + h:b][None, :] for a, h, b in zip(start, nh, samples.ptr[sel + 1])]
        return inputs, targets
