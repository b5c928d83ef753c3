#!/usr/bin/env python3
"""Golden fixture of the MB data layer (tests/golden/mb_data_small.npz), generated from the REAL reference.

Writes ``synthetic.write_mb_dataset`` (seeded, deterministic) to a temporary directory, loads it with the reference's
``load_MB_datasets`` for every MB task (MBDataset, MBExplicitDataset, MBExplicitDatasetForDecoder), extends the reference's
Qwen2Tokenizer (config/s2s-models/Qwen3Moe) with ``get_new_tokens()`` as train_MB_decoder.py:251 does, and collates every
training sample and every validation sample with ``DecoderOnlyCollator(tokenizer, only_train_response=...)`` as
train_MB_decoder.py:260-263 sets it.  Stored per task: the vocabulary, the samples' behaviours, and the collated
input_ids / attention_mask / labels of the training set (in sample order, batches of 7) and of the validation set.

Usage:  python tools/make_golden_mb_data.py     (needs the reference checkout; CPU only)
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402

TASKS = ["mb", "mb_explicit", "mb_explicit_filter", "mb_explicit_decoder", "mb_explicit_decoder_3", "mb_explicit_back"]
MAX_HIS, BATCH, NAME = 6, 7, "MBTiny"


def main():
    _ref_loader.load_reference_classes()          # (shims and package stubs)
    import importlib
    loading = importlib.import_module("SeqRec.datasets.loading_MB")
    MBds = importlib.import_module("SeqRec.datasets.MB_dataset")
    from SeqRec.datasets.collator import DecoderOnlyCollator
    from transformers import Qwen2Tokenizer
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_mb_dataset(tmp, NAME)
        # transformers 5.x's Qwen2Tokenizer refuses the reference's merges.txt next to its 14-entry vocab.json ("Token out
        # of vocabulary"); every string here consists of ADDED tokens, split off before BPE, so the merges never apply:
        # the reference's vocab.json + tokenizer_config.json with an empty merge list (as oracle/make_golden_data.py)
        tdir = os.path.join(tmp, "_tokenizer")
        os.makedirs(tdir)
        src = os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "Qwen3Moe")
        for fn in ("vocab.json", "tokenizer_config.json"):
            shutil.copy(os.path.join(src, fn), os.path.join(tdir, fn))
        with open(os.path.join(tdir, "merges.txt"), "w") as f:
            f.write("#version: 0.2\n")
        for task in TASKS:
            train, valid = loading.load_MB_datasets(dataset=NAME, data_path=tmp, max_his_len=MAX_HIS,
                                                    index_file=".index.json", tasks=task)
            first = train.datasets[0]
            tok = Qwen2Tokenizer.from_pretrained(tdir, model_max_length=1024)
            tok.add_tokens(first.get_new_tokens())
            coll = DecoderOnlyCollator(tok, only_train_response=not isinstance(first, MBds.MBExplicitDatasetForDecoder))
            t = task
            res[f"{t}::vocab_tokens"] = np.array(first.get_new_tokens())
            res[f"{t}::vocab_ids"] = np.array(tok.convert_tokens_to_ids(first.get_new_tokens()), dtype=np.int64)
            res[f"{t}::vocab_size"] = np.int64(len(tok))
            for split, ds in (("train", train), ("valid", valid)):
                samples = [ds[i] for i in range(len(ds))]
                res[f"{t}::{split}_behavior"] = np.array([s["behavior"] for s in samples])
                ids, am, lab = [], [], []
                for b0 in range(0, len(samples), BATCH):
                    out = coll(samples[b0:b0 + BATCH])
                    L = out["input_ids"].shape[1]
                    pad = lambda x, v: np.pad(x.numpy(), ((0, 0), (0, 64 - L)), constant_values=v)
                    assert L <= 64
                    ids.append(pad(out["input_ids"], -1))
                    am.append(pad(out["attention_mask"], -1))
                    lab.append(pad(out["labels"], -1))
                res[f"{t}::{split}_input_ids"] = np.concatenate(ids).astype(np.int16)
                res[f"{t}::{split}_attention_mask"] = np.concatenate(am).astype(np.int8)
                res[f"{t}::{split}_labels"] = np.concatenate(lab).astype(np.int16)
                print(task, split, len(samples))
    res["meta_json"] = np.array(json.dumps(dict(tasks=TASKS, max_his_len=MAX_HIS, batch=BATCH, name=NAME,
                                                width=64, fill=-1)))
    path = os.path.join(ROOT, "tests", "golden", "mb_data_small.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
