"""``python -m gamer_amd.train_pbatransformer``: train and test PBATransformer on the session-wise multi-behaviour (SMB) data on the
HIP engine.

Mirrors the ``--backbone PBATransformer`` branch of ``TrainSMBDecoder.invoke`` (ref:SeqRec/tasks/train_SMB_decoder.py:205-218,
279-316) and ``TestSMBDecoder`` on top of ``python -m gamer_amd.train_tiger_smb``: its flags, data (t5_mb_data.T5SMBData), collator,
training loop and per-behaviour test (trie beam search from [decoder_start, <behavior_b>]) are that command's.  What this one adds
is the model's configuration from the data, as the reference derives it:
  behavior_maps        behaviour token id -> index, in the dataset's behaviour order; num_behavior their count
  use_behavior_token   whether the dataset has behaviour tokens; without them injection is turned off in both stacks
  num_positions        the tokens of one history item (behaviour token + index tokens); num_experts follows from it
  n_positions          ``--max_his_len``;  use_user_token False
``--base_model`` holds the config.json of ref:config/s2s-models/PBATransformer.  ``--pack_rows`` is refused (the routers read the
padded rows).  The MB (train_MB_decoder) and plain sequential (train_decoder) variants of the backbone are not built.
"""
from __future__ import annotations

import sys

from . import pbatransformer, t5_mb_data, train_tiger, train_tiger_smb

TAG = "train_pbatransformer"


def parse_args(argv=None, token_count: int = 5):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gamer_amd.train_pbatransformer")
    train_tiger_smb.add_train_flags(ap, 1024)
    ap.set_defaults(backbone="PBATransformer", base_model="./config/s2s-models/PBATransformer", tasks="smb_explicit")
    ap.add_argument("--only_test", action="store_true")
    ap.add_argument("--num_beams", type=int, default=20)
    ap.add_argument("--test_batch_size", type=int, default=16)
    ap.add_argument("--metrics", default=train_tiger_smb.DEFAULT_METRICS)
    ap.add_argument("--results_file", default="./results/test.json")
    ap.add_argument("--test_task", default="smb_explicit")
    ap.add_argument("--behaviors", nargs="+", default=None)
    a = ap.parse_args(argv)
    train_tiger_smb.check_train_flags(a, TAG, backbone="PBATransformer")
    if a.pack_rows:
        raise NotImplementedError("--pack_rows: PBATransformer's routers read the padded rows; packed rows are not built")
    t = a.tasks.lower()
    if t == "seqrec" or t.startswith("mb"):
        raise NotImplementedError(f"--tasks {a.tasks}: the train_decoder (seqrec) and train_MB_decoder (mb_*) variants of PBATransformer "
                                  f"are not built; train_pbatransformer takes smb_explicit or smb_explicit_decoder[_N]")
    t5_mb_data._smb_kind(a.tasks)
    a.test_task = t5_mb_data.check_smb_test_task(a.test_task)
    train_tiger_smb.check_row_limit(a.max_his_len, token_count, a.model_max_length)
    return a


def derive_config(config: pbatransformer.PBATransformerConfig, data, max_his_len: int) -> pbatransformer.PBATransformerConfig:
    """train_SMB_decoder.py:279-312: what the reference sets on the config from the dataset before it builds the model"""
    tokens = [data.behavior_token_ids[b] for b in data.behaviors] if data.behavior_token_ids else []
    config.behavior_maps = {int(t): i for i, t in enumerate(tokens)}
    config.num_behavior = len(tokens)
    config.use_behavior_token = len(tokens) > 0
    if not config.use_behavior_token:
        config.behavior_injection = False
        config.behavior_injection_encoder, config.behavior_injection_decoder = [], []
    config.num_positions = int(data.token_count)
    config.derive_num_experts()
    config.n_positions = int(max_his_len)
    config.use_user_token = False
    return config


def make_model(a, data):
    config = derive_config(pbatransformer.PBATransformerConfig.from_pretrained(a.base_model), data, a.max_his_len)
    print(f"[{TAG}] num_positions {config.num_positions}, {config.num_experts} experts, {config.num_behavior} behaviours, sparse layers "
          f"{config.sparse_layers_encoder} / {config.sparse_layers_decoder}, injection in {config.behavior_injection_encoder} / "
          f"{config.behavior_injection_decoder}", flush=True)
    model = pbatransformer.PBATransformerForConditionalGeneration(config)
    model.set_hyper(a.temperature)
    model.resize_token_embeddings(data.vocab_size)
    return model


def test(model, data, collator, a, dev):
    out = train_tiger_smb.test(model, data, collator, a, dev)
    model.check_inputs()
    return out


def main(argv=None):
    a = parse_args(argv)
    data = t5_mb_data.T5SMBData(a.data_path, a.dataset, a.tasks, a.index_file, a.base_model)
    if a.max_his_len <= 0:
        raise NotImplementedError("--max_his_len must be positive: it is the model's n_positions")
    train_tiger_smb.check_row_limit(a.max_his_len, data.token_count, a.model_max_length)
    collator = t5_mb_data.EncDecCollator(a.model_max_length, data.token_count)
    return train_tiger.run(a, TAG, data, collator, test, make_model=make_model)


if __name__ == "__main__":
    main(sys.argv[1:])
