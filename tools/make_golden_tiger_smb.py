#!/usr/bin/env python3
"""Golden fixtures of TIGER on the SMB / MB multi-behaviour data, generated from the REAL reference classes.

Three files under tests/golden/, all from datasets that ``synthetic.write_smb_dataset`` / ``write_mb_dataset`` write from a seed (the
tests write them again; the fixtures hold tensors and JSON only, and weight SEEDS, not tables):

tiger_smb_data.npz / tiger_mb_data.npz (CPU tests of gamer_amd/t5_mb_data.py)
  * per task: the reference's dataset (``load_SMB_datasets`` / ``load_MB_datasets``), ``T5Tokenizer(legacy=True)`` of
    config/s2s-models/TIGER + ``add_tokens(get_new_tokens())`` and ``EncoderDecoderCollator``: the new tokens and their ids, the
    sample counts, every training sample in a seeded shuffle in batches of 7 (smb_explicit has batches with empty histories; the
    augmented tasks hold their seeded copies) and the validation set cut by ``model_max_length`` 12;
  * the test sets through ``EncoderDecoderTestCollator``: inputs, target items, behaviours, the history's items;
  * per behaviour the reference's ``Trie`` + ``prefix_allowed_tokens_fn``: the allowed tokens at every prefix of three items;
  * ``train_SMB_decoder`` / ``train_MB_decoder`` / ``test_SMB_decoder`` / ``test_MB_decoder`` parser defaults;
  * the beams that the real ``generate`` returns below, scored by the reference's ``get_topk_results`` / ``get_metrics_results``, with
    the duplicate ratio and the merged row computed as test_SMB_decoder.py:218-223, 287-304 compute them.

tiger_smb.npz (GPU tests): the real ``TIGER`` class at d_model 64, 2 heads of 64, 2 + 2 layers, d_ff 128 (config C of
tools/make_golden_tiger_long.py) with the FULL vocabulary (32,100 + the new tokens), dropout off, temperature 0.7
  * SMB batches collated by the real collator from smb_explicit samples with histories of 0, 1, 7 and 25 items (every row <= 128
    tokens) and of 0, 1, 26 and max_his_len = 30 items (131 and 151 tokens), one mb_explicit batch: the loss, the logits at the
    labelled positions (the new tokens' columns, every 101st base column, fp64 sum of squares of all of them), every gradient as
    tiger_weights.sample_rows + fp64 checksums; of the shared table (whose every row has a gradient: it is the tied head) also the
    rows of every token the batch holds;
  * ``generate`` per behaviour as test_SMB_decoder.py runs it (prefix [0, <behavior>], that behaviour's trie, max_new_tokens =
    sole_item_len) at 4 and 20 beams for three users of different history length and two behaviours, and the MB target-behaviour
    call (max_new_tokens = 10, the trie ends with </s>) at 4 beams.  The weight seed is redrawn until the plain beam search finds
    generate's beams and neighbouring scores differ by more than make_golden_tiger.GAP; every candidate set holds >= 20 items.

Usage:  python tools/make_golden_tiger_smb.py      (needs the reference checkout; CPU only)
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_tiger as base  # noqa: E402
from make_golden_tiger import tw  # noqa: E402
import make_golden_tiger_long as long_  # noqa: E402
from oracle import _ref_loader  # noqa: E402
from gamer_amd import synthetic  # noqa: E402

GOLDEN = os.path.join(base.ROOT, "tests", "golden")
SMB_TASKS = ["smb_explicit", "smb_explicit_decoder", "smb_explicit_decoder_2"]
MB_TASKS = ["mb", "mb_explicit", "mb_explicit_filter", "mb_explicit_decoder", "mb_explicit_decoder_3", "mb_explicit_back"]
MB_TEST_TASKS = ["mb", "mb_explicit", "mb_explicit_filter"]
DATA = dict(smb=dict(name="SMBTiny", kw={}), mb=dict(name="MBTiny", kw={}))
MAX_HIS, BATCH, CUT, FILL, ORDER_SEED = 6, 7, 12, -7, 5
# the GPU fixture's datasets: users long enough for histories of 30 items
GPU_SMB = dict(name="SMBLong", kw=dict(n_users=60, n_items=80, codebook=16, max_sessions=14, max_per_session=4, seed=3))
GPU_MB = dict(name="MBLong", kw=dict(n_users=40, n_items=80, codebook=16, min_len=6, max_len=30, seed=4))
GPU_MAX_HIS = 30
SHORT_HIST, LONG_HIST = (0, 1, 7, 25), (0, 1, 26, 30)
BEAM_BEHAVIORS = ("click", "buy")
COL_STEP = 101
METRICS = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")


def tokenizer(new_tokens, model_max_length=1024):
    from transformers import T5Tokenizer
    tok = T5Tokenizer.from_pretrained(os.path.join(_ref_loader.REF_ROOT, "config", "s2s-models", "TIGER"), legacy=True,
                                      model_max_length=model_max_length)
    tok.add_tokens(new_tokens)
    return tok


def ids_of(tok, text):
    return tok(text, add_special_tokens=False)["input_ids"]


def block(t, width, fill=FILL):
    a = t.numpy()
    assert a.shape[1] <= width
    return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=fill)


def collate_all(ds, coll, order, width):
    ids, am, lab = [], [], []
    for b0 in range(0, len(order), BATCH):
        out = coll([ds[int(i)] for i in order[b0:b0 + BATCH]])
        ids.append(block(out["input_ids"], width)), am.append(block(out["attention_mask"], width)), lab.append(block(out["labels"], 8))
    return np.concatenate(ids).astype(np.int32), np.concatenate(am).astype(np.int8), np.concatenate(lab).astype(np.int32)


def trie_probe(Trie, fn_of, seqs):
    """the allowed tokens at every prefix of the first, the middle and the last sequence"""
    fn = fn_of(Trie(seqs))
    out = []
    for s in (seqs[0], seqs[len(seqs) // 2], seqs[-1]):
        out.append(dict(sequence=s, allowed=[sorted(fn(0, torch.tensor(s[:p]))) for p in range(1, len(s) + 1)]))
    return out


def task_defaults(module, cls, name):
    base._packages("SeqRec.tasks", "SeqRec.datasets", "SeqRec.utils")
    if "SeqRec.utils.logging" not in sys.modules:                      # (it installs loguru handlers on import; only a name is needed)
        stub = types.ModuleType("SeqRec.utils.logging")
        stub.replace_progress_callback = None
        sys.modules["SeqRec.utils.logging"] = stub
    task = getattr(importlib.import_module(f"SeqRec.tasks.{module}"), cls)
    parser = argparse.ArgumentParser()
    task.add_sub_parsers(parser.add_subparsers())
    return {k: v for k, v in vars(parser.parse_args([name])).items() if isinstance(v, (int, float, str, bool, type(None)))}


def data_fixture(kind, tmp, Trie, fn_of):
    from SeqRec.datasets.collator import EncoderDecoderCollator, EncoderDecoderTestCollator
    smb = kind == "smb"
    spec = DATA[kind]
    (synthetic.write_smb_dataset if smb else synthetic.write_mb_dataset)(tmp, spec["name"], **spec["kw"])
    loading = importlib.import_module("SeqRec.datasets.loading_SMB" if smb else "SeqRec.datasets.loading_MB")
    load = loading.load_SMB_datasets if smb else loading.load_MB_datasets
    res, meta = {}, dict(name=spec["name"], kw=spec["kw"], max_his_len=MAX_HIS, batch=BATCH, cut=CUT, fill=FILL, order_seed=ORDER_SEED,
                         tasks=SMB_TASKS if smb else MB_TASKS, width=MAX_HIS * 5 + 1)
    common = dict(dataset=spec["name"], data_path=tmp, max_his_len=MAX_HIS, index_file=".index.json")
    for task in meta["tasks"]:
        train, valid = load(tasks=task, **common)
        first = train.datasets[0]
        tok = tokenizer(first.get_new_tokens())
        res[f"{task}::vocab_tokens"] = np.array(first.get_new_tokens())
        res[f"{task}::vocab_ids"] = np.array(tok.convert_tokens_to_ids(first.get_new_tokens()), dtype=np.int64)
        res[f"{task}::vocab_size"] = np.int64(len(tok))
        order = np.random.RandomState(ORDER_SEED).permutation(len(train))
        ids, am, lab = collate_all(train, EncoderDecoderCollator(tok), order, meta["width"])
        res[f"{task}::train_input_ids"], res[f"{task}::train_attention_mask"], res[f"{task}::train_labels"] = ids, am, lab
        res[f"{task}::train_behavior"] = np.array([train[int(i)]["behavior"] for i in order])
        if task == "smb_explicit":
            assert any((ids[b0:b0 + BATCH, 0] == 1).all() for b0 in range(0, len(ids), BATCH)) or (ids[:, 0] == 1).any()
        cut = tokenizer(first.get_new_tokens(), CUT)
        ids, am, lab = collate_all(valid, EncoderDecoderCollator(cut), np.arange(len(valid)), meta["width"])
        assert ids.shape[0] == len(valid) and (ids != FILL).sum(1).max() == CUT
        res[f"{task}::valid_input_ids"], res[f"{task}::valid_attention_mask"], res[f"{task}::valid_labels"] = ids, am, lab
        print(kind, task, len(train), len(valid), "vocabulary", len(tok))
    # ---- the test sets and the tries
    tests = {}
    for task in (["smb_explicit"] if smb else MB_TEST_TASKS):
        ds = (loading.load_SMB_test_dataset if smb else loading.load_MB_test_dataset)(test_task=task, **common)
        tok = tokenizer(ds.get_new_tokens())
        coll = EncoderDecoderTestCollator(tok)
        ds.get_all_items()
        entry = {}
        for b in (ds.behaviors if smb else [ds.target_behavior]):
            sub = ds.filter_by_behavior(b)
            inputs, targets = coll([sub[i] for i in range(len(sub))])
            res[f"{task}::test::{b}::input_ids"] = inputs["input_ids"].numpy().astype(np.int32)
            res[f"{task}::test::{b}::attention_mask"] = inputs["attention_mask"].numpy().astype(np.int8)
            e = dict(behavior=inputs["behavior"])
            if smb:
                e["targets"] = [[ids_of(tok, t) for t in tg] for tg in targets]            # <behavior> + item tokens
                e["history_items"] = [[ids_of(tok, t) for t in h] for h in inputs["inters_item_list"]]
            else:
                e["targets"] = [ids_of(tok, t) for t in targets]
            cand = [[0] + s for s in tok(sorted(ds.get_all_items(b)))["input_ids"]]
            e["trie"] = trie_probe(Trie, fn_of, cand)
            e["n_candidates"] = len(cand)
            entry[b] = e
        tests[task] = entry
        if not smb:
            full, _ = coll([ds[i] for i in range(len(ds))])
            res[f"{task}::test::all::input_ids"] = full["input_ids"].numpy().astype(np.int32)
    meta["tests"] = tests
    return res, meta


# ---- the model fixture -----------------------------------------------------------------------------------------------------------------
def pick(ds, tok, hist_lens, tc):
    """the first sample of every wanted history length (in items)"""
    want, out = list(hist_lens), {}
    for i in range(len(ds)):
        n = len(ids_of(tok, ds[i]["input_ids"])) // tc
        if n in want and n not in out:
            out[n] = i
    assert set(out) == set(want), (sorted(out), want)
    return [out[n] for n in want]


def record_batch(fx, tag, model, name, batch, V):
    ids, am, labels = batch["input_ids"], batch["attention_mask"], batch["labels"]
    model.zero_grad()
    out = model(input_ids=ids, attention_mask=am, labels=labels)
    out.loss.backward()
    cols = np.concatenate([np.arange(0, 32100, COL_STEP), np.arange(32100, V)])
    rows = out.logits.detach()[labels != -100]
    fx.update({f"{tag}/input_ids": ids.numpy().astype(np.int32), f"{tag}/attention_mask": am.numpy().astype(np.int8),
               f"{tag}/labels": labels.numpy().astype(np.int32), f"{tag}/loss": np.asarray(float(out.loss)),
               f"{tag}/logit_cols": cols, f"{tag}/logits": rows[:, cols].numpy(),
               f"{tag}/logits_sumsq": np.asarray(float((rows.double() ** 2).sum()))})
    touched = torch.unique(torch.cat([ids.flatten(), labels[labels != -100], torch.tensor([0, 1])]))
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach()
        r = tw.sample_rows(g.shape)
        if k == "shared.weight":
            r = torch.unique(torch.cat([r, touched]))
            fx[f"{tag}/table_rows"] = r.numpy()
        fx[f"{tag}/grad/{k}"] = g[r].numpy()
        fx[f"{tag}/grad_checksum/{k}"] = tw.checksums({k: g})[0]


def search(model, fn, ids, am, prefix, nb, hf_new, steps):
    with torch.no_grad():
        o = model.generate(input_ids=ids, attention_mask=am, decoder_input_ids=prefix, max_new_tokens=hf_new, prefix_allowed_tokens_fn=fn,
                           num_beams=nb, num_return_sequences=nb, output_scores=True, return_dict_in_generate=True, early_stopping=True)
    s, sc, gap = base.plain_beam_search(model, ids, am, prefix, fn, nb, steps)
    if not torch.equal(s, o.sequences) or float((sc - o.sequences_scores).abs().max()) > 1e-5:
        raise RuntimeError(f"the plain beam search does not find generate's beams ({nb} beams)")
    return o.sequences, o.sequences_scores, gap


def model_fixture(tmp, TIGER, T5Config, Trie, fn_of):
    from SeqRec.datasets.collator import EncoderDecoderCollator, EncoderDecoderTestCollator
    from SeqRec.evaluation.ranking import get_metrics_results, get_topk_results
    fx, meta = {}, dict(temperature=base.TEMPERATURE, gap=base.GAP, max_his_len=GPU_MAX_HIS, smb=GPU_SMB, mb=GPU_MB, configs={},
                        short_hist=list(SHORT_HIST), long_hist=list(LONG_HIST), beam_behaviors=list(BEAM_BEHAVIORS), metrics=METRICS)
    synthetic.write_smb_dataset(tmp, GPU_SMB["name"], **GPU_SMB["kw"])
    synthetic.write_mb_dataset(tmp, GPU_MB["name"], **GPU_MB["kw"])
    lsmb = importlib.import_module("SeqRec.datasets.loading_SMB")
    lmb = importlib.import_module("SeqRec.datasets.loading_MB")
    common = dict(data_path=tmp, max_his_len=GPU_MAX_HIS, index_file=".index.json")
    # ---- SMB
    train, _ = lsmb.load_SMB_datasets(dataset=GPU_SMB["name"], tasks="smb_explicit", **common)
    tok = tokenizer(train.datasets[0].get_new_tokens())
    V = len(tok)
    short = pick(train, tok, SHORT_HIST, 5)
    long = pick(train, tok, LONG_HIST, 5)
    coll = EncoderDecoderCollator(tok)
    batches = {"short": coll([train[i] for i in short]), "long": coll([train[i] for i in long])}
    assert batches["short"]["input_ids"].shape[1] == 126 and batches["long"]["input_ids"].shape[1] == 151
    meta["short_index"], meta["long_index"] = short, long
    test = lsmb.load_SMB_test_dataset(dataset=GPU_SMB["name"], test_task="smb_explicit", **common)
    test.get_all_items()
    tcoll = EncoderDecoderTestCollator(tok)
    cfg = dict(long_.CONFIGS["c"], vocab_size=V)
    meta["configs"]["s"] = cfg
    wseed = 31
    while True:
        torch.manual_seed(0)
        model = TIGER(T5Config(**cfg))
        if not hasattr(model, "model_parallel"):
            model.model_parallel = False
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
        sd = tw.init_state_dict(shapes, wseed)
        model.load_state_dict(sd)
        model.set_hyper(base.TEMPERATURE)
        model.eval()
        gap, beams, rows, counts = float("inf"), {}, [], []
        for b in BEAM_BEHAVIORS:
            sub = test.filter_by_behavior(b)
            lens = [len(ids_of(tok, sub[i]["input_ids"])) for i in range(len(sub))]
            users = [int(np.argmin(lens)), int(np.argsort(lens)[len(lens) // 2]), int(np.argmax(lens))]
            assert len({lens[u] for u in users}) == 3
            inputs, targets = tcoll([sub[u] for u in users])
            cand = [[0] + s for s in tok(sorted(test.get_all_items(b)))["input_ids"]]
            assert len(cand) >= 20
            fn = fn_of(Trie(cand))
            prefix = torch.tensor([[0] + ids_of(tok, f"<behavior_{b}>")] * 3)
            beams[b] = dict(users=users, enc_lens=[lens[u] + 1 for u in users])
            for nb in (4, 20):
                seqs, scores, g_ = search(model, fn, inputs["input_ids"], inputs["attention_mask"], prefix, nb, 4, 4)
                gap = min(gap, g_)
                fx[f"s/beams/{b}/{nb}"], fx[f"s/scores/{b}/{nb}"] = seqs.numpy().astype(np.int32), scores.numpy()
            # the reference's scoring of the 20-beam call (test_SMB_decoder.py:196-285)
            out_str = tok.batch_decode(seqs, skip_special_tokens=True)
            out_items = [s.replace(" ", "") for s in tok.batch_decode(seqs[:, 2:], skip_special_tokens=True)]
            out_items = [out_items[i * 20:(i + 1) * 20] for i in range(3)]
            dup = []
            for i in range(3):
                o, h = set(out_items[i]), set(inputs["inters_item_list"][i])
                dup.append(len(o & h) / len(o) if len(o) > 0 else 0)
            topk = get_topk_results(out_str, scores, targets, 20)
            row = {m: v / 3 for m, v in get_metrics_results(topk, METRICS, targets).items()}
            row["Avg. Duplicate Ratio"] = float(np.mean(dup))
            beams[b].update(row=row, targets=[[ids_of(tok, t)[1:] for t in tg] for tg in targets],
                            history_items=[[ids_of(tok, t) for t in h] for h in inputs["inters_item_list"]])
            rows.append(row), counts.append(3)
        if gap > base.GAP:
            break
        print(f"weight seed {wseed}: smallest gap {gap:.2e} <= {base.GAP}, redrawing")
        wseed += 100
    merged = {m: sum(r[m] * n for r, n in zip(rows, counts)) / sum(counts) for m in METRICS}
    meta["s"] = dict(weight_seed=wseed, keys=list(shapes), shapes=[list(s) for s in shapes.values()], no_grad=[],
                     param_keys=[k for k, _ in model.named_parameters()], smallest_gap=gap, beams=beams, merged=merged)
    fx["s/weight_checksums"] = tw.checksums(sd)
    for tag, b in batches.items():
        record_batch(fx, f"s/{tag}", model, "s", b, V)
        print("smb", tag, tuple(b["input_ids"].shape), float(fx[f"s/{tag}/loss"]))
    # ---- MB
    train, _ = lmb.load_MB_datasets(dataset=GPU_MB["name"], tasks="mb_explicit", **common)
    tok = tokenizer(train.datasets[0].get_new_tokens())
    V = len(tok)
    mb_index = pick(train, tok, (1, 9, 20, 26), 5)
    meta["mb_index"] = mb_index
    mb_batch = EncoderDecoderCollator(tok)([train[i] for i in mb_index])
    test = lmb.load_MB_test_dataset(dataset=GPU_MB["name"], test_task="mb_explicit", **common)
    test.get_all_items()
    sub = test.filter_by_behavior(test.target_behavior)
    lens = [len(ids_of(tok, sub[i]["input_ids"])) for i in range(len(sub))]
    users = [int(np.argmin(lens)), int(np.argsort(lens)[len(lens) // 2]), int(np.argmax(lens))]
    inputs, targets = EncoderDecoderTestCollator(tok)([sub[u] for u in users])
    cand = [[0] + s for s in tok(sorted(test.get_all_items(test.target_behavior)))["input_ids"]]
    assert len(cand) >= 20
    cfg = dict(long_.CONFIGS["c"], vocab_size=V)
    meta["configs"]["m"] = cfg
    wseed = 32
    while True:
        torch.manual_seed(0)
        model = TIGER(T5Config(**cfg))
        if not hasattr(model, "model_parallel"):
            model.model_parallel = False
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in model.state_dict().items())
        sd = tw.init_state_dict(shapes, wseed)
        model.load_state_dict(sd)
        model.set_hyper(base.TEMPERATURE)
        model.eval()
        prefix = torch.tensor([[0] + ids_of(tok, f"<behavior_{test.target_behavior}>")] * 3)
        seqs, scores, gap = search(model, fn_of(Trie(cand)), inputs["input_ids"], inputs["attention_mask"], prefix, 4, 10, 5)
        if gap > base.GAP:
            break
        print(f"weight seed {wseed}: smallest gap {gap:.2e} <= {base.GAP}, redrawing")
        wseed += 100
    fx["m/beams/4"], fx["m/scores/4"] = seqs.numpy().astype(np.int32), scores.numpy()
    meta["m"] = dict(weight_seed=wseed, keys=list(shapes), shapes=[list(s) for s in shapes.values()], no_grad=[],
                     param_keys=[k for k, _ in model.named_parameters()], smallest_gap=gap, users=users,
                     enc_lens=[lens[u] + 1 for u in users], target_behavior=test.target_behavior)
    fx["m/weight_checksums"] = tw.checksums(sd)
    record_batch(fx, "m/mb", model, "m", mb_batch, V)
    print("mb", tuple(mb_batch["input_ids"].shape), float(fx["m/mb/loss"]))
    fx["meta_json"] = np.asarray(json.dumps(meta))
    return fx


def save(name, fx):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def main():
    TIGER, T5Config, _, Trie, fn_of = base.reference_tiger()
    _ref_loader.load_reference_classes()                                # (the shims the dataset modules need)
    only = sys.argv[1:] or ["data", "model"]
    with tempfile.TemporaryDirectory() as tmp:
        model_fx = model_fixture(tmp, TIGER, T5Config, Trie, fn_of) if "model" in only else None
        if model_fx is not None:
            save("tiger_smb.npz", model_fx)
        if "data" in only:
            defaults = dict(train_SMB_decoder=task_defaults("train_SMB_decoder", "TrainSMBDecoder", "train_SMB_decoder"),
                            train_MB_decoder=task_defaults("train_MB_decoder", "TrainMBDecoder", "train_MB_decoder"),
                            test_SMB_decoder=task_defaults("test_SMB_decoder", "TestSMBDecoder", "test_SMB_decoder"),
                            test_MB_decoder=task_defaults("test_MB_decoder", "TestMBDecoder", "test_MB_decoder"))
            for kind in ("smb", "mb"):
                res, meta = data_fixture(kind, tmp, Trie, fn_of)
                meta["defaults"] = defaults
                if kind == "smb":
                    z = np.load(os.path.join(GOLDEN, "tiger_smb.npz"))
                    m = json.loads(str(z["meta_json"]))
                    meta["recorded"] = dict(beams=m["s"]["beams"], merged=m["s"]["merged"], metrics=m["metrics"])
                    for b in m["beam_behaviors"]:
                        res[f"recorded::{b}::beams"], res[f"recorded::{b}::scores"] = z[f"s/beams/{b}/20"], z[f"s/scores/{b}/20"]
                res["meta_json"] = np.array(json.dumps(meta))
                save(f"tiger_{kind}_data.npz", res)


if __name__ == "__main__":
    main()
