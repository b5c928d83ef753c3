"""The plain Qwen3 baseline (``Engine(variant="qwen3")``, ``Qwen3WithTemperature``) on the GPU against the fixtures the
real reference wrote (tools/make_golden_qwen3.py), at the bars tests/test_model_gpu.py, test_bf16_gpu.py and
test_decode.py hold the Multi variants to."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qwen3_weights  # noqa: E402
from gamer_amd import _lib, decode, ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3Config  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3 import Qwen3Engine  # noqa: E402
from gamer_amd.modeling import Qwen3WithTemperature  # noqa: E402

BF = torch.bfloat16


def _setup(golden, name, matmul=None, dtype="f32"):
    z, meta = golden(name)
    cfg = Qwen3Config(**meta["config"])
    sd = qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"])
    eng = Engine(cfg, temperature=meta["temperature"], variant="qwen3", dtype=dtype, matmul=matmul)
    assert isinstance(eng, Qwen3Engine)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "actions", "labels", "session_ids",
                                                "extended_session_ids")}
    return z, meta, eng, batch, sd


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _sample(lg, name):
    return lg if name.endswith("small") else lg[:, ::37, ::53]


def _grad_errors(eng, z):
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    sample = {}
    for k in z.files:
        if k.startswith("grad::"):
            sample[k[6:]] = _relmax(eng.grads[k[6:]].cpu().numpy(), z[k])
        elif k.startswith("gradsample::"):
            g = eng.grads[k[12:]]
            sample[k[12:]] = _relmax(g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].cpu().numpy(), z[k])
    gn = float(np.sqrt((norms ** 2).sum()))
    return gkeys, norms, rel, sample, gn


@pytest.mark.parametrize("matmul", ["split3", "split6", "f32"])
@pytest.mark.parametrize("name", ["qwen3_small", "qwen3_full"])
def test_logits_loss_and_gradients_match_reference_fixture(golden, name, matmul):
    z, meta, eng, batch, _ = _setup(golden, name, matmul)
    # the SMB collator's actions / session ids are accepted and ignored
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], batch["actions"], train=False,
                            session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])
    e_raw = _relmax(_sample(logits.cpu().numpy(), name), z["logits_raw" if name.endswith("small") else "logits_raw_sample"])
    loss, logits_s = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=False)
    e_scaled = _relmax(_sample(logits_s.cpu().numpy(), name),
                       z["logits_scaled" if name.endswith("small") else "logits_scaled_sample"])
    e_loss = abs(float(loss) - float(z["loss_mean"])) / float(z["loss_mean"])
    loss_n, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"],
                            num_items_in_batch=float(z["num_items"]), train=False)
    e_loss_n = abs(float(loss_n) - float(z["loss_sum"])) / float(z["loss_sum"])
    hidden = []
    eng.forward(batch["input_ids"], batch["attention_mask"], train=False, hidden_sink=hidden)
    keep = batch["attention_mask"].bool()[:, :, None].to(hidden[0].device)
    hs = np.array([float((h.double() * keep).sum()) for h in hidden])
    assert len(hs) == meta["config"]["num_hidden_layers"] + 1
    assert np.all(np.abs(hs - z["hidden_sum_kept"]) <= 1e-5 * z["hidden_abssum"] + 1e-6), (hs, z["hidden_sum_kept"])
    eng.check_inputs()
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert e_loss < 1e-5 and e_loss_n < 1e-5, (e_loss, e_loss_n)
    # gradients: train mode, dropout off (the fixture's p = 0)
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    gkeys, _, rel, sample, gn = _grad_errors(eng, z)
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    wk = max(sample, key=sample.get)
    assert sample[wk] < 1e-3, (wk, sample[wk])


def test_bf16_against_reference_autocast_fixture(golden):
    """dtype="bf16" against the reference under torch.autocast("cpu", bfloat16), at test_bf16_gpu.py's bars."""
    z, meta, eng, batch, _ = _setup(golden, "qwen3_small_bf16", dtype="bf16")
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], train=False)
    assert logits.dtype == BF
    ref = torch.from_numpy(z["logits_raw"])
    assert float((logits.float().cpu() - ref).abs().max()) < 1e-2 * float(ref.abs().max())
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys, norms, _, _, gn = _grad_errors(eng, z)
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    assert abs(gn - float(z["global_grad_norm"])) < 5e-3 * float(z["global_grad_norm"])
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            gt = eng.grads[k.split("::")[1]].cpu()
            got = gt.numpy() if k.startswith("grad::") else gt[::max(1, gt.shape[0] // 8), ::max(1, gt.shape[1] // 8)].numpy()
            assert np.abs(got - z[k]).max() <= 8e-2 * max(np.abs(z[k]).max(), 1e-12), k


def _launch_counters():
    lib = _lib.load()
    out = []
    for name in ("gamer_debug_gemm_as_launches", "gamer_debug_gemm_os_launches"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_longlong, []
        out.append(int(fn()))
    return out


def test_step_launches_no_multi_only_kernel_and_runs_the_dense_epilogues(golden, monkeypatch):
    """The baseline step: no router, expert-list, row-order, injection-table or cross-attention launch; with the production
    kernels' row bars lowered, the dense gate|up + SwiGLU epilogue and the down projection's SwiGLU-backward input gradient run
    on the activation- / output-stationary kernels, and the result still matches the reference."""
    def forbidden(*a, **k):
        raise AssertionError("a Qwen3Multi-only kernel was launched by the baseline")
    for name in ("router_fwd", "expert_lists", "attn_row_order", "inject_table_fwd", "inject_table_bwd", "rowtable_fwd",
                 "rowtable_bwd", "session_spans", "silu_gate_fwd", "silu_gate_bwd", "swiglu_fwd_ld_tbl", "swiglu_bwd_ld_tbl",
                 "attn_decode_cross"):
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, forbidden)
    a0, o0 = _launch_counters()
    with ops.env_switches(GAMER_GEMM_AS=1, GAMER_GEMM_AS_MIN_M=1, GAMER_GEMM_OS=1, GAMER_GEMM_OS_MIN_M=1):
        z, meta, eng, batch, _ = _setup(golden, "qwen3_full", "split3")
        eng.forward(batch["input_ids"], batch["attention_mask"], train=False)      # packed weight pieces exist from pass 2 on
        loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
        eng.zero_grad()
        eng.backward(1.0)
        torch.cuda.synchronize()
    a1, o1 = _launch_counters()
    L = meta["config"]["num_hidden_layers"]
    assert a1 - a0 >= 2 * L, (a0, a1)          # q|k|v and the fused gate|up + SwiGLU of every layer (per pass)
    assert o1 - o0 >= L, (o0, o1)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    gkeys, _, rel, sample, gn = _grad_errors(eng, z)
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3 and max(sample.values()) < 1e-3


def test_no_hidden_dropout_and_seeded_attention_dropout(golden):
    z, meta, _, batch, sd = _setup(golden, "qwen3_small", "f32")
    cfg = Qwen3Config(**{**meta["config"], "attention_dropout": 0.0})
    eng = Engine(cfg, temperature=0.7, variant="qwen3", matmul="f32")
    eng.load_state_dict(sd)
    _, lg_eval = eng.forward(batch["input_ids"], batch["attention_mask"], train=False)
    lg_eval = lg_eval.clone()
    _, lg_train = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True)
    _, lg_eval_s = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=False)
    assert torch.equal(lg_train, lg_eval_s), "a train-mode step with attention_dropout = 0 must equal the eval forward"
    # p = 0.1 (the Qwen3-Light value): seeded per step
    cfg = Qwen3Config(**{**meta["config"], "attention_dropout": 0.1})
    outs = []
    for seed in (1, 2, 1):
        e = Engine(cfg, temperature=0.7, variant="qwen3", matmul="f32")
        e.load_state_dict(sd)
        e.base_seed = seed
        loss, lg = e.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True)
        outs.append(lg.clone())
    assert not torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0], lg_eval_s)


def test_module_autograd_autocast_and_fp16_refusal(golden):
    z, meta, eng, batch, sd = _setup(golden, "qwen3_small")
    m = Qwen3WithTemperature(Qwen3Config(**meta["config"]))
    m.set_hyper(meta["temperature"])
    m.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]})
    m.eval()                       # (attention dropout off: the engine below runs the same step with dropout=False)
    sdm = m.state_dict()
    assert list(sdm) == [k for k in eng.layout.entries] + ["lm_head.weight"]
    out = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"],
            actions=batch["actions"], session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])
    out.loss.backward()
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    eng.zero_grad()
    eng.backward(1.0)
    assert abs(float(out.loss) - float(loss)) <= 1e-6 * float(loss)
    for k, p in m.named_parameters():
        torch.testing.assert_close(p.grad, eng.grads[k], rtol=1e-5, atol=1e-8, msg=k)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    assert m._amp_engine is not None and m._amp_engine.dtype == "bf16" and isinstance(m._amp_engine, Qwen3Engine)
    assert m._amp_engine.flat_p is m.engine.flat_p
    assert abs(float(out16.loss) - float(z["loss_train_mode"])) < 1e-2
    with pytest.raises(NotImplementedError):
        with torch.autocast("cuda", dtype=torch.float16):
            m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    opt = m.fused_optimizer(lr=1e-3)
    opt.step()
    assert opt.state_dict()["state"]["layout_version"] == 1


def _decode_model(fx, meta):
    cfg = Qwen3Config(**meta["config"])
    m = Qwen3WithTemperature(cfg)
    sd = qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"], scale=meta["weight_scale"])
    m.load_state_dict(sd)
    m.set_hyper(0.7)
    m.eval()
    return m


def test_generate_matches_reference_beams(golden, monkeypatch):
    """generate() as test_SMB_decoder.py:122-137 calls it, rows of different left padding: the reference's beams and scores
    (test_decode.py's bar).  The fixture tells the per-row RoPE offset apart: without it the beams change."""
    fx, meta = golden("decode_qwen3_small")
    m = _decode_model(fx, meta)
    cb, nb_beh, beams = meta["codebook"], meta["num_behavior"], meta["beams"]
    cat = torch.from_numpy(fx["catalogue"])
    items = [synthetic.item_tokens(cat, b, cb).tolist() for b in range(nb_beh)]
    runs = {}
    for tb in range(nb_beh):
        trie = decode.ItemTrie(items[tb], pad_token_id=m._cfg.pad_token_id)
        ids, am = torch.from_numpy(fx[f"b{tb}_input_ids"]), torch.from_numpy(fx[f"b{tb}_attention_mask"])
        out = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, num_beams=beams, num_return_sequences=beams,
                         prefix_allowed_tokens_fn=decode.prefix_allowed_tokens(trie), early_stopping=True)
        assert torch.equal(out.sequences.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"])), tb
        assert float((out.sequences_scores.cpu().double() - torch.from_numpy(fx[f"b{tb}_scores"])).abs().max()) < 1e-4
        # the cache-free re-run gives the same beams
        seq_r, sc_r = decode.beam_search(m.engine, ids, am, None, trie, beams, 4, use_cache=False)
        assert torch.equal(seq_r.cpu(), out.sequences.cpu()) and float((sc_r - out.sequences_scores).abs().max()) < 1e-4
        runs[tb] = (ids, am, trie)
    # the per-row offset removed from the generated tokens (position L0 + t - 1 for every row): the fixture's beams differ
    orig = decode.Qwen3DecodeSession.__init__

    def no_offset(self, engine, input_ids, attention_mask, *a, **k):
        orig(self, engine, input_ids, attention_mask, *a, **k)
        self.pos_last.fill_(input_ids.shape[1] - 1)
    monkeypatch.setattr(decode.Qwen3DecodeSession, "__init__", no_offset)
    differs = 0
    for tb, (ids, am, trie) in runs.items():
        seq, sc = decode.beam_search(m.engine, ids, am, None, trie, beams, 4)
        differs += int(not torch.equal(seq.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"])))
    assert differs >= 1


def test_evaluate_behavior_metrics_match_fixture(golden):
    from gamer_amd.evaluate import evaluate_behavior
    fx, meta = golden("decode_qwen3_small")
    m = _decode_model(fx, meta)
    cb, beams = meta["codebook"], meta["beams"]
    cat = torch.from_numpy(fx["catalogue"])
    for tb in range(meta["num_behavior"]):
        trie = decode.ItemTrie(synthetic.item_tokens(cat, tb, cb).tolist(), pad_token_id=m._cfg.pad_token_id)
        tgt = synthetic.item_tokens(torch.from_numpy(fx[f"b{tb}_targets"]), tb, cb)[:, 1:]
        batch = dict(input_ids=torch.from_numpy(fx[f"b{tb}_input_ids"]),
                     attention_mask=torch.from_numpy(fx[f"b{tb}_attention_mask"]),
                     actions=torch.from_numpy(fx[f"b{tb}_actions"]), targets=[[row.tolist()] for row in tgt])
        res = evaluate_behavior(m.engine, [batch], trie, beams, meta["metrics"])
        n = batch["input_ids"].shape[0]
        np.testing.assert_allclose([res[k] for k in meta["metrics"]], fx[f"b{tb}_metrics"] / n, atol=1e-12)


def test_train_harness_qwen3_backbone(tmp_path):
    from safetensors.torch import load_file

    from gamer_amd import train
    out = str(tmp_path / "run")
    state = train.main(["--backbone", "Qwen3", "--max_his_len", "20", "--per_device_batch_size", "16",
                        "--gradient_accumulation_steps", "1", "--epochs", "1", "--steps_per_epoch", "24",
                        "--logging_step", "4", "--learning_rate", "5e-3", "--output_dir", out, "--prefetch", "1"])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert len(losses) == 6 and losses[-1] < losses[0] - 0.05, losses       # (no position-routed experts: slower than Qwen3Multi)
    ck = os.path.join(out, "checkpoint-24")
    m = Qwen3WithTemperature.from_pretrained(ck)
    eng = Engine(Qwen3Config.from_pretrained(ck), variant="qwen3")
    eng.load_state_dict(load_file(os.path.join(ck, "model.safetensors")))
    b = synthetic.make_batch(4, 21, 256, 3, seed=5)
    _, ref = eng.forward(b["input_ids"], b["attention_mask"], train=False)
    got = m(input_ids=b["input_ids"], attention_mask=b["attention_mask"]).logits
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
    # --bf16 trains the same backbone; --fp16 stays refused
    st16 = train.main(["--backbone", "Qwen3", "--bf16", "--max_his_len", "20", "--per_device_batch_size", "16",
                       "--gradient_accumulation_steps", "1", "--epochs", "1", "--steps_per_epoch", "4", "--logging_step", "2"])
    assert all(np.isfinite(r["loss"]) for r in st16["log_history"])
    with pytest.raises(SystemExit):
        train.main(["--backbone", "Qwen3", "--fp16"])
