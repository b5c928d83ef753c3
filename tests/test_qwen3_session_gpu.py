"""The Qwen3Session baseline (``Engine(variant="qwen3_session")``, ``Qwen3SessionWithTemperature``) on the GPU against the
fixtures the real reference wrote (tools/make_golden_qwen3.py), at the bars tests/test_qwen3_baseline_gpu.py holds the
plain baseline to; and its mask kernel, gamer_session_prep, against the reference's own dense mask."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qwen3_weights  # noqa: E402
from gamer_amd import decode, ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3Config, Qwen3SessionConfig  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3 import Qwen3SessionEngine  # noqa: E402
from gamer_amd.modeling import Qwen3SessionWithTemperature  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
KEYS = ("input_ids", "attention_mask", "actions", "labels", "session_ids", "extended_session_ids")


def _setup(golden, name, matmul=None, dtype="f32"):
    z, meta = golden(name)
    cfg = Qwen3SessionConfig(**meta["config"])
    sd = qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"])
    eng = Engine(cfg, temperature=meta["temperature"], variant="qwen3_session", dtype=dtype, matmul=matmul)
    assert isinstance(eng, Qwen3SessionEngine)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in KEYS}
    return z, meta, eng, batch, sd


def _skw(batch):
    return dict(session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _prep(sid, ext, am, P=5):
    B, S = sid.shape
    i32 = dict(dtype=torch.int32, device=DEV)
    out = dict(kl_self=torch.empty(B, S, **i32), span_self=torch.empty(B, S, 4, **i32), pos_ids=torch.empty(B, S, **i32),
               empty_self=torch.empty(B, S, **i32), tile_empty_self=torch.empty(B, (S + 31) // 32, **i32),
               violations=torch.zeros(1, **i32))
    ops.session_prep(sid.to(DEV).contiguous(), None if ext is None else ext.to(DEV).contiguous(),
                     None if am is None else am.to(DEV).contiguous(), P, S, out)
    torch.cuda.synchronize()
    return out


def _allowed(out):
    """[B,S,S] bool from the kernel-side form: key spans (hi, hole_lo, hole_hi) and key levels against query level 1."""
    span, kl = out["span_self"].cpu().long(), out["kl_self"].cpu().long()
    S = kl.shape[1]
    j = torch.arange(S).view(1, 1, S)
    hi, lo, hh = span[..., 0:1], span[..., 1:2], span[..., 2:3]
    return (j <= hi) & ~((j >= lo) & (j < hh)) & (kl[:, None, :] < 1)


def _tiles(empty, S):
    B = empty.shape[0]
    n_t = (S + 31) // 32
    return torch.cat([empty, torch.zeros(B, n_t * 32 - S, dtype=torch.bool)], 1).view(B, n_t, 32).any(-1)


def test_session_prep_equals_reference_dense_mask(golden):
    """Integer work, bit-exact: the spans describe exactly the mask the reference's _update_session_wise_causal_mask built
    for the fixture's left-padded, session-grouped rows; positions are the extended ids."""
    z, _ = golden("qwen3_session_small")
    am, sid, ext = (torch.from_numpy(z[k]) for k in ("attention_mask", "session_ids", "extended_session_ids"))
    S = am.shape[1]
    ref = torch.from_numpy(z["reference_self_mask"])
    out = _prep(sid, ext, am)
    assert int(out["violations"].item()) == 0
    assert torch.equal(_allowed(out), ref)
    assert torch.equal(out["kl_self"].cpu(), torch.where(am.bool(), 0, 0x7FFFFFFF).to(torch.int32))
    assert torch.equal(out["empty_self"].cpu().bool(), ~ref.any(-1))
    assert torch.equal(out["tile_empty_self"].cpu().bool(), _tiles(~ref.any(-1), S))
    assert torch.equal(out["pos_ids"].cpu().long(), ext)
    assert bool((out["span_self"][..., 0].cpu() <= torch.arange(S)).all())
    # without extended ids the positions are 0..S-1
    assert torch.equal(_prep(sid, None, am)["pos_ids"].cpu().long(), torch.arange(S).expand_as(am))


def test_session_prep_equals_causal_prep_when_every_token_is_a_session():
    """One session per token, positions 0..S-1: the session mask is HF's causal + key-padding mask."""
    B, S = 5, 83
    am = torch.ones(B, S, dtype=torch.int64)
    for b, pad in enumerate((0, 7, 30, 64, 82)):
        am[b, :pad] = 0
    sid = torch.arange(S).expand(B, S).contiguous() * am
    out = _prep(sid, None, am)
    i32 = dict(dtype=torch.int32, device=DEV)
    kl, es, te = torch.empty(B, S, **i32), torch.empty(B, S, **i32), torch.empty(B, (S + 31) // 32, **i32)
    ops.causal_prep(am.to(DEV), B, S, kl, es, te)
    torch.cuda.synchronize()
    assert int(out["violations"].item()) == 0
    causal = (torch.arange(S)[None, :, None] >= torch.arange(S)[None, None, :]) & am.bool()[:, None, :]
    assert torch.equal(_allowed(out), causal)
    assert torch.equal(out["kl_self"], kl) and torch.equal(out["empty_self"], es) and torch.equal(out["tile_empty_self"], te)
    assert torch.equal(out["pos_ids"].cpu().long(), torch.arange(S).expand(B, S))


def test_violations_are_flagged(golden):
    z, meta, eng, batch, _ = _setup(golden, "qwen3_session_small", "f32")
    am, sid, ext = batch["attention_mask"], batch["session_ids"], batch["extended_session_ids"]
    assert int(_prep(sid, ext, am)["violations"].item()) == 0
    bad = sid.clone()
    bad[0] = bad[0].flip(0)                                     # session ids that decrease along a kept row
    assert int(_prep(bad, ext, am)["violations"].item()) > 0
    far = ext.clone()
    far[1, -1] = am.shape[1]                                    # a RoPE position outside [0, S)
    assert int(_prep(sid, far, am)["violations"].item()) == 1
    eng.forward(batch["input_ids"], am, train=False, session_ids=bad, extended_session_ids=ext)
    with pytest.raises(ValueError, match="session ids that decrease"):
        eng.check_inputs()
    eng.forward(batch["input_ids"], am, train=False, **_skw(batch))
    eng.check_inputs()


def test_forward_requires_session_ids_and_refuses_lengths_the_reference_cannot_mask(golden):
    z, meta, eng, batch, sd = _setup(golden, "qwen3_session_small", "f32")
    with pytest.raises(ValueError, match="Session IDs must be provided"):
        eng.forward(batch["input_ids"], batch["attention_mask"], train=False)
    cfg = Qwen3SessionConfig(**{**meta["config"], "model_max_length": 40})      # in-item mask of 40 rows < S = 45
    short = Engine(cfg, variant="qwen3_session", matmul="f32")
    with pytest.raises(ValueError, match="in-item mask"):
        short.forward(batch["input_ids"], batch["attention_mask"], train=False, **_skw(batch))
    long_ = Engine(Qwen3SessionConfig(**{**meta["config"], "model_max_length": 4096}), variant="qwen3_session", matmul="f32")
    ids = torch.full((1, 2050), synthetic.PAD_ID, dtype=torch.int64)
    with pytest.raises(ValueError, match="2048"):
        long_.forward(ids, torch.ones_like(ids), train=False, session_ids=torch.zeros_like(ids))


@pytest.mark.parametrize("matmul", ["split3", "split6", "f32"])
@pytest.mark.parametrize("name", ["qwen3_session_small", "qwen3_session_full"])
def test_logits_loss_and_gradients_match_reference_fixture(golden, name, matmul):
    z, meta, eng, batch, _ = _setup(golden, name, matmul)
    small = name.endswith("small")
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], batch["actions"], train=False, **_skw(batch))
    lg = logits.cpu().numpy()
    e_raw = _relmax(lg if small else lg[:, ::37, ::53], z["logits_raw" if small else "logits_raw_sample"])
    loss, logits_s = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=False, **_skw(batch))
    ls = logits_s.cpu().numpy()
    e_scaled = _relmax(ls if small else ls[:, ::37, ::53], z["logits_scaled" if small else "logits_scaled_sample"])
    e_loss = abs(float(loss) - float(z["loss_mean"])) / float(z["loss_mean"])
    loss_n, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"],
                            num_items_in_batch=float(z["num_items"]), train=False, **_skw(batch))
    e_loss_n = abs(float(loss_n) - float(z["loss_sum"])) / float(z["loss_sum"])
    hidden = []
    eng.forward(batch["input_ids"], batch["attention_mask"], train=False, hidden_sink=hidden, **_skw(batch))
    keep = batch["attention_mask"].bool()[:, :, None].to(hidden[0].device)
    hs = np.array([float((h.double() * keep).sum()) for h in hidden])
    assert np.all(np.abs(hs - z["hidden_sum_kept"]) <= 1e-5 * z["hidden_abssum"] + 1e-6), (hs, z["hidden_sum_kept"])
    eng.check_inputs()
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert e_loss < 1e-5 and e_loss_n < 1e-5, (e_loss, e_loss_n)
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False,
                          **_skw(batch))
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    gn = float(np.sqrt((norms ** 2).sum()))
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            g = eng.grads[k.split("::")[1]]
            got = g if k.startswith("grad::") else g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)]
            assert _relmax(got.cpu().numpy(), z[k]) < 1e-3, k


def test_bf16_against_reference_autocast_fixture(golden):
    z, meta, eng, batch, _ = _setup(golden, "qwen3_session_small_bf16", dtype="bf16")
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], train=False, **_skw(batch))
    assert logits.dtype == BF
    ref = torch.from_numpy(z["logits_raw"])
    assert float((logits.float().cpu() - ref).abs().max()) < 1e-2 * float(ref.abs().max())
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False,
                          **_skw(batch))
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys = [str(k) for k in z["grad_keys"]]
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    assert abs(float(np.sqrt((norms ** 2).sum())) - float(z["global_grad_norm"])) < 5e-3 * float(z["global_grad_norm"])
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            gt = eng.grads[k.split("::")[1]].cpu()
            got = gt.numpy() if k.startswith("grad::") else gt[::max(1, gt.shape[0] // 8), ::max(1, gt.shape[1] // 8)].numpy()
            assert np.abs(got - z[k]).max() <= 8e-2 * max(np.abs(z[k]).max(), 1e-12), k


def test_step_launches_only_session_prep_for_its_mask(golden, monkeypatch):
    """No router, expert-list, row-order, injection, cross-attention or causal-mask launch; one gamer_session_prep per
    forward, and the backward reuses its spans."""
    def forbidden(*a, **k):
        raise AssertionError("a kernel the Qwen3Session step must not launch was launched")
    for name in ("router_fwd", "expert_lists", "attn_row_order", "inject_table_fwd", "inject_table_bwd", "rowtable_fwd",
                 "rowtable_bwd", "session_spans", "causal_prep", "silu_gate_fwd", "silu_gate_bwd", "swiglu_fwd_ld_tbl",
                 "swiglu_bwd_ld_tbl", "attn_decode_cross"):
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, forbidden)
    calls = []
    orig = ops.session_prep
    monkeypatch.setattr(ops, "session_prep", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    z, meta, eng, batch, _ = _setup(golden, "qwen3_session_full", "split3")
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False,
                          **_skw(batch))
    assert len(calls) == 1
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert len(calls) == 1
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])


@pytest.mark.parametrize("matmul, spill", [("split3", False), ("split6", True), ("f32", True)])
def test_workspace_spill_scratch_follows_the_key_spans(golden, matmul, spill):
    """split6 / f32 send span calls to the fp32-MFMA backward, which needs the dS-spill scratch; the plain baseline in
    split6 keeps the split form and needs none."""
    z, meta, eng, batch, _ = _setup(golden, "qwen3_session_small", matmul)
    assert (eng.workspace(3, 45, True).ds_work is not None) == spill
    plain = Engine(Qwen3Config(**{k: v for k, v in meta["config"].items() if k not in ("num_positions", "model_max_length")}),
                   variant="qwen3", matmul=matmul)
    assert (plain.workspace(3, 45, True).ds_work is not None) == (matmul == "f32")


def _decode_model(meta):
    m = Qwen3SessionWithTemperature(Qwen3SessionConfig(**meta["config"]))
    m.load_state_dict(qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"], scale=meta["weight_scale"]))
    m.set_hyper(0.7)
    m.eval()
    return m


def test_generate_matches_reference_beams(golden, monkeypatch):
    """generate() as test_SMB_decoder.py:139-156 calls it: the reference's beams and scores; the cache-free re-run agrees;
    and generated tokens at the padding-offset positions of the plain baseline (kept prompt tokens + t - 1) instead of
    max(extended_session_ids) + t change the beams."""
    fx, meta = golden("decode_qwen3_session_small")
    m = _decode_model(meta)
    cb, beams = meta["codebook"], meta["beams"]
    cat = torch.from_numpy(fx["catalogue"])
    runs = {}
    for tb in range(meta["num_behavior"]):
        trie = decode.ItemTrie(synthetic.item_tokens(cat, tb, cb).tolist(), pad_token_id=m._cfg.pad_token_id)
        ids, am = torch.from_numpy(fx[f"b{tb}_input_ids"]), torch.from_numpy(fx[f"b{tb}_attention_mask"])
        sid, ext = torch.from_numpy(fx[f"b{tb}_session_ids"]), torch.from_numpy(fx[f"b{tb}_extended_session_ids"])
        out = m.generate(input_ids=ids, attention_mask=am, session_ids=sid, extended_session_ids=ext, max_new_tokens=4,
                         num_beams=beams, num_return_sequences=beams, prefix_allowed_tokens_fn=decode.prefix_allowed_tokens(trie),
                         early_stopping=True)
        assert torch.equal(out.sequences.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"])), tb
        assert float((out.sequences_scores.cpu().double() - torch.from_numpy(fx[f"b{tb}_scores"])).abs().max()) < 1e-4
        seq_r, sc_r = decode.beam_search(m.engine, ids, am, None, trie, beams, 4, use_cache=False, session_ids=sid,
                                         extended_session_ids=ext)
        assert torch.equal(seq_r.cpu(), out.sequences.cpu()) and float((sc_r - out.sequences_scores).abs().max()) < 1e-4
        runs[tb] = (ids, am, sid, ext, trie)
    with pytest.raises(ValueError, match="session_ids"):
        m.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, num_beams=beams, trie=trie)
    orig = decode.Qwen3DecodeSession.__init__

    def padding_offsets(self, engine, input_ids, attention_mask, *a, **k):
        orig(self, engine, input_ids, attention_mask, *a, **k)
        self.pos_last.copy_((attention_mask.to(self.pos_last.device).sum(1) - 1).to(torch.int32).repeat_interleave(self.nb))
    monkeypatch.setattr(decode.Qwen3DecodeSession, "__init__", padding_offsets)
    differs = 0
    for tb, (ids, am, sid, ext, trie) in runs.items():
        seq, _ = decode.beam_search(m.engine, ids, am, None, trie, beams, 4, session_ids=sid, extended_session_ids=ext)
        differs += int(not torch.equal(seq.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"])))
    assert differs >= 1


def test_evaluate_behavior_metrics_match_fixture(golden):
    from gamer_amd.evaluate import evaluate_behavior
    fx, meta = golden("decode_qwen3_session_small")
    m = _decode_model(meta)
    cb, beams = meta["codebook"], meta["beams"]
    cat = torch.from_numpy(fx["catalogue"])
    for tb in range(meta["num_behavior"]):
        trie = decode.ItemTrie(synthetic.item_tokens(cat, tb, cb).tolist(), pad_token_id=m._cfg.pad_token_id)
        tgt = synthetic.item_tokens(torch.from_numpy(fx[f"b{tb}_targets"]), tb, cb)[:, 1:]
        batch = {k: torch.from_numpy(fx[f"b{tb}_{k}"]) for k in ("input_ids", "attention_mask", "actions", "session_ids",
                                                                  "extended_session_ids")}
        batch["targets"] = [[row.tolist()] for row in tgt]
        res = evaluate_behavior(m.engine, [batch], trie, beams, meta["metrics"])
        n = batch["input_ids"].shape[0]
        np.testing.assert_allclose([res[k] for k in meta["metrics"]], fx[f"b{tb}_metrics"] / n, atol=1e-12)


def test_module_autograd_and_autocast(golden):
    z, meta, eng, batch, sd = _setup(golden, "qwen3_session_small")
    m = Qwen3SessionWithTemperature(Qwen3SessionConfig(**meta["config"]))
    m.set_hyper(meta["temperature"])
    m.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]})
    m.eval()
    assert list(m.state_dict()) == [k for k in eng.layout.entries] + ["lm_head.weight"]
    with pytest.raises(ValueError, match="Session IDs must be provided"):
        m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    out = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"],
            actions=batch["actions"], **_skw(batch))
    out.loss.backward()
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False,
                          **_skw(batch))
    eng.zero_grad()
    eng.backward(1.0)
    assert abs(float(out.loss) - float(loss)) <= 1e-6 * float(loss)
    assert abs(float(out.loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    for k, p in m.named_parameters():
        torch.testing.assert_close(p.grad, eng.grads[k], rtol=1e-5, atol=1e-8, msg=k)
    with torch.no_grad():
        lg = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], **_skw(batch)).logits
    assert _relmax(lg.cpu().numpy(), z["logits_raw"]) < 2e-5
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"], **_skw(batch))
    assert isinstance(m._amp_engine, Qwen3SessionEngine) and m._amp_engine.dtype == "bf16"
    assert m._amp_engine.flat_p is m.engine.flat_p
    assert abs(float(out16.loss) - float(z["loss_train_mode"])) < 1e-2
    bad = batch["session_ids"].clone()
    bad[0] = bad[0].flip(0)
    with pytest.raises(ValueError, match="session ids that decrease"):
        m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], session_ids=bad)


def test_train_harness_qwen3_session_backbone(tmp_path):
    from safetensors.torch import load_file

    from gamer_amd import train
    out = str(tmp_path / "run")
    state = train.main(["--backbone", "Qwen3Session", "--max_his_len", "20", "--per_device_batch_size", "16",
                        "--gradient_accumulation_steps", "1", "--epochs", "1", "--steps_per_epoch", "24",
                        "--logging_step", "4", "--learning_rate", "5e-3", "--output_dir", out, "--prefetch", "1"])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert len(losses) == 6 and losses[-1] < losses[0] - 0.05, losses
    ck = os.path.join(out, "checkpoint-24")
    cfg = Qwen3SessionConfig.from_pretrained(ck)
    assert (cfg.num_positions, cfg.model_max_length) == (5, 1024)
    m = Qwen3SessionWithTemperature.from_pretrained(ck)
    eng = Engine(cfg, variant="qwen3_session")
    eng.load_state_dict(load_file(os.path.join(ck, "model.safetensors")))
    b = synthetic.make_batch(4, 21, 256, 3, seed=5, session_mean=4.0)
    _, ref = eng.forward(b["input_ids"], b["attention_mask"], train=False, **_skw(b))
    got = m(input_ids=b["input_ids"], attention_mask=b["attention_mask"], **_skw(b)).logits
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
    st16 = train.main(["--backbone", "Qwen3Session", "--bf16", "--max_his_len", "20", "--per_device_batch_size", "16",
                       "--gradient_accumulation_steps", "1", "--epochs", "1", "--steps_per_epoch", "4", "--logging_step", "2"])
    assert all(np.isfinite(r["loss"]) for r in st16["log_history"])
