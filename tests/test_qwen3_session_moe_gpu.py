"""The Qwen3SessionMoe backbone (``Engine(variant="qwen3_session_moe")``, ``Qwen3SessionMoeWithTemperature``) on the GPU
against the fixtures the real reference class wrote (tools/make_golden_session_moe.py).

Bars, copied and not derived anew:
  fp32 forms (split3 / split6 / f32): logits 2e-5 of the largest logit, losses 1e-5, global gradient norm 1e-4, per-tensor
    gradient norms and sampled gradients 1e-3 - tests/test_qwen3moe_gpu.py::test_qwen3moe_against_reference_fixture and
    tests/test_qwen3_session_gpu.py::test_logits_loss_and_gradients_match_reference_fixture (the same numbers in both);
  bf16: logits 1e-2 of the largest logit, loss 1e-3 absolute, gradient norms rtol 3e-2, sampled gradients 8e-2 of the
    tensor's largest - ::test_qwen3moe_bf16_against_reference_autocast_fixture and ::test_bf16_against_reference_autocast_fixture;
  decode: the same beams, scores within 1e-4 - tests/test_qwen3moe_gpu.py::test_decode_beams_match_reference_generate;
  module against engine: loss 1e-6 relative, gradients rtol 1e-5 / atol 1e-8, bf16 autocast loss 1e-2 absolute -
    tests/test_qwen3_session_gpu.py::test_module_autograd_and_autocast."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qwen3moe_weights as mw  # noqa: E402
from gamer_amd import decode, ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3SessionMoeConfig  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3moe import Qwen3SessionMoeEngine  # noqa: E402
from gamer_amd.modeling import Qwen3SessionMoeWithTemperature  # noqa: E402

VARIANT = "qwen3_session_moe"
KEYS = ("input_ids", "attention_mask", "labels", "session_ids", "extended_session_ids")


def _setup(golden, name, matmul=None, dtype="f32", **cfg_over):
    z, meta = golden(name)
    cfg = Qwen3SessionMoeConfig(**{**meta["config"], **cfg_over})
    cfg.dropout_rate = 0.1                  # (the kernels get p = 0 through dropout=False)
    sd = mw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
    eng = Engine(cfg, temperature=meta["temperature"], variant=VARIANT, dtype=dtype, matmul=matmul)
    assert isinstance(eng, Qwen3SessionMoeEngine)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in KEYS}
    return z, meta, eng, batch, sd


def _skw(batch):
    return dict(session_ids=batch["session_ids"], extended_session_ids=batch["extended_session_ids"])


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _sample(g, key):
    return g if key.startswith("grad::") else g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)]


def _allowed(eng):
    """[B,S,S] bool from the kernel-side form: key spans (hi, hole_lo, hole_hi) and key levels against query level 1."""
    span, kl = eng.ws.session["span_self"].cpu().long(), eng.ws.router["kl_self"].cpu().long()
    S = kl.shape[1]
    j = torch.arange(S).view(1, 1, S)
    hi, lo, hh = span[..., 0:1], span[..., 1:2], span[..., 2:3]
    return (j <= hi) & ~((j >= lo) & (j < hh)) & (kl[:, None, :] < 1)


@pytest.mark.parametrize("matmul", ["split3", "split6", "f32"])
@pytest.mark.parametrize("name", ["session_moe_small", "session_moe_pba_small"])
def test_logits_loss_and_gradients_match_reference_fixture(golden, name, matmul):
    z, meta, eng, batch, _ = _setup(golden, name, matmul)
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    _, logits = eng.forward(ids, am, train=False, **_skw(batch))
    e_raw = _relmax(logits.cpu().numpy(), z["logits_raw"])
    # the mask the one prep launch built is the reference's own dense mask, the positions its extended ids
    assert torch.equal(_allowed(eng), torch.from_numpy(z["reference_self_mask"]))
    assert torch.equal(eng.ws.session["pos_ids"].cpu().long(), batch["extended_session_ids"])
    loss, logits_s = eng.forward(ids, am, labels=lab, train=False, **_skw(batch))
    e_scaled = _relmax(logits_s.cpu().numpy(), z["logits_scaled"])
    eng.check_inputs()
    print(f"{name} {matmul}: logits {e_raw:.2e} / {e_scaled:.2e}, loss {float(loss):.7f} (reference {float(z['loss_mean']):.7f})")
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert abs(float(loss) - float(z["loss_mean"])) < 1e-5 * float(z["loss_mean"])
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False, **_skw(batch))
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    eng.check_inputs()
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    gn = float(np.sqrt((norms ** 2).sum()))
    worst = max(_relmax(_sample(eng.grads[k.split("::")[1]], k).cpu().numpy(), z[k])
                for k in z.files if k.startswith("grad::") or k.startswith("gradsample::"))
    print(f"{name} {matmul}: gradient norm {gn:.6f} (reference {float(z['global_grad_norm']):.6f}), worst tensor norm "
          f"{float(rel.max()):.2e}, worst sample {worst:.2e}")
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            assert _relmax(_sample(eng.grads[k.split("::")[1]], k).cpu().numpy(), z[k]) < 1e-3, k
    assert all(bool(torch.isfinite(g).all()) for g in eng.grads.values())


def test_bf16_against_reference_autocast_fixture(golden):
    z, meta, eng, batch, _ = _setup(golden, "session_moe_small_bf16", dtype="bf16")
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    _, logits = eng.forward(ids, am, train=False, **_skw(batch))
    assert logits.dtype == torch.bfloat16
    ref = z["logits_raw"]
    assert float(np.abs(logits.float().cpu().numpy() - ref).max()) < 1e-2 * float(np.abs(ref).max())
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False, **_skw(batch))
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys = [str(k) for k in z["grad_keys"]]
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            got = _sample(eng.grads[k.split("::")[1]].cpu(), k).numpy()
            assert np.abs(got - z[k]).max() <= 8e-2 * max(np.abs(z[k]).max(), 1e-12), k


def test_two_identical_steps_give_the_same_gradient_bits(golden):
    z, meta, eng, batch, _ = _setup(golden, "session_moe_small")
    flats = []
    for _ in range(2):
        eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False, **_skw(batch))
        eng.zero_grad()
        eng.backward(1.0)
        flats.append(eng.flat_g.clone())
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1])


def test_step_makes_one_prep_launch(golden, monkeypatch):
    """One gamer_session_moe_prep per forward and none of the launches it replaces; the backward reuses its spans."""
    def forbidden(*a, **k):
        raise AssertionError("a prep kernel the Qwen3SessionMoe step must not launch was launched")
    for name in ("router_fwd", "moe_router_prep", "session_prep", "session_spans", "causal_prep", "router_position_table",
                 "attn_row_order"):
        monkeypatch.setattr(ops, name, forbidden)
    calls = []
    orig = ops.session_moe_prep
    monkeypatch.setattr(ops, "session_moe_prep", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    z, meta, eng, batch, _ = _setup(golden, "session_moe_small", "split3")
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False,
                          **_skw(batch))
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert len(calls) == 1
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])


def test_module_matches_engine_runs_bf16_under_autocast_and_round_trips(golden, tmp_path):
    z, meta, eng, batch, sd = _setup(golden, "session_moe_small")
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    m = Qwen3SessionMoeWithTemperature(Qwen3SessionMoeConfig(**meta["config"]))
    m.set_hyper(meta["temperature"])
    m.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]})
    m.eval()
    assert sorted(k for k in m.state_dict() if k != "lm_head.weight") == [str(k) for k in z["state_dict_keys"]]
    with pytest.raises(ValueError, match="Session IDs must be provided to generate session-wise causal mask."):
        m(input_ids=ids, attention_mask=am, labels=lab)
    out = m(input_ids=ids, attention_mask=am, labels=lab, actions=torch.zeros_like(ids), **_skw(batch))
    assert "aux_loss" not in out                      # the reference's forward is Qwen3ForCausalLM's
    out.loss.backward()
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False, **_skw(batch))
    eng.zero_grad()
    eng.backward(1.0)
    assert abs(float(out.loss.detach()) - float(loss)) <= 1e-6 * float(loss)
    assert abs(float(out.loss.detach()) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    for k, p in m.named_parameters():
        torch.testing.assert_close(p.grad, eng.grads[k], rtol=1e-5, atol=1e-8, msg=k)
    with torch.no_grad():
        lg = m(input_ids=ids, attention_mask=am, **_skw(batch)).logits
    assert _relmax(lg.cpu().numpy(), z["logits_raw"]) < 2e-5
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(input_ids=ids, attention_mask=am, labels=lab, **_skw(batch))
    assert isinstance(m._amp_engine, Qwen3SessionMoeEngine) and m._amp_engine.dtype == "bf16"
    assert m._amp_engine.flat_p is m.engine.flat_p
    assert abs(float(out16.loss.detach()) - float(z["loss_train_mode"])) < 1e-2
    out16.loss.backward()
    bad = batch["session_ids"].clone()
    bad[0] = bad[0].flip(0)
    with pytest.raises(ValueError, match="session ids that decrease"):
        m(input_ids=ids, attention_mask=am, session_ids=bad)
    m.save_pretrained(str(tmp_path))
    again = Qwen3SessionMoeWithTemperature.from_pretrained(str(tmp_path))
    assert isinstance(again._cfg, Qwen3SessionMoeConfig) and again._cfg.model_max_length == meta["config"]["model_max_length"]
    for k, v in m.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k


def test_required_inputs_and_the_three_length_limits(golden):
    z, meta, eng, batch, sd = _setup(golden, "session_moe_small", "f32")
    ids, am = batch["input_ids"], batch["attention_mask"]
    with pytest.raises(ValueError, match="Session IDs must be provided to generate session-wise causal mask."):
        eng.forward(ids, am, train=False)
    bad = batch["session_ids"].clone()
    bad[0] = bad[0].flip(0)                                     # session ids that decrease along a kept row
    eng.forward(ids, am, train=False, session_ids=bad, extended_session_ids=batch["extended_session_ids"])
    with pytest.raises(ValueError, match="session ids that decrease.*gamer_session_moe_prep"):
        eng.check_inputs()
    eng.forward(ids, am, train=False, **_skw(batch))
    eng.check_inputs()
    # S = 46 past the reference's in-item mask of 45 rows
    short = Engine(Qwen3SessionMoeConfig(**{**meta["config"], "model_max_length": 45}), variant=VARIANT, matmul="f32")
    with pytest.raises(ValueError, match="in-item mask.*= 45"):
        short.forward(ids, am, train=False, **_skw(batch))
    # S = 46 past the router's table of 9 * 5 + 1 = 46 - 0: one column fewer
    narrow = Engine(Qwen3SessionMoeConfig(**{**meta["config"], "n_positions": 8}), variant=VARIANT, matmul="f32")
    with pytest.raises(ValueError, match="router's table.*= 41"):
        narrow.forward(ids, am, train=False, **_skw(batch))
    long_ = Engine(Qwen3SessionMoeConfig(**{**meta["config"], "model_max_length": 4096, "n_positions": 500}), variant=VARIANT,
                   matmul="f32")
    far = torch.full((1, 2050), synthetic.PAD_ID, dtype=torch.int64)
    with pytest.raises(ValueError, match="2048"):
        long_.forward(far, torch.ones_like(far), train=False, session_ids=torch.zeros_like(far))


def _decode_engine(golden, **kw):
    fx, meta = golden("decode_session_moe_small")
    sd = mw.init_state_dict(meta["config"], meta["weight_seed"], meta["weight_scale"])
    return fx, meta, sd


@pytest.mark.parametrize("tb", [0, 1, 2])
def test_beam_search_matches_reference_generate(golden, tb):
    fx, meta, sd = _decode_engine(golden)
    eng = Engine(Qwen3SessionMoeConfig(**meta["config"]), temperature=0.7, variant=VARIANT)
    eng.load_state_dict(sd)
    ids, am, sid, ext = (torch.from_numpy(fx[f"b{tb}_{k}"]) for k in ("input_ids", "attention_mask", "session_ids",
                                                                     "extended_session_ids"))
    assert len(set((am == 0).sum(1).tolist())) > 1                    # rows of different left padding
    trie = decode.ItemTrie(synthetic.item_tokens(torch.from_numpy(fx["catalogue"]), tb, meta["codebook"]).tolist())
    beams, new = meta["beams"], meta["new_tokens"]
    for use_cache in (True, False):
        seq, sc = decode.beam_search(eng, ids, am, None, trie, beams, new, use_cache=use_cache, session_ids=sid,
                                     extended_session_ids=ext)
        assert torch.equal(seq.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"])), use_cache
        assert float((sc.cpu().double() - torch.from_numpy(fx[f"b{tb}_scores"])).abs().max()) < 1e-4, use_cache
    with pytest.raises(ValueError, match="session_ids"):
        decode.beam_search(eng, ids, am, None, trie, beams, new)


def test_module_generate_and_the_bf16_refusal(golden):
    fx, meta, sd = _decode_engine(golden)
    m = Qwen3SessionMoeWithTemperature(Qwen3SessionMoeConfig(**meta["config"]))
    m.set_hyper(0.7)
    m.load_state_dict(sd)
    m.eval()
    tb, beams, new = 1, meta["beams"], meta["new_tokens"]
    trie = decode.ItemTrie(synthetic.item_tokens(torch.from_numpy(fx["catalogue"]), tb, meta["codebook"]).tolist())
    ids, am, sid, ext = (torch.from_numpy(fx[f"b{tb}_{k}"]) for k in ("input_ids", "attention_mask", "session_ids",
                                                                     "extended_session_ids"))
    out = m.generate(input_ids=ids, attention_mask=am, session_ids=sid, extended_session_ids=ext, max_new_tokens=new,
                     num_beams=beams, num_return_sequences=beams, prefix_allowed_tokens_fn=decode.prefix_allowed_tokens(trie),
                     early_stopping=True)
    assert torch.equal(out.sequences.cpu(), torch.from_numpy(fx[f"b{tb}_sequences"]))
    assert float((out.sequences_scores.cpu().double() - torch.from_numpy(fx[f"b{tb}_scores"])).abs().max()) < 1e-4
    e16 = Engine(Qwen3SessionMoeConfig(**meta["config"]), temperature=0.7, variant=VARIANT, dtype="bf16")
    with pytest.raises(NotImplementedError, match="not for variant 'qwen3_session_moe'"):
        decode.beam_search(e16, ids, am, None, trie, beams, new, session_ids=sid, extended_session_ids=ext)
    with pytest.raises(NotImplementedError, match="not for variant 'qwen3_session_moe'"):
        e16.forward(ids, am, train=False, last_row_logits=True, session_ids=sid, extended_session_ids=ext)


def test_train_harness_one_epoch_on_an_smb_directory(tmp_path):
    from gamer_amd import data as gdata, train
    from gamer_amd.evaluate import evaluate_dataset
    synthetic.write_smb_dataset(str(tmp_path / "data"), "Syn", n_users=60, n_items=40, codebook=8, max_sessions=6, seed=1)
    out = tmp_path / "ckpt"
    state = train.main(["--data_path", str(tmp_path / "data"), "--dataset", "Syn", "--tasks", "smb_explicit_decoder_2",
                        "--backbone", "Qwen3SessionMoe", "--max_his_len", "8", "--per_device_batch_size", "16",
                        "--gradient_accumulation_steps", "1", "--epochs", "1", "--logging_step", "1", "--output_dir", str(out)])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert len(losses) >= 2 and all(np.isfinite(losses)), losses
    evals = [r["eval_loss"] for r in state["log_history"] if "eval_loss" in r]
    assert len(evals) == 1 and np.isfinite(evals[0])
    m = Qwen3SessionMoeWithTemperature.from_pretrained(str(out))
    assert isinstance(m.engine, Qwen3SessionMoeEngine) and m.engine.layout.numel == len(m.engine.flat_p)
    assert (m._cfg.num_positions, m._cfg.model_max_length, m._cfg.n_positions) == (5, 1024, 9)
    # the evaluation path on top, unchanged: per-behaviour beam search over the dataset's test users
    res = evaluate_dataset(m.engine, gdata.SMBData(str(tmp_path / "data"), "Syn"), 8, num_beams=4, batch_size=16,
                           metric_list=("hit@1", "ndcg@5"))
    assert res and all(r["samples"] > 0 and 0.0 <= r["hit@1"] <= 1.0 for r in res.values())
