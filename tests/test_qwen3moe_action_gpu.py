"""The Qwen3MoeAction backbone (``Engine(variant="qwen3moe_action")``, ``Qwen3ActionMoeWithTemperature``) on the GPU against
the fixtures the real reference class wrote (tools/make_golden_moe_action.py).

Bars, copied from tests/test_qwen3moe_gpu.py and not derived anew:
  fp32 forms (split3 / split6 / f32): logits 2e-5 of the largest logit, losses 1e-5, global gradient norm 1e-4, per-tensor
    gradient norms and sampled gradients 1e-3 - ::test_qwen3moe_against_reference_fixture;
  bf16: logits 1e-2 of the largest logit, loss 1e-3 absolute, gradient norms rtol 3e-2, sampled gradients 8e-2 of the
    tensor's largest - ::test_qwen3moe_bf16_against_reference_autocast_fixture;
  decode: the same beams, scores within 1e-4 - ::test_decode_beams_match_reference_generate;
  module against engine: loss 1e-6 relative, gradients rtol 1e-5 / atol 1e-8, bf16 autocast loss 1e-2 absolute -
    tests/test_qwen3_session_moe_gpu.py::test_module_matches_engine_runs_bf16_under_autocast_and_round_trips.
The fixtures keep the sampled gradients in one array (``grad_samples``, in ``grad_keys`` order): a vector whole, of a matrix
every (rows // 8)-th row and (columns // 8)-th column, as the other fixtures keep them per tensor."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qwen3moe_action_weights as aw  # noqa: E402
from gamer_amd import decode, ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeActionConfig  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3moe import Qwen3MoeActionEngine  # noqa: E402
from gamer_amd.modeling import Qwen3ActionMoeWithTemperature  # noqa: E402

VARIANT = "qwen3moe_action"
KEYS = ("input_ids", "attention_mask", "labels")
FP32_CASES = ["moe_action_small", "moe_action_mixed_small", "moe_action_bo_small"]


def _setup(golden, name, matmul=None, dtype="f32", **cfg_over):
    z, meta = golden(name)
    cfg = Qwen3MoeActionConfig(**{**meta["config"], **cfg_over})
    cfg.dropout_rate = 0.1                  # (the kernels get p = 0 through dropout=False)
    sd = aw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
    eng = Engine(cfg, temperature=meta["temperature"], variant=VARIANT, dtype=dtype, matmul=matmul)
    assert isinstance(eng, Qwen3MoeActionEngine)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in KEYS}
    return z, meta, eng, batch, sd


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _sample(g):
    return g if g.dim() == 1 else g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)]


def _samples(z, grads):
    """(key, ours, the reference's) per gradient tensor: the slices of ``grad_samples``."""
    at, flat = 0, z["grad_samples"]
    for k in (str(k) for k in z["grad_keys"]):
        got = _sample(grads[k]).cpu().numpy()
        yield k, got, flat[at:at + got.size].reshape(got.shape)
        at += got.size
    assert at == flat.size


@pytest.mark.parametrize("matmul", ["split3", "split6", "f32"])
@pytest.mark.parametrize("name", FP32_CASES)
def test_logits_loss_and_gradients_match_reference_fixture(golden, name, matmul):
    z, meta, eng, batch, _ = _setup(golden, name, matmul)
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    _, logits = eng.forward(ids, am, train=False)
    e_raw = _relmax(logits.cpu().numpy(), z["logits_raw"])
    # the routing the one prep launch built is the real router's and the real FFN's index
    r = eng.ws.router
    assert np.array_equal(r["act_idx"].cpu().numpy(), z["router_action"])
    assert np.array_equal(r["beh_idx"].cpu().numpy(), z["router_behavior"])
    assert np.array_equal(r["expert"].cpu().numpy(), z["ffn_index"])
    # 16 experts x 4 behaviour indices fit the inject table's 64 groups at this size; behaviour-only routing never takes it
    assert eng.split_inject == (name == "moe_action_small")
    loss, logits_s = eng.forward(ids, am, labels=lab, train=False)
    e_scaled = _relmax(logits_s.cpu().numpy(), z["logits_scaled"])
    eng.check_inputs()
    print(f"{name} {matmul}: logits {e_raw:.2e} / {e_scaled:.2e}, loss {float(loss):.7f} (reference {float(z['loss_mean']):.7f})")
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert abs(float(loss) - float(z["loss_mean"])) < 1e-5 * float(z["loss_mean"])
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    eng.check_inputs()
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    # (an expert no token reaches has gradient 0 on both sides: |0 - 0| / 1e-12 = 0)
    gn = float(np.sqrt((norms ** 2).sum()))
    errs = {k: _relmax(got, ref) for k, got, ref in _samples(z, eng.grads) if np.abs(ref).max() > 0}
    zero = [k for k, got, ref in _samples(z, eng.grads) if np.abs(ref).max() == 0 and np.abs(got).max() != 0]
    wk = max(errs, key=errs.get)
    print(f"{name} {matmul}: gradient norm {gn:.6f} (reference {float(z['global_grad_norm']):.6f}), worst tensor norm "
          f"{float(rel.max()):.2e}, worst sample {errs[wk]:.2e} ({wk})")
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    assert errs[wk] < 1e-3, (wk, errs[wk])
    assert not zero, zero
    assert all(bool(torch.isfinite(g).all()) for g in eng.grads.values())


def test_the_concatenated_inject_path_matches_too(golden, monkeypatch):
    """What the shipped 21 experts x 5 behaviour indices take in the fp32 forms: ``split_inject`` off."""
    monkeypatch.setenv("GAMER_SPLIT_INJECT", "0")
    z, meta, eng, batch, _ = _setup(golden, "moe_action_small", "split3")
    assert not eng.split_inject
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    _, logits = eng.forward(ids, am, train=False)
    assert _relmax(logits.cpu().numpy(), z["logits_raw"]) < 2e-5
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    gkeys = [str(k) for k in z["grad_keys"]]
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    gn = float(np.sqrt((norms ** 2).sum()))
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float((np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)).max()) < 1e-3
    assert max(_relmax(got, ref) for k, got, ref in _samples(z, eng.grads) if np.abs(ref).max() > 0) < 1e-3
    # the shipped size switches the table off by itself
    big = Qwen3MoeActionConfig(**{**meta["config"], "num_behavior": 4, "vocab_size": 60,
                                  "behavior_maps": {"46": 0, "47": 1, "48": 2, "49": 3}})
    monkeypatch.delenv("GAMER_SPLIT_INJECT")
    e21 = Engine(big, variant=VARIANT)
    assert big.num_ffn_experts == 21 and not e21.split_inject


def test_bf16_against_reference_autocast_fixture(golden):
    z, meta, eng, batch, _ = _setup(golden, "moe_action_small_bf16", dtype="bf16")
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    _, logits = eng.forward(ids, am, train=False)
    assert logits.dtype == torch.bfloat16
    ref = z["logits_raw"]
    assert float(np.abs(logits.float().cpu().numpy() - ref).max()) < 1e-2 * float(np.abs(ref).max())
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys = [str(k) for k in z["grad_keys"]]
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    for k, got, ref in _samples(z, eng.grads):
        assert np.abs(got - ref).max() <= 8e-2 * max(np.abs(ref).max(), 1e-12), k


def test_two_identical_steps_give_the_same_gradient_bits(golden):
    z, meta, eng, batch, _ = _setup(golden, "moe_action_small")
    flats = []
    for _ in range(2):
        eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
        eng.zero_grad()
        eng.backward(1.0)
        flats.append(eng.flat_g.clone())
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1])


def test_step_makes_one_prep_launch(golden, monkeypatch):
    """One gamer_moe_action_router_prep per forward and none of the launches it stands for; the backward launches none."""
    def forbidden(*a, **k):
        raise AssertionError("a prep kernel the Qwen3MoeAction step must not launch was launched")
    for name in ("router_fwd", "moe_router_prep", "session_moe_prep", "session_prep", "session_spans", "causal_prep",
                 "router_position_table", "attn_row_order"):
        monkeypatch.setattr(ops, name, forbidden)
    calls = []
    orig = ops.moe_action_router_prep
    monkeypatch.setattr(ops, "moe_action_router_prep", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    z, meta, eng, batch, _ = _setup(golden, "moe_action_small", "split3")
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    assert len(calls) == 1
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])


def test_module_matches_engine_runs_bf16_under_autocast_and_round_trips(golden, tmp_path):
    z, meta, eng, batch, sd = _setup(golden, "moe_action_small")
    ids, am, lab = batch["input_ids"], batch["attention_mask"], batch["labels"]
    m = Qwen3ActionMoeWithTemperature(Qwen3MoeActionConfig(**meta["config"]))
    m.set_hyper(meta["temperature"])
    m.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]})
    m.eval()
    keys = sorted(k for k in m.state_dict() if k != "lm_head.weight")
    assert keys == [str(k) for k in z["state_dict_keys"]]
    assert "model.layers.0.mlp.experts.expert_15.down_proj.weight" in keys
    out = m(input_ids=ids, attention_mask=am, labels=lab, actions=torch.zeros_like(ids))
    assert out["aux_loss"] == 0 and len(out["router_logits"]) == meta["config"]["num_hidden_layers"]     # model.py:585-604
    out.loss.backward()
    loss, _ = eng.forward(ids, am, labels=lab, train=True, dropout=False)
    eng.zero_grad()
    eng.backward(1.0)
    assert abs(float(out.loss.detach()) - float(loss)) <= 1e-6 * float(loss)
    assert abs(float(out.loss.detach()) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    for k, p in m.named_parameters():
        torch.testing.assert_close(p.grad, eng.grads[k], rtol=1e-5, atol=1e-8, msg=k)
    with torch.no_grad():
        lg = m(input_ids=ids, attention_mask=am).logits
    assert _relmax(lg.cpu().numpy(), z["logits_raw"]) < 2e-5
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(input_ids=ids, attention_mask=am, labels=lab)
    assert isinstance(m._amp_engine, Qwen3MoeActionEngine) and m._amp_engine.dtype == "bf16"
    assert m._amp_engine.flat_p is m.engine.flat_p
    assert abs(float(out16.loss.detach()) - float(z["loss_train_mode"])) < 1e-2
    out16.loss.backward()
    m.save_pretrained(str(tmp_path))
    again = Qwen3ActionMoeWithTemperature.from_pretrained(str(tmp_path))
    assert isinstance(again._cfg, Qwen3MoeActionConfig) and again._cfg.num_ffn_experts == 16
    for k, v in m.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k
    with pytest.raises(ValueError, match="mlp_type 'Qwen3' only"):
        Qwen3ActionMoeWithTemperature({**meta["config"], "mlp_type": "PBATransformer"})


def _decode_fixture(golden):
    fx, meta = golden("decode_moe_action_small")
    sd = aw.init_state_dict(meta["config"], meta["weight_seed"], meta["weight_scale"])
    cat = torch.from_numpy(fx["catalogue"])
    items = [t for b in range(meta["num_behavior"]) for t in synthetic.item_tokens(cat, b, meta["codebook"]).tolist()]
    return fx, meta, sd, items


@pytest.mark.parametrize("mix", [0, 1, 2])
def test_beam_search_matches_reference_generate(golden, mix):
    fx, meta, sd, items = _decode_fixture(golden)
    eng = Engine(Qwen3MoeActionConfig(**meta["config"]), temperature=0.7, variant=VARIANT)
    eng.load_state_dict(sd)
    ids, am = (torch.from_numpy(fx[f"m{mix}_{k}"]) for k in ("input_ids", "attention_mask"))
    assert len(set((am == 0).sum(1).tolist())) > 1                    # rows of different left padding
    assert len(set(ids[:, -1].tolist())) > 1                          # users of different target behaviours
    trie = decode.ItemTrie(items)                                     # the items under every behaviour token
    beams, new = meta["beams"], meta["new_tokens"]
    for use_cache in (True, False):
        seq, sc, trace = decode.beam_search(eng, ids, am, None, trie, beams, new, use_cache=use_cache, return_trace=True)
        assert torch.equal(seq.cpu(), torch.from_numpy(fx[f"m{mix}_sequences"])), use_cache
        assert float((sc.cpu().double() - torch.from_numpy(fx[f"m{mix}_scores"])).abs().max()) < 1e-4, use_cache
        # the first step - the prompt pass alone, which the fixture's router wrapper does not touch
        _, tok0, sc0 = trace[0]
        assert torch.equal(tok0.cpu(), torch.from_numpy(fx[f"m{mix}_first_tokens"])), use_cache
        assert float((sc0.cpu().double() - torch.from_numpy(fx[f"m{mix}_first_scores"])).abs().max()) < 1e-4, use_cache
    # the prompt pass kept the reference's action 0 in the last column; the steps' rows sit in several experts
    session = decode.Qwen3MoeActionDecodeSession(eng, ids, am, beams, new)
    assert int(eng.ws.router["act_idx"][:, -1].abs().sum()) == 0
    off = session.lists[(ids.shape[1]) % 5][2].cpu()
    assert int((off[1:] > off[:-1]).sum()) == len(set(ids[:, -1].tolist())) and int(off[-1]) == ids.shape[0] * beams
    with pytest.raises(ValueError, match="n \\* num_positions \\+ 1 tokens"):
        decode.beam_search(eng, ids[:, 1:], am[:, 1:], None, trie, beams, new)


def test_decode_step_graph_replay_equals_the_eager_step(golden, monkeypatch):
    """The rows' expert lists live at fixed addresses and the step has no host loop over experts: from the third session of a
    shape on it is a hipGraph replay (GAMER_DECODE_GRAPH=1) with the bits of the eager step, also for users in another order
    - other target behaviours per row, hence other lists under the same graph."""
    fx, meta, sd, items = _decode_fixture(golden)
    ids, am = (torch.from_numpy(fx[f"m0_{k}"]) for k in ("input_ids", "attention_mask"))
    rev = torch.arange(ids.shape[0] - 1, -1, -1)
    ids2, am2 = ids[rev], am[rev]
    assert ids2[:, -1].tolist() != ids[:, -1].tolist()
    trie = decode.ItemTrie(items)
    beams, new = meta["beams"], meta["new_tokens"]

    def engine():
        e = Engine(Qwen3MoeActionConfig(**meta["config"]), temperature=0.7, variant=VARIANT)
        e.load_state_dict(sd)
        return e
    monkeypatch.setenv("GAMER_DECODE_GRAPH", "0")
    eng0 = engine()
    ref1 = decode.beam_search(eng0, ids, am, None, trie, beams, new)
    ref2 = decode.beam_search(eng0, ids2, am2, None, trie, beams, new)
    assert not eng0._decode_static[next(iter(eng0._decode_static))].graphs
    assert torch.equal(ref1[0].cpu(), torch.from_numpy(fx["m0_sequences"]))
    monkeypatch.setenv("GAMER_DECODE_GRAPH", "1")
    eng = engine()
    outs = [decode.beam_search(eng, ids, am, None, trie, beams, new) for _ in range(4)]
    st = eng._decode_static[next(iter(eng._decode_static))]
    assert sorted(st.graphs) == [1, 2, 3]                       # captured in the third session, replayed in the fourth
    for seq, sc in outs:
        assert torch.equal(seq, ref1[0]) and torch.equal(sc, ref1[1])
    seq2, sc2 = decode.beam_search(eng, ids2, am2, None, trie, beams, new)
    assert torch.equal(seq2, ref2[0]) and torch.equal(sc2, ref2[1])


def test_module_generate_evaluate_and_the_bf16_refusal(golden):
    from gamer_amd.evaluate import evaluate_behavior
    fx, meta, sd, items = _decode_fixture(golden)
    m = Qwen3ActionMoeWithTemperature(Qwen3MoeActionConfig(**meta["config"]))
    m.set_hyper(0.7)
    m.load_state_dict(sd)
    m.eval()
    mix, beams, new = 1, meta["beams"], meta["new_tokens"]
    trie = decode.ItemTrie(items)
    ids, am = (torch.from_numpy(fx[f"m{mix}_{k}"]) for k in ("input_ids", "attention_mask"))
    out = m.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, num_beams=beams, num_return_sequences=beams,
                     prefix_allowed_tokens_fn=decode.prefix_allowed_tokens(trie), early_stopping=True)
    want = torch.from_numpy(fx[f"m{mix}_sequences"])
    assert torch.equal(out.sequences.cpu(), want)
    assert float((out.sequences_scores.cpu().double() - torch.from_numpy(fx[f"m{mix}_scores"])).abs().max()) < 1e-4
    # the evaluation loop dispatches on the variant through beam_search: the reference's best beam as the held-out item
    targets = [[want[b * beams, -new:].tolist()] for b in range(ids.shape[0])]
    res = evaluate_behavior(m.engine, [dict(input_ids=ids, attention_mask=am, actions=None, targets=targets)], trie,
                            num_beams=beams, metric_list=("hit@1", "ndcg@5"), item_len=new)
    assert res["samples"] == ids.shape[0] and res["hit@1"] == 1.0
    e16 = Engine(Qwen3MoeActionConfig(**meta["config"]), temperature=0.7, variant=VARIANT, dtype="bf16")
    with pytest.raises(NotImplementedError, match="not for variant 'qwen3moe_action'"):
        decode.beam_search(e16, ids, am, None, trie, beams, new)
    with pytest.raises(NotImplementedError, match="not for variant 'qwen3moe_action'"):
        e16.forward(ids, am, train=False, last_row_logits=True)


def test_train_harness_one_epoch_on_an_mb_directory(tmp_path):
    from gamer_amd import train
    synthetic.write_mb_dataset(str(tmp_path), "MBTiny", n_users=40)
    out = tmp_path / "out"
    state = train.main(["--data_path", str(tmp_path), "--dataset", "MBTiny", "--tasks", "mb_explicit_decoder_2", "--backbone",
                        "Qwen3MoeAction", "--max_his_len", "6", "--per_device_batch_size", "8", "--gradient_accumulation_steps",
                        "1", "--epochs", "1", "--logging_step", "1", "--output_dir", str(out)])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert len(losses) >= 2 and all(np.isfinite(losses)), losses
    evals = [r["eval_loss"] for r in state["log_history"] if "eval_loss" in r]
    assert len(evals) == 1 and np.isfinite(evals[0])
    m = Qwen3ActionMoeWithTemperature.from_pretrained(str(out))
    assert isinstance(m.engine, Qwen3MoeActionEngine) and m.engine.layout.numel == len(m.engine.flat_p)
    cfg = m._cfg
    assert cfg.num_positions == 5 and cfg.n_positions == 7 and cfg.num_experts == 6
    assert cfg.num_ffn_experts == 5 * cfg.num_behavior + 1 and m.engine.W[0].ne == cfg.num_ffn_experts
