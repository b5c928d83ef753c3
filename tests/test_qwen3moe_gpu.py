"""The Qwen3Moe model on the HIP engine against the real reference (tests/golden/moe_*.npz, decode_moe_small.npz from
tools/make_golden_qwen3moe.py): gamer_moe_router_prep against the reference router in every routing mode and against
gamer_causal_prep's predicates bit for bit; logits, losses and gradients of the shipped config, the mode without behaviour
tokens and a PBATransformer ablation in the fp32 forms and bf16; beam search against generate(); the module surface.
Bars: those of the FFN ablation fixtures (tests/test_ffn_ablation_gpu.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gamer_amd import ops, synthetic  # noqa: E402
from gamer_amd.config import Qwen3MoeConfig  # noqa: E402
from gamer_amd.decode import ItemTrie, beam_search  # noqa: E402
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3moe import Qwen3MoeEngine  # noqa: E402
from gamer_amd.modeling import Qwen3MoeWithTemperature  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import qwen3moe_weights as mw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
F32_CASES = ["moe_small", "moe_nobeh_small", "moe_pba_small"]


def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta_json"]))
    sd = mw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
    return z, meta, sd


def _engine(name, **kw):
    z, meta, sd = _load(name)
    cfg = Qwen3MoeConfig(**meta["config"])
    cfg.dropout_rate = 0.1                  # (the kernels get p = 0 through dropout=False)
    eng = Engine(cfg, temperature=meta["temperature"], variant="qwen3moe", **kw)
    assert isinstance(eng, Qwen3MoeEngine)
    eng.load_state_dict(sd)
    batch = {k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels")}
    return z, eng, batch


def _relmax(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _grad_errors(eng, z):
    gkeys = [str(k) for k in z["grad_keys"]]
    assert sorted(eng.grads) == gkeys
    norms = np.array([float(eng.grads[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - z["grad_norms"]) / np.maximum(z["grad_norms"], 1e-12)
    samples = {}
    for k in z.files:
        if k.startswith("grad::"):
            samples[k[6:]] = _relmax(eng.grads[k[6:]].cpu().numpy(), z[k])
        elif k.startswith("gradsample::"):
            g = eng.grads[k[12:]]
            samples[k[12:]] = _relmax(g[::max(1, g.shape[0] // 8), ::max(1, g.shape[1] // 8)].cpu().numpy(), z[k])
    return gkeys, norms, rel, samples


def _prep(cfg, ids, am, rope=False):
    B, S = ids.shape
    i32 = dict(dtype=torch.int32, device=DEV)
    out = {k: torch.full((B, S), -7, **i32) for k in ("expert", "beh_idx", "kl_self", "empty_self")}
    out["tile_empty_self"] = torch.full((B, (S + 31) // 32), -7, **i32)
    out["bad_token"] = torch.zeros(1, **i32)
    tbl = cfg.position_experts()
    table = None if tbl == list(range(1, cfg.num_positions + 1)) else torch.tensor(tbl, **i32)
    pos, nxt = (torch.full((B, S), -7, **i32), torch.full((B,), -7, **i32)) if rope else (None, None)
    ops.moe_router_prep(ids.to(DEV), am.to(DEV) if am is not None else None, cfg.behavior_lut().to(DEV), table,
                        cfg.num_positions, cfg.n_positions, cfg.use_behavior_token, cfg.pad_token_id, cfg.eos_token_id,
                        out, pos_ids=pos, next_pos=nxt)
    return out, pos, nxt


def test_moe_router_prep_equals_the_reference_router_and_causal_prep():
    z = np.load(os.path.join(GOLDEN, "moe_router.npz"))
    meta = json.loads(str(z["meta_json"]))
    for mode in meta["modes"]:
        cfg = Qwen3MoeConfig(**mode["config"])
        for kind in ("train", "prompt"):
            tag = f"{mode['tag']}_{kind}"
            ids, am = torch.from_numpy(z[tag + "_ids"]), torch.from_numpy(z[tag + "_attention_mask"])
            for mask in (am, None):
                out, pos, nxt = _prep(cfg, ids, mask, rope=True)
                assert torch.equal(out["expert"].cpu().long(), torch.from_numpy(z[tag + "_position"]).long()), tag
                assert torch.equal(out["beh_idx"].cpu().long(), torch.from_numpy(z[tag + "_behavior"]).long()), tag
                assert int(out["bad_token"]) == 0
                B, S = ids.shape
                i32 = dict(dtype=torch.int32, device=DEV)
                ref = {k: torch.empty(B, S, **i32) for k in ("kl_self", "empty_self", "pos_ids")}
                ref["tile_empty_self"] = torch.empty(B, (S + 31) // 32, **i32)
                ref["next_pos"] = torch.empty(B, **i32)
                ops.causal_prep(mask.to(DEV) if mask is not None else None, B, S, ref["kl_self"], ref["empty_self"],
                                ref["tile_empty_self"], pos_ids=ref["pos_ids"], next_pos=ref["next_pos"])
                for k in ("kl_self", "empty_self", "tile_empty_self"):
                    assert torch.equal(out[k], ref[k]), (tag, k)
                assert torch.equal(pos, ref["pos_ids"]) and torch.equal(nxt, ref["next_pos"]), tag
    # an item start outside behavior_maps is counted (the reference fails in its embedding there)
    cfg = Qwen3MoeConfig(**meta["modes"][0]["config"])
    ids = torch.from_numpy(z[meta["modes"][0]["tag"] + "_train_ids"]).clone()
    ids[0, 0] = 20
    out, _, _ = _prep(cfg, ids, None)
    assert int(out["bad_token"]) == 1 and int(out["beh_idx"][0, 1]) == 0


@pytest.mark.parametrize("matmul", ["f32", "split3", "split6"])
@pytest.mark.parametrize("name", F32_CASES)
def test_qwen3moe_against_reference_fixture(name, matmul):
    z, eng, batch = _engine(name, matmul=matmul)
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], train=False)
    e_raw = _relmax(logits.cpu().numpy(), z["logits_raw"])
    loss, logits_s = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=False)
    e_scaled = _relmax(logits_s.cpu().numpy(), z["logits_scaled"])
    assert e_raw < 2e-5 and e_scaled < 2e-5, (e_raw, e_scaled)
    assert abs(float(loss) - float(z["loss_mean"])) < 1e-5 * float(z["loss_mean"])
    assert torch.equal(eng.ws.router["expert"].cpu().long(), torch.from_numpy(z["router_position"]).long())
    assert torch.equal(eng.ws.router["beh_idx"].cpu().long(), torch.from_numpy(z["router_behavior"]).long())
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-5 * float(z["loss_train_mode"])
    eng.zero_grad()
    eng.backward(1.0)
    eng.check_inputs()
    gkeys, norms, rel, samples = _grad_errors(eng, z)
    gn = float(np.sqrt((norms ** 2).sum()))
    assert abs(gn - float(z["global_grad_norm"])) < 1e-4 * float(z["global_grad_norm"])
    assert float(rel.max()) < 1e-3, gkeys[int(rel.argmax())]
    wk = max(samples, key=samples.get)
    assert samples[wk] < 1e-3, (wk, samples[wk])
    assert all(bool(torch.isfinite(g).all()) for g in eng.grads.values())


def test_qwen3moe_bf16_against_reference_autocast_fixture():
    z, eng, batch = _engine("moe_small_bf16", dtype="bf16")
    _, logits = eng.forward(batch["input_ids"], batch["attention_mask"], train=False)
    assert logits.dtype == torch.bfloat16
    ref = z["logits_raw"]
    assert float(np.abs(logits.float().cpu().numpy() - ref).max()) < 1e-2 * float(np.abs(ref).max())
    loss, _ = eng.forward(batch["input_ids"], batch["attention_mask"], labels=batch["labels"], train=True, dropout=False)
    assert abs(float(loss) - float(z["loss_train_mode"])) < 1e-3
    eng.zero_grad()
    eng.backward(1.0)
    torch.cuda.synchronize()
    gkeys, norms, rel, _ = _grad_errors(eng, z)
    np.testing.assert_allclose(norms, z["grad_norms"], rtol=3e-2, atol=1e-9)
    for k in z.files:
        if k.startswith("grad::") or k.startswith("gradsample::"):
            gt = eng.grads[k.split("::")[1]].cpu()
            got = gt.numpy() if k.startswith("grad::") else gt[::max(1, gt.shape[0] // 8), ::max(1, gt.shape[1] // 8)].numpy()
            assert np.abs(got - z[k]).max() <= 8e-2 * max(np.abs(z[k]).max(), 1e-12), k


@pytest.mark.parametrize("tb", [0, 1, 2])
@pytest.mark.parametrize("name", ["decode_moe_small", "decode_moe_behonly_small"])
def test_decode_beams_match_reference_generate(name, tb):
    z, meta, sd = _load(name)
    eng = Engine(Qwen3MoeConfig(**meta["config"]), temperature=0.7, variant="qwen3moe")
    eng.load_state_dict(sd)
    ids, am = (torch.from_numpy(z[f"b{tb}_{k}"]) for k in ("input_ids", "attention_mask"))
    assert len(set((am == 0).sum(1).tolist())) > 1                    # rows of different left padding
    trie = ItemTrie(synthetic.item_tokens(torch.from_numpy(z["catalogue"]), tb, meta["codebook"]).tolist())
    beams = meta["beams"]
    for use_cache in (True, False):
        seq, sc = beam_search(eng, ids, am, None, trie, beams, 4, use_cache=use_cache)
        assert torch.equal(seq.cpu(), torch.from_numpy(z[f"b{tb}_sequences"])), use_cache
        assert float((sc.cpu().double() - torch.from_numpy(z[f"b{tb}_scores"])).abs().max()) < 1e-4, use_cache


def test_module_surface(tmp_path):
    z, meta, sd = _load("moe_small")
    model = Qwen3MoeWithTemperature(Qwen3MoeConfig(**meta["config"]), matmul="f32")
    model.set_hyper(meta["temperature"])
    model.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]})
    assert sorted(k for k in model.state_dict() if k != "lm_head.weight") == [str(k) for k in z["state_dict_keys"]]
    ids, am, lab = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    # the collator's actions / session ids are accepted and ignored
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=am, labels=lab, actions=torch.zeros_like(ids), session_ids=ids)
    assert abs(float(out.loss) - float(z["loss_mean"])) < 1e-5 * float(z["loss_mean"])
    assert out.aux_loss == 0 and len(out.router_logits) == meta["config"]["num_hidden_layers"]
    model.train()
    out = model(input_ids=ids, attention_mask=am, labels=lab)
    out.loss.backward()
    model.save_pretrained(str(tmp_path))
    again = Qwen3MoeWithTemperature.from_pretrained(str(tmp_path), matmul="f32")
    for k, v in model.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k


def test_module_generate_matches_reference_generate_and_checks_its_bounds():
    z, meta, sd = _load("decode_moe_small")
    model = Qwen3MoeWithTemperature(Qwen3MoeConfig(**meta["config"]), matmul="split3")
    model.set_hyper(0.7)
    model.load_state_dict(sd)
    trie = ItemTrie(synthetic.item_tokens(torch.from_numpy(z["catalogue"]), 1, meta["codebook"]).tolist())
    ids, am = torch.from_numpy(z["b1_input_ids"]), torch.from_numpy(z["b1_attention_mask"])
    out = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, num_beams=meta["beams"],
                         num_return_sequences=meta["beams"], trie=trie)
    assert torch.equal(out.sequences.cpu(), torch.from_numpy(z["b1_sequences"]))
    assert float((out.sequences_scores.cpu().double() - torch.from_numpy(z["b1_scores"])).abs().max()) < 1e-4
    # columns past the router's table (n_positions * num_positions + 1) are refused, as the reference fails there
    n = model.engine.max_len() - ids.shape[1] + 2
    with pytest.raises(ValueError, match="router's table"):
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=n, num_beams=2, num_return_sequences=2, trie=trie)
    # no behaviour tokens: trained and scored, not generated from
    zb, metab, sdb = _load("moe_nobeh_small")
    nob = Engine(Qwen3MoeConfig(**metab["config"]), variant="qwen3moe")
    with pytest.raises(NotImplementedError, match="behaviour tokens"):
        beam_search(nob, torch.from_numpy(zb["input_ids"])[:, :8], torch.ones(3, 8, dtype=torch.int64), None, trie, 2, 4)


@pytest.mark.parametrize("backbone,task", [("Qwen3Moe", "mb_explicit_decoder_2"), ("Qwen3Moe", "mb"),
                                           ("Qwen3", "mb_explicit_back")])
def test_train_two_steps_on_mb_data(tmp_path, backbone, task):
    from gamer_amd import train
    synthetic.write_mb_dataset(str(tmp_path), "MBTiny", n_users=40)
    state = train.main(["--data_path", str(tmp_path), "--dataset", "MBTiny", "--tasks", task, "--backbone", backbone,
                        "--max_his_len", "6", "--per_device_batch_size", "8", "--gradient_accumulation_steps", "1",
                        "--epochs", "1", "--logging_step", "1", "--output_dir", str(tmp_path / "out")])
    losses = [r["loss"] for r in state["log_history"] if "loss" in r]
    assert len(losses) >= 2 and all(np.isfinite(losses)), losses
    assert any("eval_loss" in r and np.isfinite(r["eval_loss"]) for r in state["log_history"])
    cls = Qwen3MoeWithTemperature if backbone == "Qwen3Moe" else __import__("gamer_amd.modeling").modeling.Qwen3WithTemperature
    model = cls.from_pretrained(str(tmp_path / "out"))
    assert model.engine.layout.numel == len(model.engine.flat_p)


def test_train_refuses_mb_explicit_back_for_qwen3moe(tmp_path):
    from gamer_amd import train
    synthetic.write_mb_dataset(str(tmp_path), "MBTiny")
    with pytest.raises(ValueError, match="mb_explicit_back"):
        train.main(["--data_path", str(tmp_path), "--dataset", "MBTiny", "--tasks", "mb_explicit_back", "--backbone",
                    "Qwen3Moe", "--max_his_len", "6", "--per_device_batch_size", "8"])
