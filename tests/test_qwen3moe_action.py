"""The Qwen3MoeAction backbone (--backbone Qwen3MoeAction) without a GPU: its config (round trip, the two refusals, the FFN's
expert count next to the router's), the parameter layout against the real reference class's state-dict key list and shapes
stored in the fixtures (tools/make_golden_moe_action.py), the torch restatement of the routing rule against the router
outputs the real class stored, the engine class ``Engine(variant=...)`` constructs, the harness's refusals before device
set-up, and what the fixtures must exercise."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import moe_action_routing as routing  # noqa: E402
import qwen3moe_action_weights as aw  # noqa: E402
from gamer_amd import train  # noqa: E402
from gamer_amd.config import (Qwen3MoeActionConfig, Qwen3MoeConfig, Qwen3MultiConfig, Qwen3SessionMoeConfig,  # noqa: E402
                              apply_mb_runtime_fields, base_model_config_moe_action)
from gamer_amd.engine import Engine  # noqa: E402
from gamer_amd.engine_qwen3moe import Qwen3MoeActionEngine, Qwen3MoeEngine, Qwen3MoeLayout  # noqa: E402

TRAIN_CASES = ["moe_action_small", "moe_action_mixed_small", "moe_action_bo_small", "moe_action_small_bf16"]
CASES = TRAIN_CASES + ["decode_moe_action_small"]
RUNTIME = dict(num_behavior=4, behavior_maps={"46": 0, "47": 1, "48": 2, "49": 3}, num_positions=5, n_positions=21)


def test_expert_counts_the_routers_and_the_ffns():
    cfg = Qwen3MoeActionConfig(**RUNTIME)
    cfg.validate()
    assert isinstance(cfg, Qwen3MoeConfig)
    assert (cfg.num_experts, cfg.num_ffn_experts) == (6, 21)              # the shipped five positions, four behaviours
    bo = Qwen3MoeActionConfig(**{**RUNTIME, "Moe_behavior_only": True, "num_experts": 2})
    bo.validate()
    assert (bo.num_experts, bo.num_ffn_experts) == (2, 5)
    assert "num_ffn_experts" not in cfg.to_dict()                          # derived, not a config.json key
    # the base configs: one count for both
    for base in (Qwen3MultiConfig(num_behavior=3), Qwen3MoeConfig(**RUNTIME),
                 Qwen3SessionMoeConfig(**RUNTIME, model_max_length=1024)):
        assert base.num_ffn_experts == base.num_experts == 6
    with pytest.raises(ValueError, match="num_experts"):
        Qwen3MoeActionConfig(**{**RUNTIME, "num_experts": 21}).validate()  # (stays the router's count)
    with pytest.raises(ValueError, match="at most 64 groups"):
        Qwen3MoeActionConfig(**{**RUNTIME, "num_positions": 16, "num_experts": 17, "num_behavior": 4}).validate()


def test_the_two_refusals():
    with pytest.raises(ValueError, match="PBATransformerSparseMLP.forward with four arguments"):
        Qwen3MoeActionConfig(**RUNTIME, mlp_type="PBATransformer")        # at construction
    cfg = Qwen3MoeActionConfig(**RUNTIME)
    cfg.mlp_type = "PBATransformer"
    with pytest.raises(ValueError, match="mlp_type 'Qwen3' only"):
        cfg.validate()
    nobeh = Qwen3MoeActionConfig(num_positions=4, num_experts=5, n_positions=21, num_behavior=0, behavior_maps={},
                                 use_behavior_token=False, behavior_injection_decoder=[])
    Qwen3MoeConfig(**nobeh.to_dict()).validate()                          # (Qwen3Moe runs this mode)
    with pytest.raises(ValueError, match="needs behaviour tokens.*one expert"):
        nobeh.validate()


def test_round_trip_coerce_and_base_model(tmp_path):
    c = Qwen3MoeActionConfig.coerce({**RUNTIME, "vocab_size": 60})
    assert Qwen3MoeActionConfig.coerce(c) is c and c.vocab_size == 60
    c.save_pretrained(str(tmp_path / "ours"))
    again = Qwen3MoeActionConfig.from_pretrained(str(tmp_path / "ours"))
    assert again.to_dict() == c.to_dict() and again.num_ffn_experts == 21
    # a config.json without mlp_type is the reference's "PBATransformer": refused when read
    d = c.to_dict()
    d.pop("mlp_type")
    (tmp_path / "config.json").write_text(json.dumps(d))
    with pytest.raises(ValueError, match="without mlp_type falls back"):
        Qwen3MoeActionConfig.from_pretrained(str(tmp_path))
    d["mlp_type"] = "Qwen3"
    for k in ("num_positions", "num_behavior", "behavior_maps", "n_positions"):
        d.pop(k)
    (tmp_path / "config.json").write_text(json.dumps(d))
    b = base_model_config_moe_action(str(tmp_path), 145, 4, {46: 0, 47: 1, 48: 2, 49: 3}, 5, max_his_len=20, pad_token_id=4)
    assert isinstance(b, Qwen3MoeActionConfig)
    assert (b.vocab_size, b.num_positions, b.n_positions, b.num_experts, b.num_ffn_experts) == (145, 5, 21, 6, 21)
    b.validate()
    transformers = pytest.importorskip("transformers")
    base = {k: v for k, v in Qwen3MoeConfig().to_dict().items()
            if k not in ("num_positions", "num_behavior", "behavior_maps", "n_positions", "mlp_type", "torch_dtype",
                         "architectures", "model_type")}
    hf = transformers.Qwen3MoeConfig(**base)
    apply_mb_runtime_fields(hf, 4, {46: 0, 47: 1, 48: 2, 49: 3}, True, 5, 20)
    with pytest.raises(ValueError, match="mlp_type 'Qwen3' only"):
        Qwen3MoeActionConfig.coerce(hf)                                   # (no mlp_type attribute: "PBATransformer")
    hf.mlp_type = "Qwen3"
    h = Qwen3MoeActionConfig.coerce(hf)
    assert (h.num_experts, h.num_ffn_experts, h.behavior_maps["48"]) == (6, 21, 2)
    h.validate()


@pytest.mark.parametrize("name", CASES)
def test_layout_has_the_reference_state_dict_names_and_shapes(golden, name):
    z, meta = golden(name)
    assert meta["model"] == "Qwen3ActionMoeWithTemperature"
    cfg = Qwen3MoeActionConfig(**meta["config"])
    cfg.validate()
    lay = Qwen3MoeActionEngine._layout_cls(cfg)
    assert isinstance(lay, Qwen3MoeLayout)
    keys = [str(k) for k in z["state_dict_keys"]]
    assert sorted(lay.entries) == keys
    sparse = cfg.sparse_layers_decoder[0]
    n = sum(k.startswith(f"model.layers.{sparse}.mlp.experts.") and k.endswith("down_proj.weight") for k in keys)
    assert n == cfg.num_ffn_experts == (cfg.num_experts - 1) * 3 + 1
    ours = {k: tuple(s) for k, (_, s) in lay.entries.items()}
    if "state_dict_shapes" in z.files:
        assert ours == {k: tuple(json.loads(str(s))) for k, s in zip(keys, z["state_dict_shapes"])}
    assert ours == dict(aw.state_dict_shapes(meta["config"]))
    wkeys, sums = aw.fp64_checksums(aw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0)))
    assert wkeys == [str(k) for k in z["weight_keys"]]
    np.testing.assert_allclose(sums, z["weight_checksums"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_routing_restatement_equals_the_reference_routers_outputs(golden, name):
    z, meta = golden(name)
    got = routing.route_config(torch.from_numpy(z["input_ids"]), meta["config"])
    for ours, theirs in (("position", "router_position"), ("behavior", "router_behavior"), ("action", "router_action"),
                         ("ffn_index", "ffn_index")):
        assert np.array_equal(got[ours].numpy(), z[theirs].astype(np.int64)), (name, ours)
    assert got["bad_token"] == 0


def test_fixtures_exercise_what_the_routing_can_get_wrong(golden):
    z, meta = golden("moe_action_small")
    am, ids, act, idx = z["attention_mask"], z["input_ids"], z["router_action"], z["ffn_index"]
    assert am.shape == (3, 46) and meta["config"]["num_positions"] == 5 and meta["num_ffn_experts"] == 16
    assert [int(a.sum()) for a in am] == [46, 25, 38]                     # a full row, right padding, a ragged tail
    # the last column of 9 * 5 + 1 tokens is a behaviour token - not special - and still has action 0
    assert str(int(ids[0, -1])) in meta["config"]["behavior_maps"] and act[0, -1] == 0 and idx[0, -1] == 0
    assert set(np.unique(act[am == 1])) == {0, 1, 2, 3}
    assert (act[:, 0] > 0).all()                                          # the behaviour token itself carries its action
    assert len(np.unique(idx)) == 16
    zb, mb = golden("moe_action_bo_small")
    n = mb["num_ffn_experts"]
    assert n == 4 and zb["ffn_index"].max() == n                          # rows whose index names no expert
    pairs = {(int(a), int(p)) for a, p, i in zip(zb["router_action"].ravel(), zb["router_position"].ravel(),
                                                 zb["ffn_index"].ravel()) if i == 2}
    assert len(pairs) > 1                                                 # index collisions: two (action, position) pairs
    zm, mm = golden("moe_action_mixed_small")
    assert mm["config"]["sparse_layers_decoder"] == [0, 2]
    fx, md = golden("decode_moe_action_small")
    for m, mix in enumerate(fx["mixes"]):
        assert len(set(mix.tolist())) >= 2                                # users of different target behaviours
        ids0 = fx[f"m{m}_input_ids"]
        assert ids0.shape[1] % 5 == 1 and len(set((fx[f"m{m}_attention_mask"] == 0).sum(1).tolist())) > 1
        maps = md["config"]["behavior_maps"]
        assert [maps[str(int(t))] for t in ids0[:, -1]] == mix.tolist()


def test_engine_variant_dispatches_to_the_action_class():
    cfg = Qwen3MoeActionConfig(**RUNTIME)
    eng = Engine.__new__(Engine, cfg, variant="qwen3moe_action")          # (the class only: construction needs the device)
    assert type(eng) is Qwen3MoeActionEngine and isinstance(eng, Qwen3MoeEngine)
    assert Qwen3MoeActionEngine._VARIANTS == ("qwen3moe_action",) and Qwen3MoeActionEngine._config_cls is Qwen3MoeActionConfig
    assert type(Engine.__new__(Engine, cfg, variant="qwen3moe")) is Qwen3MoeEngine
    # the class adds the routing launch and the FFN of rows in several experts; the loops are Qwen3Moe's
    assert Qwen3MoeActionEngine.backward is Qwen3MoeEngine.backward and Qwen3MoeActionEngine._route is not Qwen3MoeEngine._route


def test_harness_accepts_the_backbone_and_refuses_tasks_without_behaviour_tokens_before_device_setup(tmp_path, monkeypatch):
    args = train.parse_args(["--backbone", "Qwen3MoeAction", "--bf16", "--tasks", "mb_explicit", "--base_model", "x"])
    assert args.backbone == "Qwen3MoeAction" and args.bf16 and args.base_model == "x"

    def no_device(*a, **k):
        raise AssertionError("the device was set up before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit, match="needs behaviour tokens: task mb has none"):
        train.main(["--backbone", "Qwen3MoeAction", "--data_path", str(tmp_path), "--dataset", "none", "--tasks", "mb"])
    with pytest.raises(SystemExit, match="MB tasks with behaviour tokens"):
        train.main(["--backbone", "Qwen3MoeAction", "--data_path", str(tmp_path), "--dataset", "none", "--tasks",
                    "smb_explicit_decoder_2"])
    with pytest.raises(SystemExit):
        train.parse_args(["--backbone", "Qwen3MoEAction"])
