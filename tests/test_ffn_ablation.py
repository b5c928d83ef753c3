"""Qwen3Multi's FFN ablation switches (mlp_type, sparse_layers_decoder, Moe_behavior_only) on the host: the config accepts
them and applies the reference's num_experts rule, the parameter layout has exactly the reference's state-dict names and shapes
(tests/golden/ablate_*.npz store the key list of the real reference model), the weight recipe matches the fixtures' checksums,
the shipped layout is unchanged and ``train.py --base_model`` reads a config.json.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

from gamer_amd import synthetic
from gamer_amd.config import Qwen3MultiConfig, apply_runtime_fields, base_model_config, expected_num_experts
from gamer_amd.engine import ParamLayout

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ffn_ablation_weights as fw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["ablate_dense_small", "ablate_pba_small", "ablate_behonly_small", "ablate_pba_small_bf16", "ablate_session_small",
         "decode_ablate_small"]


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta_json"]))


def test_config_accepts_the_ablation_switches_and_keeps_the_other_refusals():
    for kw in (dict(mlp_type="PBATransformer"), dict(sparse_layers_decoder=[0, 3, 5]), dict(sparse_layers_decoder=[]),
               dict(Moe_behavior_only=True, num_experts=2)):
        Qwen3MultiConfig(**kw).validate()
    bad = [dict(mlp_type="T5"), dict(sparse_layers_decoder=[8]), dict(Moe_behavior_only=True),
           dict(num_experts=2), dict(use_user_token=True), dict(use_behavior_token=False), dict(head_dim=128),
           dict(num_key_value_heads=1), dict(hidden_act="gelu")]
    for kw in bad:
        with pytest.raises(ValueError):
            Qwen3MultiConfig(**kw).validate()
    assert Qwen3MultiConfig().mlp_type == "Qwen3"       # (the reference falls back to PBATransformer when the key is missing)
    assert Qwen3MultiConfig().shipped_ffn


def test_num_experts_rule_and_position_table():
    cfg = Qwen3MultiConfig()
    assert expected_num_experts(cfg) == 6 and cfg.position_experts() == [1, 2, 3, 4, 5]
    cfg.Moe_behavior_only = True
    assert expected_num_experts(cfg) == 2 and cfg.position_experts() == [1, 2, 2, 2, 2]
    apply_runtime_fields(cfg, 3, {"10": 0, "11": 1, "12": 2}, num_positions=4)
    assert cfg.num_experts == 2 and cfg.num_positions == 4 and cfg.position_experts() == [1, 2, 2, 2]
    cfg.Moe_behavior_only = False
    apply_runtime_fields(cfg, 3, {"10": 0, "11": 1, "12": 2}, num_positions=4)
    assert cfg.num_experts == 5
    cfg.validate()


@pytest.mark.parametrize("name", CASES)
def test_layout_names_and_shapes_equal_the_reference_state_dict(name):
    z, meta = _fixture(name)
    cfg = Qwen3MultiConfig(**meta["config"])
    cfg.validate()
    lay = ParamLayout(cfg)
    ref = [str(k) for k in z["state_dict_keys"]]
    assert sorted(lay.entries) == ref
    shapes = fw.state_dict_shapes(meta["config"])
    assert {k: tuple(s) for k, (_, s) in lay.entries.items()} == dict(shapes)
    # HF Trainer's decay grouping: every matrix decays, the RMSNorm weights do not
    for k, (off, shp) in lay.entries.items():
        assert (off < lay.n_decay) == (len(shp) == 2), k


@pytest.mark.parametrize("name", CASES)
def test_weight_recipe_matches_the_fixture_checksums(name):
    z, meta = _fixture(name)
    sd = fw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0))
    keys, sums = fw.fp64_checksums(sd)
    assert keys == [str(k) for k in z["weight_keys"]]
    np.testing.assert_allclose(sums, z["weight_checksums"], rtol=1e-12, atol=1e-9)


def test_router_position_table_of_the_fixtures():
    """The reference router's expert index per token: [1, 2, 3, 4, 5] per item, or [1, 2, 2, 2, 2] behaviour-only; pad/eos 0."""
    for name in ("ablate_pba_small", "ablate_behonly_small"):
        z, meta = _fixture(name)
        cfg = Qwen3MultiConfig(**meta["config"])
        ids, pos = z["input_ids"], z["router_position"]
        table = np.array([0] + cfg.position_experts())
        real = (ids != cfg.pad_token_id) & (ids != cfg.eos_token_id)
        col = np.arange(ids.shape[1]) % cfg.num_positions
        np.testing.assert_array_equal(pos[real], table[col + 1][None, :].repeat(ids.shape[0], 0)[real])
        assert (pos[~real] == 0).all()


def test_shipped_layout_is_unchanged():
    cfg = Qwen3MultiConfig(vocab_size=1041, num_behavior=3)
    lay = ParamLayout(cfg)
    assert ParamLayout.VERSION == 2
    names = list(lay.entries)
    assert names[1:5] == [f"model.layers.0.self_attn.{k}_proj.weight" for k in "qkvo"]
    l0 = [n for n in names if n.startswith("model.layers.0.mlp.")]
    assert l0 == ([f"model.layers.0.mlp.experts.expert_{e}.{k}.weight" for e in range(6) for k in ("gate_proj", "up_proj")] +
                  [f"model.layers.0.mlp.experts.expert_{e}.down_proj.weight" for e in range(6)] +
                  ["model.layers.0.mlp.behavior_embedding.weight"])


def test_base_model_argument(tmp_path):
    from gamer_amd import train
    d = tmp_path / "m"
    Qwen3MultiConfig(mlp_type="PBATransformer", sparse_layers_decoder=[0, 2, 4, 6], Moe_behavior_only=True).save_pretrained(str(d))
    args = train.parse_args(["--base_model", str(d), "--max_his_len", "20"])
    assert args.base_model == str(d)
    cfg = train.synthetic_base_model_config(args.base_model, args.max_his_len)
    assert (cfg.mlp_type, cfg.sparse_layers_decoder, cfg.Moe_behavior_only) == ("PBATransformer", [0, 2, 4, 6], True)
    assert cfg.num_experts == 2 and cfg.n_positions == 21 and cfg.vocab_size == synthetic.vocab_size(256, 3)
    cfg.validate()
    assert train.parse_args([]).base_model == ""
    # a config.json without the run-time fields (the reference's shipped files): base_model_config sets them
    raw = {k: v for k, v in Qwen3MultiConfig(mlp_type="PBATransformer").to_dict().items()
           if k not in ("num_behavior", "behavior_maps", "num_positions", "num_experts")}
    (tmp_path / "r").mkdir()
    (tmp_path / "r" / "config.json").write_text(json.dumps(raw))
    cfg = base_model_config(str(tmp_path / "r"), 40, 2, {"30": 0, "31": 1}, 4, 11)
    assert (cfg.num_experts, cfg.num_positions, cfg.num_behavior, cfg.vocab_size) == (5, 4, 2, 40)
    cfg.validate()
