"""The Qwen3Moe model on the host: its config accepts the reference's routing modes (including the one without behaviour
tokens, which Qwen3Multi's refuses) and refuses what the engine does not run, its parameter layout has exactly the reference
model's state-dict names and shapes (tests/golden/moe_*.npz store the key list of the real reference), the weight recipe
matches the fixtures' checksums, and a restatement of gamer_moe_router_prep's rule equals the reference router in every mode
(tests/golden/moe_router.npz).  No GPU."""
import json
import os
import sys
import types

import numpy as np
import pytest

from gamer_amd.config import Qwen3MoeConfig, Qwen3MultiConfig, apply_mb_runtime_fields, base_model_config_moe
from gamer_amd.engine_qwen3moe import Qwen3MoeLayout

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import qwen3moe_weights as mw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MODEL_CASES = ["moe_small", "moe_nobeh_small", "moe_pba_small", "moe_small_bf16", "decode_moe_small",
               "decode_moe_behonly_small"]


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta_json"]))


def _nobeh(**kw):
    d = dict(num_behavior=0, behavior_maps={}, use_behavior_token=False, behavior_injection_decoder=[], num_positions=4,
             num_experts=5)
    return Qwen3MoeConfig(**{**d, **kw})


def test_config_defaults_are_the_reference_config_json():
    cfg = Qwen3MoeConfig()
    assert cfg.cross_attention_decoder == [] and cfg.dropout_rate == 0.1 and cfg.attention_dropout == 0.1
    assert cfg.behavior_injection_decoder == [0, 1, 2, 3] and cfg.sparse_layers_decoder == list(range(8))
    assert cfg.router_aux_loss_coef == 0.001 and cfg.mlp_type == "Qwen3"


def test_config_accepts_the_routing_modes_and_refuses_the_rest():
    Qwen3MoeConfig(num_behavior=3, behavior_maps={"46": 0}).validate()
    _nobeh().validate()
    _nobeh(Moe_behavior_only=True, num_experts=2).validate()
    assert _nobeh(Moe_behavior_only=True, num_experts=2).position_experts() == [1, 1, 1, 1]
    assert Qwen3MoeConfig(Moe_behavior_only=True, num_experts=2).position_experts() == [1, 2, 2, 2, 2]
    assert _nobeh().position_experts() == [1, 2, 3, 4]
    # Qwen3Multi keeps refusing the mode without behaviour tokens
    with pytest.raises(ValueError, match="use_behavior_token"):
        Qwen3MultiConfig(use_behavior_token=False).validate()
    for bad, msg in ((dict(cross_attention_decoder=[3]), "cross attention"),
                     (dict(use_behavior_token=False), "behavior_injection_decoder"),
                     (dict(use_behavior_token=False, behavior_injection_decoder=[], num_behavior=2), "num_behavior"),
                     (dict(num_experts=3), "num_experts"), (dict(use_user_token=True), "user token"),
                     (dict(mlp_type="T5"), "mlp_type"), (dict(n_positions=0), "n_positions")):
        with pytest.raises(ValueError, match=msg):
            Qwen3MoeConfig(**bad).validate()


def test_config_from_files_and_hf_objects_falls_back_to_pbatransformer(tmp_path):
    d = Qwen3MoeConfig().to_dict()
    d.pop("mlp_type")
    (tmp_path / "config.json").write_text(json.dumps(d))
    cfg = base_model_config_moe(str(tmp_path), 60, 0, {}, False, 4, max_his_len=20)
    assert cfg.mlp_type == "PBATransformer"       # model.py:50-53
    assert (cfg.n_positions, cfg.num_positions, cfg.num_experts, cfg.behavior_injection_decoder) == (21, 4, 5, [])
    cfg.validate()
    hf = types.SimpleNamespace(**{k: v for k, v in d.items() if k != "cross_attention_decoder"})
    apply_mb_runtime_fields(hf, 3, {46: 0, 47: 1, 48: 2}, True, 5, max_his_len=10)
    got = Qwen3MoeConfig.coerce(hf)
    assert got.mlp_type == "PBATransformer" and got.cross_attention_decoder == [] and got.n_positions == 11
    assert got.behavior_maps == {"46": 0, "47": 1, "48": 2}
    got.validate()
    with pytest.raises(ValueError, match="run-time fields"):
        Qwen3MoeConfig.coerce(types.SimpleNamespace(hidden_size=256))


@pytest.mark.parametrize("name", MODEL_CASES)
def test_layout_has_the_reference_state_dict_names_and_shapes(name):
    z, meta = _fixture(name)
    cfg = Qwen3MoeConfig(**meta["config"])
    cfg.validate()
    lay = Qwen3MoeLayout(cfg)
    assert sorted(lay.entries) == [str(k) for k in z["state_dict_keys"]]
    shapes = mw.state_dict_shapes(meta["config"])
    assert {k: tuple(s) for k, (_, s) in lay.entries.items()} == dict(shapes)
    keys, sums = mw.fp64_checksums(mw.init_state_dict(meta["config"], meta["weight_seed"], meta.get("weight_scale", 1.0)))
    assert keys == [str(k) for k in z["weight_keys"]]
    np.testing.assert_allclose(sums, z["weight_checksums"], rtol=1e-12, atol=1e-9)


def router_rule(ids, cfg):
    """gamer_moe_router_prep's routing rule restated on the host: (expert, behaviour index) of every token."""
    P, n_items = int(cfg.num_positions), int(cfg.n_positions)
    table = cfg.position_experts()
    bmap = {int(k): int(v) for k, v in cfg.behavior_maps.items()}
    B, S = ids.shape
    ex, bi = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64)
    for b in range(B):
        for t in range(S):
            tok = int(ids[b, t])
            if tok in (cfg.pad_token_id, cfg.eos_token_id) or t >= n_items * P:
                continue
            ex[b, t] = table[t % P]
            if cfg.use_behavior_token and t % P:
                bi[b, t] = bmap.get(int(ids[b, t - t % P]), -1) + 1
    return ex, bi


def test_router_rule_equals_the_reference_router_in_every_mode():
    z, meta = _fixture("moe_router")
    assert len(meta["modes"]) == 4
    for mode in meta["modes"]:
        cfg = Qwen3MoeConfig(**mode["config"])
        cfg.validate()
        for kind in ("train", "prompt"):
            ids = z[f"{mode['tag']}_{kind}_ids"]
            ex, bi = router_rule(ids, cfg)
            np.testing.assert_array_equal(ex, z[f"{mode['tag']}_{kind}_position"], err_msg=f"{mode['tag']} {kind}")
            np.testing.assert_array_equal(bi, z[f"{mode['tag']}_{kind}_behavior"], err_msg=f"{mode['tag']} {kind}")
        # the fixtures cover pad and eos, and the left-padded prompts
        assert (z[f"{mode['tag']}_train_ids"] == cfg.pad_token_id).any()
        assert (z[f"{mode['tag']}_prompt_attention_mask"][:, 0] == 0).any()
    assert any((z[f"{m['tag']}_train_ids"] == 8).any() for m in meta["modes"])     # an eos token
