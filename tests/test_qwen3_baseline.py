"""The plain Qwen3 baseline (--backbone Qwen3) without a GPU: config coercion and validation, the parameter layout
against the reference's state-dict key list stored in the fixture, the harness's parser, and the seeded weight recipe
against the fixtures' checksums."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import qwen3_weights  # noqa: E402
from gamer_amd import train  # noqa: E402
from gamer_amd.config import Qwen3Config  # noqa: E402
from gamer_amd.engine_qwen3 import Qwen3Layout  # noqa: E402

LIGHT = dict(hidden_size=256, num_hidden_layers=8, num_attention_heads=6, num_key_value_heads=3, head_dim=64,
             intermediate_size=512, tie_word_embeddings=True, rope_theta=1000000.0, vocab_size=1041)


def test_defaults_are_qwen3_light():
    c = Qwen3Config()
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == (256, 8, 6, 3, 64)
    assert (c.intermediate_size, c.attention_dropout, c.rms_norm_eps, c.rope_theta) == (512, 0.1, 1e-6, 1000000)
    assert c.tie_word_embeddings and "num_positions" not in c and "behavior_maps" not in c
    c.validate()


def test_coerce_from_hf_config_object_and_config_json(tmp_path):
    transformers = pytest.importorskip("transformers")
    hf = transformers.Qwen3Config(**LIGHT)
    c = Qwen3Config.coerce(hf)
    assert c.vocab_size == 1041 and c.hidden_size == 256 and float(c.rope_theta) == 1e6 and c.tie_word_embeddings
    c.validate()
    hf.save_pretrained(str(tmp_path))          # transformers 5.x writes rope_theta inside rope_parameters
    c2 = Qwen3Config.from_pretrained(str(tmp_path))
    assert float(c2.rope_theta) == 1e6 and c2.num_key_value_heads == 3
    c3 = Qwen3Config.coerce(transformers.AutoConfig.from_pretrained(str(tmp_path)))
    assert float(c3.rope_theta) == 1e6 and c3.vocab_size == 1041
    c.save_pretrained(str(tmp_path / "ours"))
    assert Qwen3Config.from_pretrained(str(tmp_path / "ours")).to_dict() == c.to_dict()
    assert Qwen3Config.coerce({"vocab_size": 20}).vocab_size == 20


@pytest.mark.parametrize("bad, msg", [(dict(head_dim=128), "head_dim=64"), (dict(num_key_value_heads=1), "GQA group"),
                                      (dict(hidden_size=2048), "hidden_size"), (dict(hidden_size=258), "hidden_size"),
                                      (dict(tie_word_embeddings=False), "tied")])
def test_unsupported_shapes_raise(bad, msg):
    with pytest.raises(ValueError, match=msg):
        Qwen3Config(**bad).validate()


@pytest.mark.parametrize("name", ["qwen3_small", "qwen3_full"])
def test_layout_names_and_shapes_equal_reference_state_dict(golden, name):
    z, meta = golden(name)
    cfg = Qwen3Config(**meta["config"])
    lay = Qwen3Layout(cfg)
    ref = {str(k): tuple(json.loads(str(s))) for k, s in zip(z["reference_state_dict_keys"], z["reference_state_dict_shapes"])}
    assert ref.pop("lm_head.weight") == ref["model.embed_tokens.weight"]         # tied head: not a parameter of its own
    assert {k: tuple(s) for k, (_, s) in lay.entries.items()} == ref
    assert dict(qwen3_weights.state_dict_shapes(meta["config"])) == ref
    # norms (no weight decay) behind every decayed matrix, one boundary
    for k, (off, shp) in lay.entries.items():
        assert (off >= lay.n_decay) == k.endswith("norm.weight"), k
    # the fused operands: q|k|v and gate|up adjacent
    H, I = cfg.hidden_size, cfg.intermediate_size
    e = lay.entries
    assert e["model.layers.0.self_attn.k_proj.weight"][0] == e["model.layers.0.self_attn.q_proj.weight"][0] + \
        cfg.num_attention_heads * 64 * H
    assert e["model.layers.0.mlp.up_proj.weight"][0] == e["model.layers.0.mlp.gate_proj.weight"][0] + I * H


def test_module_state_dict_names_on_meta_device(golden):
    """The module's parameter tree without a GPU: the names its _register_views hangs the flat buffer on."""
    z, meta = golden("qwen3_small")
    lay = Qwen3Layout(Qwen3Config(**meta["config"]))
    from gamer_amd import modeling
    with torch.device("meta"):
        flat = torch.empty(lay.numel)
    m = modeling.Qwen3WithTemperature.__new__(modeling.Qwen3WithTemperature)
    torch.nn.Module.__init__(m)
    m._param_keys = list(lay.entries)
    m.engine = type("E", (), {"params": lay.views(flat)})()
    m._register_views()
    keys = [str(k) for k in z["reference_state_dict_keys"] if str(k) != "lm_head.weight"]
    assert sorted(n for n, _ in m.named_parameters()) == sorted(keys)
    assert all(tuple(p.shape) == tuple(json.loads(str(s))) for (n, p), s in
               zip(sorted(m.named_parameters()), [dict(zip(z["reference_state_dict_keys"], z["reference_state_dict_shapes"]))[k]
                                                  for k in sorted(keys)]))


def test_train_parser_accepts_qwen3_backbone():
    args = train.parse_args(["--backbone", "Qwen3", "--bf16"])
    assert args.backbone == "Qwen3" and args.bf16


@pytest.mark.parametrize("name", ["qwen3_small", "qwen3_full", "qwen3_small_bf16", "decode_qwen3_small"])
def test_fixture_checksums_equal_seeded_recipe(golden, name):
    z, meta = golden(name)
    sd = qwen3_weights.init_state_dict(meta["config"], seed=meta["weight_seed"], scale=meta.get("weight_scale", 1.0))
    keys, sums = qwen3_weights.fp64_checksums(sd)
    assert [str(k) for k in z["weight_keys"]] == keys
    np.testing.assert_allclose(sums, z["weight_checksums"], rtol=1e-12, atol=1e-9)
