"""MBSTR on the HIP path, the parts that need no GPU: the config surface, the parameter layout and the seeded init against the
real reference class (tests/golden/mbstr_small.npz, tools/make_golden_mbstr.py), the refusals, the host bucket table against the
reference's rule, and the arguments of train_mbstr."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import mbstr_weights as mw  # noqa: E402

from gamer_amd import train_mbstr, train_rec
from gamer_amd.mbstr import MBSTR, MBSTRConfig, relative_position_buckets

FX = os.path.join(os.path.dirname(__file__), "golden", "mbstr_small.npz")
DEFAULTS = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, dropout_prob=0.2, hidden_act="relu", layer_norm_eps=1e-12,
                initializer_range=0.02, mask_ratio=0.2, loss_type="CE", num_buckets=32, max_distance=40, behavior_head=True,
                behavior_attention=True, behavior_moe=True, behavior_position_bias=True, n_shared_experts=3, n_specific_experts=1)


def _meta():
    return json.loads(str(np.load(FX)["meta_json"]))


def _build(m):
    return MBSTR(MBSTRConfig(**m["config"]), m["n_items"], m["max_his_len"], m["n_behaviors"])


def test_config_defaults_and_unknown_keys(tmp_path):
    assert MBSTRConfig().to_dict() == DEFAULTS
    c = MBSTRConfig(foo=1, hidden_size=32)
    assert c.hidden_size == 32 and not hasattr(c, "foo") and _meta()["unknown_key_dropped"]
    assert MBSTRConfig.from_dict(dict(DEFAULTS, mask_ratio=0.4, bar=2)).to_dict() == dict(DEFAULTS, mask_ratio=0.4)
    (tmp_path / "config.json").write_text(json.dumps(dict(DEFAULTS, n_layers=3)))
    assert MBSTRConfig.from_pretrained(str(tmp_path)).to_dict() == dict(DEFAULTS, n_layers=3)
    with pytest.raises(ValueError):
        MBSTRConfig.from_pretrained(str(tmp_path / "missing"))


@pytest.mark.parametrize("second", [False, True])
def test_state_dict_keys_shapes_and_aliasing_equal_the_reference(second):
    m = _meta()["second"] if second else _meta()
    model = _build(m)
    sd = model.state_dict()
    assert list(sd) == m["keys"] and [list(v.shape) for v in sd.values()] == m["shapes"]
    assert [n for n, _ in model.named_parameters()] == m["parameter_names"]
    assert "head.token_embeddings.weight" not in m["parameter_names"] and m["table_keys_alias"]
    assert sd["item_embedding.weight"].data_ptr() == sd["head.token_embeddings.weight"].data_ptr()
    assert model.head.token_embeddings is model.item_embedding
    assert sd["item_embedding.weight"].shape[0] == m["n_items"] + 2
    assert not any("position_embedding" in k for k in sd)


def test_shipped_config_has_the_reference_key_and_parameter_counts():
    m = _meta()
    model = MBSTR(MBSTRConfig(), m["init_n_items"], m["init_max_his_len"], m["n_behaviors"])
    assert len(model.state_dict()) == m["init_keys"] == 123
    assert sum(p.numel() for p in model.parameters()) == m["init_parameters"] == 487008


def test_seeded_weights_load_strict_and_are_pinned():
    m = _meta()
    model = _build(m)
    sd = mw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    assert np.array_equal(mw.checksums(sd), np.load(FX)["weight_checksums"])
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.item_embedding.weight, sd["head.token_embeddings.weight"])
    assert m["conditions"]["gradient_scales_ok"] and m["conditions"]["every_pair_index_occurs"]


def test_seeded_init_equals_the_reference_bit_for_bit():
    m = _meta()
    torch.manual_seed(m["init_seed"])
    model = MBSTR(MBSTRConfig(), m["init_n_items"], m["init_max_his_len"], m["n_behaviors"])
    assert np.array_equal(mw.checksums(model.state_dict()), np.load(FX)["init_checksums"])
    a = model.trm_encoder.layer[0].multi_head_attention
    assert float(a.query.detach().std()) < 0.03 < 0.5 < float(a.W1.detach().std())      # query redrawn, W1 keeps torch.randn
    assert float(model.head.w_gates.detach().std()) > 0.5


def test_expert_layernorms_are_outside_the_graph():
    m = _meta()
    assert all(".FFN." in k and ".LayerNorm." in k for k in m["no_grad"]) and len(m["no_grad"]) == 2 * 2 * m["n_behaviors"]
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"] and m["m0_no_grad"] == m["no_grad"]
    model = MBSTR(MBSTRConfig(**m["config"]), 50, 8, m["n_behaviors"])
    empty = torch.empty(0, dtype=torch.long)
    loss = model._loss(torch.zeros(2, 8, dtype=torch.long), torch.zeros(2, 8, dtype=torch.int32), empty, empty)
    assert torch.isnan(loss)
    loss.backward()
    assert [n for n, p in model.named_parameters() if p.grad is None] == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_refusals():
    m = _meta()
    quoted = "'FeedForward' object has no attribute 'dropout'"
    assert m["reference_errors"] == dict(behavior_moe_false="AttributeError: " + quoted, n_behaviors_1="AttributeError: " + quoted)
    with pytest.raises(NotImplementedError, match=quoted):
        MBSTR(MBSTRConfig(behavior_moe=False), 10, 8, 4)
    with pytest.raises(NotImplementedError, match=quoted):
        MBSTR(MBSTRConfig(), 10, 8, 1)
    with pytest.raises(NotImplementedError, match="behavior_attention=False"):
        MBSTR(MBSTRConfig(behavior_attention=False), 10, 8, 4)
    with pytest.raises(NotImplementedError, match="CE"):
        MBSTR(MBSTRConfig(loss_type="BPR"), 10, 8, 4)
    with pytest.raises(NotImplementedError, match="hidden size"):
        MBSTR(MBSTRConfig(hidden_size=66), 10, 8, 4)
    with pytest.raises(NotImplementedError, match="hidden size"):
        MBSTR(MBSTRConfig(hidden_size=512, n_heads=8), 10, 8, 4)
    with pytest.raises(NotImplementedError, match="head size"):
        MBSTR(MBSTRConfig(hidden_size=256, n_heads=2), 10, 8, 4)
    with pytest.raises(NotImplementedError, match="n_behaviors <= 8"):
        MBSTR(MBSTRConfig(), 10, 8, 9)
    model = MBSTR(MBSTRConfig(), 10, 8, 4)
    ids, n = torch.ones(2, 8, dtype=torch.long), torch.tensor([8, 8])
    inter = dict(inputs=ids, behaviors=ids, seq_len=n)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.calculate_loss(inter)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.reconstruct_train_data(ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.full_sort_topk(inter, 5)
    with pytest.raises(NotImplementedError, match="candidates"):
        model(ids, ids, ids, candidates=ids)
    with pytest.raises(NotImplementedError, match="candidates"):
        model.sample_sort_predict(inter)


def test_bucket_table_equals_the_reference_rule():
    z, m = np.load(FX), _meta()
    assert [tuple(c) for c in m["bucket_cases"]] == [(L, nb, md) for nb, md in ((32, 40), (16, 20)) for L in (1, 50, 128)]
    for L, nb, md in m["bucket_cases"]:
        got = relative_position_buckets(L, nb, md)
        assert got.dtype == torch.int32 and got.shape == (2 * L - 1,)
        assert np.array_equal(got.numpy(), z[f"buckets/{L}_{nb}_{md}"]), (L, nb, md)
        assert int(got.min()) >= 0 and int(got.max()) < nb


def test_train_mbstr_arguments():
    a = train_mbstr.parse_args([])
    assert (a.backbone, a.tasks, a.test_task, a.base_model) == ("MBSTR", "smb_dis_decoder", "smb_dis_target", "./config/dis-models/MBSTR")
    r = train_rec.parse_args([])
    same = [k for k in vars(a) if k not in ("backbone", "tasks", "test_task", "base_model")]
    assert same and all(getattr(a, k) == getattr(r, k) for k in same)
    with pytest.raises(NotImplementedError):
        train_mbstr.parse_args(["--backbone", "SASRec"])
    with pytest.raises(NotImplementedError):
        train_rec.parse_args(["--backbone", "MBSTR"])
