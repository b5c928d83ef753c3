"""PBAT on the HIP path, the parts that need no GPU: the config surface, the parameter layout and the seeded init against the real
reference class (tests/golden/pbat_small.npz, tools/make_golden_pbat.py), the refusals and limits, and the arguments of
train_pbat."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pbat_weights as pw  # noqa: E402

from gamer_amd import ops, train_pbat, train_rec
from gamer_amd.pbat import PBAT, PBATConfig

FX = os.path.join(os.path.dirname(__file__), "golden", "pbat_small.npz")
DEFAULTS = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, dropout_prob=0.2, hidden_act="elu", layer_norm_eps=1e-12,
                initializer_range=0.02, mask_ratio=0.2, loss_type="CE")


def _meta():
    return json.loads(str(np.load(FX)["meta_json"]))


def _build(m):
    return PBAT(PBATConfig(**m["config"]), m["n_items"], m["n_users"], m["max_his_len"], m["n_behaviors"])


def test_config_defaults_and_unknown_keys(tmp_path):
    assert PBATConfig().to_dict() == DEFAULTS == _meta()["config_defaults"] and len(DEFAULTS) == 10
    c = PBATConfig(foo=1, hidden_size=32)
    assert c.hidden_size == 32 and not hasattr(c, "foo") and _meta()["unknown_key_dropped"]
    assert PBATConfig.from_dict(dict(DEFAULTS, mask_ratio=0.4, bar=2)).to_dict() == dict(DEFAULTS, mask_ratio=0.4)
    (tmp_path / "config.json").write_text(json.dumps(dict(DEFAULTS, n_layers=3)))
    assert PBATConfig.from_pretrained(str(tmp_path)).to_dict() == dict(DEFAULTS, n_layers=3)
    with pytest.raises(ValueError):
        PBATConfig.from_pretrained(str(tmp_path / "missing"))


@pytest.mark.parametrize("second", [False, True])
def test_state_dict_keys_shapes_and_aliasing_equal_the_reference(second):
    m = _meta()["second"] if second else _meta()
    model = _build(m)
    sd = model.state_dict()
    assert list(sd) == m["keys"] and [list(v.shape) for v in sd.values()] == m["shapes"]
    assert [n for n, _ in model.named_parameters()] == m["parameter_names"]
    assert m["table_keys_alias"]
    for alias, key in pw.ALIASES.items():
        assert alias not in m["parameter_names"] and sd[alias].data_ptr() == sd[key].data_ptr()
        assert sd[key].shape[0] == m["n_items"] + 2
    assert model.head.token_embeddings_m is model.item_embedding_m.embedding
    assert model.head.token_embeddings_c is model.item_embedding_c.embedding
    assert sd["user_embedding_m.embedding.weight"].shape[0] == m["n_users"] + 1
    assert sd["type_relation_embedding_c.embedding.weight"].shape[0] == m["n_behaviors"] ** 2 + 1


def test_shipped_config_has_the_reference_key_and_parameter_counts():
    m = _meta()
    model = PBAT(PBATConfig(), m["init_n_items"], m["init_n_users"], m["init_max_his_len"], m["init_n_behaviors"])
    assert list(model.state_dict()) == m["init_state_keys"] and len(model.state_dict()) == m["init_keys"] == 146
    assert sum(p.numel() for p in model.parameters()) == m["init_parameters"]


def test_seeded_weights_load_strict_and_are_pinned():
    m = _meta()
    for mm, prefix in ((m, ""), (m["second"], "b/")):
        model = _build(mm)
        sd = pw.init_state_dict({k: tuple(s) for k, s in zip(mm["keys"], mm["shapes"])}, mm["weight_seed"])
        assert np.array_equal(pw.checksums(sd), np.load(FX)[prefix + "weight_checksums"])
        model.load_state_dict(sd, strict=True)
        assert torch.equal(model.item_embedding_c.embedding.weight, sd["head.token_embeddings_c.weight"])
        c = mm["conditions"]
        assert c["gradient_scales_ok"] and c["every_type_pair_occurs"] and c["every_type_occurs"] and c["rows_of_length_1_and_full"]


def test_seeded_init_equals_the_reference_bit_for_bit():
    m = _meta()
    torch.manual_seed(m["init_seed"])
    model = PBAT(PBATConfig(), m["init_n_items"], m["init_n_users"], m["init_max_his_len"], m["init_n_behaviors"])
    assert np.array_equal(pw.checksums(model.state_dict()), np.load(FX)["init_checksums"])
    assert float(model.Wub.weight.detach().std()) < 0.03 and not bool(model.Wub.bias.detach().any())


def test_expert_layernorms_are_outside_the_graph():
    m = _meta()
    assert all(".FFN." in k and ".LayerNorm." in k for k in m["no_grad"]) and len(m["no_grad"]) == 2 * 2 * m["n_behaviors"]
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"] and m["m0_no_grad"] == m["no_grad"] and m["zero_grad"] == []
    model = PBAT(PBATConfig(**m["config"]), 50, 5, 8, m["n_behaviors"])
    empty = torch.empty(0, dtype=torch.long)
    loss = model._loss(torch.zeros(2, 8, dtype=torch.long), torch.zeros(2, 8, dtype=torch.int32), torch.ones(2, dtype=torch.long),
                       empty, empty)
    assert torch.isnan(loss)
    loss.backward()
    assert [n for n, p in model.named_parameters() if p.grad is None] == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_reference_quirks_recorded():
    m = _meta()
    assert m["b1_error"].startswith("IndexError")                      # B = 1 does not run in the reference; it runs here (GPU test)
    assert m["h1_error"].startswith("RuntimeError: shape")             # nor does one head: .squeeze() drops the head axis
    assert m["m1_logits_dim"] == 1 and m["type_error"].startswith("IndexError")


def test_refusals_and_limits():
    with pytest.raises(NotImplementedError, match="CE"):
        PBAT(PBATConfig(loss_type="BPR"), 10, 5, 8, 4)
    with pytest.raises(ValueError, match="not a multiple of the number of attention heads"):
        PBAT(PBATConfig(hidden_size=64, n_heads=3), 10, 5, 8, 4)
    with pytest.raises(NotImplementedError, match="hidden size <= 128"):
        PBAT(PBATConfig(hidden_size=256, n_heads=4), 10, 5, 8, 4)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        PBAT(PBATConfig(hidden_size=66, n_heads=1), 10, 5, 8, 4)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        PBAT(PBATConfig(hidden_size=36, n_heads=6), 10, 5, 8, 4)             # head size 6
    with pytest.raises(NotImplementedError, match="head size <= 64"):
        PBAT(PBATConfig(hidden_size=128, n_heads=1), 10, 5, 8, 4)
    with pytest.raises(NotImplementedError, match="n_behaviors <= 8"):
        PBAT(PBATConfig(), 10, 5, 8, 9)
    for bad in (dict(L=129), dict(d=68), dict(d=30), dict(H=132), dict(b=9), dict(b=0), dict(L=0)):
        kw = dict(dict(L=50, H=64, d=32, b=4), **bad)
        with pytest.raises(NotImplementedError, match="PBAT on the HIP path"):
            ops.pbat_check_limits(kw["L"], kw["H"], kw["d"], kw["b"])
    ops.pbat_check_limits(128, 128, 64, 8)
    model = PBAT(PBATConfig(), 10, 5, 8, 4)
    ids, n, u = torch.ones(2, 8, dtype=torch.long), torch.tensor([8, 8]), torch.ones(2, dtype=torch.long)
    inter = dict(inputs=ids, behaviors=ids, uid=u, seq_len=n)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.calculate_loss(inter)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.reconstruct_train_data(ids)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.full_sort_topk(inter, 5)
    with pytest.raises(NotImplementedError, match="candidates"):
        model(ids, ids, u, ids, candidates=ids)
    with pytest.raises(NotImplementedError, match="candidates"):
        model.sample_sort_predict(inter)


def test_head_table_hook_default_is_the_item_table():
    from gamer_amd.bert4rec import BERT4Rec, BERT4RecConfig
    model = BERT4Rec(BERT4RecConfig(), 10, 8)
    E, bias, V, shared = model._head_table("token")
    assert E is model.item_embedding.weight and bias is model.head.bias and V == 11 and shared == "token"


def test_train_pbat_arguments():
    a = train_pbat.parse_args([])
    assert (a.backbone, a.tasks, a.test_task, a.base_model) == ("PBAT", "smb_dis_decoder", "smb_dis_target", "./config/dis-models/PBAT")
    r = train_rec.parse_args([])
    same = [k for k in vars(a) if k not in ("backbone", "tasks", "test_task", "base_model")]
    assert same and all(getattr(a, k) == getattr(r, k) for k in same)
    with pytest.raises(NotImplementedError):
        train_pbat.parse_args(["--backbone", "MBSTR"])
    with pytest.raises(NotImplementedError):
        train_rec.parse_args(["--backbone", "PBAT"])
