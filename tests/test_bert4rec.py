"""BERT4Rec on the HIP path, the parts that need no GPU: the config surface, the parameter layout and the seeded init against
the real reference class (tests/golden/bert4rec_small.npz, tools/make_golden_bert4rec.py), the refusals and the arguments of
train_bert4rec (train_rec still refuses the backbone)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import bert4rec_weights as bw  # noqa: E402

from gamer_amd import train_bert4rec, train_rec
from gamer_amd.bert4rec import BERT4Rec, BERT4RecConfig

FX = os.path.join(os.path.dirname(__file__), "golden", "bert4rec_small.npz")
DEFAULTS = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, dropout_prob=0.2, hidden_act="gelu", layer_norm_eps=1e-12,
                initializer_range=0.02, mask_ratio=0.2, ft_ratio=0.5, loss_type="CE")


def _meta():
    return json.loads(str(np.load(FX)["meta_json"]))


def test_config_defaults_and_unknown_keys():
    assert BERT4RecConfig().to_dict() == DEFAULTS
    c = BERT4RecConfig(foo=1, hidden_size=32)
    assert c.hidden_size == 32 and not hasattr(c, "foo") and _meta()["unknown_key_dropped"]
    assert BERT4RecConfig.from_dict(dict(DEFAULTS, mask_ratio=0.4, bar=2)).to_dict() == dict(DEFAULTS, mask_ratio=0.4)


def test_from_pretrained(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(dict(DEFAULTS, n_layers=3)))       # the reference's shipped keys
    assert BERT4RecConfig.from_pretrained(str(tmp_path)).to_dict() == dict(DEFAULTS, n_layers=3)
    with pytest.raises(ValueError):
        BERT4RecConfig.from_pretrained(str(tmp_path / "missing"))


def test_state_dict_keys_shapes_and_aliasing_equal_the_reference():
    m = _meta()
    model = BERT4Rec(BERT4RecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    sd = model.state_dict()
    assert list(sd) == m["keys"] and list(sd)[0] == "output_bias"
    assert [list(v.shape) for v in sd.values()] == m["shapes"]
    assert [n for n, _ in model.named_parameters()] == m["parameter_names"]
    assert "head.token_embeddings.weight" not in m["parameter_names"] and m["table_keys_alias"]
    assert sd["item_embedding.weight"].data_ptr() == sd["head.token_embeddings.weight"].data_ptr()
    assert model.head.token_embeddings is model.item_embedding
    assert sd["item_embedding.weight"].shape[0] == m["n_items"] + 2 and sd["head.bias"].shape == (1, m["n_items"] + 1)


def test_seeded_weights_load_strict_and_are_pinned():
    m = _meta()
    model = BERT4Rec(BERT4RecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    sd = bw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    assert np.array_equal(bw.checksums(sd), np.load(FX)["weight_checksums"])
    model.load_state_dict(sd, strict=True)
    assert float(model.head.bias.detach().abs().mean()) > 0.1                # the fixture's bias is not the zero the class starts with
    assert torch.equal(model.item_embedding.weight, sd["head.token_embeddings.weight"])


def test_seeded_init_equals_the_reference_bit_for_bit():
    m = _meta()
    torch.manual_seed(m["init_seed"])
    model = BERT4Rec(BERT4RecConfig(**m["config"]), m["init_n_items"], m["init_max_his_len"])
    assert np.array_equal(bw.checksums(model.state_dict()), np.load(FX)["init_checksums"])
    # rows 0 and <MASK> are drawn like the rest; LayerNorms untouched; biases zero
    w = model.item_embedding.weight
    assert float(w[0].detach().abs().sum()) > 0 and float(w[-1].detach().abs().sum()) > 0
    assert float(model.head.bias.detach().abs().sum()) == 0 and float(model.output_bias.detach().abs().sum()) == 0


def test_output_bias_is_outside_the_graph():
    """forward never reads output_bias (the reference leaves its .grad None): the M = 0 loss, the one graph that exists without
    a GPU, reaches every other trained parameter with a zero gradient and not output_bias"""
    m = _meta()
    assert "output_bias" in m["no_grad"] and "output_bias" in m["m0_no_grad"]
    assert m["m0_loss_is_nan"] and m["m0_grads_all_zero"]
    model = BERT4Rec(BERT4RecConfig(**m["config"]), 50, 8)
    empty = torch.empty(0, dtype=torch.long)
    loss = model._loss(torch.zeros(2, 8, dtype=torch.long), empty, empty)
    assert torch.isnan(loss)
    loss.backward()
    none = [n for n, p in model.named_parameters() if p.grad is None]
    assert none == m["m0_no_grad"]
    assert all(bool((p.grad == 0).all()) for p in model.parameters() if p.grad is not None)


def test_refusals():
    with pytest.raises(NotImplementedError, match="CE"):
        BERT4Rec(BERT4RecConfig(loss_type="BPR"), 10, 8)
    with pytest.raises(NotImplementedError, match="hidden_size"):
        BERT4Rec(BERT4RecConfig(hidden_size=66), 10, 8)
    with pytest.raises(NotImplementedError, match="hidden_size"):
        BERT4Rec(BERT4RecConfig(hidden_size=512, n_heads=8), 10, 8)
    model = BERT4Rec(BERT4RecConfig(), 10, 8)
    ids, n = torch.ones(2, 8, dtype=torch.long), torch.tensor([8, 8])
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.calculate_loss(dict(inputs=ids, seq_len=n))
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.reconstruct_train_data(ids, n)
    with pytest.raises(RuntimeError, match="HIP device only"):
        model.full_sort_topk(dict(inputs=ids, seq_len=n), 5)
    with pytest.raises(NotImplementedError, match="candidates"):
        model(ids, ids, candidates=ids)


def test_train_bert4rec_arguments():
    a = train_bert4rec.parse_args([])
    assert (a.backbone, a.tasks, a.test_task, a.base_model) == ("BERT4Rec", "smb_dis_decoder", "smb_dis_target",
                                                                "./config/dis-models/BERT4Rec")
    r = train_rec.parse_args([])
    same = [k for k in vars(a) if k not in ("backbone", "tasks", "test_task", "base_model")]
    assert same and all(getattr(a, k) == getattr(r, k) for k in same)
    a = train_bert4rec.parse_args(["--tasks", "smb_dis_diff_decoder", "--test_task", "smb_dis_target_diff", "--max_his_len", "50"])
    assert (a.tasks, a.test_task, a.max_his_len) == ("smb_dis_diff_decoder", "smb_dis_target_diff", 50)
    with pytest.raises(NotImplementedError):
        train_bert4rec.parse_args(["--backbone", "SASRec"])
    with pytest.raises(NotImplementedError):
        train_rec.parse_args(["--backbone", "BERT4Rec"])
    assert (r.backbone, r.tasks, r.test_task) == ("SASRec", "smb_dis", "smb_dis") and set(train_rec.BACKBONES) == {"SASRec", "GRU4Rec"}
