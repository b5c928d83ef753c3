"""SASRec on the HIP path, the parts that need no GPU: the config surface and the parameter layout against the real reference
class (tests/golden/sasrec_small.npz, tools/make_golden_sasrec.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import sasrec_weights as sw  # noqa: E402

from gamer_amd.sasrec import SASRec, SASRecConfig

FX = os.path.join(os.path.dirname(__file__), "golden", "sasrec_small.npz")


def _meta():
    return json.loads(str(np.load(FX)["meta_json"]))


def test_config_defaults_are_the_reference_config_json():
    c = SASRecConfig()
    assert c.to_dict() == dict(n_layers=2, n_heads=2, hidden_size=128, inner_size=256, dropout_prob=0.5, hidden_act="gelu",
                               layer_norm_eps=1e-12, initializer_range=0.02, loss_type="CE")


def test_config_from_pretrained(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(dict(hidden_size=64, n_heads=4, dropout_prob=0.2)))
    c = SASRecConfig.from_pretrained(str(tmp_path))
    assert (c.hidden_size, c.n_heads, c.dropout_prob, c.n_layers, c.inner_size) == (64, 4, 0.2, 2, 256)
    with pytest.raises(ValueError):
        SASRecConfig.from_pretrained(str(tmp_path / "missing"))
    (tmp_path / "config.json").write_text(json.dumps(dict(hidden_sise=64)))
    with pytest.raises(ValueError):
        SASRecConfig.from_pretrained(str(tmp_path))


def test_bpr_loss_refused():
    with pytest.raises(NotImplementedError):
        SASRec(SASRecConfig(loss_type="BPR"), 10, 5)


def test_state_dict_keys_and_shapes_equal_the_reference():
    m = _meta()
    model = SASRec(SASRecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    sd = model.state_dict()
    assert list(sd) == m["keys"]
    assert [list(v.shape) for v in sd.values()] == m["shapes"]


def test_reference_weights_load_and_are_pinned():
    m = _meta()
    model = SASRec(SASRecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    shapes = {k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}
    sd = sw.init_state_dict(shapes, m["weight_seed"])
    np.testing.assert_allclose(sw.checksums(sd), np.load(FX)["weight_checksums"], rtol=1e-12, atol=1e-9)
    model.load_state_dict(sd)                       # strict: a reference best_model.pth has exactly these keys
    assert torch.equal(model.item_embedding.weight[0], sd["item_embedding.weight"][0])


def test_init_draws_the_padding_row_like_the_reference():
    torch.manual_seed(3)
    model = SASRec(SASRecConfig(hidden_size=64), 50, 8)
    assert float(model.item_embedding.weight[0].abs().sum()) > 0          # apply(_init_weights) overwrites row 0 too
    assert torch.equal(model.LayerNorm.weight, torch.ones(64))


def test_forward_refuses_the_cpu():
    model = SASRec(SASRecConfig(hidden_size=64), 50, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        model(torch.ones(2, 3, dtype=torch.long), torch.tensor([3, 2]))


@pytest.mark.parametrize("lens", [[0, 2], [3, 4], [1]])
def test_seq_len_outside_the_rows_is_refused(lens):
    model = SASRec(SASRecConfig(hidden_size=64), 50, 8)
    with pytest.raises(IndexError, match="seq_len"):
        model(torch.ones(2, 3, dtype=torch.long), torch.tensor(lens))
