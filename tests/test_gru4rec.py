"""GRU4Rec on the HIP path, the parts that need no GPU: the config surface, the parameter layout and init against the real
reference class (tests/golden/gru4rec_small.npz, tools/make_golden_gru4rec.py), the refusals and train_rec's arguments."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import gru4rec_weights as gw  # noqa: E402

from gamer_amd import train_rec
from gamer_amd.gru4rec import GRU4Rec, GRU4RecConfig

FX = os.path.join(os.path.dirname(__file__), "golden", "gru4rec_small.npz")
# config/dis-models/GRU4Rec/config.json as the reference ships it
SHIPPED = {"embedding_size": 64, "hidden_size": 128, "num_layers": 1, "dropout_prob": 0.3, "loss_type": "CE"}


def _meta():
    return json.loads(str(np.load(FX)["meta_json"]))


def test_config_defaults_are_the_reference_class_defaults():
    assert GRU4RecConfig().to_dict() == dict(embedding_size=64, hidden_size=128, n_layers=1, dropout=0.3, loss_type="CE")


def test_shipped_config_loads_like_the_reference(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(SHIPPED))
    with pytest.warns(UserWarning, match="dropout_prob.*num_layers"):
        c = GRU4RecConfig.from_pretrained(str(tmp_path))
    assert (c.n_layers, c.dropout) == (1, 0.3)
    m = _meta()
    assert m["shipped_json"] == SHIPPED
    assert c.to_dict() == m["shipped_effective"]                   # what the reference's pydantic class made of the same file
    (tmp_path / "config.json").write_text(json.dumps(dict(n_layers=2, dropout=0.1, hidden_size=64)))
    c = GRU4RecConfig.from_pretrained(str(tmp_path))
    assert (c.n_layers, c.dropout, c.hidden_size, c.embedding_size) == (2, 0.1, 64, 64)
    with pytest.raises(ValueError):
        GRU4RecConfig.from_pretrained(str(tmp_path / "missing"))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_state_dict_keys_and_shapes_equal_the_reference(tag):
    m = _meta()
    c = m["configs"][tag]
    model = GRU4Rec(GRU4RecConfig(**c["config"]), m["n_items"], max_his_len=m["max_his_len"], n_users=3)
    sd = model.state_dict()
    assert list(sd) == c["keys"]
    assert [list(v.shape) for v in sd.values()] == c["shapes"]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_weights_load_and_are_pinned(tag):
    m = _meta()
    c = m["configs"][tag]
    model = GRU4Rec(GRU4RecConfig(**c["config"]), m["n_items"])
    sd = gw.init_state_dict({k: tuple(s) for k, s in zip(c["keys"], c["shapes"])}, c["weight_seed"])
    np.testing.assert_allclose(gw.checksums(sd), np.load(FX)[tag + "/weight_checksums"], rtol=1e-12, atol=1e-9)
    model.load_state_dict(sd)                       # strict: a reference best_model.pth has exactly these keys
    assert torch.equal(model.gru_layers.weight_hh_l0, sd["gru_layers.weight_hh_l0"])


def test_init_follows_the_reference_quirks():
    torch.manual_seed(3)
    model = GRU4Rec(GRU4RecConfig(embedding_size=32, hidden_size=64, n_layers=2), 500)
    E = model.item_embedding.weight.detach()
    assert float(E[0].abs().sum()) > 0                              # xavier_normal_ over the whole table, row 0 included
    assert abs(float(E.std()) - (2.0 / (501 + 32)) ** 0.5) < 0.1 * (2.0 / (501 + 32)) ** 0.5
    for name, (fo, fi) in (("weight_ih_l0", (192, 32)), ("weight_hh_l0", (192, 64))):
        w = getattr(model.gru_layers, name)
        bound = (6.0 / (fo + fi)) ** 0.5                            # xavier_uniform_ on layer 0
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound, name
    default = 1.0 / 64 ** 0.5                                       # nn.GRU's own uniform(-1/sqrt(H), 1/sqrt(H)) above layer 0
    for name in ("weight_ih_l1", "weight_hh_l1"):
        w = getattr(model.gru_layers, name)
        assert float(w.abs().max()) <= default and float(w.abs().max()) > 0.9 * default, name
    assert float(model.dense.weight.abs().max()) <= default      # nn.Linear's default init


def test_bpr_and_unsupported_sizes_are_refused():
    with pytest.raises(NotImplementedError):
        GRU4Rec(GRU4RecConfig(loss_type="BPR"), 10)
    for kw in (dict(hidden_size=100), dict(hidden_size=512), dict(embedding_size=6), dict(embedding_size=512),
               dict(hidden_size=8)):
        with pytest.raises(NotImplementedError):
            GRU4Rec(GRU4RecConfig(**kw), 10)


def test_forward_refuses_the_cpu():
    model = GRU4Rec(GRU4RecConfig(hidden_size=64), 50)
    with pytest.raises(RuntimeError, match="HIP device"):
        model(torch.ones(2, 3, dtype=torch.long), torch.tensor([3, 2]))


@pytest.mark.parametrize("lens", [[0, 2], [3, 4], [1]])
def test_seq_len_outside_the_rows_is_refused(lens):
    model = GRU4Rec(GRU4RecConfig(hidden_size=64), 50)
    with pytest.raises(IndexError, match="seq_len"):
        model(torch.ones(2, 3, dtype=torch.long), torch.tensor(lens))
    with pytest.raises(IndexError, match="seq_len"):
        model.calculate_loss(dict(inputs=torch.ones(2, 3, dtype=torch.long), seq_len=torch.tensor(lens),
                                  target=torch.ones(2, dtype=torch.long)))


def test_train_rec_arguments():
    a = train_rec.parse_args(["--backbone", "GRU4Rec"])
    assert a.backbone == "GRU4Rec" and a.base_model == "./config/dis-models/GRU4Rec"
    a = train_rec.parse_args(["--backbone", "GRU4Rec", "--base_model", "/x/y", "--max_his_len", "-1"])
    assert a.base_model == "/x/y" and a.max_his_len == -1
    assert train_rec.BACKBONES["GRU4Rec"] == (GRU4Rec, GRU4RecConfig)
    # SASRec's path and defaults are unchanged
    a = train_rec.parse_args([])
    assert (a.backbone, a.base_model, a.max_his_len, a.batch_size, a.learning_rate) == \
        ("SASRec", "./config/dis-models/SASRec", 20, 256, 5e-4)
    for other in ("BERT4Rec", "MBHT"):
        with pytest.raises(NotImplementedError):
            train_rec.parse_args(["--backbone", other])
