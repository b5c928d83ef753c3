"""The RQ-VAE item tokenizer's host side (no GPU): parameter names and initialisation, the refusals, the positives sampler and
the Sinkhorn restatement against the real reference classes' recordings (tests/golden/rqvae_small.npz,
tools/make_golden_rqvae.py), the data rule, the checkpoint format and the commands' arguments."""
import argparse
import json
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

from gamer_amd import rqvae, tokenize_items, train_rqvae
from gamer_amd.rqvae import RQVAE


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rqvae_small")


def _small(meta, cfg="a", **kw):
    c = dict(meta["configs"][cfg])
    c.update(kw)
    return RQVAE(in_dim=meta["in_dim"], num_emb_list=meta["num_emb_list"], e_dim=meta["e_dim"], layers=meta["layers"], **c)


@pytest.mark.parametrize("cfg", ["a", "b"])
def test_state_dict_keys_and_shapes_are_the_references(fx, cfg):
    z, meta = fx
    sd = _small(meta, cfg, cluster_backend="sklearn").state_dict()
    assert list(sd.keys()) == meta[f"{cfg}_keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == meta[f"{cfg}_shapes"]


def test_initialisation():
    torch.manual_seed(0)
    m = RQVAE(in_dim=96, num_emb_list=[16, 40], e_dim=8, layers=[128, 64], sk_epsilons=[0.0, 0.0], beta=0.0, cluster_backend="none")
    for name, p in m.named_parameters():
        if name.endswith(".bias"):
            assert float(p.detach().abs().max()) == 0.0
        elif "mlp_layers" in name:
            n_out, n_in = p.shape
            std = math.sqrt(2.0 / (n_in + n_out))                     # Xavier-normal
            assert abs(float(p.detach().std()) - std) < 0.1 * std, name
            assert abs(float(p.detach().mean())) < 0.1 * std, name
    for q, k in zip(m.rq.vq_layers, [16, 40]):
        w = q.embedding.weight.detach()
        assert q.initted and float(w.abs().max()) <= 1.0 / k and float(w.abs().max()) > 0.5 / k
    m = RQVAE(in_dim=96, num_emb_list=[16, 40], e_dim=8, layers=[32], sk_epsilons=[0.0, 0.0], kmeans_init=True, cluster_backend="sklearn")
    for q in m.rq.vq_layers:
        assert not q.initted and float(q.embedding.weight.abs().max()) == 0.0
    a = m.args
    assert isinstance(a, argparse.Namespace)
    assert sorted(vars(a)) == sorted(["in_dim", "num_emb_list", "e_dim", "layers", "dropout_prob", "bn", "loss_type", "quant_loss_weight",
                                      "kmeans_init", "kmeans_iters", "sk_epsilons", "sk_iters", "alpha", "beta", "n_clusters",
                                      "sample_strategy"])


@pytest.mark.parametrize("kw, err", [
    (dict(bn=True), NotImplementedError),
    (dict(dropout_prob=0.1), NotImplementedError),
    (dict(e_dim=68), NotImplementedError),
    (dict(e_dim=6), NotImplementedError),
    (dict(num_emb_list=[16, 1025]), NotImplementedError),
    (dict(num_emb_list=[4] * 9, sk_epsilons=[0.0] * 9), NotImplementedError),
    (dict(cluster_backend="none", beta=1e-4), ValueError),
    (dict(cluster_backend="none", beta=0.0, kmeans_init=True), ValueError),
    (dict(cluster_backend="nope"), ValueError),
])
def test_refusals(kw, err):
    base = dict(in_dim=16, num_emb_list=[16, 16], e_dim=8, layers=[16], sk_epsilons=[0.0, 0.0], cluster_backend="sklearn")
    base.update(kw)
    with pytest.raises(err):
        RQVAE(**base)


def test_forward_refuses_the_cpu():
    m = RQVAE(in_dim=16, num_emb_list=[16, 16], e_dim=8, layers=[16], sk_epsilons=[0.0, 0.0], beta=0.0, cluster_backend="none")
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(3, 16), None)


def test_a_cluster_of_one_code_is_an_error_not_a_spin():
    labels = [j % 10 for j in range(12)]                # clusters 2 .. 9 hold one code each
    assert rqvae.sample_positives([0, 11, 1], labels, level=2) in ([10, 1, 11],)
    with pytest.raises(ValueError, match=r"level 2 cluster 5 .* other than 5"):
        rqvae.sample_positives([0, 5], labels, level=2)


def test_positives_sampler_reproduces_the_references_draws(fx):
    z, meta = fx
    labels = json.loads(str(z["labels_json"]))
    idx, want = z["b/indices"], z["b/positives"]
    random.seed(meta["py_seed"])
    got = np.array([rqvae.sample_positives(idx[:, l].tolist(), labels[str(l)], l) for l in range(idx.shape[1])]).T
    assert np.array_equal(got, want)
    assert (got != idx).all()
    for l in range(idx.shape[1]):
        assert all(labels[str(l)][g] == labels[str(l)][i] for g, i in zip(got[:, l], idx[:, l]))


def test_sinkhorn_gives_the_references_plan(fx):
    z, meta = fx
    cfg = meta["configs"]["b"]
    d = torch.from_numpy(z["b/dist_last"])
    assert d.dtype == torch.float32
    Q = rqvae.sinkhorn_algorithm(rqvae.center_distance_for_constraint(d).double(), cfg["sk_epsilons"][-1], cfg["sk_iters"])
    want = torch.from_numpy(z["b/Q_last"])
    assert Q.dtype == torch.float64 and want.dtype == torch.float64
    assert float(((Q - want).abs() / want.abs().clamp_min(1e-300)).max()) <= 1e-12
    assert torch.equal(Q.argmax(-1), torch.from_numpy(z["b/indices"][:, -1]))
    assert torch.equal(rqvae.sinkhorn_indices(d, cfg["sk_epsilons"][-1], cfg["sk_iters"]), Q.argmax(-1))
    assert float(z["b/dist_gap"][:, :-1].min()) >= 1e-4 and float(z["b/q_gap"].min()) >= 1e-2


def test_sinkhorn_warns_about_nan(monkeypatch):
    monkeypatch.setattr(rqvae, "sinkhorn_algorithm", lambda d, eps, it: torch.full_like(d, float("nan")))
    with pytest.warns(UserWarning, match="nan/inf"):
        rqvae.sinkhorn_indices(torch.tensor([[0.0, 1.0], [1.0, 2.0]]), 0.003, 2)


def test_emb_dataset_divides_a_low_std_set_by_its_std(tmp_path):
    g = np.random.default_rng(0)
    low, high = (0.05 * g.standard_normal((50, 6))).astype(np.float32), g.standard_normal((50, 6)).astype(np.float32)
    np.save(tmp_path / "low.npy", low)
    np.save(tmp_path / "high.npy", high)
    d = train_rqvae.EmbDataset(str(tmp_path / "low.npy"))
    assert np.allclose(d.embeddings, low / low.std(), rtol=1e-6) and abs(float(d.embeddings.std()) - 1.0) < 1e-5
    d = train_rqvae.EmbDataset(str(tmp_path / "high.npy"))
    assert np.array_equal(d.embeddings, high) and d.dim == 6 and len(d) == 50
    x, i = d[3]
    assert i == 3 and torch.equal(x, torch.from_numpy(high[3]))


def _trainer(tmp_path, **kw):
    np.save(tmp_path / "emb.npy", np.random.default_rng(1).standard_normal((20, 16)).astype(np.float32))
    argv = ["--data_path", str(tmp_path / "emb.npy"), "--ckpt_dir", str(tmp_path / "ckpt"), "--num_emb_list", "8", "8", "--e_dim", "8",
            "--layers", "16", "--sk_epsilons", "0", "0.003", "--kmeans_init", "False", "--cluster_backend", "sklearn", "--epochs", "3"]
    a = train_rqvae.build_parser().parse_args(argv)
    for k, v in kw.items():
        setattr(a, k, v)
    data = train_rqvae.EmbDataset(a.data_path)
    model = RQVAE(in_dim=data.dim, num_emb_list=a.num_emb_list, e_dim=a.e_dim, layers=a.layers, kmeans_init=a.kmeans_init,
                  sk_epsilons=a.sk_epsilons, alpha=a.alpha, beta=a.beta, cluster_backend=a.cluster_backend)
    return train_rqvae.Trainer(model, a, data, torch.device("cpu")), model


def test_checkpoint_keys_and_file_names(tmp_path):
    tr, model = _trainer(tmp_path)
    assert re.fullmatch(r"[A-Z][a-z]{2}-\d\d-\d{4}_\d\d-\d\d-\d\d", os.path.basename(tr.ckpt_dir))
    assert os.path.dirname(tr.ckpt_dir) == str(tmp_path / "ckpt")
    p1 = tr.save_checkpoint(7, 0.12345)
    p2 = tr.save_checkpoint(7, 0.12345, tr.best_collision_ckpt)
    assert os.path.basename(p1) == "epoch_7_collision_0.1235_model.pth" and os.path.basename(p2) == "best_collision_model.pth"
    ck = torch.load(p1, map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["args", "epoch", "best_loss", "best_collision_rate", "state_dict", "optimizer"]
    assert ck["epoch"] == 7 and list(ck["state_dict"].keys()) == list(model.state_dict().keys())
    a = ck["args"]
    assert a.num_emb_list == [8, 8] and a.learner == "AdamW" and a.eval_step == 3 and a.ckpt_dir == tr.ckpt_dir and a.lr == 1e-3
    assert isinstance(tr.optimizer, torch.optim.AdamW)
    for name, cls in [("adam", torch.optim.Adam), ("SGD", torch.optim.SGD), ("Adagrad", torch.optim.Adagrad),
                      ("rmsprop", torch.optim.RMSprop), ("lion", torch.optim.Adam)]:
        assert type(train_rqvae.build_optimizer(model, name, 1e-3, 1e-4)) is cls


def test_tokenizer_accepts_num_code_list_and_module_prefixed_keys(tmp_path):
    tr, model = _trainer(tmp_path)
    path = tr.save_checkpoint(0, 0.5)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    got, _ = tokenize_items.load_model(path, 16, torch.device("cpu"), "none")
    args = vars(ck["args"]).copy()
    args["num_code_list"] = args.pop("num_emb_list")
    ck["args"] = argparse.Namespace(**args)
    ck["state_dict"] = {"module." + k: v for k, v in ck["state_dict"].items()}
    torch.save(ck, tmp_path / "ddp.pth")
    got2, _ = tokenize_items.load_model(str(tmp_path / "ddp.pth"), 16, torch.device("cpu"), "none")
    for m in (got, got2):
        assert m.num_emb_list == [8, 8] and not m.training
        for k, v in model.state_dict().items():
            assert torch.equal(m.state_dict()[k], v), k


def test_argument_defaults_are_the_reference_tasks(fx):
    _, meta = fx
    got = vars(train_rqvae.build_parser().parse_args([]))
    assert got.pop("cluster_backend") == "k_means_constrained"
    assert got == meta["task_defaults"]
    a = train_rqvae.build_parser().parse_args(["--kmeans_init", "False", "--bn", "0"])
    assert a.kmeans_init is False and a.bn is False
    t = vars(tokenize_items.build_parser().parse_args(["--data_path", "x.npy"]))
    assert (t["dataset"], t["output_dir"], t["root_path"], t["alpha"], t["beta"], t["epoch"], t["checkpoint"]) == \
        ("Instruments", "./data/", "./checkpoint/RQ-VAE", "0.2", "0.0001", 20000, "best_collision_model.pth")


def test_missing_cluster_package_names_the_other_choices(monkeypatch):
    monkeypatch.setitem(sys.modules, "k_means_constrained", None)           # importing it raises ImportError, installed or not
    with pytest.raises(ImportError, match=r"sklearn.*none"):
        rqvae.constrained_km(np.zeros((30, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        rqvae.constrained_km(np.zeros((30, 4), dtype=np.float32), backend="none")


def test_sklearn_backend_leaves_no_cluster_of_one():
    g = np.random.default_rng(3)
    codes = np.concatenate([g.standard_normal((24, 4)), 50 + g.standard_normal((1, 4))]).astype(np.float32)       # one far outlier
    centers, labels = rqvae.constrained_km(codes, backend="sklearn")
    assert len(labels) == 25 and min(np.bincount(labels)[np.unique(labels)]) >= 2
    rqvae.sample_positives(list(range(25)), labels)                                                                # does not raise
