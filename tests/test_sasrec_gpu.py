"""SASRec's catalogue kernels and model on the GPU: the fused CE head, top K and large-table embedding gradient against fp64
torch, and the model against the real reference class (tests/golden/sasrec_small.npz, tools/make_golden_sasrec.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import sasrec_weights as sw  # noqa: E402

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "sasrec_small.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from gamer_amd import build
    build.build()


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _ce_case(V, R, H, seed, gaps=True):
    from gamer_amd import ops
    g = torch.Generator().manual_seed(seed)
    n_rows = 2 * R + 3 if gaps else R
    hfull = torch.randn(n_rows, H, generator=g, dtype=torch.float64) * 0.3        # scores of O(1), as a trained head gives
    E = torch.randn(V, H, generator=g, dtype=torch.float64) * 0.5
    rows = (torch.randperm(n_rows, generator=g)[:R] if gaps else torch.arange(R)).to(torch.int64)
    tgt = torch.randint(0, V, (R,), generator=g)
    hd, Ed = hfull.float().to(DEV), E.float().to(DEV).contiguous()
    rows_d, tgt_d = rows.to(DEV), tgt.to(DEV)
    lse, loss = torch.empty(R, device=DEV), torch.empty((), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.catalog_ce_fwd(hd, rows_d, Ed, tgt_d, lse, loss, bad)
    dE = torch.zeros_like(Ed)
    dh = torch.zeros_like(hd)
    dl = torch.full((), 1.5, device=DEV)
    ops.catalog_ce_bwd(hd, rows_d, Ed, tgt_d, lse, dl, 1.0 / R, dE=dE, dh=dh)
    torch.cuda.synchronize()
    # fp64 reference on the fp32-rounded inputs
    h64 = hd.double().cpu()[rows].requires_grad_(True)
    E64 = Ed.double().cpu().requires_grad_(True)
    logits = h64 @ E64.t()
    ref_loss = torch.nn.functional.cross_entropy(logits, tgt)
    (1.5 * ref_loss).backward()
    ref_dh = torch.zeros(n_rows, H, dtype=torch.float64)
    ref_dh[rows] = h64.grad
    return dict(lse=lse, loss=loss, dE=dE, dh=dh, bad=bad, ref_lse=torch.logsumexp(logits, 1).detach(), ref_loss=ref_loss.detach(),
                ref_dE=E64.grad, ref_dh=ref_dh)


@pytest.mark.parametrize("V", [1, 17, 8193, 40009])
@pytest.mark.parametrize("R", [1, 5, 300])
@pytest.mark.parametrize("H", [64, 128])
def test_catalog_ce_against_fp64(V, R, H):
    c = _ce_case(V, R, H, seed=V * 7 + R * 3 + H)
    assert int(c["bad"].item()) == 0
    assert abs(float(c["loss"]) - float(c["ref_loss"])) <= 1e-6 * max(1.0, abs(float(c["ref_loss"])))
    assert _rel(c["lse"], c["ref_lse"]) < 1e-6
    assert _rel(c["dE"], c["ref_dE"]) < 1e-5
    assert _rel(c["dh"], c["ref_dh"]) < 1e-5


def test_catalog_ce_repeatable_and_int32_rows():
    from gamer_amd import ops
    a = _ce_case(8193, 300, 128, seed=1)
    b = _ce_case(8193, 300, 128, seed=1)
    for k in ("lse", "loss", "dE", "dh"):
        assert torch.equal(a[k], b[k]), k
    g = torch.Generator().manual_seed(2)
    h = torch.randn(40, 64, generator=g).to(DEV)
    E = torch.randn(300, 64, generator=g).to(DEV)
    rows = torch.arange(0, 40, 2, device=DEV)
    tgt = torch.randint(0, 300, (20,), generator=g).to(DEV)
    out = []
    for r in (rows, rows.int()):
        lse, loss, bad = torch.empty(20, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.catalog_ce_fwd(h, r, E, tgt, lse, loss, bad)
        out.append(lse.clone())
    assert torch.equal(out[0], out[1])


def test_catalog_ce_flags_bad_targets():
    from gamer_amd import ops
    h, E = torch.randn(4, 64, device=DEV), torch.randn(10, 64, device=DEV)
    tgt = torch.tensor([0, 10, -1, 3], device=DEV)
    lse, loss, bad = torch.empty(4, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.catalog_ce_fwd(h, None, E, tgt, lse, loss, bad)
    assert int(bad.item()) == 2


def test_training_step_does_not_materialise_logits():
    from gamer_amd import rec_common
    from gamer_amd.sasrec import SASRec, SASRecConfig
    R, V, S = 4096, 200_000, 20
    limit = R * V * 4                               # one [R, V] fp32 logits tensor: 3.3 GB
    torch.manual_seed(0)
    model = SASRec(SASRecConfig(dropout_prob=0.0, n_layers=1, hidden_size=64, inner_size=128), V - 1, S).to(DEV)
    g = torch.Generator().manual_seed(1)
    inputs = torch.randint(1, V, (R, S), generator=g).to(DEV)
    inter = dict(inputs=inputs, seq_len=torch.full((R,), S, device=DEV), target=torch.randint(1, V, (R,), generator=g).to(DEV))
    model.train()

    def peak_of(fn):
        fn()                                          # warm the cached workspaces
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def step():
        model.zero_grad(set_to_none=True)
        loss = model.calculate_loss(inter)
        loss.backward()
        assert torch.isfinite(loss)
    peak = peak_of(step)
    assert peak < 0.3 * limit, peak                   # the whole step, encoder activations included
    h = torch.randn(R, 64, device=DEV, requires_grad=True)
    E = model.item_embedding.weight

    def head():
        E.grad = None
        rec_common.CatalogCEFn.apply(h, torch.arange(R, device=DEV), E, inter["target"]).backward()
    peak = peak_of(head)
    assert peak < 0.05 * limit, peak                  # the head alone: dE, dh and the workspace


@pytest.mark.parametrize("H", [64, 256])
def test_topk_against_torch_topk(H):
    from gamer_amd import ops
    g = torch.Generator().manual_seed(3)
    R, V = 37, 5000
    # every row scores the items on its own permutation of a 1e-3 grid (column r of h picks column r of E): neighbours
    # differ far more than the fp32 error, and a row written to the wrong place cannot pass
    E = torch.zeros(V, H, dtype=torch.float64)
    for r in range(R):
        E[:, r] = torch.randperm(V, generator=g).double() * 1e-3
    h = torch.zeros(R, H, dtype=torch.float64)
    h[torch.arange(R), torch.arange(R)] = 1.0
    Ed = E.float().to(DEV)
    for k, (s, e) in [(10, (0, V)), (64, (0, V)), (1, (0, V)), (10, (1000, 3000)), (20, (4990, 5000)), (5, (7, 9))]:
        idx, sc = ops.catalog_topk(h.float().to(DEV), Ed, k, s, e)
        scores = h @ E[s:e].t()
        kk = min(k, e - s)
        ref_s, ref_i = torch.topk(scores, kk, dim=1)
        assert torch.equal(idx[:, :kk].cpu(), ref_i + s), (k, s, e)
        assert torch.allclose(sc[:, :kk].double().cpu(), ref_s, atol=1e-5)
        if kk < k:
            assert bool((idx[:, kk:] == -1).all()) and bool(torch.isinf(sc[:, kk:]).all())


def test_catalog_ce_h256():
    c = _ce_case(3001, 70, 256, seed=256)
    assert abs(float(c["loss"]) - float(c["ref_loss"])) <= 1e-6 * max(1.0, abs(float(c["ref_loss"])))
    assert _rel(c["dE"], c["ref_dE"]) < 1e-5 and _rel(c["dh"], c["ref_dh"]) < 1e-5


def test_wrappers_refuse_bad_dtypes_and_layouts():
    from gamer_amd import ops
    h, E = torch.randn(4, 64, device=DEV), torch.randn(10, 64, device=DEV)
    lse, loss, bad = torch.empty(4, device=DEV), torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="target"):
        ops.catalog_ce_fwd(h, None, E, torch.zeros(4, dtype=torch.int32, device=DEV), lse, loss, bad)
    with pytest.raises(RuntimeError, match="E must be contiguous"):
        ops.catalog_ce_fwd(h, None, torch.randn(64, 10, device=DEV).t(), torch.zeros(4, dtype=torch.long, device=DEV), lse, loss, bad)
    with pytest.raises(RuntimeError, match="dh must be contiguous"):
        ops.catalog_ce_bwd(h, None, E, torch.zeros(4, dtype=torch.long, device=DEV), lse, None, 0.25,
                           dh=torch.zeros(64, 4, device=DEV).t())
    with pytest.raises(RuntimeError, match="ids"):
        ops.embedding_bwd_large(torch.zeros(4, dtype=torch.int32, device=DEV), h, 0, E)


def test_topk_ties_take_the_lower_index():
    from gamer_amd import ops
    g = torch.Generator().manual_seed(4)
    R, V, H = 9, 3000, 128
    base = torch.randn(50, H, generator=g)
    E = base[torch.randint(0, 50, (V,), generator=g)]          # many duplicated rows: exact ties
    h = torch.randn(R, H, generator=g)
    idx, _ = ops.catalog_topk(h.to(DEV), E.to(DEV), 40)
    scores = (h.double() @ E.double().t())
    ref = torch.argsort(-scores, dim=1, stable=True)[:, :40]
    assert torch.equal(idx.cpu(), ref)


def test_embedding_grad_large_table():
    from gamer_amd import ops
    g = torch.Generator().manual_seed(5)
    V, T, H = 70_000, 4000, 64
    ids = torch.randint(0, V, (T,), generator=g)
    ids[::7] = 0                                              # padding tokens
    ids[1::5] = 12345                                         # a popular item
    ids[2::5] = 777                                           # and a second one
    dx = torch.randn(T, H, generator=g)
    outs = []
    for _ in range(2):
        dW = torch.full((V, H), 0.25, device=DEV)
        ops.embedding_bwd_large(ids.to(DEV), dx.to(DEV), 0, dW)
        outs.append(dW.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = torch.full((V, H), 0.25, dtype=torch.float64)
    keep = ids != 0
    ref.index_add_(0, ids[keep], dx.double()[keep])
    assert torch.equal(outs[0][0], torch.full((H,), 0.25))
    assert _rel(outs[0] - 0.25, ref - 0.25) < 1e-5


def test_position_grad():
    from gamer_amd import ops
    dx = torch.randn(300, 7, 64)
    dP = torch.zeros(9, 64, device=DEV)
    ops.position_bwd(dx.to(DEV), dP[:7])
    assert _rel(dP[:7], dx.double().sum(0)) < 1e-6 and float(dP[7:].abs().sum()) == 0


# ---- the model against the real reference class ------------------------------------------------------------------------------
def _model():
    from gamer_amd.sasrec import SASRec, SASRecConfig
    z = np.load(FX)
    m = json.loads(str(z["meta_json"]))
    model = SASRec(SASRecConfig(**m["config"]), m["n_items"], m["max_his_len"])
    sd = sw.init_state_dict({k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}, m["weight_seed"])
    model.load_state_dict(sd)
    inter = dict(inputs=torch.from_numpy(z["inputs"]).to(DEV), seq_len=torch.from_numpy(z["seq_len"]).to(DEV),
                 target=torch.from_numpy(z["target"]).to(DEV))
    return model.to(DEV), z, m, inter


def test_sasrec_forward_loss_and_grads_match_reference():
    model, z, m, inter = _model()
    model.eval()
    with torch.no_grad():
        out = model(inter["inputs"], inter["seq_len"])
    assert _rel(out, z["out"]) < 2e-5
    model.train()
    model.zero_grad()
    loss = model.calculate_loss(inter)
    loss.backward()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    for k, p in model.named_parameters():
        if k.endswith("key.bias"):
            # softmax is invariant to a per-row shift: the key bias gradient is zero up to rounding on both sides
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6
        elif "grad/" + k in z.files:
            assert p.grad is not None and _rel(p.grad, z["grad/" + k]) < 2e-4, k
    gi = model.item_embedding.weight.grad
    rows = torch.from_numpy(z["rows"])
    assert _rel(gi.cpu()[rows], z["grad_item_rows"]) < 2e-4
    assert float(gi[0].abs().sum()) > 0                  # the head reaches the padding row
    ck = sw.checksums({"g": gi.cpu()})[0]
    ref = z["grad_item_checksum"]
    assert abs(ck[0] - ref[0]) < 2e-4 * np.sqrt(ref[1]) * 10 and abs(ck[1] - ref[1]) < 1e-3 * ref[1]


@pytest.mark.parametrize("ranged", [False, True])
def test_sasrec_full_sort_matches_reference(ranged):
    model, z, m, inter = _model()
    model.eval()
    if ranged:
        inter = dict(inter, item_range=tuple(m["item_range"]))
    with torch.no_grad():
        scores = model.full_sort_predict(dict(inter))
    cols = torch.from_numpy(z["cols"])
    ref = torch.from_numpy(z["scores_r_cols" if ranged else "scores_cols"])
    got = scores.cpu()[:, cols]
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin)
    assert _rel(got[fin], ref[fin]) < 2e-5
    idx, sc = model.full_sort_topk(dict(inter), 10)
    ref_top = torch.from_numpy(z["top10_r" if ranged else "top10"])
    full = scores.cpu()
    for b in range(idx.shape[0]):
        for q in range(10):
            a, r = int(idx[b, q]), int(ref_top[b, q])
            # identical ranks unless two neighbours' scores lie within fp32 noise of each other
            assert a == r or abs(float(full[b, a]) - float(full[b, r])) < 1e-5, (b, q, a, r)


def test_sasrec_dropout_training_is_finite_and_repeatable():
    from gamer_amd import rec_common
    model, z, m, inter = _model()
    model.dropout_prob = 0.5
    for layer in model.trm_encoder.layer:
        layer.dropout_p = 0.5
    model.train()
    res = []
    for _ in range(2):
        rec_common._Seeds.value = 77
        from gamer_amd import modules
        modules._SeedCounter.value = 99
        model.zero_grad()
        loss = model.calculate_loss(inter)
        loss.backward()
        res.append((loss.detach().clone(), model.item_embedding.weight.grad.clone(), model.position_embedding.weight.grad.clone()))
    assert torch.isfinite(res[0][0])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_train_rec_two_epochs_and_only_test(tmp_path):
    import subprocess
    from gamer_amd import synthetic
    synthetic.write_smb_dataset(str(tmp_path), "syn", n_users=60, n_items=40, seed=5, min_sessions=3)
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    (cfg / "config.json").write_text(json.dumps(dict(hidden_size=64, inner_size=128, dropout_prob=0.1)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--base_model", str(cfg), "--data_path", str(tmp_path), "--dataset", "syn", "--tasks", "smb_dis_diff",
              "--test_task", "smb_dis_diff", "--max_his_len", "8", "--batch_size", "32", "--learning_rate", "3e-3",
              "--output_dir", str(tmp_path / "out"), "--result_dir", str(tmp_path / "res"), "--seed", "1"]
    run = lambda extra: subprocess.run([sys.executable, "-m", "gamer_amd.train_rec", *common, *extra], cwd=root, capture_output=True,
                                       text=True, timeout=300)
    r = run(["--epochs", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if " loss " in l]
    assert len(losses) == 2 and losses[1] < losses[0], r.stdout
    meta = json.loads(str(np.load(FX)["meta_json"]))
    sd = torch.load(tmp_path / "out" / "best_model.pth", map_location="cpu")
    assert len(sd) == len(meta["keys"]) and all(k in sd for k in meta["keys"])
    res = json.load(open(tmp_path / "res" / "result-smb_dis_diff.json"))
    metrics = "hit@1,hit@5,hit@10,recall@1,recall@5,recall@10,ndcg@5,ndcg@10".split(",")
    assert [e["eval_type"] for e in res] == ["Behavior click", "Behavior cart", "Behavior buy", "Merged Behavior"]
    assert all(all(m in e for m in metrics) for e in res)
    r2 = run(["--only_test"])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert json.load(open(tmp_path / "res" / "result-smb_dis_diff.json")) == res
